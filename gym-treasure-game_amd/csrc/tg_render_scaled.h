// tg_render_scaled.h — per-output-pixel composition of the downscaled / grayscale frame
// (tg_render_scaled of include/tg_amd.h), shared by the gfx950 kernel (tg_render.hip
// k_render_scaled) and the host-only check build (tests/native_scaled), plus the host-side
// pooling of the static layer and the cell tiles.
//
// Definition (an extension: the reference has no such mode).  F = the env's full frame as
// tg_render writes it, s a divisor of 48:
//   S[y][x][c]   = sum of F[s*y + dy][s*x + dx][c] over dy, dx < s
//   out[y][x][c] = (2*S + s*s) / (2*s*s)              (the mean, halves round up)
//   gray         = (77*R + 150*G + 29*B + 128) >> 8   of the averaged RGB bytes
// SDL's blend d + ((s - d)*a >> 8) does not commute with averaging: the items are composited
// at full resolution, then summed.  Every s x s box lies inside one 48x48 cell, so the pooled
// static layer and the pooled (cell, sprite) tiles are exact wherever nothing else covers the
// box; elsewhere (the hero, a shaft or knob, two items in one cell) the box is composed pixel
// by pixel with tg_render.h's apply_layer in draw order.
#pragma once
#include "tg_render.h"

namespace tg {

constexpr int NSCALE = 10;  // the divisors of 48
inline int scale_index(int s) {
  const int d[NSCALE] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 48};
  for (int i = 0; i < NSCALE; ++i)
    if (d[i] == s) return i;
  return -1;
}

struct ScaledArgs {
  RenderArgs A;                 // the full-resolution tables (general path)
  const uint32_t* bg_small;     // pooled static layer [h][w] XRGB
  const uint32_t* tiles_small;  // pooled tiles [H*W][D_COUNT][cs][cs] XRGB
  int s, cs, w, h;              // scale, 48 / s, output pixels
  int ch;                       // 3 (RGB) or 1 (gray)
  int fast;                     // scaled_pixel only (the host check): 0 composes every pixel
                                // by the general path.  k_render_scaled does not read it.
};

// k_render_scaled's division of the work (tg_render.hip, where the passes are described): the
// frames of a group of SG envs are one run of SG * h * w output pixels, a workgroup takes a span
// of SSPAN of them and queues up to SQCAP boxes that scaled_lookup declines.  Here so that the
// host check counts a span's declined boxes with the kernel's own arithmetic.
constexpr int SG = 4;        // envs per group
constexpr int SSPAN = 4096;  // output pixels per workgroup
constexpr int SQCAP = 1024;  // queued boxes per workgroup

// pixel p of a group's run -> env k of the group and (x, y) in its frame of fp = h * w pixels
TG_HD void span_pixel(int p, int fp, int w, int& k, int& x, int& y) {
  k = p / fp;
  const int r = p - k * fp;
  y = r / w, x = r - y * w;
}

TG_HD uint32_t luma_px(uint32_t c) {
  return (77u * ((c >> 16) & 255u) + 150u * ((c >> 8) & 255u) + 29u * (c & 255u) + 128u) >> 8;
}

TG_HD uint32_t round_mean(uint32_t sum, uint32_t n) { return (2u * sum + n) / (2u * n); }

// items of `live` whose bounding box overlaps [X0, X1) x [Y0, Y1)
TG_HD uint32_t box_items(const Layer* lay, uint32_t live, int X0, int X1, int Y0, int Y1) {
  uint32_t hit = 0;
  for (uint32_t m = live; m; m &= m - 1) {
    const int i = __builtin_ctz(m);
    const Layer& l = lay[i];
    if (X0 < l.x1 && X1 > l.x0 && Y0 < l.y1 && Y1 > l.y0) hit |= 1u << i;
  }
  return hit;
}

// The general path: output pixel (x, y) from its s*s source pixels, each the static layer with
// the items `hit` over it in draw order (always correct for any superset of the box's items).
// One source row Y of the box: the three channel sums, SUM_BITS apart (a box sums to at most
// 255 * 48 * 48 < 2^20 per channel, so rows add up without carries between the fields).
constexpr int SUM_BITS = 21;
TG_HD uint64_t scaled_compose_row(const RenderArgs& A, const Layer* lay, uint32_t hit, int s, int x,
                                  int Y) {
  const uint8_t* p =
      reinterpret_cast<const uint8_t*>(A.bg) + ((size_t)Y * (size_t)A.Wpx + (size_t)(s * x)) * 3;
  const uint32_t rm = row_items(lay, hit, Y);
  uint32_t sr = 0, sg = 0, sb = 0;
  for (int dx = 0; dx < s; ++dx, p += 3) {
    uint32_t c = ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
    for (uint32_t m = rm; m; m &= m - 1) c = apply_layer(lay[__builtin_ctz(m)], A, c, s * x + dx, Y);
    sr += (c >> 16) & 255u, sg += (c >> 8) & 255u, sb += c & 255u;
  }
  return (uint64_t)sr | ((uint64_t)sg << SUM_BITS) | ((uint64_t)sb << (2 * SUM_BITS));
}
// the box's rounded means as XRGB from its summed rows
TG_HD uint32_t scaled_finish(uint64_t sums, int s) {
  const uint32_t n = (uint32_t)(s * s), mask = (1u << SUM_BITS) - 1u;
  return (round_mean((uint32_t)sums & mask, n) << 16) |
         (round_mean((uint32_t)(sums >> SUM_BITS) & mask, n) << 8) |
         round_mean((uint32_t)(sums >> (2 * SUM_BITS)) & mask, n);
}
TG_HD uint32_t scaled_compose(const RenderArgs& A, const Layer* lay, uint32_t hit, int s, int x,
                              int y) {
  uint64_t sums = 0;
  for (int dy = 0; dy < s; ++dy) sums += scaled_compose_row(A, lay, hit, s, x, s * y + dy);
  return scaled_finish(sums, s);
}

// Output pixel (x, y) of one env where a pooled table holds it: `live` = the env's items on
// the frame, `hit` = those whose bounding boxes overlap the pixel's box.  Untouched boxes come
// from bg_small; a box under one cell-aligned item alone in its cell, with no hero and no shaft
// or knob over it, from tiles_small.  Returns false where the box has to be composed.
TG_HD bool scaled_lookup(const ScaledArgs& P, const Layer* lay, uint32_t live, uint32_t hit, int x,
                         int y, uint32_t& c) {
  const int s = P.s, X0 = s * x, Y0 = s * y, X1 = X0 + s, Y1 = Y0 + s;
  if (hit) {
    const int cx = X0 / RS, cy = Y0 / RS;
    int n = 0, spr = 0;  // cell-aligned items on this cell (doors, bases, key, bolt, gold)
    for (uint32_t m = live & 0xFFu; m; m &= m - 1) {
      const Layer& l = lay[__builtin_ctz(m)];
      if (l.ox == cx * RS && l.oy == cy * RS) ++n, spr = l.spr;
    }
    bool full = n > 1 || (hit & HERO_ITEM) != 0u;
    for (uint32_t m = hit & HANDLE_ITEMS; m; m &= m - 1) {
      const Layer& l = lay[__builtin_ctz(m)];
      full |= X0 < l.sx1 && X1 > l.sx0 && Y0 < l.sy1 && Y1 > l.sy0;
    }
    if (full) return false;
    if (n) {
      c = P.tiles_small[(((size_t)(cy * P.A.W + cx) * D_COUNT + (size_t)spr) * (size_t)P.cs +
                         (size_t)(y - cy * P.cs)) * (size_t)P.cs + (size_t)(x - cx * P.cs)];
      return true;
    }
  }
  c = P.bg_small[(size_t)y * (size_t)P.w + (size_t)x];
  return true;
}

TG_HD uint32_t pixel_items(const ScaledArgs& P, const Layer* lay, uint32_t live, int x, int y) {
  return box_items(lay, live, P.s * x, P.s * x + P.s, P.s * y, P.s * y + P.s);
}

// Output pixel (x, y) of one env as XRGB (the averaged RGB bytes): the lookup, else the box
// composed in place.  The host check's driver; k_render_scaled calls scaled_lookup,
// scaled_compose_row and scaled_finish itself, with the composition spread over its threads.
TG_HD uint32_t scaled_pixel(const ScaledArgs& P, const Layer* lay, uint32_t live, int x, int y) {
  const uint32_t hit = pixel_items(P, lay, live, x, y);
  uint32_t c;
  if (P.fast && scaled_lookup(P, lay, live, hit, x, y, c)) return c;
  return scaled_compose(P.A, lay, hit, P.s, x, y);
}

// All 9 items of one env and the mask of those on the frame; returns the TG_ERR_RENDER bits
// (host check; the kernel makes one item per thread with the same make_layer and test).
TG_HD uint32_t make_layers(const RenderArgs& A, const uint4 st, const double2 ang, Layer* lay,
                           uint32_t& live) {
  uint32_t err = 0;
  live = 0;
  for (int i = 0; i < NLAYER; ++i) {
    bool on = false;
    err |= make_layer(A, i, st, ang, lay[i], on);
    if (on && lay[i].x1 > 0 && lay[i].x0 < A.Wpx && lay[i].y1 > 0 && lay[i].y0 < A.Hpx)
      live |= 1u << i;
  }
  return err;
}

// ---- host: pooling (first tg_render_scaled call per scale) -------------------------------
// XRGB image [rows][cols] -> [rows / s][cols / s], the rounded mean per channel.
inline std::vector<uint32_t> pool_xrgb(const uint32_t* px, size_t rows, size_t cols, int s) {
  const size_t h = rows / (size_t)s, w = cols / (size_t)s;
  std::vector<uint32_t> out(h * w);
  const uint32_t n = (uint32_t)(s * s);
  for (size_t y = 0; y < h; ++y)
    for (size_t x = 0; x < w; ++x) {
      uint32_t sr = 0, sg = 0, sb = 0;
      for (int dy = 0; dy < s; ++dy)
        for (int dx = 0; dx < s; ++dx) {
          const uint32_t c = px[(y * (size_t)s + (size_t)dy) * cols + x * (size_t)s + (size_t)dx];
          sr += (c >> 16) & 255u, sg += (c >> 8) & 255u, sb += c & 255u;
        }
      out[y * w + x] = (round_mean(sr, n) << 16) | (round_mean(sg, n) << 8) | round_mean(sb, n);
    }
  return out;
}

// bg_small from the static layer; tiles_small from cell_tiles' [cells * D_COUNT] stack of
// 48x48 tiles (s divides 48, so no box crosses a tile).
inline std::vector<uint32_t> pooled_static(const std::vector<uint32_t>& bg32, int W, int H, int s) {
  return pool_xrgb(bg32.data(), (size_t)H * RS, (size_t)W * RS, s);
}
inline std::vector<uint32_t> pooled_tiles(const std::vector<uint32_t>& bg32, int W, int H,
                                          const std::vector<uint32_t>& dyn, int s) {
  const std::vector<uint32_t> t = cell_tiles(bg32, W, H, dyn);
  return pool_xrgb(t.data(), t.size() / RS, RS, s);
}

}  // namespace tg
