// tg_render_view.h — the agent-centred window of the frame (tg_render_view of include/tg_amd.h):
// the window's origin from an env's state word, the mapping of a window pixel to a pixel of the
// full downscaled frame, and the per-pixel driver, shared by the gfx950 kernel (tg_render.hip
// k_render_view) and the host-only check build (tests/native_view).
//
// Definition (an extension: the reference has no such mode).  F = the env's full frame as
// tg_render writes it.  The hero's cell is the reference's get_player_cell (IM/:441-445) with
// floor division, xc = playerx // 48, yc = (playery + 24) // 48; for a radius r in 1..7 the
// window is the (2r+1) x (2r+1) cells with origin (ox, oy) = (xc - r, yc - r):
//   V[y][x][c] = F[48*oy + y][48*ox + x][c] inside F, 0 outside            (y, x < 48*(2r+1))
//   out        = tg_render_scaled's function of V (tg_render_scaled.h)
// The origin is cell-aligned and s divides 48, so every s x s box of V is one box of F or lies
// wholly outside it: out is the zero-padded crop at (cs*ox, cs*oy), cs = 48 / s, of side
// cs*(2r+1), of tg_render_scaled's frame (the gray of black is 0).  The hero's sprite at
// (playerx - 24, playery) lies inside the window for every r >= 1.
#pragma once
#include "tg_render_scaled.h"

// What the host check makes of a condition on an index this header forms (a failure flag); the
// kernel compiles it away.
#ifndef TG_VIEW_ASSERT
#define TG_VIEW_ASSERT(cond) ((void)0)
#endif

namespace tg {

constexpr int VIEW_RMAX = 7;  // radius 1..7: a window of at most 15 x 15 cells

struct ViewArgs {
  ScaledArgs P;  // the full frame's tables at this scale; P.fast is view_pixel's switch
  int r, n;      // radius; output pixels per side, cs * (2r + 1)
};

// k_render_view's division of the work (tg_render.hip): the frames of a group of G envs are one
// run of G * n * n output pixels, a workgroup takes a span of VSPAN of them and queues up to
// VQCAP boxes that scaled_lookup declines.  G is a multiple of 4 (a group starts on a dword
// whatever the frame size) and grows as the frame shrinks, so that a workgroup of small frames
// still has a span to fill: 12 envs of 18 x 18 pixels; at most VGMAX, whose Layers and the span's
// buffers keep the workgroup under 40 KB of LDS (four workgroups per CU).
constexpr int VSPAN = 4096;  // output pixels per workgroup
constexpr int VQCAP = 1024;  // queued boxes per workgroup
constexpr int VGMAX = 12;    // envs per group at most (each keeps its NLAYER Layers in LDS)
TG_HD int view_group(int frame_px) {
  const int g = (VSPAN / frame_px) & ~3;
  return g < 4 ? 4 : (g > VGMAX ? VGMAX : g);
}

// the window's origin in cells, through the st4 codec
TG_HD void view_origin(const uint4 st, int r, int& ox, int& oy) {
  Env e;
  unpack_st4(st, e);
  ox = floordiv(e.px, RS) - r;
  oy = floordiv(e.py + RS / 2, RS) - r;
}

// Window output pixel (vx, vy) -> output pixel (x, y) of the full frame at this scale; false
// where it lies outside the frame (the pixel is 0 and no table is read for it).  |ox|, |oy| <=
// 32768 / 48 + 8, so the products stay far inside an int.
TG_HD bool view_map(const ScaledArgs& P, int ox, int oy, int vx, int vy, int& x, int& y) {
  x = ox * P.cs + vx, y = oy * P.cs + vy;
  return x >= 0 && x < P.w && y >= 0 && y < P.h;
}

// the items of `live` (those on the frame) whose bounding boxes overlap the window
TG_HD bool view_overlaps(const Layer& l, int ox, int oy, int r) {
  const int n = RS * (2 * r + 1), X0 = RS * ox, Y0 = RS * oy;
  return X0 < l.x1 && X0 + n > l.x0 && Y0 < l.y1 && Y0 + n > l.y0;
}
TG_HD uint32_t view_items(const Layer* lay, uint32_t live, int ox, int oy, int r) {
  uint32_t in = 0;
  for (uint32_t m = live; m; m &= m - 1) {
    const int i = __builtin_ctz(m);
    if (view_overlaps(lay[i], ox, oy, r)) in |= 1u << i;
  }
  return in;
}

// One source row Y of a box that the hero alone touches, as scaled_compose_row sums it.  The hero
// is in every window, so most boxes scaled_lookup declines are these.  scaled_compose_row walks a
// row pixel after pixel, each one's sprite texel loaded after its static bytes have come back;
// here the N static pixels and N texels of a stretch of the row are loaded together (every
// address is valid whether or not the hero covers the pixel: a texel off the sprite is replaced
// by alpha 0, which blend_px leaves alone), then blended.  N divides s.
template <int N>
TG_HD void hero_stretch(const uint8_t* p, const uint32_t* sp, bool row, int u0, uint32_t& sr,
                        uint32_t& sg, uint32_t& sb) {
  uint32_t c[N], t[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool on = row && (unsigned)(u0 + j) < (unsigned)RS;
    c[j] = ((uint32_t)p[3 * j] << 16) | ((uint32_t)p[3 * j + 1] << 8) | p[3 * j + 2];
    t[j] = sp[on ? u0 + j : 0];
    t[j] = on ? t[j] : 0u;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const uint32_t v = blend_px(c[j], t[j]);
    sr += (v >> 16) & 255u, sg += (v >> 8) & 255u, sb += v & 255u;
  }
}
TG_HD uint64_t view_hero_row(const RenderArgs& A, const Layer& hero, int s, int x, int Y) {
  const uint8_t* p =
      reinterpret_cast<const uint8_t*>(A.bg) + ((size_t)Y * (size_t)A.Wpx + (size_t)(s * x)) * 3;
  const int v = Y - hero.oy, u0 = s * x - hero.ox;
  const bool row = (unsigned)v < (unsigned)RS;
  const uint32_t* sp = A.spr + hero.spr * RS2 + (row ? v : 0) * RS;
  uint32_t sr = 0, sg = 0, sb = 0;
  if (s % 8 == 0) {
    for (int d = 0; d < s; d += 8) hero_stretch<8>(p + 3 * d, sp, row, u0 + d, sr, sg, sb);
  } else if (s % 6 == 0) {
    for (int d = 0; d < s; d += 6) hero_stretch<6>(p + 3 * d, sp, row, u0 + d, sr, sg, sb);
  } else if (s == 4) {
    hero_stretch<4>(p, sp, row, u0, sr, sg, sb);
  } else if (s == 3) {
    hero_stretch<3>(p, sp, row, u0, sr, sg, sb);
  } else if (s == 2) {
    hero_stretch<2>(p, sp, row, u0, sr, sg, sb);
  } else {
    hero_stretch<1>(p, sp, row, u0, sr, sg, sb);
  }
  return (uint64_t)sr | ((uint64_t)sg << SUM_BITS) | ((uint64_t)sb << (2 * SUM_BITS));
}

// A box's source row and a whole box with the items `hit` over it: the hero's own path where
// it alone touches the box, else tg_render_scaled.h's general one.
TG_HD uint64_t view_compose_row(const RenderArgs& A, const Layer* lay, uint32_t hit, int s, int x,
                                int Y) {
  return hit == HERO_ITEM ? view_hero_row(A, lay[NLAYER - 1], s, x, Y)
                          : scaled_compose_row(A, lay, hit, s, x, Y);
}
TG_HD uint32_t view_compose(const RenderArgs& A, const Layer* lay, uint32_t hit, int s, int x, int y) {
  uint64_t sums = 0;
  for (int dy = 0; dy < s; ++dy) sums += view_compose_row(A, lay, hit, s, x, s * y + dy);
  return scaled_finish(sums, s);
}

// Window output pixel (vx, vy) of one env as XRGB: 0 outside the frame, else the pooled tables'
// pixel where scaled_lookup holds it, else the box composed (with P.fast == 0 every box is).
// `live` = view_items: an item outside the window touches none of its boxes, and an item on a
// cell of the window is in it, so scaled_lookup counts a cell's items as it does for the whole
// frame.  The host check's driver; k_render_view calls scaled_lookup, view_compose_row and
// scaled_finish itself, with the composition spread over its threads.
TG_HD uint32_t view_pixel(const ViewArgs& V, const Layer* lay, uint32_t live, int ox, int oy,
                          int vx, int vy) {
  int x, y;
  if (!view_map(V.P, ox, oy, vx, vy, x, y)) return 0u;
  // every table index below derives from (x, y): the pooled static layer's [y][x], the cell
  // (x / cs, y / cs) of the pooled tiles, rows s*y .. s*y + s - 1 of the static layer
  TG_VIEW_ASSERT((size_t)y * (size_t)V.P.w + (size_t)x < (size_t)V.P.h * (size_t)V.P.w);
  TG_VIEW_ASSERT(x / V.P.cs < V.P.A.W && y / V.P.cs < V.P.A.H);
  TG_VIEW_ASSERT(V.P.s * x + V.P.s <= V.P.A.Wpx && V.P.s * y + V.P.s <= V.P.A.Hpx);
  const uint32_t hit = pixel_items(V.P, lay, live, x, y);
  uint32_t c;
  if (V.P.fast && scaled_lookup(V.P, lay, live, hit, x, y, c)) return c;
  return view_compose(V.P.A, lay, hit, V.P.s, x, y);
}

}  // namespace tg
