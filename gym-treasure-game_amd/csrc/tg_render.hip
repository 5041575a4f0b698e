// tg_render.hip — TreasureGame.render('rgb_array') for a whole batch (tg_render_init /
// tg_render / tg_frame_shape of include/tg_amd.h), and the downscaled / grayscale form
// (tg_frame_shape_scaled / tg_render_scaled, k_render_scaled below).
//
// Reference: TG/:98-105 render() -> _TreasureGameDrawer.draw_domain (DR/:136-163) and
// draw_object (DR/:238-269); ObservationWrapper (TG/:38-51) renders after every reset/step.
// DR/ = _treasure_game_impl/_treasure_game_drawer.py.
//
// A frame is the env's screen as RGB bytes, [H*48][W*48][3] (surfarray.array3d().swapaxes(0,1)).
// It splits into
//   * a STATIC layer, identical for every env and every step: black, then one 48x48 sprite per
//     description cell — wall or floor (a wall under a non-wall) or background, each a
//     Random(12).choice over 5 variants in row-major cell order (draw_domain reseeds the
//     generator every frame, DR/:137), ladders fixed.  Built once on the host at
//     tg_render_init and kept in HBM (a few MB, L2-resident while the kernel streams);
//   * a DYNAMIC layer of <= 9 items drawn over it in the reference's order: the 8 objects in
//     file order (3 doors open/closed, 2 handles = 5-px shaft + r=4 knob + base sprite, key
//     and gold unless moved off-screen, bolt open/locked), then the hero (mirrored when facing
//     left).  They cover ~6 % of the pixels.
// k_render: one workgroup per (group of 4 envs, band of 48 pixel rows), one wave per row,
// one lane per 16-B chunk of the row's RGB bytes (coalesced, every byte of every frame written
// exactly once).  The lane loads its static chunk once and stores it into the 4 frames,
// except where a dynamic item touches the chunk: there it composites the chunk's 6 pixels in
// draw order and repacks.  The kernel is HBM-write bound: 1,257,984 B per frame of the
// default level; the static layer is read once per 4 frames (from L2 / Infinity Cache).
//
// The per-chunk composition and the static-layer construction live in tg_render.h (shared
// with the host-only check build); the pixel rules are listed there.  PARITY UNPINNED against
// the reference (pygame is absent here); pinned against the oracle's restatement.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "tg_batch.h"
#include "tg_level.h"
#include "tg_render.h"
#include "tg_render_scaled.h"
#include "tg_render_view.h"

namespace tg {

constexpr int RBLOCK = 256;  // 4 waves (1,024 threads lost 1.5-9 ms)

struct RenderState {
  DevBuf<uint4> bg;              // static layer, RGB bytes [Hpx][Wpx*3]
  DevBuf<uint4> tiles;           // static layer + each cell-aligned sprite, per cell
  DevBuf<uint32_t> spr;          // [D_COUNT][48*48] ARGB
  // tg_render_scaled: the host's static layer and sprites (pooled on a scale's first call)
  // and the per-scale device tables, by scale_index
  std::vector<uint32_t> bg32, dyn;
  DevBuf<uint32_t> bg_small[NSCALE];
  DevBuf<uint32_t> tiles_small[NSCALE];
};

void render_free(RenderState* rs) { delete rs; }

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// frame stores are non-temporal: streamed once, never re-read here (plain, sc1, sc0 sc1 and
// nt sc1 stores measured equal or up to 0.8 ms slower)
__device__ __forceinline__ void store16(uint4* p, const uint4 x) {
  u32x4 v = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
}

constexpr int RG = 4;  // envs per workgroup: each static-layer chunk is loaded once per RG frames
constexpr int MAX_W = 128;  // cell columns (levels are at most 120 wide, tg_level.h)

// block = (group of RG envs, band of 48 rows): lane l of wave w renders chunks 64w + l,
// 64(w + 4) + l, ... of the band, for each env of the group in turn: the static chunk is
// loaded once and stored RG times (composited where an item covers it).
__global__ __launch_bounds__(RBLOCK) void k_render(RenderArgs A, const uint4* __restrict__ st4,
                                                   const double2* __restrict__ angs,
                                                   int64_t first, int64_t count,
                                                   uint4* __restrict__ out) {
  __shared__ Layer lay[RG][NLAYER];
  __shared__ uint32_t live[RG];
  __shared__ uint16_t rows[RG][RS];  // items covering each row of the band, per env
  __shared__ uint16_t sel[RG][MAX_W];  // each cell's source, per env
  const int64_t grp = blockIdx.x / A.H;
  const int band = (int)(blockIdx.x - grp * A.H);
  const int ylo = band * RS;
  const int64_t e0 = grp * RG;
  const int ne = (int)(count - e0 < RG ? count - e0 : RG);
  if (threadIdx.x < RG) live[threadIdx.x] = 0u;
  __syncthreads();
  for (int t = threadIdx.x; t < RG * NLAYER; t += RBLOCK) {
    const int k = t / NLAYER, i = t - k * NLAYER;
    if (k < ne) {
      Layer l;
      bool on = false;
      const int64_t g = first + e0 + k;
      const uint32_t err = make_layer(A, i, st4[g], angs[g], l, on);
      if (err) atomicOr(A.err, err);
      if (on && l.y1 > ylo && l.y0 < ylo + RS && l.x1 > 0 && l.x0 < A.Wpx) {
        lay[k][i] = l;
        atomicOr(&live[k], 1u << i);
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < RG * RS; t += RBLOCK) {
    const int k = t / RS, r = t - k * RS;
    rows[k][r] = (uint16_t)(k < ne ? row_items(lay[k], live[k], ylo + r) : 0u);
  }
  if (threadIdx.x < RG && (int)threadIdx.x < ne)
    cell_sources(lay[threadIdx.x], live[threadIdx.x], band, A.W, sel[threadIdx.x]);
  __syncthreads();
  // The band is one contiguous, 128-B aligned run of 48 * CH chunks in every frame (a frame
  // row, 2,016 B, is not a whole number of 128-B lines): waves take 1-KB segments of it, so
  // every store instruction writes 8 whole lines; a segment may straddle two pixel rows.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t frame_chunks = (int64_t)A.Hpx * A.CH;
  const int band_chunks = RS * A.CH;
  uint4* const base = out + e0 * frame_chunks + (int64_t)ylo * A.CH;
  const uint4* const bgb = A.bg + (int64_t)ylo * A.CH;
  for (int c0 = wave * 64; c0 < band_chunks; c0 += RBLOCK) {
    const int c = c0 + lane;
    if (c >= band_chunks) break;
    const int rs = c0 / A.CH;                            // wave-uniform first row of the segment
    const int r = c - rs * A.CH >= A.CH ? rs + 1 : rs;  // this lane's row
    const int q = c - r * A.CH;
    const uint4 v = bgb[c];
    uint4* dst = base + c;
    for (int k = 0; k < ne; ++k, dst += frame_chunks) {
      const uint32_t rm = rows[k][r];
      store16(dst, rm ? render_chunk(A, lay[k], rm, sel[k], band, r, q, v) : v);
    }
  }
}

// ---- tg_render_scaled ----------------------------------------------------------------------
// The frames of a group of SG envs are one run of SG * h * w output pixels; a workgroup takes
// a span of SSPAN of them and builds it in LDS in three passes:
//   1. every pixel is classified (scaled_lookup): those a pooled table holds are copied, the
//      rest (under the hero, a shaft or knob, a two-item cell: a few dozen per env) are queued;
//   2. the queued boxes are composed at full resolution, one source row of a box per thread
//      (a box per lane would leave one lane walking s*s dependent loads while 63 wait), the
//      rows' channel sums added into the box's LDS word;
//   3. the span is stored, 4 pixels per thread (12 B of RGB or 4 B of gray) as whole dwords:
//      SG is a multiple of 4, so a group starts on a dword whatever the frame size.  Only a
//      short last group's tail is stored byte by byte, so nothing outside
//      [out, out + count * frame bytes) is written.
// SG (envs per group), SSPAN (output pixels per workgroup), SQCAP and span_pixel are
// tg_render_scaled.h's, shared with the host check's count of a span's declined boxes.
constexpr int SPX = 4;       // pixels per thread per store
// SQCAP: queued boxes per workgroup.  Past it a thread composes its own box inline
// (scaled_compose: the same rows, summed in the lane).  A span holds about 4096 * 48 / Wpx hero
// boxes plus as many again per handle, so only a level narrower than about 12 cells can get
// there: none of the shipped levels does.  tests/test_gpu_render_sweep.py reaches that branch on
// the 8-cell level tests/golden/levels/narrow at scales 1 and 2, where the host check counts
// more than SQCAP declined boxes in a span (hcs_span_queue_max); scaled_compose
// itself is also what the host check runs for every pixel with fast = 0.

__global__ __launch_bounds__(RBLOCK) void k_render_scaled(ScaledArgs P,
                                                          const uint4* __restrict__ st4,
                                                          const double2* __restrict__ angs,
                                                          int64_t first, int64_t count, int spans,
                                                          uint8_t* __restrict__ out) {
  __shared__ Layer lay[SG][NLAYER];
  __shared__ uint32_t live[SG];
  __shared__ uint32_t px[SSPAN];             // the span's pixels, XRGB
  __shared__ unsigned long long acc[SQCAP];  // a queued box's channel sums
  __shared__ uint16_t queue[SQCAP];          // its pixel within the span
  __shared__ uint32_t qn;
  const int tid = (int)threadIdx.x;
  const int64_t grp = blockIdx.x / spans;
  const int span = (int)(blockIdx.x - grp * spans);
  const int64_t e0 = grp * SG;
  const int ne = (int)(count - e0 < SG ? count - e0 : SG);
  const int fp = P.h * P.w;  // output pixels per frame
  const int gpx = ne * fp;   // and in this group
  const int pb = span * SSPAN;
  if (pb >= gpx) return;     // a short last group needs fewer spans (block-uniform)
  const int npx = gpx - pb < SSPAN ? gpx - pb : SSPAN;
  if (tid < SG) live[tid] = 0u;
  if (tid == 0) qn = 0u;
  for (int e = tid; e < SQCAP; e += RBLOCK) acc[e] = 0ull;
  __syncthreads();
  if (tid < SG * NLAYER) {
    const int k = tid / NLAYER, i = tid - k * NLAYER;
    if (k < ne) {
      Layer l;
      bool on = false;
      const int64_t g = first + e0 + k;
      const uint32_t err = make_layer(P.A, i, st4[g], angs[g], l, on);
      if (err) atomicOr(P.A.err, err);
      if (on && l.x1 > 0 && l.x0 < P.A.Wpx && l.y1 > 0 && l.y0 < P.A.Hpx) {
        lay[k][i] = l;
        atomicOr(&live[k], 1u << i);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < npx; i += RBLOCK) {
    int k, x, y;
    span_pixel(pb + i, fp, P.w, k, x, y);
    const uint32_t hit = pixel_items(P, lay[k], live[k], x, y);
    uint32_t c;
    if (!scaled_lookup(P, lay[k], live[k], hit, x, y, c)) {
      const uint32_t slot = atomicAdd(&qn, 1u);
      if (slot < (uint32_t)SQCAP) {
        queue[slot] = (uint16_t)i;
        continue;
      }
      c = scaled_compose(P.A, lay[k], hit, P.s, x, y);
    }
    px[i] = c;
  }
  __syncthreads();
  const int nq = (int)(qn < (uint32_t)SQCAP ? qn : (uint32_t)SQCAP);
  for (int wi = tid; wi < nq * P.s; wi += RBLOCK) {
    const int e = wi / P.s, dy = wi - e * P.s;
    int k, x, y;
    span_pixel(pb + queue[e], fp, P.w, k, x, y);
    const uint32_t hit = pixel_items(P, lay[k], live[k], x, y);
    atomicAdd(&acc[e], (unsigned long long)scaled_compose_row(P.A, lay[k], hit, P.s, x, P.s * y + dy));
  }
  __syncthreads();
  for (int e = tid; e < nq; e += RBLOCK) px[queue[e]] = scaled_finish(acc[e], P.s);
  __syncthreads();
  uint8_t* const gout = out + (e0 * (int64_t)fp + pb) * P.ch;
  for (int i0 = tid * SPX; i0 < npx; i0 += RBLOCK * SPX) {
    const int np = npx - i0 < SPX ? npx - i0 : SPX;
    uint32_t c[SPX];
#pragma unroll
    for (int j = 0; j < SPX; ++j) c[j] = j < np ? px[i0 + j] : 0u;
    if (P.ch == 3) {
      uint8_t* d = gout + (int64_t)i0 * 3;
      const uint32_t a0 = px3(c[0]), a1 = px3(c[1]), a2 = px3(c[2]), a3 = px3(c[3]);
      if (np == SPX) {
        uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
        d4[0] = a0 | (a1 << 24);
        d4[1] = (a1 >> 8) | (a2 << 16);
        d4[2] = (a2 >> 16) | (a3 << 8);
      } else {
        const uint32_t a[SPX] = {a0, a1, a2, a3};
        for (int j = 0; j < np; ++j)
          for (int b = 0; b < 3; ++b) d[3 * j + b] = (uint8_t)(a[j] >> (8 * b));
      }
    } else {
      uint8_t* d = gout + i0;
      const uint32_t g0 = luma_px(c[0]), g1 = luma_px(c[1]), g2 = luma_px(c[2]), g3 = luma_px(c[3]);
      if (np == SPX) {
        *reinterpret_cast<uint32_t*>(d) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
      } else {
        const uint32_t a[SPX] = {g0, g1, g2, g3};
        for (int j = 0; j < np; ++j) d[j] = (uint8_t)a[j];
      }
    }
  }
}

// ---- tg_render_view ------------------------------------------------------------------------
// The window of (2r+1) x (2r+1) cells around each env's hero (tg_render_view.h), n x n output
// pixels.  k_render_scaled's three passes over a span of VSPAN output pixels of a group's run
// of frames, with what a window changes:
//   * a window frame is 9 B to 1.5 MB, so the group is G = view_group(n * n) envs, a multiple
//     of 4: 12 frames of 18 x 18 fill one span, one frame of 720 x 720 takes 127 spans;
//   * a workgroup makes the Layers of the envs its span touches only (one env of the 4 at
//     r = 7, scale 1), yet every env's nine items pass make_layer in some workgroup, so
//     TG_ERR_RENDER is raised as tg_render_scaled raises it; the workgroup holding an env's
//     first pixel writes its origin;
//   * the items are culled against the window, not the frame: a handle outside it costs
//     nothing after its make_layer;
//   * a window pixel outside the frame is 0 and forms no table index (view_map);
//   * the hero is in every frame: at scale 8 it declines up to 49 of a window's 324 boxes,
//     where the full frame's 6,552 had the same 49.  The declined boxes are composed one
//     source row per thread over all 256 threads, as k_render_scaled's pass 2 is, so the
//     share that matters is divided evenly whatever lanes the hero's pixels fell on; and a
//     row of a box that the hero alone touches (most of them) takes view_hero_row, which
//     loads a stretch of the row's static pixels and sprite texels together where
//     scaled_compose_row waits for one pixel's loads before it asks for the next's.
// VSPAN, VQCAP, VGMAX and view_group are tg_render_view.h's.  Past VQCAP queued boxes (a span
// at scale 1 can hold 28 rows of the hero's 48 pixels) a thread composes its own box inline.
__device__ __forceinline__ void store_px4(const uint32_t* px, int np, int ch, uint8_t* d) {
  uint32_t c[SPX];
#pragma unroll
  for (int j = 0; j < SPX; ++j) c[j] = j < np ? px[j] : 0u;
  if (ch == 3) {
    const uint32_t a0 = px3(c[0]), a1 = px3(c[1]), a2 = px3(c[2]), a3 = px3(c[3]);
    if (np == SPX) {
      uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
      d4[0] = a0 | (a1 << 24);
      d4[1] = (a1 >> 8) | (a2 << 16);
      d4[2] = (a2 >> 16) | (a3 << 8);
    } else {
      const uint32_t a[SPX] = {a0, a1, a2, a3};
      for (int j = 0; j < np; ++j)
        for (int b = 0; b < 3; ++b) d[3 * j + b] = (uint8_t)(a[j] >> (8 * b));
    }
  } else {
    const uint32_t g0 = luma_px(c[0]), g1 = luma_px(c[1]), g2 = luma_px(c[2]), g3 = luma_px(c[3]);
    if (np == SPX) {
      *reinterpret_cast<uint32_t*>(d) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    } else {
      const uint32_t a[SPX] = {g0, g1, g2, g3};
      for (int j = 0; j < np; ++j) d[j] = (uint8_t)a[j];
    }
  }
}

__global__ __launch_bounds__(RBLOCK) void k_render_view(ViewArgs V, const uint4* __restrict__ st4,
                                                        const double2* __restrict__ angs,
                                                        int64_t first, int64_t count, int G,
                                                        int spans, uint8_t* __restrict__ out,
                                                        int32_t* __restrict__ origin) {
  __shared__ Layer lay[VGMAX][NLAYER];
  __shared__ uint32_t live[VGMAX];
  __shared__ int org[VGMAX][2];              // each env's window origin in cells
  __shared__ uint32_t px[VSPAN];             // the span's pixels, XRGB
  __shared__ unsigned long long acc[VQCAP];  // a queued box's channel sums
  __shared__ uint16_t queue[VQCAP];          // its pixel within the span
  __shared__ uint32_t qn;
  const ScaledArgs& P = V.P;
  const int tid = (int)threadIdx.x;
  const int64_t grp = blockIdx.x / spans;
  const int span = (int)(blockIdx.x - grp * spans);
  const int64_t e0 = grp * G;
  const int ne = (int)(count - e0 < G ? count - e0 : G);
  const int fp = V.n * V.n;  // output pixels per frame
  const int gpx = ne * fp;   // and in this group
  const int pb = span * VSPAN;
  if (pb >= gpx) return;     // a short last group needs fewer spans (block-uniform)
  const int npx = gpx - pb < VSPAN ? gpx - pb : VSPAN;
  const int k0 = pb / fp, nk = (pb + npx - 1) / fp - k0 + 1;  // the envs this span touches
  if (tid < VGMAX) live[tid] = 0u;
  if (tid == 0) qn = 0u;
  for (int e = tid; e < VQCAP; e += RBLOCK) acc[e] = 0ull;
  __syncthreads();
  if (tid < nk * NLAYER) {
    const int k = k0 + tid / NLAYER, i = tid % NLAYER;
    const int64_t g = first + e0 + k;
    const uint4 st = st4[g];
    int ox, oy;
    view_origin(st, V.r, ox, oy);
    Layer l;
    bool on = false;
    const uint32_t err = make_layer(P.A, i, st, angs[g], l, on);
    if (err) atomicOr(P.A.err, err);
    if (on && l.x1 > 0 && l.x0 < P.A.Wpx && l.y1 > 0 && l.y0 < P.A.Hpx &&
        view_overlaps(l, ox, oy, V.r)) {
      lay[k][i] = l;
      atomicOr(&live[k], 1u << i);
    }
    if (i == NLAYER - 1) {
      org[k][0] = ox, org[k][1] = oy;
      if (origin && k * fp >= pb) origin[2 * (e0 + k)] = ox, origin[2 * (e0 + k) + 1] = oy;
    }
  }
  __syncthreads();
  for (int i = tid; i < npx; i += RBLOCK) {
    int k, vx, vy, x, y;
    span_pixel(pb + i, fp, V.n, k, vx, vy);
    uint32_t c = 0u;
    if (view_map(P, org[k][0], org[k][1], vx, vy, x, y)) {
      const uint32_t hit = pixel_items(P, lay[k], live[k], x, y);
      if (!scaled_lookup(P, lay[k], live[k], hit, x, y, c)) {
        const uint32_t slot = atomicAdd(&qn, 1u);
        if (slot < (uint32_t)VQCAP) {
          queue[slot] = (uint16_t)i;
          continue;
        }
        c = view_compose(P.A, lay[k], hit, P.s, x, y);
      }
    }
    px[i] = c;
  }
  __syncthreads();
  const int nq = (int)(qn < (uint32_t)VQCAP ? qn : (uint32_t)VQCAP);
  for (int wi = tid; wi < nq * P.s; wi += RBLOCK) {
    const int e = wi / P.s, dy = wi - e * P.s;
    int k, vx, vy, x, y;
    span_pixel(pb + queue[e], fp, V.n, k, vx, vy);
    view_map(P, org[k][0], org[k][1], vx, vy, x, y);  // queued: inside the frame
    const uint32_t hit = pixel_items(P, lay[k], live[k], x, y);
    atomicAdd(&acc[e], (unsigned long long)view_compose_row(P.A, lay[k], hit, P.s, x, P.s * y + dy));
  }
  __syncthreads();
  for (int e = tid; e < nq; e += RBLOCK) px[queue[e]] = scaled_finish(acc[e], P.s);
  __syncthreads();
  uint8_t* const gout = out + (e0 * (int64_t)fp + pb) * P.ch;
  for (int i0 = tid * SPX; i0 < npx; i0 += RBLOCK * SPX)
    store_px4(px + i0, npx - i0 < SPX ? npx - i0 : SPX, P.ch, gout + (int64_t)i0 * P.ch);
}

}  // namespace
}  // namespace tg

using namespace tg;

// the kernels' view of the renderer's tables and the level's object cells
static RenderArgs render_args(const tg_batch* h) {
  const RenderState& rs = *h->rs;
  RenderArgs A;
  render_level(h->L, A);
  A.bg = rs.bg.get(), A.tiles = rs.tiles.get(), A.spr = rs.spr.get(), A.err = h->err.get();
  return A;
}
// `who`'s envs [first, first + count) of the handle into `out`
static int check_frames(const tg_batch* h, const char* who, int64_t first, int64_t count,
                        const uint8_t* out) {
  if (first < 0 || count < 0 || first + count > h->n || (count && !out))
    return fail(TG_E_INVAL, "%s: envs [%lld, %lld) outside [0, %lld)", who, (long long)first,
                (long long)(first + count), (long long)h->n);
  if (((uintptr_t)out & 15u) != 0) return fail(TG_E_INVAL, "%s: the output must be 16-B aligned", who);
  return TG_OK;
}

// The scaled kernels' arguments at `scale` (scale_index si).  A scale's first call, from
// tg_render_scaled or tg_render_view, pools the static layer and the cell tiles on the host and
// uploads them (it synchronises); later calls read the cache.
static int scaled_args(tg_batch* h, int si, int32_t scale, int32_t channels, ScaledArgs& P) {
  RenderState* rs = h->rs.get();
  const int W = h->L.W, H = h->L.H;
  if (!rs->bg_small[si]) {
    const std::vector<uint32_t> b = pooled_static(rs->bg32, W, H, scale);
    const std::vector<uint32_t> t = pooled_tiles(rs->bg32, W, H, rs->dyn, scale);
    DevBuf<uint32_t> db, dt;  // installed once both are uploaded
    TG_TRY(db.upload(b.data(), b.size(), "a scale's static layer"));
    TG_TRY(dt.upload(t.data(), t.size(), "a scale's cell tiles"));
    rs->bg_small[si] = std::move(db), rs->tiles_small[si] = std::move(dt);
  }
  P.A = render_args(h);
  P.bg_small = rs->bg_small[si].get(), P.tiles_small = rs->tiles_small[si].get();
  P.s = scale, P.cs = RS / scale, P.w = P.A.Wpx / scale, P.h = P.A.Hpx / scale;
  P.ch = channels, P.fast = 1;  // fast: scaled_pixel's switch (host check); the kernels have none
  return TG_OK;
}

extern "C" {

int tg_render_init(tg_batch* h, const uint8_t* sprites, int32_t sw, int32_t sh) {
  BIND(h);
  if (!sprites || sw <= 0 || sh <= 0 || sw > 4096 || sh > 4096)
    return fail(TG_E_INVAL, "tg_render_init: bad sprite sheet");
  // description cells (get_file_description, IM/:180-202)
  std::vector<std::string> desc;
  for (auto& l : lines_of(h->domain.c_str())) desc.push_back(strip(l));
  while (!desc.empty() && desc.back().empty()) desc.pop_back();
  const int W = h->L.W, H = h->L.H, Wpx = W * RS, Hpx = H * RS;
  if ((int)desc.size() != H) return fail(TG_E_INVAL, "tg_render_init: level text mismatch");
  // handle shafts + knobs must stay on the surface: x - 5 .. x + 53, y + 8 .. y + 50 (angles
  // in [0, 1]: end point within 26 px across and 12..36 px above the pivot (x + 24, y + 48))
  for (int k = 0; k < 2; ++k) {
    const int x = h->L.handle_cx[k] * RS, y = h->L.handle_cy[k] * RS;
    if (x - 6 < 0 || x + 55 > Wpx || y + 52 > Hpx)
      return fail(TG_E_INVAL, "tg_render_init: handle %d's shaft would leave the screen", k);
  }
  const std::vector<uint32_t> sc = scale_sprites(sprites, sw, sh);
  const std::vector<uint32_t> bg32 = static_layer(desc, W, H, sc);
  const std::vector<uint8_t> rgb = rgb_bytes(bg32);
  const std::vector<uint32_t> dyn = dynamic_sprites(sc);
  const std::vector<uint8_t> tiles = rgb_bytes(cell_tiles(bg32, W, H, dyn));
  std::unique_ptr<RenderState, RenderDelete> rs(new RenderState());
  rs->bg32 = bg32, rs->dyn = dyn;  // kept for tg_render_scaled's pooling
  // (whole 16-B chunks: a row is W * 144 bytes)
  TG_TRY(rs->bg.upload(rgb.data(), rgb.size() / 16, "the renderer's static layer"));
  TG_TRY(rs->tiles.upload(tiles.data(), tiles.size() / 16, "the renderer's cell tiles"));
  TG_TRY(rs->spr.upload(dyn.data(), dyn.size(), "the renderer's sprites"));
  h->rs = std::move(rs);  // (in place of an earlier one)
  return TG_OK;
}

int tg_frame_shape(const tg_batch* h, int32_t* height, int32_t* width) {
  if (!h) return fail(TG_E_INVAL, "null handle");
  if (height) *height = h->L.H * RS;
  if (width) *width = h->L.W * RS;
  return TG_OK;
}

int tg_render(tg_batch* h, int64_t first, int64_t count, uint8_t* rgb, void* stream) {
  BIND(h);
  if (!h->rs) return fail(TG_E_STATE, "tg_render: call tg_render_init first");
  TG_TRY(check_frames(h, "tg_render", first, count, rgb));
  if (!count) return TG_OK;
  const RenderArgs A = render_args(h);
  const int64_t blocks = (count + RG - 1) / RG * h->L.H;
  if (blocks > 0x7FFFFFFF) return fail(TG_E_INVAL, "tg_render: too many envs in one call");
  hipLaunchKernelGGL(k_render, dim3((unsigned)blocks), dim3(RBLOCK), 0, (hipStream_t)stream, A,
                     h->S.st4, h->S.ang, first, count, reinterpret_cast<uint4*>(rgb));
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

static int scaled_dims(const tg_batch* h, int32_t scale, int* si) {
  if (!h) return fail(TG_E_INVAL, "null handle");
  *si = scale_index(scale);
  if (*si < 0) return fail(TG_E_INVAL, "scale %d is not a divisor of 48", (int)scale);
  return TG_OK;
}

int tg_frame_shape_scaled(const tg_batch* h, int32_t scale, int32_t* height, int32_t* width) {
  int si;
  TG_TRY(scaled_dims(h, scale, &si));
  if (height) *height = h->L.H * RS / scale;
  if (width) *width = h->L.W * RS / scale;
  return TG_OK;
}

int tg_render_scaled(tg_batch* h, int64_t first, int64_t count, int32_t scale, int32_t channels,
                     uint8_t* out, void* stream) {
  BIND(h);
  if (!h->rs) return fail(TG_E_STATE, "tg_render_scaled: call tg_render_init first");
  int si;
  TG_TRY(scaled_dims(h, scale, &si));
  if (channels != TG_FRAME_RGB && channels != TG_FRAME_GRAY)
    return fail(TG_E_INVAL, "tg_render_scaled: channels must be TG_FRAME_RGB or TG_FRAME_GRAY");
  TG_TRY(check_frames(h, "tg_render_scaled", first, count, out));
  if (!count) return TG_OK;
  ScaledArgs P;
  TG_TRY(scaled_args(h, si, scale, channels, P));
  const int64_t group_px = (int64_t)SG * P.h * P.w;
  if (group_px > 0x7FFFFFFF - SSPAN)
    return fail(TG_E_INVAL, "tg_render_scaled: frame too large at this scale");
  const int spans = (int)((group_px + SSPAN - 1) / SSPAN);
  const int64_t blocks = (count + SG - 1) / SG * spans;
  if (blocks > 0x7FFFFFFF) return fail(TG_E_INVAL, "tg_render_scaled: too many envs in one call");
  hipLaunchKernelGGL(k_render_scaled, dim3((unsigned)blocks), dim3(RBLOCK), 0, (hipStream_t)stream,
                     P, h->S.st4, h->S.ang, first, count, spans, out);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

static int view_dims(const tg_batch* h, int32_t radius, int32_t scale, int* si) {
  TG_TRY(scaled_dims(h, scale, si));
  if (radius < 1 || radius > VIEW_RMAX)
    return fail(TG_E_INVAL, "radius %d is outside 1..%d", (int)radius, VIEW_RMAX);
  return TG_OK;
}

int tg_frame_shape_view(const tg_batch* h, int32_t radius, int32_t scale, int32_t* height,
                        int32_t* width) {
  int si;
  TG_TRY(view_dims(h, radius, scale, &si));
  if (height) *height = RS * (2 * radius + 1) / scale;
  if (width) *width = RS * (2 * radius + 1) / scale;
  return TG_OK;
}

int tg_render_view(tg_batch* h, int64_t first, int64_t count, int32_t radius, int32_t scale,
                   int32_t channels, uint8_t* out, int32_t* origin, void* stream) {
  BIND(h);
  if (!h->rs) return fail(TG_E_STATE, "tg_render_view: call tg_render_init first");
  int si;
  TG_TRY(view_dims(h, radius, scale, &si));
  if (channels != TG_FRAME_RGB && channels != TG_FRAME_GRAY)
    return fail(TG_E_INVAL, "tg_render_view: channels must be TG_FRAME_RGB or TG_FRAME_GRAY");
  TG_TRY(check_frames(h, "tg_render_view", first, count, out));
  if (!count) return TG_OK;
  ViewArgs V;
  TG_TRY(scaled_args(h, si, scale, channels, V.P));
  V.r = radius, V.n = V.P.cs * (2 * radius + 1);
  const int fp = V.n * V.n;  // at most 720 * 720
  const int G = view_group(fp);
  const int spans = (int)(((int64_t)G * fp + VSPAN - 1) / VSPAN);
  const int64_t blocks = (count + G - 1) / G * spans;
  if (blocks > 0x7FFFFFFF) return fail(TG_E_INVAL, "tg_render_view: too many envs in one call");
  hipLaunchKernelGGL(k_render_view, dim3((unsigned)blocks), dim3(RBLOCK), 0, (hipStream_t)stream, V,
                     h->S.st4, h->S.ang, first, count, G, spans, out, origin);
  HIP_TRY(hipGetLastError());
  return TG_OK;
}

}  // extern "C"
