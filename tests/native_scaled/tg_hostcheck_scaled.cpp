// tg_hostcheck_scaled.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the downscaled renderer's per-output-pixel functions
// (gym-treasure-game_amd/csrc/tg_render_scaled.h): the classification and table lookups
// (scaled_lookup), the full-resolution composition of a box row by row (scaled_compose_row,
// scaled_finish) and the host pooling, checked against the pooled oracle frames on a machine
// without a GPU.  It drives them through scaled_pixel, one pixel after the other.  What
// k_render_scaled adds around the same functions — the span-to-pixel mapping, the LDS queue
// of boxes, the rows' sums added into LDS words, the packed stores — runs only on the GPU and
// is covered by tests/test_gpu_render_scaled.py and tests/test_gpu_render_sweep.py;
// hcs_span_queue_max counts, with the kernel's span arithmetic, how full that queue gets.  The
// env states are given (hcs_render_states) or reached as tests/native/tg_hostcheck.cpp's
// hc_render_run reaches them (tests/native/host_env.h).  The product library never contains or
// calls this.  Built by tests/native_scaled/Makefile with hipcc --offload-host-only.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../gym-treasure-game_amd/csrc/tg_render_scaled.h"
#include "../native/host_env.h"

using namespace tg;

namespace {
// The scaled renderer's tables for one level, sprite sheet and scale, built by the product's
// host code, and one frame made from an env's state words pixel by pixel (scaled_pixel).  The
// one copy of that loop: hcs_render_run and hcs_render_states differ only in how they reach the
// state words.
struct HostScaled {
  std::vector<uint8_t> bg;
  std::vector<uint32_t> dyn, bgs, tls;
  ScaledArgs P;
  HostScaled(const HostLevel& hl, const uint8_t* sprites, int sw, int sh, int scale, int channels,
             int fast) {
    const Level& L = hl.L;
    std::vector<std::string> desc;
    for (auto& l : lines_of(hl.dom)) desc.push_back(strip(l));
    while (!desc.empty() && desc.back().empty()) desc.pop_back();
    const std::vector<uint32_t> sc = scale_sprites(sprites, sw, sh);
    const std::vector<uint32_t> bg32 = static_layer(desc, L.W, L.H, sc);
    bg = rgb_bytes(bg32);
    dyn = dynamic_sprites(sc);
    bgs = pooled_static(bg32, L.W, L.H, scale);
    if (fast) tls = pooled_tiles(bg32, L.W, L.H, dyn, scale);  // the general path reads no pooled table
    RenderArgs& A = P.A;
    A.bg = reinterpret_cast<const uint4*>(bg.data());
    A.tiles = nullptr;  // the full-size tiles are not read by the scaled paths
    A.spr = dyn.data();
    A.err = nullptr;  // the error bits are frame()'s return value
    render_level(L, A);
    P.bg_small = bgs.data(), P.tiles_small = tls.data();
    P.s = scale, P.cs = RS / scale, P.w = A.Wpx / scale, P.h = A.Hpx / scale;
    P.ch = channels, P.fast = fast;
  }
  HostScaled(const HostScaled&) = delete;
  HostScaled& operator=(const HostScaled&) = delete;
  size_t frame_bytes() const { return (size_t)P.h * P.w * P.ch; }
  // o [h][w][channels]; returns the TG_ERR_RENDER bits
  uint32_t frame(const uint4 st, const double2 an, uint8_t* o) const {
    Layer lay[NLAYER];
    uint32_t live = 0;
    const uint32_t err = make_layers(P.A, st, an, lay, live);
    for (int y = 0; y < P.h; ++y)
      for (int x = 0; x < P.w; ++x) {
        const uint32_t c = scaled_pixel(P, lay, live, x, y);
        if (P.ch == 3) {
          *o++ = (uint8_t)(c >> 16), *o++ = (uint8_t)(c >> 8), *o++ = (uint8_t)c;
        } else {
          *o++ = (uint8_t)luma_px(c);
        }
      }
    return err;
  }
};

// state words and angles of case i of case-major checkpoint arrays, through the product's codec
void case_words(const int32_t* pos, const uint32_t* flags, const int32_t* cells, const double* ang,
                int64_t i, uint4& st, double2& an) {
  Env t{};
  t.px = pos[2 * i], t.py = pos[2 * i + 1];
  t.f = flags[i];
  t.kx = cells[4 * i], t.ky = cells[4 * i + 1], t.gx = cells[4 * i + 2], t.gy = cells[4 * i + 3];
  st = pack(t);
  an.x = ang[2 * i], an.y = ang[2 * i + 1];
}

template <class Work>
void on_threads(int64_t n, int threads, const Work& work) {
  if (threads < 1) threads = 1;
  if (threads > 16) threads = 16;
  std::vector<std::thread> pool;
  const int64_t share = (n + threads - 1) / threads;
  for (int w = 0; w < threads; ++w) {
    const int64_t lo = w * share, hi = lo + share < n ? lo + share : n;
    if (lo < hi) pool.emplace_back(work, w, lo, hi);
  }
  for (auto& th : pool) th.join();
}
}  // namespace

extern "C" {

// Frames of envs g = seed_base + envs[i] after `steps` steps of the hc_run action stream at
// `scale` with `channels` (3 or 1): out [n][H*48/scale][W*48/scale][channels].  fast = 1 takes
// scaled_pixel's three paths as the kernel does, fast = 0 composes every pixel by the general
// path.  states (optional) [n][4]: each env's state words as the kernel reads them (position,
// flags, key / gold cells, 0) and angs (optional) [n][2] its handle angles, so a test can say
// which item states its frames cover.  Returns the OR of the TG_ERR_RENDER bits, -1 for a bad
// level, -2 for a bad scale or channel count.
int hcs_render_run(const char* dom, const char* objs, const char* inter, uint64_t seed_base,
                   const int64_t* envs, int64_t n, int steps, uint64_t a0, int policy,
                   int autoreset, const uint8_t* sprites, int sw, int sh, int scale, int channels,
                   int fast, uint8_t* out, uint32_t* states, double* angs) {
  if (scale_index(scale) < 0 || (channels != 3 && channels != 1)) return -2;
  HostLevel hl;
  if (!hl.load(dom, objs, inter)) return -1;
  const HostScaled hs(hl, sprites, sw, sh, scale, channels, fast);
  uint32_t err = 0;
  HostReplay env(hl, false);
  for (int64_t i = 0; i < n; ++i) {
    env.start(seed_base + (uint64_t)envs[i]);
    for (int t = 0; t < steps; ++t) env.step(a0, policy, autoreset != 0, envs[i], t);
    const Env& e = env.e;
    const uint4 st = pack(e);  // the SoA state words the kernel reads
    double2 an;
    an.x = e.ang0, an.y = e.ang1;
    if (states) states[4 * i] = st.x, states[4 * i + 1] = st.y, states[4 * i + 2] = st.z, states[4 * i + 3] = 0u;
    if (angs) angs[2 * i] = an.x, angs[2 * i + 1] = an.y;
    err |= hs.frame(st, an, out + (size_t)i * hs.frame_bytes());
  }
  return (int)err;
}

// The same frames of n given states (the checkpoint format, case-major arrays: pos [n][2],
// flags [n], cells [n][4], ang [n][2]) on `threads` workers.  Returns as hcs_render_run.
int hcs_render_states(const char* dom, const char* objs, const char* inter, int64_t n,
                      const int32_t* pos, const uint32_t* flags, const int32_t* cells,
                      const double* ang, const uint8_t* sprites, int sw, int sh, int scale,
                      int channels, int fast, uint8_t* out, int threads) {
  if (scale_index(scale) < 0 || (channels != 3 && channels != 1)) return -2;
  HostLevel hl;
  if (!hl.load(dom, objs, inter)) return -1;
  const HostScaled hs(hl, sprites, sw, sh, scale, channels, fast);
  std::vector<uint32_t> errs(16, 0u);
  on_threads(n, threads, [&](int w, int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      uint4 st;
      double2 an;
      case_words(pos, flags, cells, ang, i, st, an);
      errs[(size_t)w] |= hs.frame(st, an, out + (size_t)i * hs.frame_bytes());
    }
  });
  uint32_t err = 0;
  for (uint32_t e : errs) err |= e;
  return (int)err;
}

// How full k_render_scaled's queue gets on n given states rendered in one call at `scale`: the
// maximum over (group of SG envs, span of SSPAN output pixels) of the pixels scaled_lookup
// declines, with the kernel's own span arithmetic (SG, SSPAN, span_pixel of tg_render_scaled.h).
// A count above SQCAP (*sqcap, optional) means the kernel composes the excess inline.  Returns
// the maximum, -1 for a bad level, -2 for a bad scale.  No sprite sheet: the count is geometry.
int64_t hcs_span_queue_max(const char* dom, const char* objs, const char* inter, int64_t n,
                           const int32_t* pos, const uint32_t* flags, const int32_t* cells,
                           const double* ang, int scale, int* sqcap) {
  if (sqcap) *sqcap = SQCAP;
  if (scale_index(scale) < 0) return -2;
  HostLevel hl;
  if (!hl.load(dom, objs, inter)) return -1;
  ScaledArgs P;
  P.A.bg = nullptr, P.A.tiles = nullptr, P.A.spr = nullptr, P.A.err = nullptr;
  render_level(hl.L, P.A);
  P.s = scale, P.cs = RS / scale, P.w = P.A.Wpx / scale, P.h = P.A.Hpx / scale;
  P.ch = 3, P.fast = 1;
  // scaled_lookup reads a table where it accepts a pixel: blank ones of the real sizes
  const std::vector<uint32_t> bgs((size_t)P.h * P.w, 0u),
      tls((size_t)hl.L.W * hl.L.H * D_COUNT * P.cs * P.cs, 0u);
  P.bg_small = bgs.data(), P.tiles_small = tls.data();
  const int fp = P.h * P.w;
  int64_t worst = 0;
  for (int64_t e0 = 0; e0 < n; e0 += SG) {
    const int ne = (int)(n - e0 < SG ? n - e0 : SG);
    Layer lay[SG][NLAYER];
    uint32_t live[SG];
    for (int k = 0; k < ne; ++k) {
      uint4 st;
      double2 an;
      case_words(pos, flags, cells, ang, e0 + k, st, an);
      make_layers(P.A, st, an, lay[k], live[k]);
    }
    const int gpx = ne * fp;
    for (int pb = 0; pb < gpx; pb += SSPAN) {
      const int npx = gpx - pb < SSPAN ? gpx - pb : SSPAN;
      int64_t declined = 0;
      for (int i = 0; i < npx; ++i) {
        int k, x, y;
        span_pixel(pb + i, fp, P.w, k, x, y);
        uint32_t c;
        declined += !scaled_lookup(P, lay[k], live[k], pixel_items(P, lay[k], live[k], x, y), x, y, c);
      }
      if (declined > worst) worst = declined;
    }
  }
  return worst;
}

// the flag word's facing bit and first object bit (tg_state.h)
void hcs_flag_bits(uint32_t* facing, int* obj) { *facing = F_FACING, *obj = F_OBJ; }

}  // extern "C"
