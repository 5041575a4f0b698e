// tg_hostcheck_scaled.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the downscaled renderer's per-output-pixel functions
// (gym-treasure-game_amd/csrc/tg_render_scaled.h): the classification and table lookups
// (scaled_lookup), the full-resolution composition of a box row by row (scaled_compose_row,
// scaled_finish) and the host pooling, checked against the pooled oracle frames on a machine
// without a GPU.  It drives them through scaled_pixel, one pixel after the other.  What
// k_render_scaled adds around the same functions — the span-to-pixel mapping, the LDS queue
// of boxes, the rows' sums added into LDS words, the packed stores — runs only on the GPU and
// is covered by tests/test_gpu_render_scaled.py.  The env states are reached as
// tests/native/tg_hostcheck.cpp's hc_render_run reaches them.  The product library never
// contains or calls this.  Built by tests/native_scaled/Makefile with hipcc --offload-host-only.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../gym-treasure-game_amd/csrc/tg_core.h"
#include "../../gym-treasure-game_amd/csrc/tg_level.h"
#include "../../gym-treasure-game_amd/csrc/tg_render_scaled.h"

using namespace tg;

namespace {
uint64_t sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
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
  Level Lv;
  std::vector<uint8_t> grid;
  std::string perr;
  if (!dom) dom = kDefaultDomain, objs = kDefaultObjects, inter = kDefaultInteractions;
  if (parse_level(dom, objs, inter, Lv, grid, perr) != 0) return -1;
  const std::vector<uint32_t> tab = build_gotab(Lv, grid);
  Lv.gotab = tab.data();
  const std::vector<uint32_t> mk = build_masks(Lv, grid);
  Lv.masks = mk.empty() ? nullptr : mk.data();
  const std::vector<double> oq = build_obs_q(Lv);
  Lv.obs_q = oq.data();
  const Level* L = &Lv;
  std::vector<std::string> desc;
  for (auto& l : lines_of(dom)) desc.push_back(strip(l));
  while (!desc.empty() && desc.back().empty()) desc.pop_back();
  const std::vector<uint32_t> sc = scale_sprites(sprites, sw, sh);
  const std::vector<uint32_t> bg32 = static_layer(desc, L->W, L->H, sc);
  const std::vector<uint8_t> bg = rgb_bytes(bg32);
  const std::vector<uint32_t> dyn = dynamic_sprites(sc);
  const std::vector<uint32_t> bgs = pooled_static(bg32, L->W, L->H, scale);
  const std::vector<uint32_t> tls =  // the general path reads no pooled table
      fast ? pooled_tiles(bg32, L->W, L->H, dyn, scale) : std::vector<uint32_t>();
  uint32_t err = 0;
  ScaledArgs P;
  RenderArgs& A = P.A;
  A.bg = reinterpret_cast<const uint4*>(bg.data());
  A.tiles = nullptr;  // the full-size tiles are not read by the scaled paths
  A.spr = dyn.data();
  A.err = &err;
  render_level(*L, A);
  P.bg_small = bgs.data(), P.tiles_small = tls.data();
  P.s = scale, P.cs = RS / scale, P.w = A.Wpx / scale, P.h = A.Hpx / scale;
  P.ch = channels, P.fast = fast;
  uint32_t gen[MT_N];
  genrand_prefix(gen);
  const Map m{grid.data(), L->W, L->H};
  const uint32_t* trig = &L->trig[0][0];
  std::vector<uint32_t> mt(MT_WORDS);
  const size_t fb = (size_t)P.h * P.w * channels;
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t g = (uint64_t)envs[i];
    init_mt(mt.data(), gen, seed_base + g);
    Env e{};
    for (int r = 0; r < 2; ++r) {  // construct + reset
      Rng rng(mt.data(), e.mti);
      reset_env(*L, e, rng);
      e.mti = refill_after(mt.data(), rng.finish());
    }
    for (int t = 0; t < steps; ++t) {
      const uint64_t hh = sm64(sm64(a0 ^ sm64(g)) ^ (uint64_t)t);
      int a = (int)(hh % 9ull);
      if (policy == 1) {
        const uint32_t amk = available_mask(*L, m, e);
        const int c = __builtin_popcount(amk);
        if (c) {
          uint32_t k = (uint32_t)(hh % (uint64_t)c), mm = amk;
          while (k--) mm &= mm - 1u;
          a = __builtin_ctz(mm);
        }
      }
      e.mti = refill_after(mt.data(), e.mti);
      Rng rng(mt.data(), e.mti);
      const StepResult r = env_step(*L, trig, m, e, a, rng);
      if (autoreset && r.done) reset_env(*L, e, rng);
      e.mti = rng.finish();
    }
    const uint4 st = pack(e);  // the SoA state words the kernel reads
    double2 an;
    an.x = e.ang0, an.y = e.ang1;
    if (states) states[4 * i] = st.x, states[4 * i + 1] = st.y, states[4 * i + 2] = st.z, states[4 * i + 3] = 0u;
    if (angs) angs[2 * i] = an.x, angs[2 * i + 1] = an.y;
    Layer lay[NLAYER];
    uint32_t live = 0;
    err |= make_layers(A, st, an, lay, live);
    uint8_t* o = out + (size_t)i * fb;
    for (int y = 0; y < P.h; ++y)
      for (int x = 0; x < P.w; ++x) {
        const uint32_t c = scaled_pixel(P, lay, live, x, y);
        if (channels == 3) {
          *o++ = (uint8_t)(c >> 16), *o++ = (uint8_t)(c >> 8), *o++ = (uint8_t)c;
        } else {
          *o++ = (uint8_t)luma_px(c);
        }
      }
  }
  return (int)err;
}

// the flag word's facing bit and first object bit (tg_core.h)
void hcs_flag_bits(uint32_t* facing, int* obj) { *facing = F_FACING, *obj = F_OBJ; }

}  // extern "C"
