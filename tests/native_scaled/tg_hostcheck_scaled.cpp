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
// tests/native/tg_hostcheck.cpp's hc_render_run reaches them (tests/native/host_env.h).  The product library never
// contains or calls this.  Built by tests/native_scaled/Makefile with hipcc --offload-host-only.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../gym-treasure-game_amd/csrc/tg_render_scaled.h"
#include "../native/host_env.h"

using namespace tg;

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
  const Level* L = &hl.L;
  std::vector<std::string> desc;
  for (auto& l : lines_of(hl.dom)) desc.push_back(strip(l));
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
  HostReplay env(hl, false);
  const size_t fb = (size_t)P.h * P.w * channels;
  for (int64_t i = 0; i < n; ++i) {
    env.start(seed_base + (uint64_t)envs[i]);
    for (int t = 0; t < steps; ++t) env.step(a0, policy, autoreset != 0, envs[i], t);
    const Env& e = env.e;
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

// the flag word's facing bit and first object bit (tg_state.h)
void hcs_flag_bits(uint32_t* facing, int* obj) { *facing = F_FACING, *obj = F_OBJ; }

}  // extern "C"
