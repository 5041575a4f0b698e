// tg_hostcheck_view.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the agent-centred window's per-pixel code
// (gym-treasure-game_amd/csrc/tg_render_view.h): the window origin from the state word, the
// mapping of a window pixel to a pixel of the full frame or "outside", the culling of the items
// against the window, and view_pixel over scaled_lookup / scaled_compose, checked against the
// zero-padded crop of the pooled oracle frames on a machine without a GPU.  What k_render_view
// adds around the same functions — the span-to-pixel mapping, the LDS queue, the packed stores —
// runs only on the GPU and is covered by tests/test_gpu_render_view.py.  The tables and the
// state plumbing are tests/native_scaled's (HostScaled, case_words, on_threads), included as
// source so that there is one copy of them.  Every index the window code forms is asserted to
// lie inside its table (TG_VIEW_ASSERT below; a failure makes the calls return -3), and with
// HCV_MAIN the file is a stand-alone program that renders windows of off-level states, for a
// run under a host sanitizer (make asan).  The product library never contains or calls this.
#include <atomic>
#include <cstdio>

static std::atomic<int> hcv_failed{0};
#define TG_VIEW_ASSERT(cond) ((cond) ? (void)0 : (void)(hcv_failed = 1))

#include "../../gym-treasure-game_amd/csrc/tg_render_view.h"
#include "../native_scaled/tg_hostcheck_scaled.cpp"

namespace {
struct HostView {
  const HostScaled& hs;
  ViewArgs V;
  HostView(const HostScaled& s, int radius) : hs(s) {
    V.P = s.P;
    V.r = radius, V.n = s.P.cs * (2 * radius + 1);
  }
  size_t frame_bytes() const { return (size_t)V.n * V.n * V.P.ch; }
  // o [n][n][channels], org (optional) [2]; returns the TG_ERR_RENDER bits
  uint32_t frame(const uint4 st, const double2 an, uint8_t* o, int32_t* org) const {
    Layer lay[NLAYER];
    uint32_t live = 0;
    const uint32_t err = make_layers(V.P.A, st, an, lay, live);  // all nine items, as the kernel
    int ox, oy;
    view_origin(st, V.r, ox, oy);
    if (org) org[0] = ox, org[1] = oy;
    live = view_items(lay, live, ox, oy, V.r);
    for (uint32_t m = live; m; m &= m - 1) {  // a live item's sprite and cell index the tables
      const int i = __builtin_ctz(m);
      const Layer& l = lay[i];
      TG_VIEW_ASSERT(l.spr >= 0 && l.spr < D_COUNT);
      TG_VIEW_ASSERT(i == NLAYER - 1 || (l.ox >= 0 && l.ox + RS <= V.P.A.Wpx && l.oy >= 0 &&
                                         l.oy + RS <= V.P.A.Hpx));
    }
    for (int y = 0; y < V.n; ++y)
      for (int x = 0; x < V.n; ++x) {
        const uint32_t c = view_pixel(V, lay, live, ox, oy, x, y);
        if (V.P.ch == 3) {
          *o++ = (uint8_t)(c >> 16), *o++ = (uint8_t)(c >> 8), *o++ = (uint8_t)c;
        } else {
          *o++ = (uint8_t)luma_px(c);
        }
      }
    return err;
  }
};

bool bad_args(int radius, int scale, int channels) {
  return radius < 1 || radius > VIEW_RMAX || scale_index(scale) < 0 || (channels != 3 && channels != 1);
}
}  // namespace

extern "C" {

// Windows of radius `radius` of envs g = seed_base + envs[i] after `steps` steps of the hc_run
// action stream: out [n][side][side][channels], side = 48 * (2 * radius + 1) / scale, and origin
// (optional) [n][2] in cells.  fast as hcs_render_run's.  Returns the OR of the TG_ERR_RENDER
// bits, -1 for a bad level, -2 for a bad radius, scale or channel count, -3 where an index
// left its table.
int hcv_render_run(const char* dom, const char* objs, const char* inter, uint64_t seed_base,
                   const int64_t* envs, int64_t n, int steps, uint64_t a0, int policy,
                   int autoreset, const uint8_t* sprites, int sw, int sh, int radius, int scale,
                   int channels, int fast, uint8_t* out, int32_t* origin) {
  if (bad_args(radius, scale, channels)) return -2;
  HostLevel hl;
  if (!hl.load(dom, objs, inter)) return -1;
  const HostScaled hs(hl, sprites, sw, sh, scale, channels, fast);
  const HostView hv(hs, radius);
  hcv_failed = 0;
  uint32_t err = 0;
  HostReplay env(hl, false);
  for (int64_t i = 0; i < n; ++i) {
    env.start(seed_base + (uint64_t)envs[i]);
    for (int t = 0; t < steps; ++t) env.step(a0, policy, autoreset != 0, envs[i], t);
    double2 an;
    an.x = env.e.ang0, an.y = env.e.ang1;
    err |= hv.frame(pack(env.e), an, out + (size_t)i * hv.frame_bytes(), origin ? origin + 2 * i : nullptr);
  }
  return hcv_failed ? -3 : (int)err;
}

// The same windows of n given states (the checkpoint format, case-major arrays, as
// hcs_render_states) on `threads` workers.  Returns as hcv_render_run.
int hcv_render_states(const char* dom, const char* objs, const char* inter, int64_t n,
                      const int32_t* pos, const uint32_t* flags, const int32_t* cells,
                      const double* ang, const uint8_t* sprites, int sw, int sh, int radius,
                      int scale, int channels, int fast, uint8_t* out, int32_t* origin,
                      int threads) {
  if (bad_args(radius, scale, channels)) return -2;
  HostLevel hl;
  if (!hl.load(dom, objs, inter)) return -1;
  const HostScaled hs(hl, sprites, sw, sh, scale, channels, fast);
  const HostView hv(hs, radius);
  hcv_failed = 0;
  std::vector<uint32_t> errs(16, 0u);
  on_threads(n, threads, [&](int w, int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      uint4 st;
      double2 an;
      case_words(pos, flags, cells, ang, i, st, an);
      errs[(size_t)w] |= hv.frame(st, an, out + (size_t)i * hv.frame_bytes(),
                                  origin ? origin + 2 * i : nullptr);
    }
  });
  uint32_t err = 0;
  for (uint32_t e : errs) err |= e;
  return hcv_failed ? -3 : (int)err;
}

// envs per group of k_render_view for a frame of frame_px output pixels (tg_render_view.h)
int hcv_view_group(int frame_px) { return view_group(frame_px); }

}  // extern "C"

#ifdef HCV_MAIN
// Stand-alone: windows of the built-in level's start state moved to positions on, across and far
// off every edge (any int16 pair is a valid position), radii 1, 2 and 7, scales 1, 8 and 48, both
// channel counts, fast paths on and off, on a flat sprite sheet.  Its tables are exactly sized
// heap arrays, so a build with -fsanitize=address stops at the first index outside one.
int main() {
  std::vector<uint8_t> sprites((size_t)TG_SPR_COUNT * 4 * 4 * 4, 0x80);
  const int xs[] = {-32768, -1000, -49, -48, -1, 0, 47, 48, 300, 671, 672, 719, 720, 5000, 32767};
  const int ys[] = {-32768, -1000, -73, -72, -25, -24, 23, 24, 300, 599, 600, 623, 624, 5000, 32767};
  std::vector<int32_t> pos, cells;
  std::vector<uint32_t> flags;
  std::vector<double> ang;
  for (int x : xs)
    for (int y : ys)
      for (int f = 0; f < 2; ++f) {
        pos.push_back(x), pos.push_back(y);
        flags.push_back((f ? F_FACING : 0u) | (0x3Fu << F_OBJ));
        const int c[4] = {f ? 2 : -1, f ? 3 : -1, 127, f ? 127 : -128};  // key / gold: on, off, far
        cells.insert(cells.end(), c, c + 4);
        ang.push_back(0.9), ang.push_back(0.95);
      }
  const int64_t n = (int64_t)flags.size();
  long long frames = 0;
  for (int r : {1, 2, VIEW_RMAX})
    for (int s : {1, 8, 48})
      for (int ch : {3, 1})
        for (int fast : {1, 0}) {
          if (s == 1 && r > 1) continue;  // (many more pixels that form no new index)
          const size_t side = (size_t)RS * (2 * r + 1) / s;
          std::vector<uint8_t> out((size_t)n * side * side * ch);
          std::vector<int32_t> org((size_t)n * 2);
          const int rc = hcv_render_states(nullptr, nullptr, nullptr, n, pos.data(), flags.data(),
                                           cells.data(), ang.data(), sprites.data(), 4, 4, r, s, ch,
                                           fast, out.data(), org.data(), 8);
          if (rc != 0) {
            std::printf("hcv_render_states(r %d, s %d, ch %d, fast %d) = %d\n", r, s, ch, fast, rc);
            return 1;
          }
          frames += n;
        }
  std::printf("ok: %lld windows, every index inside its table\n", frames);
  return 0;
}
#endif
