// tg_hostcheck.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the product's per-env core (gym-treasure-game_amd/csrc/tg_core.h), so
// the exact code the gfx950 kernel runs per lane can be checked against the oracle on the
// build machine, which has no GPU.  It replays k_step's per-lane sequence (env_step, observe,
// optional auto-reset) one env at a time (host_env.h: the level load and the replay, shared with
// tests/native_scaled).  The product library never contains or calls this.
// Built by tests/native/Makefile with hipcc --offload-host-only.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../gym-treasure-game_amd/csrc/tg_render.h"
#include "../../gym-treasure-game_amd/csrc/tg_srv_word.h"
#include "host_env.h"

using namespace tg;

namespace {
uint64_t rec_hash(uint64_t h, const double o[9], int32_t r, int v, int d) {
  for (int i = 0; i < 9; ++i) {
    uint64_t b;
    memcpy(&b, &o[i], 8);
    h = sm64(h ^ b);
  }
  return sm64(h ^ ((uint64_t)(uint32_t)r | ((uint64_t)v << 32) | ((uint64_t)d << 40)));
}

// The renderer's tables for one level and sprite sheet, built by tg_render_init's host code, and
// one frame composed from an env's state words exactly as k_render's lanes do it (band by band,
// row by row, 16-B chunk by chunk).  The one copy of that loop: hc_render_run and
// hc_render_states differ only in how they reach the state words.
struct HostFrames {
  std::vector<uint8_t> bg, tiles;
  std::vector<uint32_t> dyn;
  RenderArgs A;
  HostFrames(const HostLevel& hl, const uint8_t* sprites, int sw, int sh) {
    const Level& L = hl.L;
    std::vector<std::string> desc;
    for (auto& l : lines_of(hl.dom)) desc.push_back(strip(l));
    while (!desc.empty() && desc.back().empty()) desc.pop_back();
    const std::vector<uint32_t> sc = scale_sprites(sprites, sw, sh);
    const std::vector<uint32_t> bg32 = static_layer(desc, L.W, L.H, sc);
    bg = rgb_bytes(bg32);
    dyn = dynamic_sprites(sc);
    tiles = rgb_bytes(cell_tiles(bg32, L.W, L.H, dyn));
    A.bg = reinterpret_cast<const uint4*>(bg.data());
    A.tiles = reinterpret_cast<const uint4*>(tiles.data());
    A.spr = dyn.data();
    A.err = nullptr;  // the error bits are frame()'s return value
    render_level(L, A);
  }
  HostFrames(const HostFrames&) = delete;
  HostFrames& operator=(const HostFrames&) = delete;
  size_t frame_bytes() const { return (size_t)A.Hpx * A.Wpx * 3; }
  // frame [H*48][W*48][3]; returns the TG_ERR_RENDER bits
  uint32_t frame(const uint4 st, const double2 an, uint8_t* frame) const {
    uint32_t err = 0;
    uint4* out = reinterpret_cast<uint4*>(frame);
    std::vector<uint16_t> sel((size_t)A.W);
    for (int band = 0; band < A.H; ++band) {
      const int ylo = band * RS;
      Layer lay[NLAYER];
      uint32_t live_mask = 0;
      for (int k = 0; k < NLAYER; ++k) {
        bool live = false;
        err |= make_layer(A, k, st, an, lay[k], live);
        live = live && lay[k].y1 > ylo && lay[k].y0 < ylo + RS && lay[k].x1 > 0 && lay[k].x0 < A.Wpx;
        live_mask |= (uint32_t)live << k;
      }
      cell_sources(lay, live_mask, band, A.W, sel.data());
      for (int r = 0; r < RS; ++r) {
        const int y = ylo + r;
        const uint32_t rm = row_items(lay, live_mask, y);
        for (int q = 0; q < A.CH; ++q) {
          const uint4 v = A.bg[(size_t)y * A.CH + q];
          out[(size_t)y * A.CH + q] = rm ? render_chunk(A, lay, rm, sel.data(), band, r, q, v) : v;
        }
      }
    }
    return err;
  }
};
}  // namespace

extern "C" {

// go_left / go_right answered from the GoTable as on the device (1, default) or directly (0)
static int g_gotab = 1;
void hc_set_gotab(int on) { g_gotab = on; }
// the level bitmasks (tg_map.h Map::mk) as on the device's option loops (1, default) or not (0)
static int g_masks = 1;
void hc_set_masks(int on) { g_masks = on; }

// Level texts as tg_create takes them (NULL = built-in default).
// obs/final_obs [n][steps+1][9], reward/valid/done [n][steps+1], hash/draws/ticks [n]
int hc_run(const char* dom, const char* objs, const char* inter, uint64_t seed_base, int64_t g0,
           int64_t n, int steps, uint64_t a0, int policy, int autoreset, double* obs,
           int32_t* reward, uint8_t* valid, uint8_t* done, double* final_obs, uint64_t* hash,
           int64_t* draws, int64_t* ticks) {
  HostLevel hl;
  if (!hl.load(dom, objs, inter, g_gotab, g_masks)) return -1;
  HostReplay env(hl, true);
  const int64_t T1 = (int64_t)steps + 1;
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t g = (uint64_t)(g0 + i);
    env.start(seed_base + g);
    double o[9], fo[9];
    observe(hl.L, env.e, o);
    uint64_t h = rec_hash(g, o, 0, 0, 0);
    int64_t nt = 0;
    if (obs) memcpy(&obs[i * T1 * 9], o, sizeof o);
    if (final_obs) memcpy(&final_obs[i * T1 * 9], o, sizeof o);
    if (reward) reward[i * T1] = 0;
    if (valid) valid[i * T1] = 0;
    if (done) done[i * T1] = 0;
    for (int t = 0; t < steps; ++t) {
      const StepResult r = env.step(a0, policy, autoreset != 0, (int64_t)g, t, fo);
      nt += r.ticks;
      observe(hl.L, env.e, o);  // fo, or the reset env's
      h = rec_hash(h, fo, r.reward, r.ran, r.done);
      const int64_t j = i * T1 + t + 1;
      if (obs) memcpy(&obs[j * 9], o, sizeof o);
      if (final_obs) memcpy(&final_obs[j * 9], fo, sizeof fo);
      if (reward) reward[j] = r.reward;
      if (valid) valid[j] = (uint8_t)r.ran;
      if (done) done[j] = (uint8_t)r.done;
    }
    if (hash) hash[i] = h;
    if (draws) draws[i] = env.draws;  // includes the 8 construct + reset draws
    if (ticks) ticks[i] = nt;
  }
  return 0;
}

// One step from each of n given states (the checkpoint format of tg_read_state / tg_write_state,
// case-major arrays): the state goes through the product's own codec (pack, then unpack, as
// tg_write_state stores it and the kernels load it) into the core's Env, with a ring built as
// tg_write_state builds it (the given generation first, its successors after it); then
// available_mask and one env_step(actions[i]).  Outputs as the oracle's tgo_step_states: obs
// [n][9], reward / valid / done [n], mask [n], the state after (flags2 with the error bits;
// (mt2, mt_pos2) as tg_read_state reports them: the generation holding the position, index
// 0..622), ticks and draws [n].  actions null: the masks only (mt may be null).  `threads`
// workers, each on a contiguous share of the cases.
int hc_step_states(const char* dom, const char* objs, const char* inter, int64_t n,
                   const int32_t* pos, const uint32_t* flags, const int32_t* cells,
                   const double* ang, const uint32_t* mt, const uint32_t* mt_pos,
                   const int32_t* actions, double* obs, int32_t* reward, uint8_t* valid,
                   uint8_t* done, uint16_t* mask, int32_t* pos2, uint32_t* flags2, int32_t* cells2,
                   double* ang2, uint32_t* mt2, uint32_t* mt_pos2, int64_t* ticks, int64_t* draws,
                   int threads) {
  HostLevel hl;
  if (!hl.load(dom, objs, inter, g_gotab, g_masks)) return -1;
  if (actions && (!mt || !mt_pos)) return -1;
  const Level& L = hl.L;
  const Map m = hl.map(true);
  const uint32_t* const trig = &L.trig[0][0];
  const auto work = [&](int64_t lo, int64_t hi) {
    std::vector<uint32_t> ring(MT_STORE), gen(MT_N);
    for (int64_t i = lo; i < hi; ++i) {
      Env t{};
      t.px = pos[2 * i], t.py = pos[2 * i + 1];
      t.f = flags[i];
      t.kx = cells[4 * i], t.ky = cells[4 * i + 1], t.gx = cells[4 * i + 2], t.gy = cells[4 * i + 3];
      t.mti = mt_pos ? mt_pos[i] : 0u;
      double2 an;
      an.x = ang[2 * i], an.y = ang[2 * i + 1];
      Env e{};
      unpack(pack(t), an, e);
      if (mask) mask[i] = (uint16_t)available_mask(L, m, e);
      if (!actions) continue;
      // ring generation 0 = the given words; 1 .. 15 by plain twists, the even ones stored
      memcpy(ring.data(), mt + i * MT_N, sizeof(uint32_t) * MT_N);
      memcpy(gen.data(), ring.data(), sizeof(uint32_t) * MT_N);
      for (int g = 1; g < 2 * MT_HALF_GENS; ++g) {
        twist_gen_inplace(gen.data());
        if (!(g & 1)) memcpy(ring.data() + mt_store_off((uint32_t)g), gen.data(), sizeof(uint32_t) * MT_N);
      }
      Rng rng(ring.data(), e.mti);
      const StepResult r = env_step(L, trig, m, e, actions[i], rng);
      e.mti = rng.finish();
      if (obs) observe(L, e, obs + 9 * i);
      if (reward) reward[i] = r.reward;
      if (valid) valid[i] = (uint8_t)r.ran;
      if (done) done[i] = (uint8_t)r.done;
      if (ticks) ticks[i] = r.ticks;
      if (draws) draws[i] = rng.draws;
      if (pos2) pos2[2 * i] = e.px, pos2[2 * i + 1] = e.py;
      if (flags2) flags2[i] = e.f;
      if (cells2) cells2[4 * i] = e.kx, cells2[4 * i + 1] = e.ky, cells2[4 * i + 2] = e.gx, cells2[4 * i + 3] = e.gy;
      if (ang2) ang2[2 * i] = e.ang0, ang2[2 * i + 1] = e.ang1;
      const uint32_t p = e.mti & MT_POS_MASK, g = p / (uint32_t)MT_N;
      if (mt_pos2) mt_pos2[i] = p - g * (uint32_t)MT_N;
      if (mt2) {  // the generation holding p: stored, or the twist of the stored one before it
        if (g & 1u) twist_gen(ring.data() + mt_store_off(g - 1u), mt2 + i * MT_N);
        else memcpy(mt2 + i * MT_N, ring.data() + mt_store_off(g), sizeof(uint32_t) * MT_N);
      }
    }
  };
  if (threads < 1) threads = 1;
  if (threads > 16) threads = 16;
  std::vector<std::thread> pool;
  const int64_t share = (n + threads - 1) / threads;
  for (int w = 0; w < threads; ++w) {
    const int64_t lo = w * share, hi = lo + share < n ? lo + share : n;
    if (lo < hi) pool.emplace_back(work, lo, hi);
  }
  for (auto& th : pool) th.join();
  return 0;
}

// random.seed(seed); then launches[j] calls of random() per "launch", the generation buffer
// handled as the kernels do: a stale half is refilled before launch j when j % defer == 0
// (the classify pass), otherwise the launch starts with it stale and must regenerate it
// itself if it gets there.  out = every value, in order.
int hc_rng_stream(uint64_t seed, const int32_t* launches, int nl, int defer, double* out) {
  uint32_t gen[MT_N];
  genrand_prefix(gen);
  std::vector<uint32_t> mt(MT_WORDS);
  init_mt(mt.data(), gen, seed);
  uint32_t state = 0;
  int64_t k = 0;
  for (int j = 0; j < nl; ++j) {
    if (defer > 0 && j % defer == 0) state = refill_after(mt.data(), state);
    Rng rng(mt.data(), state);
    for (int d = 0; d < launches[j]; ++d) out[k++] = rng.random();
    state = rng.finish();
  }
  return 0;
}

// code_of_top27 against draw_code at both ends of every top-27-bit interval it decides (the
// outcomes are monotone in r, so the ends decide the interval); returns the mismatches and the
// number of intervals left to the exact path
int64_t hc_check_code_top27(int64_t* slow) {
  int64_t bad = 0, ns = 0;
  for (uint32_t a = 0; a < (1u << 27); ++a) {
    const uint32_t c = tg::code_of_top27(a);
    if (c == tg::CODE_SLOW) {
      ++ns;
      continue;
    }
    const double lo = (a * 67108864.0) * (1.0 / 9007199254740992.0);
    const double hi = (a * 67108864.0 + 67108863.0) * (1.0 / 9007199254740992.0);
    bad += (tg::draw_code(lo) != c) + (tg::draw_code(hi) != c);
  }
  *slow = ns;
  return bad;
}

// mt_pair (branch-free, RngCodes on the device), mt_pair_branchy (tg::Rng) and the plain
// twist against each other and against full generations: a seeded ring, every even position
// of all 16 generations.  Returns the mismatches.
int64_t hc_check_mt_pair(uint64_t seed) {
  uint32_t gen[MT_N];
  genrand_prefix(gen);
  std::vector<uint32_t> mt(MT_STORE), full((size_t)(2 * MT_HALF_GENS + 1) * MT_N);
  init_mt(mt.data(), gen, seed);
  seed_mt(full.data(), gen, seed);  // generation -1, then 16 twists: the ring's generations
  for (int g = 0; g < 2 * MT_HALF_GENS; ++g) twist_gen(&full[(size_t)g * MT_N], &full[(size_t)(g + 1) * MT_N]);
  int64_t bad = 0;
  for (uint32_t p = 0; p < (uint32_t)MT_WORDS; p += 2) {
    uint32_t a0, a1, b0, b1;
    mt_pair(mt.data(), p, a0, a1);
    mt_pair_branchy(mt.data(), p, b0, b1);
    const WordPair c = mt_pair_ool(mt.data(), p);
    const uint32_t f0 = full[MT_N + p], f1 = full[MT_N + p + 1];
    bad += (a0 != f0) + (a1 != f1) + (b0 != f0) + (b1 != f1) + (c.w0 != f0) + (c.w1 != f1);
  }
  return bad;
}

// top27_code / top27_slow (the wave twist's code pass, tg_twist.h) against code_of_top27 for
// every a: equal wherever top27_slow is false, and top27_slow covers every CODE_SLOW interval;
// returns the mismatches and the number of slow intervals
int64_t hc_check_code_lean(int64_t* slow) {
  int64_t bad = 0, ns = 0;
  for (uint32_t a = 0; a < (1u << 27); ++a) {
    const uint32_t c = tg::code_of_top27(a);
    if (tg::top27_slow(a)) {
      ++ns;
      continue;
    }
    bad += (c == tg::CODE_SLOW) + (tg::top27_code(a) != c);
  }
  *slow = ns;
  return bad;
}

// The st4 codec (tg_core.h pack / unpack): round trips at the field extremes, and three words
// computed by hand, so the format is pinned and not only self-consistent.  Returns the mismatches.
int64_t hc_check_st4_codec(void) {
  int64_t bad = 0;
  const int p16[4] = {-32768, -1, 0, 32767}, c8[4] = {-128, -1, 0, 127};
  const uint32_t w32[2] = {0u, 0xFFFFFFFFu};
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b)
      for (int c = 0; c < 256; ++c)  // the four object cells, two bits each
        for (int d = 0; d < 4; ++d) {
          Env e{};
          e.px = p16[a], e.py = p16[b];
          e.kx = c8[c & 3], e.ky = c8[(c >> 2) & 3], e.gx = c8[(c >> 4) & 3], e.gy = c8[c >> 6];
          e.f = w32[d & 1], e.mti = w32[d >> 1];
          e.ang0 = 0.25 * a, e.ang1 = -0.5 * b;
          const uint4 s = pack(e);
          double2 an;
          an.x = e.ang0, an.y = e.ang1;
          Env r{};
          unpack(s, an, r);  // (unpack_st4, then the angles)
          bad += r.px != e.px || r.py != e.py || r.f != e.f || r.kx != e.kx || r.ky != e.ky ||
                 r.gx != e.gx || r.gy != e.gy || r.mti != e.mti || r.ang0 != e.ang0 || r.ang1 != e.ang1;
          bad += s.y != e.f || s.w != e.mti || st4_flags(s) != e.f;
        }
  Env e{};
  e.px = -2, e.py = 3;
  bad += pack(e).x != 0x0003FFFEu;
  e = Env{};
  e.kx = -1, e.ky = 2, e.gx = 3, e.gy = -4;
  bad += pack(e).z != 0xFC0302FFu;
  e = Env{};
  e.f = 0x89ABCDEFu;
  bad += pack(e).y != 0x89ABCDEFu || pack(e).x != 0u || pack(e).z != 0u || pack(e).w != 0u;
  return bad;
}

// The N = 1 server's command word (tg_srv_word.h): the host's encoder, and k_serve1's decoders
// into out[5] = kind, action, warm, has_gauss, q0.  hc_option_index: what the device's step makes
// of a decoded action (tg_core.h option_index; -1: out of range, TG_ERR_ACTION).
uint32_t hc_srv_word(uint32_t kind, int32_t action, int warm, int has_gauss, uint32_t q0) {
  return srv_word(kind, action, warm != 0, has_gauss != 0, q0);
}
void hc_srv_fields(uint32_t word, int32_t* out) {
  out[0] = (int32_t)srv_kind(word);
  out[1] = srv_action(word);
  out[2] = srv_warm(word);
  out[3] = srv_has_gauss(word);
  out[4] = (int32_t)srv_q0(word);
}
int hc_option_index(int action) { return option_index(action); }

// the six collision predicates at a pixel position / door state (same bit order as the
// oracle's tgo_predicates)
unsigned hc_predicates(int px, int py, unsigned door_bits) {
  static HostLevel hl;
  if (hl.grid.empty() && !hl.load(nullptr, nullptr, nullptr, g_gotab, g_masks)) return ~0u;
  const Map m = hl.map(false);
  Env e{};
  e.px = px;
  e.py = py;
  e.f = (door_bits & 7u) << F_OBJ;
  return (unsigned)m.up_clear(e) | (unsigned)m.can_go_up(e) << 1 | (unsigned)m.can_go_down(e) << 2 |
         (unsigned)m.can_go_side(e, -1) << 3 | (unsigned)m.can_go_side(e, +1) << 4 |
         (unsigned)m.can_fall(e) << 5;
}

void hc_predicate_table(int x0, int x1, int y0, int y1, unsigned door_bits, uint8_t* out) {
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x)
      out[(size_t)(y - y0) * (size_t)(x1 - x0) + (size_t)(x - x0)] =
          (uint8_t)hc_predicates(x, y, door_bits);
}

// render('rgb_array') of env g = seed_base + envs[i] after `steps` steps of the hc_run
// action stream, composed by tg_render.h exactly as k_render's lanes do (band by band, row by
// row, 16-B chunk by chunk), with the static layer built by tg_render_init's host code.
// frames [n][H*48][W*48][3].  Returns the OR of the TG_ERR_RENDER bits, or -1.
int hc_render_run(const char* dom, const char* objs, const char* inter, uint64_t seed_base,
                  const int64_t* envs, int64_t n, int steps, uint64_t a0, int policy,
                  int autoreset, const uint8_t* sprites, int sw, int sh, uint8_t* frames) {
  HostLevel hl;
  if (!hl.load(dom, objs, inter, g_gotab, g_masks)) return -1;
  const HostFrames hf(hl, sprites, sw, sh);
  HostReplay env(hl, false);
  uint32_t err = 0;
  for (int64_t i = 0; i < n; ++i) {
    env.start(seed_base + (uint64_t)envs[i]);
    for (int t = 0; t < steps; ++t) env.step(a0, policy, autoreset != 0, envs[i], t);
    const Env& e = env.e;
    double2 an;
    an.x = e.ang0, an.y = e.ang1;
    err |= hf.frame(pack(e), an, frames + (size_t)i * hf.frame_bytes());  // the SoA state words
  }
  return (int)err;
}

// The same composition of n given states (the checkpoint format, case-major arrays as
// hc_step_states takes them): each goes through the product's codec into the state words
// k_render reads.  `threads` workers, each on a contiguous share of the cases.
int hc_render_states(const char* dom, const char* objs, const char* inter, int64_t n,
                     const int32_t* pos, const uint32_t* flags, const int32_t* cells,
                     const double* ang, const uint8_t* sprites, int sw, int sh, uint8_t* frames,
                     int threads) {
  HostLevel hl;
  if (!hl.load(dom, objs, inter, g_gotab, g_masks)) return -1;
  const HostFrames hf(hl, sprites, sw, sh);
  std::vector<uint32_t> errs(16, 0u);
  const auto work = [&](int w, int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      Env t{};
      t.px = pos[2 * i], t.py = pos[2 * i + 1];
      t.f = flags[i];
      t.kx = cells[4 * i], t.ky = cells[4 * i + 1], t.gx = cells[4 * i + 2], t.gy = cells[4 * i + 3];
      double2 an;
      an.x = ang[2 * i], an.y = ang[2 * i + 1];
      errs[(size_t)w] |= hf.frame(pack(t), an, frames + (size_t)i * hf.frame_bytes());
    }
  };
  if (threads < 1) threads = 1;
  if (threads > 16) threads = 16;
  std::vector<std::thread> pool;
  const int64_t share = (n + threads - 1) / threads;
  for (int w = 0; w < threads; ++w) {
    const int64_t lo = w * share, hi = lo + share < n ? lo + share : n;
    if (lo < hi) pool.emplace_back(work, w, lo, hi);
  }
  for (auto& th : pool) th.join();
  uint32_t err = 0;
  for (uint32_t e : errs) err |= e;
  return (int)err;
}

}  // extern "C"
