// tg_mt.h — CPython's random on one env: the ring of pre-twisted MT19937 generations (twist,
// temper, the stored even generations and mt_pair*), the draw codes (draw_code, code_of_top27,
// top27_code, gen_codes), a half's per-lane regeneration (twist_half), the direct-load consumer
// `Rng` with refill_after, and seeding (genrand_prefix, seed_mt, init_mt).  `__host__ __device__`.
// The whole-wave regeneration is tg_twist.h's, the option loops' LDS window tg_dev.h's RngCodesT.
#pragma once
#include "tg_state.h"

namespace tg {

// ==========================================================================================
// CPython random over a ring of pre-twisted generations.
//   CPython (_randommodule.c genrand_uint32) regenerates all 624 words at once ("twist")
//   whenever its index reaches 624, then tempers one word per call; random() takes two.
//   Here each env keeps a ring of 2 x MT_HALF_GENS consecutive generations, two halves of
//   MT_HALF_GENS generations each (words [0, MT_HALF) and [MT_HALF, MT_WORDS)), and a position
//   pos in [0, MT_WORDS) (always even: random() is the only consumer).  Consumption only
//   reads: the generation holding pos is CPython's mt[] with index pos % 624, and the ring
//   always holds the NEXT generations after it, so crossing a generation or half boundary
//   continues the stream without a twist.
//   The half a lane has left is stale (2 x MT_HALF_GENS generations behind) until it is
//   regenerated: MT_HALF_GENS twists in sequence from the last generation of the half the
//   lane is in (twist_half); the env's state word carries MT_STALE meanwhile.  The kernels
//   regenerate it later, a whole wavefront per env, coalesced, the chained twists in LDS
//   (tg_twist.h twist_chain: k_regen every 16 steps, k_reset, k_step).  A launch that
//   would enter a stale half (> MT_HALF draws since the refill) regenerates it first, per
//   lane.  Seeding (init_by_array) fills the ring's last generation; 2 x MT_HALF_GENS twists
//   then give generations 1 .. 2 x MT_HALF_GENS, pos 0 (init_mt).
//   Why a ring of 8 + 8: a half's regeneration reads one generation (its
//   source) and writes MT_HALF_GENS of them, 3,120 B per generation instead of the 5,304 of
//   a two-generation ring whose every twist re-reads its source from HBM, and the refill
//   list is an eighth as long (A/B, 1M envs: 2 + 2 / 4 + 4 / 8 + 8 per half: uniform 0.172 /
//   0.168 / 0.164 ms, masked 0.399 / 0.391 / 0.368 ms per step; 1 + 1: 0.176 / 0.483).
//   Stored words (round 4): only the EVEN generations of the ring (gens 0, 2, ..., 14 of the
//   16; MT_STORE words per env, mt_store_off), the codes of all.  The option loops read codes;
//   the words serve the rare draws that need their double (handle angles, an auto-reset's
//   gauss) and the twists.  An odd generation's word is the twist of the stored generation
//   before it (twist_at: <= 4 twist_word evaluations on that generation's words, mt_pair), and
//   a half's regeneration starts from the other half's generation 7 = the twist of its stored
//   generation 6.  A regenerated generation costs 312 B of codes + 1,248 B of words instead of
//   312 + 2,496.  20 KB of words + 5 KB of codes per env.
// ==========================================================================================
constexpr int MT_HALF_GENS = 8;                // generations per half
constexpr int MT_HALF = MT_HALF_GENS * MT_N;   // ring positions per half (words of 8 generations)
constexpr int MT_WORDS = 2 * MT_HALF;          // ring positions per env
constexpr int MT_STORE = MT_WORDS / 2;         // words stored per env: the even generations
static_assert(MT_HALF_GENS % 2 == 0, "a half starts on a stored generation");
// word offset in the stored words of ring generation g (even; g = ring position / MT_N)
TG_HD uint32_t mt_store_off(uint32_t g) { return (g >> 1) * (uint32_t)MT_N; }
constexpr uint32_t MT_STALE = 1u << 31;   // state word: the half not holding pos is stale
constexpr uint32_t MT_LISTED = 1u << 30;  // state word: that stale half is on a refill list (k_regen)
constexpr uint32_t MT_POS_MASK = 0xFFFFu;
static_assert(MT_WORDS <= (int)MT_POS_MASK, "positions fit the state word");
constexpr uint32_t MT_UPPER = 0x80000000u, MT_LOWER = 0x7fffffffu;

TG_HD uint32_t mt_twist(uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t y = (a & MT_UPPER) | (b & MT_LOWER);
  return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
TG_HD uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}
// random_random (53-bit) from two consecutive words, exact in double (FMA-safe)
TG_HD double mt_double(uint32_t w0, uint32_t w1) {
  const uint32_t a = mt_temper(w0) >> 5, b = mt_temper(w1) >> 6;
  return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0);
}
// dst = the generation after src (genrand_uint32's twist, out of place)
TG_HD void twist_gen(const uint32_t* src, uint32_t* dst) {
  for (int p = 0; p < MT_N - MT_M; ++p) dst[p] = mt_twist(src[p], src[p + 1], src[p + MT_M]);
  for (int p = MT_N - MT_M; p < MT_N - 1; ++p)
    dst[p] = mt_twist(src[p], src[p + 1], dst[p - (MT_N - MT_M)]);
  dst[MT_N - 1] = mt_twist(src[MT_N - 1], dst[0], dst[MT_M - 1]);
}
// the same in place: twist_gen reads src only at or after the word it writes and dst only
// before it, so src == dst is CPython's own in-place loop
TG_HD void twist_gen_inplace(uint32_t* w) { twist_gen(w, w); }
// Word i (< 623) of the generation after g, from g's words alone: new word i reads new word
// i - 227 for i >= 227 (twist_gen), so it is a chain of d = i / 227 (0-2) twist words on top of
// new word j0 = i - 227 d (< 227, which reads old words only).  The chain's old words are at
// fixed offsets from j0 and all load unconditionally (indices clamped into the generation):
// one memory round trip, and no divergence between lanes of different chain lengths.
// (Ld: how a stored word is read — plain, or k_flow's L1-bypassing load, tg_flow.h)
struct PlainLd {
  TG_HD uint32_t operator()(const uint32_t* p) const { return *p; }
};
template <class Ld = PlainLd>
TG_HD uint32_t twist_at_lo(const uint32_t* g, int i, const Ld& ld = Ld()) {
  constexpr int K = MT_N - MT_M;  // 227
  const int d = i >= 2 * K ? 2 : i >= K ? 1 : 0;
  const int j0 = i - K * d;
  const int c2 = j0 + 2 * K < MT_N - 1 ? j0 + 2 * K : MT_N - 2;
  const uint32_t a0 = ld(g + j0), b0 = ld(g + j0 + 1), c0 = ld(g + j0 + MT_M);
  const uint32_t a1 = ld(g + j0 + K), b1 = ld(g + j0 + K + 1);
  const uint32_t a2 = ld(g + c2), b2 = ld(g + c2 + 1);
  uint32_t w = mt_twist(a0, b0, c0);
  const uint32_t w1 = mt_twist(a1, b1, w);
  w = d >= 1 ? w1 : w;
  const uint32_t w2 = mt_twist(a2, b2, w);
  return d >= 2 ? w2 : w;
}
// word i of the generation after g (word 623 reads new words 0 and 396)
TG_HD uint32_t twist_at(const uint32_t* g, int i) {
  return i < MT_N - 1 ? twist_at_lo(g, i)
                      : mt_twist(g[MT_N - 1], twist_at_lo(g, 0), twist_at_lo(g, MT_M - 1));
}
// The two words at ring position p (even) from the stored generations: an even generation's
// are stored, an odd one's are twisted from the generation before it (the rare draws that need
// their double).  Branch-free: every lane issues the loads of both cases (~20 words) at once,
// so a wave whose lanes sit in even and odd generations pays one memory round trip, not two.
template <class Ld = PlainLd>
TG_HD void mt_pair(const uint32_t* mt, uint32_t p, uint32_t& w0, uint32_t& w1, const Ld& ld = Ld()) {
  const uint32_t g = p / (uint32_t)MT_N, i = p - g * (uint32_t)MT_N;  // i even, <= 622
  const uint32_t* const cur = mt + mt_store_off(g & ~1u);  // g's own words if g is even
  const uint32_t* const prev = mt + mt_store_off(g == 0u ? 0u : (g - 1u) & ~1u);
  const uint32_t e0 = ld(cur + i), e1 = ld(cur + i + 1);
  const uint32_t o0 = twist_at_lo(prev, (int)i, ld);
  // word i + 1: a chain of its own, or, for i + 1 = 623, the twist of old word 623 with new
  // words 0 and 396
  const bool last = i + 1u == (uint32_t)MT_N - 1u;
  const uint32_t x = twist_at_lo(prev, last ? MT_M - 1 : (int)i + 1, ld);
  const uint32_t y0 = twist_at_lo(prev, 0, ld);
  const uint32_t o1 = last ? mt_twist(ld(prev + MT_N - 1), y0, x) : x;
  w0 = (g & 1u) ? o0 : e0;
  w1 = (g & 1u) ? o1 : e1;
}
// the same with a branch (few registers, inline: tg::Rng, whose draws of doubles in the step
// kernels are resets of envs whose option did not run, rarer still)
TG_HD void mt_pair_branchy(const uint32_t* mt, uint32_t p, uint32_t& w0, uint32_t& w1) {
  const uint32_t g = p / (uint32_t)MT_N, i = p - g * (uint32_t)MT_N;
  if (g & 1u) {
    const uint32_t* const prev = mt + mt_store_off(g - 1u);
    w0 = twist_at(prev, (int)i);
    w1 = twist_at(prev, (int)i + 1);
  } else {
    w0 = mt[mt_store_off(g) + i];
    w1 = mt[mt_store_off(g) + i + 1];
  }
}
// mt_pair out of line (RngCodes, the option loops' draws: its loads and chains would
// otherwise add ~30 VGPRs to k_run's allocation)
struct WordPair {
  uint32_t w0, w1;
};
__host__ __device__ inline __attribute__((noinline)) WordPair mt_pair_ool(const uint32_t* mt, uint32_t p) {
  WordPair r;
  mt_pair(mt, p, r.w0, r.w1);
  return r;
}
// word offset of the half holding word position pos
TG_HD uint32_t mt_half(uint32_t pos) { return pos >= (uint32_t)MT_HALF ? (uint32_t)MT_HALF : 0u; }

// ---- draw codes ------------------------------------------------------------------------------
// Every random() value the option loops consume decides one of four things, each a comparison
// of the double r against constants, computed with the reference's own IEEE expressions:
//   noisy(+4) (IM/:361-366): int(round(uniform(2.0, 4)))   = rint(2.0 + 2.0 * r) in {2, 3, 4}
//   noisy(-4):                int(round(uniform(-4, -2.0))) = rint(-4.0 + 2.0 * r) in {-4, -3, -2}
//   the jump ticker (IM/:317-319): random() > 0.25
//   handle.flip (OB/:117-122):     uniform(0, 1) <= 0.8  (== r exactly)
// so each generation is stored twice: its 624 words (for the next twist and for the rare
// draws that need the double itself: handle angles, the reset's gauss) and one code byte per
// draw (MT_CODES per env, the generation at word offset g at g / 2) holding those four
// outcomes.  Whoever regenerates a half writes both.  Tick loops read bytes (16 draws per 16-B
// load) and do no f64 work.
constexpr int MT_CODES = MT_WORDS / 2;  // one per random() draw of the ring
constexpr uint32_t CODE_POS = 3u;        // rint(2 + 2r) - 2
constexpr uint32_t CODE_NEG_SHIFT = 2;   // rint(-4 + 2r) + 4, bits 2-3
constexpr uint32_t CODE_JUMP = 1u << 4;  // r > 0.25
constexpr uint32_t CODE_FLIP = 1u << 5;  // r <= 0.8
TG_HD uint32_t draw_code(double r) {
  const uint32_t pos = (uint32_t)((int)rint(2.0 + 2.0 * r) - 2);
  const uint32_t neg = (uint32_t)((int)rint(-4.0 + 2.0 * r) + 4);
  return pos | (neg << CODE_NEG_SHIFT) | (r > 0.25 ? CODE_JUMP : 0u) | (r <= 0.8 ? CODE_FLIP : 0u);
}
// draw_code from the draw's first word: r lies in [a / 2^27, (a + 1) / 2^27) for a = the top
// 27 bits (mt_double), and every outcome in draw_code is monotone in r, so the code is constant
// on that interval unless one of the thresholds 0.25, 0.75, 0.8 lies in it or next to it
// (CODE_SLOW: then the exact f64 path, ~3 draws in 2^25).  Checked for every a against
// draw_code at both ends of its interval (tests/test_core_host.py).  k_regen's code pass takes
// it: one word tempered instead of two, integer compares instead of f64 work.
constexpr uint32_t CODE_SLOW = 0xFFu;
TG_HD uint32_t code_of_top27(uint32_t a) {
  constexpr uint32_t Q1 = 1u << 25, Q3 = 3u << 25, F8 = 107374182u;  // floor(x * 2^27)
  if (a - (Q1 - 1u) < 3u || a - (Q3 - 1u) < 3u || a - (F8 - 1u) < 3u) return CODE_SLOW;
  constexpr uint32_t LOW = CODE_FLIP;                                            // r < 0.25
  constexpr uint32_t MID = 1u | (1u << CODE_NEG_SHIFT) | CODE_JUMP | CODE_FLIP;  // < 0.75
  constexpr uint32_t HIGH = 2u | (2u << CODE_NEG_SHIFT) | CODE_JUMP;             // > 0.75
  return a < Q1 ? LOW : a < Q3 ? MID : a < F8 ? (HIGH | CODE_FLIP) : HIGH;
}
TG_HD uint32_t draw_code_words(uint32_t w0, uint32_t w1) {
  const uint32_t c = code_of_top27(mt_temper(w0) >> 5);
  return c != CODE_SLOW ? c : draw_code(mt_double(w0, w1));
}
// code_of_top27 in fewer instructions (the wave twist's code pass, tg_twist.h, is VALU-bound):
// for an `a` that is not next to a threshold the outcome classes r < 0.25 | < 0.75 | <= 0.8 |
// > 0.8 are a's top two bits (0 | 1, 2 | 3) plus one compare against F8 (F8 >= 3 * 2^25: only
// class 3 splits); byte k of TOP27_LUT is class k's code.  top27_slow is a superset of
// code_of_top27's CODE_SLOW set (a within one of any multiple of 2^25 — 0.25 and 0.75 are 2^25
// and 3 * 2^25, the others harmless extra slow cases — or of F8): there the exact f64 path
// runs.  Checked against code_of_top27 for every a (tests/test_core_host.py).
constexpr uint32_t TOP27_F8 = 107374182u;  // floor(0.8 * 2^27), as code_of_top27
constexpr uint32_t TOP27_LUT = CODE_FLIP |
                               ((1u | (1u << CODE_NEG_SHIFT) | CODE_JUMP | CODE_FLIP) << 8) |
                               ((1u | (1u << CODE_NEG_SHIFT) | CODE_JUMP | CODE_FLIP) << 16) |
                               ((2u | (2u << CODE_NEG_SHIFT) | CODE_JUMP | CODE_FLIP) << 24);
static_assert(TOP27_F8 >= (3u << 25), "only the top class splits at 0.8");
TG_HD bool top27_slow(uint32_t a) {
  return (((a + 1u) & 0x1FFFFFFu) < 3u) | (a - (TOP27_F8 - 1u) < 3u);
}
TG_HD uint32_t top27_code(uint32_t a) {
  const uint32_t c = (TOP27_LUT >> ((a >> 22) & 0x18u)) & 0xFFu;
  return a >= TOP27_F8 ? c ^ CODE_FLIP : c;
}
// the noisy step of a code: +2..+4 (DIR > 0: RIGHT / DOWN) or -4..-2 (LEFT / UP)
TG_HD int code_step(uint32_t c, bool neg) {
  return neg ? (int)((c >> CODE_NEG_SHIFT) & 3u) - 4 : (int)(c & CODE_POS) + 2;
}
TG_HD void gen_codes(const uint32_t* words, uint8_t* c) {
  for (int k = 0; k < MT_N / 2; ++k) c[k] = (uint8_t)draw_code(mt_double(words[2 * k], words[2 * k + 1]));
}
// Regenerate half h (ring position 0 / MT_HALF): its generations in sequence from the one
// before it — the other half's generation 7, the twist of its stored generation 6, or, with
// seeded, the 624 words already in the half's last stored slot (init_mt) — its even
// generations' words and, with mc, all its codes (per-lane form of tg_twist.h twist_chain).
// The half's 4 stored slots are the work space: slot 3 holds the source until generation 5,
// each odd generation goes to the next slot and becomes the even one after it in place;
// generation 7 (codes only) is twisted in place over generation 6, which is then made again
// from generation 4 (two extra twists on this rare per-lane path, no other scratch).
// (Ops: the whole-generation loops, inline here; tg_dev.h's regen_half calls them out of line
// so that k_run's register allocation does not grow around its rare call)
struct GenOps {
  TG_HD void twist(const uint32_t* src, uint32_t* dst) const { twist_gen(src, dst); }
  TG_HD void codes(const uint32_t* w, uint8_t* c) const { gen_codes(w, c); }
};
template <class Ops = GenOps>
TG_HD void twist_half(uint32_t* mt, uint32_t h, uint8_t* mc = nullptr, bool seeded = false,
                      const Ops& op = Ops()) {
  const uint32_t g0 = h / (uint32_t)MT_N;  // ring generation of the half's first (0 / 8)
  uint32_t* const s = mt + mt_store_off(g0);
  uint32_t* const s3 = s + 3 * MT_N;
  if (!seeded) op.twist(mt + mt_store_off((g0 + (uint32_t)MT_HALF_GENS + 6u) % (2u * MT_HALF_GENS)), s3);
  uint8_t* const c = mc ? mc + h / 2 : nullptr;
  // generation g: 0 from slot 3 into slot 0; odd 2k + 1 from slot k into slot k + 1; even
  // 2k + 2 in place in slot k + 1; 7 (codes only) in place in slot 3
  const int last = c ? MT_HALF_GENS : MT_HALF_GENS - 1;
  for (int g = 0; g < last; ++g) {
    const int to = (g + 1) >> 1 < 3 ? (g + 1) >> 1 : 3;
    const uint32_t* const from = g == 0 ? s3 : (g & 1) ? s + (g >> 1) * MT_N : s + to * MT_N;
    op.twist(from, s + to * MT_N);
    if (c) op.codes(s + to * MT_N, c + g * (MT_N / 2));
  }
  if (c) {  // generation 6 again, from 4 through 5
    op.twist(s + 2 * MT_N, s3);
    op.twist(s3, s3);
  }
}

// (tg_walk.h's, which a unit that calls Rng::walk includes)
template <int DIR, class R>
TG_HD int walk_ticks(R& rng, int& x, int lim, int cap);

// Direct-load consumer (few draws per launch: create/reset/classify, and the host checks).
struct Rng {
  uint32_t* mt;    // this env's MT_STORE stored words (the ring's even generations)
  uint32_t pos;    // [0, MT_WORDS), even
  uint32_t draws;  // random() calls (instrumentation for the roofline)
  bool crossed;    // the half not holding pos is stale (MT_STALE on entry, or entered one)
  bool entered;    // entered a half in this launch (the one left is stale)
  uint8_t* mc;     // the env's MT_CODES (device), kept in step when a half is regenerated

  TG_HD Rng(uint32_t* m, uint32_t state, uint8_t* c = nullptr)
      : mt(m), pos(state & MT_POS_MASK), draws(0u), crossed((state & MT_STALE) != 0u),
        entered(false), mc(c) {}

  TG_HD double random() {
    uint32_t w0, w1;
    mt_pair_branchy(mt, pos, w0, w1);
    pos += 2;
    if (pos == (uint32_t)MT_WORDS) pos = 0u;
    if (pos == 0u || pos == (uint32_t)MT_HALF) {
      // entering the other half; a second crossing in one launch finds it stale (a whole ring
      // behind): regenerate it from the half just left before reading it
      if (crossed) twist_half(mt, pos, mc);
      crossed = entered = true;
    }
    ++draws;
    return mt_double(w0, w1);
  }
  // Random.uniform = a + (b-a)*random(); built with -ffp-contract=off (no FMA)
  TG_HD double uniform(double a, double b) { return a + (b - a) * random(); }
  // a draw consumed for its outcome only (see draw_code)
  TG_HD uint32_t code() { return draw_code(random()); }
  // draws come straight from the words: nothing to stage (the device's RngCodes stages codes)
  TG_HD void reserve(uint32_t) {}
  TG_HD bool has(uint32_t) const { return true; }
  TG_HD bool overrun() const { return false; }
  TG_HD void phase(int) {}  // per-phase timing hook of the diagnostic build (tg_dev.h RngCodes)
  template <int DIR>
  TG_HD int walk(int& x, int lim, int cap) { return walk_ticks<DIR>(*this, x, lim, cap); }
  // the state word to store: position, and whether the other half is stale
  TG_HD uint32_t finish() const { return pos | (crossed ? MT_STALE : 0u); }
  // the same when a refill of the half that was stale on entry is already queued
  TG_HD uint32_t finish_queued() const { return pos | (entered ? MT_STALE : 0u); }
};
// regenerate the stale half (per-lane form of wave_refill); returns the clean state word
TG_HD uint32_t refill_after(uint32_t* mt, uint32_t state, uint8_t* mc = nullptr) {
  const uint32_t pos = state & MT_POS_MASK;
  if (state & MT_STALE) twist_half(mt, (uint32_t)MT_HALF - mt_half(pos), mc);
  return pos;
}

// init_genrand(19650218): the common prefix of every init_by_array (seed_mt's genrand19650218)
inline void genrand_prefix(uint32_t gen[MT_N]) {
  gen[0] = 19650218u;
  for (int i = 1; i < MT_N; ++i) gen[i] = 1812433253u * (gen[i - 1] ^ (gen[i - 1] >> 30)) + (uint32_t)i;
}
// init_by_array([seed lo, seed hi?]) into 624 words (CPython's state before its first twist)
TG_HD void seed_mt(uint32_t* mt, const uint32_t* genrand19650218, uint64_t seed) {
  const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
  const uint32_t klen = key1 ? 2u : 1u;
  // pass 1: k = max(N, klen) = N iterations starting at i = 1 (wraps once onto mt[1])
  uint32_t prev = genrand19650218[0];
  uint32_t m0 = prev;
  uint32_t j = 0;
  uint32_t i = 1;
  for (int k = 0; k < MT_N; ++k) {
    const uint32_t cur = (i == 1 && k == MT_N - 1) ? mt[1] : genrand19650218[i];
    const uint32_t key = (j == 0) ? key0 : key1;
    const uint32_t v = (cur ^ ((prev ^ (prev >> 30)) * 1664525u)) + key + j;
    mt[i] = v;
    prev = v;
    ++i;
    ++j;
    if (i >= (uint32_t)MT_N) { m0 = mt[MT_N - 1]; prev = m0; i = 1; }
    if (j >= klen) j = 0;
  }
  mt[0] = m0;
  // pass 2: N-1 iterations
  for (int k = 0; k < MT_N - 1; ++k) {
    const uint32_t cur = mt[i];
    const uint32_t v = (cur ^ ((prev ^ (prev >> 30)) * 1566083941u)) - i;
    mt[i] = v;
    prev = v;
    ++i;
    if (i >= (uint32_t)MT_N) { mt[0] = mt[MT_N - 1]; prev = mt[0]; i = 1; }
  }
  mt[0] = 0x80000000u;
}
// random.seed(seed) into an env's ring (per-lane form of tg_create: k_create + k_gen_twist):
// the seeded words (the state before the first twist) in half 0's last stored slot, then the
// ring's generations from them, pos 0
constexpr uint32_t MT_SEED_OFF = 3 * MT_N;  // mt_store_off(6)
TG_HD void init_mt(uint32_t* mt, const uint32_t* genrand19650218, uint64_t seed,
                   uint8_t* mc = nullptr) {
  seed_mt(mt + MT_SEED_OFF, genrand19650218, seed);
  twist_half(mt, 0u, mc, true);
  twist_half(mt, (uint32_t)MT_HALF, mc);
}

}  // namespace tg
