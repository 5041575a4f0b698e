// tg_option.h — one env-step: TreasureGame.step -> _Option.run.  `StepResult`, the plain-span
// limits of the go and ladder options (go_plain_limit, ladder_plain_limit), the fused air and
// ladder ticks, counted_tick, span_loop, run_option_k / run_option, option_index and env_step.
// `__host__ __device__`.  The hot loops: their form was measured against alternatives (see the
// comments at counted_tick and span_loop) — compare the kernels' resource usage after an edit.
#pragma once
#include "tg_rules.h"
#include "tg_walk.h"

namespace tg {

// ==========================================================================================
// One env-step: TreasureGame.step (TG/:91-96) -> _Option.run (OP/:20-36)
// ==========================================================================================
struct StepResult {
  int reward;  // sum of tick rewards (0 when the option could not run)
  int ran;     // 0 == the reference returns reward None
  int done;    // got gold and back in row 0
  int ticks;
};
// ==========================================================================================
// Plain go ticks.  While a go option walks on flat ground, its tick (policy MO/:74-85 +
// IM/:290-359) probes the same cells and finds: not close to the target, side clear, no
// jump ticker, no fall, no object in reach.  Such a tick is exactly: one draw, px += the
// noisy step, facing set, reward -1.  go_plain_limit() returns how far px may go in the
// direction of motion with all of those facts unchanged (INT_MIN / INT_MAX: not at all):
//   * the probed columns px + 16*dir (can_go_side) and px -/+ 10 (can_fall) stay in their
//     48-px cells (rows fixed: py does not change);
//   * close_x: |T - px| >= 4 until 4 px short of the target centre T;
//   * near_cell(key | gold): dx^2 + dy^2 < 24^2 needs |dx| < 24, so an object whose row is
//     within reach bounds the span 24 px short of its centre.
// Motion is monotonic (steps of 2-4 px in dir), so one bound per fact suffices.  A plain
// tick whose step leaves the span checks the pickups at its new px as the full tick does;
// the next tick is a full one, which computes the next span.
// ==========================================================================================
template <int DIR>
TG_HD int go_plain_limit(const Map& m, const Env& e, int tx) {
  constexpr int NONE = DIR > 0 ? -0x40000000 : 0x40000000;
  if ((e.f & F_JT) || !m.can_go_side(e, DIR) || m.can_fall(e) || close_x(e, tx)) return NONE;
  const int P = e.px;
  // target and objects (px never reaches them inside the span)
  const int T = tx * S + S / 2;
  int lim = DIR > 0 ? T - INCR : T + INCR;
  const int ocx[2] = {e.kx, e.gx}, ocy[2] = {e.ky, e.gy};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int dy = e.py - ocy[j] * S;
    if (dy * dy >= R2_OBJ) continue;
    const int X = ocx[j] * S + S / 2;
    if ((P - X < 0 ? X - P : P - X) < S / 2) return NONE;
    if (DIR > 0 && X > P) lim = min(lim, X - S / 2);
    if (DIR < 0 && X < P) lim = max(lim, X + S / 2);
  }
  if (DIR > 0 ? lim < P : lim > P) return NONE;
  // the probed rows are fixed (py does not change in the span)
  const uint32_t dc = Map::dc_of(e.f);
  const int rs1 = m.rowy(e.py + INCR), rs2 = m.rowy(e.py + S - INCR);  // can_go_side
  const int rf1 = m.rowy(e.py), rf2 = m.rowy(e.py + S + 2);            // can_fall
  if (m.mk) {  // the same two scans as bit scans over the rows' column masks (below)
    const int off = DIR * (HALFW + INCR);
    const int c0 = m.colx(P + off) + PAD, c1 = m.colx(lim + off) + PAD;  // bit indices
    const uint32_t blk = m.mk_rowblk(dc, rs1) | m.mk_rowblk(dc, rs2);
    // columns strictly ahead of c0 up to c1
    const uint32_t ahead = DIR > 0 ? ~((2u << c0) - 1u) & ((2u << c1) - 1u)
                                   : ((1u << c0) - 1u) & ~((1u << c1) - 1u);
    const uint32_t hit = blk & ahead;
    if (hit) {
      const int c = (DIR > 0 ? __builtin_ctz(hit) : 31 - __builtin_clz(hit)) - PAD;
      lim = DIR > 0 ? min(lim, c * S - off - 1) : max(lim, c * S + S - 1 - off + 1);
    }
    // can_fall: F(c) = both probed cells of column c OPEN; F(lead0) bounds the span at once
    // (the trailing probe reaches lead0); else the first F column ahead, up to lead1, does
    // when the trailing probe reaches it (the loop below: an F column right after an F lead0
    // would bound it later than lead0 already has)
    const int d = HALFW - 2;  // 10
    const int l0 = m.colx(P + DIR * d) + PAD, l1 = m.colx(lim + DIR * d) + PAD;
    const uint32_t F = m.mk_rowopen(dc, rf1) & m.mk_rowopen(dc, rf2);
    int cf = -1000;
    if ((F >> l0) & 1u) {
      cf = l0;
    } else {
      const uint32_t fa = F & (DIR > 0 ? ~((2u << l0) - 1u) & ((2u << l1) - 1u)
                                       : ((1u << l0) - 1u) & ~((1u << l1) - 1u));
      if (fa) cf = DIR > 0 ? __builtin_ctz(fa) : 31 - __builtin_clz(fa);
    }
    if (cf != -1000) {
      const int c = cf - PAD;
      const int p_both = DIR > 0 ? c * S + d : c * S + S - 1 - d;
      lim = DIR > 0 ? min(lim, p_both - 1) : max(lim, p_both + 1);
    }
    return lim;
  }
  // can_go_side(p) reads column colx(p + 16*dir): the span ends before the first column ahead
  // whose two cells hold a WALL or a closed door
  {
    const int off = DIR * (HALFW + INCR);
    const int c0 = m.colx(P + off), c1 = m.colx(lim + off);
    for (int c = c0 + DIR; DIR > 0 ? c <= c1 : c >= c1; c += DIR) {
      const uint32_t ta = m.cellb(c, rs1), tb = m.cellb(c, rs2);
      if (Map::is_wall(ta | tb) | Map::is_door(ta, dc) | Map::is_door(tb, dc)) {
        // first p with colx(p + off) == c
        lim = DIR > 0 ? min(lim, c * S - off - 1) : max(lim, c * S + S - 1 - off + 1);
        break;
      }
    }
  }
  // can_fall(p) = F(colx(p - 10)) & F(colx(p + 10)), F(c) = both probed cells OPEN: the span
  // ends before the first p ahead where the leading column and the trailing one are both F
  {
    const int d = HALFW - 2;  // 10
    const int lead0 = m.colx(P + DIR * d), lead1 = m.colx(lim + DIR * d);
    bool fprev = Map::is_open(m.cellb(lead0, rf1), dc) & Map::is_open(m.cellb(lead0, rf2), dc);
    if (fprev) {  // the trailing probe (not F now: can_fall is false) reaches lead0
      const int p_both = DIR > 0 ? lead0 * S + d : lead0 * S + S - 1 - d;
      lim = DIR > 0 ? min(lim, p_both - 1) : max(lim, p_both + 1);
    }
    for (int c = lead0 + DIR; DIR > 0 ? c <= lead1 : c >= lead1; c += DIR) {
      const bool fc = Map::is_open(m.cellb(c, rf1), dc) & Map::is_open(m.cellb(c, rf2), dc);
      if (fc) {
        // the leading probe enters c at p_in; the trailing one reaches c at p_both
        const int p_in = DIR > 0 ? c * S - d : c * S + S - 1 + d;
        const int p_both = DIR > 0 ? c * S + d : c * S + S - 1 - d;
        const int p = fprev ? p_in : p_both;
        lim = DIR > 0 ? min(lim, p - 1) : max(lim, p + 1);
        break;
      }
      fprev = fc;
    }
  }
  return lim;
}

// ==========================================================================================
// Plain ladder ticks.  While up_ladder / down_ladder (MO/:160-189) climbs with its ladder
// predicate true, can_fall false, no jump ticker and no key / gold in reach, its tick (policy
// + IM/:290-359) is exactly: one draw, py += noisy(-4) or noisy(+4), reward -1 (x, facing and
// everything else unchanged; a DOWN tick's can_fall4 finds can_fall false).  The predicates
// depend on py only through the rows their probes fall in (px is fixed), so they are constant
// between row breakpoints: ladder_plain_limit() walks those intervals in the direction of
// motion (at most LADDER_SPAN_INTERVALS of them) and returns the farthest py such that every
// start position between it and the current py makes a plain tick (INT_MIN / INT_MAX: none).
// near_cell (OB/:46-53) with px fixed bounds the span before any object's reach.
// ==========================================================================================
constexpr int LADDER_SPAN_INTERVALS = 8;
TG_HD int isqrt_below(int v) {  // largest t >= 0 with t * t < v (v >= 1)
  int t = (int)sqrtf((float)v);
  while (t * t >= v) --t;
  while ((t + 1) * (t + 1) < v) ++t;
  return t;
}
// (the predicates at px for a start position py: the cell probes, or the level bitmasks)
struct LadProbe {
  const Map& m;
  const Env& e;
  TG_HD bool lad(int dir, int y) const {
    Env p = e;
    p.py = y;
    return dir < 0 ? m.can_go_up(p) : m.can_go_down(p);
  }
  TG_HD bool fall(uint32_t dc, int y) const { return m.can_fall_at(dc, e.px, y); }
};
struct LadProbeMk {
  const Map& m;
  const LadMasks& lm;
  TG_HD bool lad(int dir, int y) const { return dir < 0 ? lm.can_go_up(m, y) : lm.can_go_down(m, y); }
  TG_HD bool fall(uint32_t, int y) const { return lm.can_fall(m, y); }
};
template <int DIR, class P = LadProbe>  // -1: up_ladder (py decreases), +1: down_ladder
TG_HD int ladder_plain_limit(const Map& m, const Env& e, const P& pr) {
  constexpr int NONE = DIR > 0 ? -0x40000000 : 0x40000000;
  if (e.f & F_JT) return NONE;
  const uint32_t dc = Map::dc_of(e.f);
  // objects: near(y) <=> (y - oy*48)^2 < R2_OBJ - dx^2; the span stops short of that range
  int bound = DIR > 0 ? 0x3FFFFFFF : -0x3FFFFFFF;
  const int ocx[2] = {e.kx, e.gx}, ocy[2] = {e.ky, e.gy};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int dx = e.px - (ocx[j] * S + S / 2);
    if (dx * dx >= R2_OBJ) continue;
    const int t = isqrt_below(R2_OBJ - dx * dx), Y = ocy[j] * S;  // near <=> |y - Y| <= t
    if ((e.py - Y < 0 ? Y - e.py : e.py - Y) <= t) return NONE;
    if (DIR < 0 && Y < e.py) bound = max(bound, Y + t + 1);
    if (DIR > 0 && Y > e.py) bound = min(bound, Y - t - 1);
  }
  if (DIR < 0) bound = max(bound, 2);  // can_go_up needs py > 1
  int y = e.py, lim = NONE;
  for (int it = 0; it < LADDER_SPAN_INTERVALS; ++it) {
    if (DIR < 0 ? y < bound : y > bound) break;
    if (!pr.lad(DIR, y) || pr.fall(dc, y)) break;
    // the interval of start positions whose probes (rows of y + o) all stay in their rows
    int end;
    if (DIR < 0) {  // can_go_up: y - 4, y, y + 44; can_fall: y, y + 50
      end = max(max(floordiv(y - INCR, S) * S + INCR, floordiv(y, S) * S),
                max(floordiv(y + S - INCR, S) * S - (S - INCR), floordiv(y + S + 2, S) * S - (S + 2)));
      end = max(end, bound);
    } else {        // can_go_down: y, y + 24, y + 51; can_fall: y, y + 50
      end = min(min(floordiv(y, S) * S + S - 1, floordiv(y + S / 2, S) * S + S - 1 - S / 2),
                min(floordiv(y + S + INCR - 1, S) * S + S - 1 - (S + INCR - 1),
                    floordiv(y + S + 2, S) * S + S - 1 - (S + 2)));
      end = min(end, bound);
    }
    lim = end;
    y = end + DIR;
  }
  return lim;
}

// ==========================================================================================
// Fused air tick: policy<K> (jump_left / jump_right MO/:297-314, 367-384; down_left /
// down_right MO/:231-244, 426-439) after its first tick, followed by the primitive tick
// (IM/:290-359), with every predicate the pair may need at the start position evaluated once
// and up front (their lookups issue as one batch): can_fall (the policy's, and the tick's
// gravity test at the same position), can_go_side both ways (the policy's back test, the
// tick's precondition), up_clear (the jump ticker's rise).  Same outcomes and draws as
// policy<K> + tick<prims_of(K)>.
// ==========================================================================================
// ac: the option loop's AirCells, rebuilt only when the player leaves its window (a jump
// changes cell column or row every ~12 ticks)
template <int K, class R>
TG_HD int air_tick(const Level& L, const uint32_t* trig, const Map& m, Env& e, Opt& o, R& rng,
                   AirCells& ac) {
  constexpr int DIR = (K == O_JUMP_LEFT || K == O_DOWN_LEFT) ? -1 : 1;
  constexpr bool JUMP = K == O_JUMP_LEFT || K == O_JUMP_RIGHT;
  const uint32_t dc = Map::dc_of(e.f);
  if (!ac.holds(dc, e.px, e.py)) {
    ac = m.air_cells(dc, e.px, e.py);
    if (!ac.holds(dc, e.px, e.py)) {  // a clamped window (a player past the border): full tick
      const int prim = policy<K>(L, m, e, o);
      return tick<prims_of(K), R>(L, trig, m, e, prim, rng);
    }
  }
  const AirProbe ap(ac, e.px, e.py);
  const bool cf0 = ap.can_fall();
  const bool fwd = ap.side(DIR);
  int mv = 0;  // the primitive: -1 LEFT, +1 RIGHT, 0 NOP
  if (close_x(e, o.tx)) {
    if (!cf0) o.done = true;
  } else {
    mv = (JUMP && !cf0 && !fwd) ? -DIR : DIR;  // MO/:311-314: back off when blocked on the floor
  }
  int xd = 0, yd = 0;
  // can_go_left / can_go_right (IM/:303-311): forward is fwd; backward only after !fwd, when
  // it is the other side's blockers
  if (mv != 0 && (mv == DIR ? fwd : ap.side(-DIR))) {
    xd = code_step(rng.code(), mv < 0);
    e.f = mv > 0 ? (e.f | F_FACING) : (e.f & ~F_FACING);
  }
  const uint32_t jt = e.f & F_JT;  // IM/:331-337, at the pre-move x
  if (jt > 0) {
    if (ap.up_clear()) yd = -INCR;
    e.f = (e.f & ~F_JT) | (jt - 1);
  } else if (cf0) {
    yd = INCR;
  }
  e.px += xd;
  if (yd > 0) yd = ap.fall(e.px, yd);  // IM/:341-348
  e.py += yd;
  pickups(L, e);
  return -1;  // STEP_REWARD (no JUMP after the first tick)
}

// A ladder option's full tick from the level bitmasks: policy<K> (MO/:168-173, 184-189) and
// tick<prims_of(K)> (IM/:290-359) fused — UP / DOWN when the ladder predicate holds (the tick
// re-tests it at the same state: the same answer), else NOP and done; then the jump ticker /
// gravity, the fall integration and the pickups, as tick<>.  Same outcomes and draws.
template <int DIR, class R>
TG_HD int ladder_tick(const Level& L, const Map& m, const LadMasks& lm, Env& e, Opt& o, R& rng) {
  int yd = 0;
  if (DIR < 0 ? lm.can_go_up(m, e.py) : lm.can_go_down(m, e.py)) yd = code_step(rng.code(), DIR < 0);
  else o.done = true;
  const uint32_t jt = e.f & F_JT;  // IM/:331-337
  if (jt > 0) {
    if (lm.up_clear(m, e.py)) yd = -INCR;
    e.f = (e.f & ~F_JT) | (jt - 1);
  } else if (lm.can_fall(m, e.py)) {
    yd = INCR;
  }
  if (yd > 0) yd = lm.fall_dist(m, e.py, yd);
  e.py += yd;
  pickups(L, e);
  return -1;  // STEP_REWARD
}

// One full tick of an option's while-not-done loop (OP/:28-31), counted: the staged draws
// restocked (rng.reserve: the one refill site of every loop), the tick itself (`full()` runs it
// and yields its reward), then the tick count against TICK_CAP (E_TICKCAP).  Returns whether the
// loop may go on.  rng.phase marks the segments for the diagnostic build's per-phase clock
// (tg_run_diag.h): up to 1 the plain walk, up to 2 the refill, up to 3 the full tick.
// (k_run's register allocation is sensitive to the form of this helper and of span_loop's loop
// condition: with `full` taken by value, or with `if (!counted_tick(..)) break; } while (!o.done)`
// there, the ladder loops took k_run from 92-94 to 109-110 VGPRs, 4 instead of 5 waves per SIMD.
// Compare the kernels' resource usage after an edit here.)
template <class R, class Full>
TG_HD bool counted_tick(Env& e, R& rng, StepResult& r, uint32_t draws, const Full& full) {
  rng.phase(1);
  rng.reserve(draws);
  rng.phase(2);
  r.reward += full();
  rng.phase(3);
  if (++r.ticks < TICK_CAP) return true;
  e.f |= E_TICKCAP;
  return false;
}

// The go and ladder options' loop along one axis (`x`: e.px or e.py).  Two phases per round.
// Plain phase: every lane inside its span (go_plain_limit / ladder_plain_limit) takes plain
// ticks, one draw and x += noisy each, as the full tick there, until it leaves the span.  Full
// phase: then no lane of the wave is in a span, and each takes one full tick, `full(lim)`, which
// yields the tick's reward and, when the option goes on, the next span's limit.  Each lane's own
// tick sequence is the reference's; only the interleaving across lanes differs, and the full
// tick's code runs once per round.  FACE: a run of plain ticks sets the facing bit (go).
// The plain phase is per lane: a lane leaves when its span ends, the wave when all have (a
// ballot-driven loop, with the idle lanes kept inside, made the compiler copy ~26 loop-carried
// registers per iteration and was slower).  It also ends when the staged draws run low: the full
// tick restocks them in rng.reserve, so the plain loop's body holds no refill code.  It is
// rng.walk: multi-draw hops on the device.  (The earlier batched walk, each dword's codes
// applied one by one, took k_run from 82 to 98 VGPRs on the ladders: 4 instead of 5 waves per
// SIMD; with walk_hops k_run stays at 5.)
template <int DIR, bool FACE, class R, class Full>
TG_HD void span_loop(const Level& L, Env& e, int& x, const Opt& o, R& rng, StepResult& r,
                     const Full& full) {
  int lim = DIR > 0 ? -0x40000000 : 0x40000000;  // no plain tick before the first full one
  do {
    rng.phase(0);
    if (const int t = rng.template walk<DIR>(x, lim, TICK_CAP - r.ticks)) {  // plain ticks
      if (FACE) e.f = DIR > 0 ? (e.f | F_FACING) : (e.f & ~F_FACING);
      r.reward -= t;
      r.ticks += t;
      if (DIR > 0 ? x > lim : x < lim) pickups(L, e);  // left the span: as the full tick
      if (r.ticks >= TICK_CAP) {
        e.f |= E_TICKCAP;
        break;
      }
    }
  } while (counted_tick(e, rng, r, TICK_DRAWS, [&]() { return full(lim); }) && !o.done);
}

// the while-not-done loop of _Option.run (OP/:28-31) for option K, whose can_run held
template <int K, class R>
TG_HD void run_option_k(const Level& L, const uint32_t* trig, const Map& m, Env& e, R& rng,
                        StepResult& r) {
  r.ran = 1;
  Opt o{0, false, false};
  const auto policy_tick = [&]() {  // the option's policy and the primitive tick it chose
    const int prim = policy<K>(L, m, e, o);
    return tick<prims_of(K), R>(L, trig, m, e, prim, rng);
  };
  if constexpr (K == O_GO_LEFT || K == O_GO_RIGHT) {
    constexpr int DIR = K == O_GO_LEFT ? -1 : 1;
    span_loop<DIR, true>(L, e, e.px, o, rng, r, [&](int& lim) {
      const int rew = policy_tick();
      if (!o.done) lim = go_plain_limit<DIR>(m, e, o.tx);
      return rew;
    });
  } else if constexpr (K == O_UP_LADDER || K == O_DOWN_LADDER) {
    constexpr int DIR = K == O_UP_LADDER ? -1 : 1;
    if (m.mk) {  // the level bitmasks: full ticks and span limits test bits, no cell probes
      const LadMasks lm(m, Map::dc_of(e.f), e.px);
      span_loop<DIR, false>(L, e, e.py, o, rng, r, [&](int& lim) {
        const int rew = ladder_tick<DIR>(L, m, lm, e, o, rng);
        if (!o.done) lim = ladder_plain_limit<DIR>(m, e, LadProbeMk{m, lm});
        return rew;
      });
    } else {
      span_loop<DIR, false>(L, e, e.py, o, rng, r, [&](int& lim) {
        const int rew = policy_tick();
        if (!o.done) lim = ladder_plain_limit<DIR>(m, e, LadProbe{m, e});
        return rew;
      });
    }
  } else if constexpr (K == O_JUMP_LEFT || K == O_JUMP_RIGHT || K == O_DOWN_LEFT ||
                       K == O_DOWN_RIGHT) {
    AirCells ac{0u, 0u, 0u, 0u, -0x40000000, 0, 0u};  // holds nothing: built on the first air tick
    // the first tick (the jump itself; the drop's target), outside the air ticks' loop
    rng.phase(0);
    if (!counted_tick(e, rng, r, TICK_DRAWS, policy_tick)) return;
    while (!o.done) {
      rng.phase(0);
      if (!counted_tick(e, rng, r, TICK_DRAWS,
                        [&]() { return air_tick<K>(L, trig, m, e, o, rng, ac); }))
        break;
    }
  } else {
    const uint32_t draws = K == O_INTERACT ? L.interact_draws : TICK_DRAWS;
    while (counted_tick(e, rng, r, draws, policy_tick) && !o.done) {  // a round is one full tick
    }
  }
}
template <class R>
TG_HD void run_option(const Level& L, const uint32_t* trig, const Map& m, Env& e, int k,
                      R& rng, StepResult& r) {
  switch (k) {
    case O_GO_LEFT: run_option_k<O_GO_LEFT>(L, trig, m, e, rng, r); break;
    case O_GO_RIGHT: run_option_k<O_GO_RIGHT>(L, trig, m, e, rng, r); break;
    case O_UP_LADDER: run_option_k<O_UP_LADDER>(L, trig, m, e, rng, r); break;
    case O_DOWN_LADDER: run_option_k<O_DOWN_LADDER>(L, trig, m, e, rng, r); break;
    case O_INTERACT: run_option_k<O_INTERACT>(L, trig, m, e, rng, r); break;
    case O_DOWN_LEFT: run_option_k<O_DOWN_LEFT>(L, trig, m, e, rng, r); break;
    case O_DOWN_RIGHT: run_option_k<O_DOWN_RIGHT>(L, trig, m, e, rng, r); break;
    case O_JUMP_LEFT: run_option_k<O_JUMP_LEFT>(L, trig, m, e, rng, r); break;
    default: run_option_k<O_JUMP_RIGHT>(L, trig, m, e, rng, r); break;
  }
}
// option_list[a] (TG/:92): -1 for an out-of-range action (the reference raises IndexError)
TG_HD int option_index(int a) {
  if (a < -O_COUNT || a >= O_COUNT) return -1;
  return a < 0 ? a + O_COUNT : a;  // Python negative indexing
}
template <class R>
TG_HD StepResult env_step(const Level& L, const uint32_t* trig, const Map& m, Env& e, int a,
                          R& rng) {
  StepResult r{0, 0, 0, 0};
  const int k = option_index(a);
  if (k < 0) e.f |= E_ACTION;
  else if (can_run(L, m, e, k)) run_option(L, trig, m, e, k, rng, r);  // OP/:22-23 gate
  r.done = is_done(e);
  return r;
}

}  // namespace tg
