// tg_rules.h — the game's rules on one env: objects, bag and the trigger cascade, the primitive
// tick (`tick<PM>`), the options' can_run (with the GoTable lookup), available_mask, the synthetic
// policies' action (policy_action), policy<K>, observe, is_done and the two resets.  `__host__
// __device__`; the draws come through a template parameter (tg::Rng, or tg_dev.h's RngCodesT).
#pragma once
#include "../../include/tg_amd.h"
#include "tg_hash.h"
#include "tg_map.h"
#include "tg_mt.h"

namespace tg {

// ==========================================================================================
// Objects, bag, triggers (OB/, IM/:402-445)
// ==========================================================================================
// near_enough (OB/:46-53) for the player probe (px, py + 24): centre (cx*48+24, cy*48+24)
TG_HD bool near_cell(const Env& e, int cx, int cy, int r2) {
  const int dx = e.px - (cx * S + S / 2);
  const int dy = e.py - cy * S;
  return dx * dx + dy * dy < r2;
}
constexpr int R2_OBJ = (S / 2) * (S / 2);            // radius xscale/2 (OB/:23)
constexpr int R2_HANDLE = (S * 3 / 4) * (S * 3 / 4);  // radius xscale*0.75 (OB/:115)

TG_HD int bag_len(uint32_t f) { return (f >> F_BAGLEN) & 7; }
TG_HD uint32_t bag_items(uint32_t f) { return (f >> F_BAGITEM) & 0x7F; }
TG_HD bool got_key(uint32_t f) {   // player_got_key (IM/:418-422)
  const uint32_t live = (1u << bag_len(f)) - 1u;
  return (~bag_items(f) & live) != 0;
}
TG_HD bool got_gold(uint32_t f) {  // player_got_goldcoin (IM/:424-428)
  const uint32_t live = (1u << bag_len(f)) - 1u;
  return (bag_items(f) & live) != 0;
}
TG_HD void bag_push(uint32_t& f, bool gold) {
  const int n = bag_len(f);
  if (n >= 7) { f |= E_BAG; return; }
  f = (f & ~(7u << F_BAGLEN)) | ((uint32_t)(n + 1) << F_BAGLEN);
  if (gold) f |= 1u << (F_BAGITEM + n);
}
// drop_key (IM/:434-439): remove the first key, move it to (-1,-1)
TG_HD void drop_key(Env& e) {
  const int n = bag_len(e.f);
  const uint32_t items = bag_items(e.f);
  const uint32_t keys = ~items & ((1u << n) - 1u);
  if (!keys) return;
  const int i = __builtin_ctz(keys);
  const uint32_t lo = items & ((1u << i) - 1u), hi = (items >> (i + 1)) << i;
  e.f = (e.f & ~((7u << F_BAGLEN) | (0x7Fu << F_BAGITEM))) | ((uint32_t)(n - 1) << F_BAGLEN) |
        ((lo | hi) << F_BAGITEM);
  e.kx = -1;
  e.ky = -1;
}

// is_object_at (IM/:402-409): handles, closed doors, bolt, gold, key at the cell
TG_HD bool is_object_at(const Level& L, const Env& e, int xc, int yc) {
  bool r = ((xc == L.handle_cx[0]) & (yc == L.handle_cy[0])) |
           ((xc == L.handle_cx[1]) & (yc == L.handle_cy[1])) |
           ((xc == L.bolt_cx) & (yc == L.bolt_cy)) | ((xc == e.gx) & (yc == e.gy)) |
           ((xc == e.kx) & (yc == e.ky));
#pragma unroll
  for (int i = 0; i < 3; ++i)
    r |= (xc == L.door_cx[i]) & (yc == L.door_cy[i]) & (((e.f >> (F_OBJ + i)) & 1u) != 0);
  return r;
}
// is_closed_door_at (IM/:411-416)
TG_HD bool is_closed_door_at(const Level& L, const Env& e, int xc, int yc) {
  bool r = false;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    r |= (xc == L.door_cx[i]) & (yc == L.door_cy[i]) & (((e.f >> (F_OBJ + i)) & 1u) != 0);
  return r;
}

// handle.set_angle_wiggle (OB/:127-131)
template <class R>
TG_HD void wiggle(Env& e, int h, R& rng) {
  const bool up = (e.f >> (F_OBJ + 3 + h)) & 1u;
  const double a = up ? rng.uniform(0.85, 1.0) : rng.uniform(0, 0.15);
  if (h == 0) e.ang0 = a; else e.ang1 = a;
}
// set_val of door (OB/:231-235) / handle (OB/:145-149) / bolt (OB/:175-178): apply only
template <class R>
TG_HD bool set_val(Env& e, int o, int v, R& rng) {
  const uint32_t bit = 1u << (F_OBJ + o);
  if ((((e.f & bit) != 0) ? 1 : 0) == v) return false;
  e.f ^= bit;
  if (o == 3 || o == 4) wiggle(e, o - 3, rng);
  return true;
}
// set_val(o0, v0) followed by the process_trigger cascade (OB/:76-94), depth-first in file
// order with the previously_triggered guard; frames are 8 bits of one u64.  `trig` is the
// level's [6][2] trigger table (LDS on device).
template <class R>
TG_HD void cascade(const uint32_t* trig, Env& e, int o0, int v0, R& rng) {
  if (!set_val(e, o0, v0, rng)) return;
  uint64_t stack = (uint64_t)(o0 | (v0 << 3));
  uint32_t prev = 1u << o0;
  int depth = 1;
  while (depth > 0) {
    const uint32_t fr = (uint32_t)(stack & 0xFFu);
    const int o = fr & 7, v = (fr >> 3) & 1, ei = fr >> 4;
    const uint32_t list = trig[o * 2 + v];
    if (ei < (int)(list & 0xFu)) {
      stack += 0x10u;
      const uint32_t edge = (list >> (4 + 4 * ei)) & 0xFu;
      const int t = edge & 7, tv = (edge >> 3) & 1;
      if (!(prev & (1u << t)) && set_val(e, t, tv, rng)) {
        stack = (stack << 8) | (uint64_t)(t | (tv << 3));
        prev |= 1u << t;
        ++depth;
      }
    } else {
      stack >>= 8;
      prev &= ~(1u << o);
      --depth;
    }
  }
}
// handle.flip (OB/:117-122): uniform(0, 1) <= 0.8 (== random() exactly: CODE_FLIP)
template <class R>
TG_HD void flip(const uint32_t* trig, Env& e, int h, R& rng) {
  if (rng.code() & CODE_FLIP) {
    const int up = (e.f >> (F_OBJ + 3 + h)) & 1u;
    cascade(trig, e, 3 + h, !up, rng);
  } else {
    wiggle(e, h, rng);
  }
}

// pickups in object order: key then goldcoin (IM/:350-354).  near_cell needs |dx| < 24 for
// r = 24, so a tick whose player is 24 px or more from both objects' centres in x (nearly every
// tick) skips the rest with one combined test.
TG_HD void pickups(const Level& L, Env& e) {
  const int dkx = e.px - (e.kx * S + S / 2), dgx = e.px - (e.gx * S + S / 2);
  if (((uint32_t)(dkx + (S / 2 - 1)) >= (uint32_t)(S - 1)) & ((uint32_t)(dgx + (S / 2 - 1)) >= (uint32_t)(S - 1)))
    return;
  if (near_cell(e, e.kx, e.ky, R2_OBJ)) {
    e.kx = L.W - 1 - bag_len(e.f);
    e.ky = L.H - 1;
    bag_push(e.f, false);
  }
  if (near_cell(e, e.gx, e.gy, R2_OBJ)) {
    e.gx = L.W - 1 - bag_len(e.f);
    e.gy = L.H - 1;
    bag_push(e.f, true);
  }
}

// ==========================================================================================
// Primitive tick: _TreasureGameImpl.step (IM/:290-359).  PM is the set of primitive actions
// the caller can issue (a compile-time mask); the others compile away.
// ==========================================================================================
constexpr uint32_t PM_ALL = 0x7Fu;
template <uint32_t PM>
TG_HD bool may(int prim, int p) { return ((PM >> p) & 1u) && prim == p; }

template <uint32_t PM, class R>
TG_HD int tick(const Level& L, const uint32_t* trig, const Map& m, Env& e, int prim, R& rng) {
  int xd = 0, yd = 0;
  // the action's precondition (IM/:297-319); moves and the jump share one draw site
  bool ok = false;
  if (may<PM>(prim, P_UP)) ok = m.can_go_up(e);
  else if (may<PM>(prim, P_DOWN)) ok = m.can_go_down(e);
  else if (may<PM>(prim, P_LEFT)) ok = m.can_go_side(e, -1);
  else if (may<PM>(prim, P_RIGHT)) ok = m.can_go_side(e, +1);
  else if (may<PM>(prim, P_JUMP)) ok = !m.can_go_down(e) && m.up_clear(e);
  if (ok) {
    const uint32_t c = rng.code();
    if (may<PM>(prim, P_JUMP)) {  // jump_ticker = 22, or 23 if random() > 0.25 (IM/:317-319)
      e.f = (e.f & ~F_JT) | ((c & CODE_JUMP) ? 23u : 22u);
    } else {
      // noisy(+-4) (IM/:361-366): int(round(uniform(-4, -2.0))) or int(round(uniform(2.0, 4))),
      // uniform = a + (b-a)*r with b-a = 2.0 exactly; round() half-to-even == rint (draw_code)
      const bool neg = may<PM>(prim, P_UP) | may<PM>(prim, P_LEFT);
      const int d = code_step(c, neg);
      if (may<PM>(prim, P_LEFT) | may<PM>(prim, P_RIGHT)) {
        xd = d;
        e.f = may<PM>(prim, P_RIGHT) ? (e.f | F_FACING) : (e.f & ~F_FACING);
      } else {
        yd = d;
      }
    }
  }
  if (may<PM>(prim, P_INTERACT)) {  // object list order: handles (3,4) before the bolt (6)
    if (near_cell(e, L.handle_cx[0], L.handle_cy[0], R2_HANDLE)) flip(trig, e, 0, rng);
    if (near_cell(e, L.handle_cx[1], L.handle_cy[1], R2_HANDLE)) flip(trig, e, 1, rng);
    if (near_cell(e, L.bolt_cx, L.bolt_cy, R2_OBJ) && got_key(e.f)) {
      cascade(trig, e, 5, 0, rng);  // try_unlock -> bolt.unlock (IM/:430-432)
      drop_key(e);
    }
  }
  // jump ticker / gravity (IM/:331-337), both at the pre-move x
  const uint32_t jt = e.f & F_JT;
  if (jt > 0) {
    if (m.up_clear(e)) yd = -INCR;
    e.f = (e.f & ~F_JT) | (jt - 1);
  } else if (m.can_fall(e)) {
    yd = INCR;  // jump_ticker already 0
  }
  e.px += xd;
  // integrate y (IM/:341-348): with yd > 0 and can_fall, fall pixel by pixel while can_fall
  // holds: the distance is the first k in 1..yd-1 with !can_fall(py + k), else yd (yd <= 4)
  if (yd > 0) yd = m.fall(Map::dc_of(e.f), e.px, e.py, yd);
  e.py += yd;
  pickups(L, e);
  return may<PM>(prim, P_JUMP) ? -5 : -1;  // JUMP_REWARD / STEP_REWARD (IM/:15-16)
}

// ==========================================================================================
// Options (MO/)
// ==========================================================================================
TG_HD void player_cell(const Env& e, int& xc, int& yc) {  // IM/:441-445
  xc = floordiv48(e.px);  // floordiv(px, S); players stay inside the level
  yc = floordiv48(e.py + S / 2);
}
// close_enough_to / close_enough_x: |tx*48 + 24 - px| < 4 (MO/:69-72 and its copies)
TG_HD bool close_x(const Env& e, int txc) {
  const int d = txc * S + S / 2 - e.px;
  return (d < 0 ? -d : d) < INCR;
}
// go_left / go_right is_target_cell (MO/:54-67, 126-139)
TG_HD bool go_is_target(const Level& L, const Map& m, const Env& e, int dir, int xc, int yc) {
  const uint32_t dc = Map::dc_of(e.f);
  const uint32_t up = m.cellb(xc, yc - 1), dn = m.cellb(xc, yc + 1), sd = m.cellb(xc + dir, yc),
                 sdn = m.cellb(xc + dir, yc + 1);
  return Map::is_ladder(up | dn) | Map::is_wall(sd) | is_object_at(L, e, xc, yc) |
         is_closed_door_at(L, e, xc + dir, yc) | Map::is_open(sdn, dc);
}
// get_target_cell (MO/:43-52; MO/:115-124 whose xc<0 test can never fire going right, and
// terminates because OOB is WALL)
TG_HD bool go_target(const Level& L, const Map& m, const Env& e, int dir, int xc, int yc, int& tx) {
  int x = xc + dir;
  while (!go_is_target(L, m, e, dir, x, yc)) {
    x += dir;
    if (x < 0) return false;
  }
  tx = x;
  return true;
}
// jump landing (MO/:281-287)
TG_HD bool landing(const Map& m, const Env& e, int xc, int yc) {
  return m.open_cell(Map::dc_of(e.f), xc, yc) & Map::is_wall(m.cellb(xc, yc + 1));
}

// ---- GoTable: the go options' can_run and target, precomputed --------------------------------
// go_left / go_right's can_run (MO/:23-41, 95-113) and target (MO/:43-67, 115-139) read only
// the player's cell (xc, yc), cell types of rows yc - 1 .. yc + 1, the door states and, through
// is_object_at (IM/:402-409), the key's and the gold's cells on row yc.  The key is at home, in
// the bag (row H - 1) or at (-1, -1); the gold at home or in the bag.  So for a player cell
// inside the grid whose row holds neither a moved key nor a bagged gold (row H - 1 is a wall
// in every playable level), the answer depends on (cell, door state, key at home, gold at
// home) only: entry ((yc * W + xc) * 8 + doors) * 4 + key_home * 2 + gold_home holds
// bit 0 / 1 = can_run left / right, bits 8-15 / 16-23 = target column + 1.
TG_HD bool go_lookup(const Level& L, const Env& e, int xc, int yc, uint32_t& out) {
  if (!L.gotab || xc < 0 || xc >= L.W || yc < 0 || yc >= L.H) return false;
  const bool kh = e.kx == L.key_cx && e.ky == L.key_cy, gh = e.gx == L.gold_cx && e.gy == L.gold_cy;
  if ((!kh && e.ky == yc) || (!gh && e.gy == yc)) return false;
  out = L.gotab[((yc * L.W + xc) * 8 + (int)Map::dc_of(e.f)) * 4 + (kh ? 2 : 0) + (gh ? 1 : 0)];
  return true;
}
TG_HD bool can_run(const Level& L, const Map& m, const Env& e, int k) {
  int xc, yc;
  player_cell(e, xc, yc);
  const uint32_t dc = Map::dc_of(e.f);
  switch (k) {
    case O_GO_LEFT:
    case O_GO_RIGHT: {  // MO/:23-41, 95-113
      const int dir = k == O_GO_LEFT ? -1 : 1;
      uint32_t gt;
      if (go_lookup(L, e, xc, yc, gt)) return (gt >> (k == O_GO_LEFT ? 0 : 1)) & 1u;
      int tc;
      if (!go_target(L, m, e, dir, xc, yc, tc)) return false;
      for (int x = xc; dir < 0 ? x >= tc : x <= tc; x += dir) {
        if (!m.open_cell(dc, x, yc)) return false;
        if (m.open_cell(dc, x, yc + 1)) return false;
      }
      return true;
    }
    case O_UP_LADDER: return m.can_go_up(e);      // MO/:165-166
    case O_DOWN_LADDER: return m.can_go_down(e);  // MO/:181-182
    case O_INTERACT:                              // MO/:446-455
      return near_cell(e, L.handle_cx[0], L.handle_cy[0], R2_HANDLE) ||
             near_cell(e, L.handle_cx[1], L.handle_cy[1], R2_HANDLE) ||
             (near_cell(e, L.bolt_cx, L.bolt_cy, R2_OBJ) && got_key(e.f));
    case O_DOWN_LEFT:
    case O_DOWN_RIGHT: {  // MO/:199-209, 394-404
      const int dir = k == O_DOWN_LEFT ? -1 : 1;
      return m.open_cell(dc, xc + dir, yc) & m.open_cell(dc, xc + dir, yc + 1);
    }
    case O_JUMP_LEFT:
    case O_JUMP_RIGHT: {  // MO/:254-267, 324-337
      const int dir = k == O_JUMP_LEFT ? -1 : 1;
      return m.open_cell(dc, xc, yc - 1) & m.open_cell(dc, xc + dir, yc - 1) &
             (landing(m, e, xc + dir, yc - 1) | landing(m, e, xc + 2 * dir, yc - 1));
    }
  }
  return false;
}

TG_HD uint32_t available_mask(const Level& L, const Map& m, const Env& e) {  // TG/:83-89
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < O_COUNT; ++k) r |= (uint32_t)can_run(L, m, e, k) << k;
  return r;
}

// the synthetic policies (tg_policy_actions): a[t, g] = h(a0, g, t) % 9, or the k-th set bit
// of available_mask with k = h % popcount (masked-uniform; h % 9 when nothing can run).  The one
// copy: the kernels' (step_env, classify_env) and the host replay's (tests/native/host_env.h)
TG_HD int policy_action(const Level& L, const Map& m, const Env& e, int policy, uint64_t a0,
                        int64_t g, int64_t t) {
  const uint64_t h = sm64(sm64(a0 ^ sm64((uint64_t)g)) ^ (uint64_t)t);
  int a = (int)(h % 9ull);
  if (policy == TG_POLICY_MASKED) {
    const uint32_t mk = available_mask(L, m, e);
    const int c = __builtin_popcount(mk);  // (__popc / __ffs, spelled as HIP defines them)
    if (c) {
      uint32_t k = (uint32_t)(h % (uint64_t)c);
      uint32_t mm = mk;
      while (k--) mm &= mm - 1u;
      a = (mm == 0 ? -1 : __builtin_ctz(mm)) + 1 - 1;
    }
  }
  return a;
}

// option-local state (start_cell / target_cell are None between steps, MO/:80-83 etc.)
struct Opt {
  int tx;      // target cell x
  bool init;   // target computed
  bool done;
};

// primitive actions each option's policy can return
constexpr uint32_t prims_of(int k) {
  return k == O_GO_LEFT ? (1u << P_LEFT)
       : k == O_GO_RIGHT ? (1u << P_RIGHT)
       : k == O_UP_LADDER ? (1u << P_UP) | (1u << P_NOP)
       : k == O_DOWN_LADDER ? (1u << P_DOWN) | (1u << P_NOP)
       : k == O_INTERACT ? (1u << P_INTERACT)
       : k == O_DOWN_LEFT ? (1u << P_LEFT) | (1u << P_NOP)
       : k == O_DOWN_RIGHT ? (1u << P_RIGHT) | (1u << P_NOP)
       : (1u << P_JUMP) | (1u << P_LEFT) | (1u << P_RIGHT) | (1u << P_NOP);
}

// policy_step of option K (MO/)
template <int K>
TG_HD int policy(const Level& L, const Map& m, const Env& e, Opt& o) {
  int xc, yc;
  if (K == O_GO_LEFT || K == O_GO_RIGHT) {  // MO/:74-85, 146-157
    constexpr int dir = K == O_GO_LEFT ? -1 : 1;
    if (!o.init) {
      player_cell(e, xc, yc);
      uint32_t gt;
      if (go_lookup(L, e, xc, yc, gt)) o.tx = (int)((gt >> (dir < 0 ? 8 : 16)) & 0xFFu) - 1;
      else go_target(L, m, e, dir, xc, yc, o.tx);  // exists: can_run checked it
      o.init = true;
    }
    if (close_x(e, o.tx)) o.done = true;
    return dir < 0 ? P_LEFT : P_RIGHT;
  } else if (K == O_UP_LADDER) {  // MO/:168-173
    if (!m.can_go_up(e)) { o.done = true; return P_NOP; }
    return P_UP;
  } else if (K == O_DOWN_LADDER) {  // MO/:184-189
    if (!m.can_go_down(e)) { o.done = true; return P_NOP; }
    return P_DOWN;
  } else if (K == O_INTERACT) {  // MO/:457-460
    o.done = true;
    return P_INTERACT;
  } else if (K == O_DOWN_LEFT || K == O_DOWN_RIGHT) {  // MO/:231-244, 426-439
    constexpr int dir = K == O_DOWN_LEFT ? -1 : 1;
    if (!o.init) {
      // get_target_cell (MO/:211-221, 406-416) scans down column xc+dir for the first
      // non-open cell; only its x is ever used (close_enough_x).  It returns None only if
      // the scan leaves the grid, after which the reference raises TypeError; the bottom
      // row of a walled level never lets that happen.
      player_cell(e, xc, yc);
      o.tx = xc + dir;
      o.init = true;
    }
    if (close_x(e, o.tx)) {
      if (!m.can_fall(e)) o.done = true;
      return P_NOP;
    }
    return dir < 0 ? P_LEFT : P_RIGHT;
  } else {  // O_JUMP_LEFT / O_JUMP_RIGHT (MO/:297-314, 367-384)
    constexpr int dir = K == O_JUMP_LEFT ? -1 : 1;
    if (!o.init) {
      player_cell(e, xc, yc);
      o.tx = landing(m, e, xc + dir, yc - 1) ? xc + dir : xc + 2 * dir;  // MO/:269-279
      o.init = true;
      return P_JUMP;
    }
    if (close_x(e, o.tx)) {
      if (!m.can_fall(e)) o.done = true;
      return P_NOP;
    }
    const bool back = !m.can_fall(e) && !m.can_go_side(e, dir);
    return (back ? -dir : dir) < 0 ? P_LEFT : P_RIGHT;
  }
}

// ==========================================================================================
// Observation (IM/:368-378 + OB/:157-158,186-190,202-203,215-216) and done (TG/:95)
// ==========================================================================================
// v / d, from the level's quotient table when v is inside it (the table holds the same IEEE
// quotients: an f64 division is ~11 VALU instructions on the device, the reciprocal among them)
TG_HD double obs_div(const Level& L, int v, int base, int n, double d) {
  const uint32_t i = (uint32_t)(v - Q_MIN);
  return (L.obs_q && i < (uint32_t)n) ? L.obs_q[base + (int)i] : (double)v / d;
}
TG_HD void observe(const Level& L, const Env& e, double o[9]) {
  const double w = (double)(L.W * S), h = (double)(L.H * S);
  o[0] = obs_div(L, e.px, 0, L.qx_n, w);
  o[1] = obs_div(L, e.py, L.qx_n, L.qy_n, h);
  o[2] = e.ang0;
  o[3] = e.ang1;
  o[4] = obs_div(L, e.kx * S, 0, L.qx_n, w);
  o[5] = obs_div(L, e.ky * S, L.qx_n, L.qy_n, h);
  o[6] = ((e.f >> (F_OBJ + 5)) & 1u) ? 1.0 : 0.0;
  o[7] = obs_div(L, e.gx * S, 0, L.qx_n, w);
  o[8] = obs_div(L, e.gy * S, L.qx_n, L.qy_n, h);
}
TG_HD bool is_done(const Env& e) {
  int xc, yc;
  player_cell(e, xc, yc);
  return got_gold(e.f) && yc == 0;
}

// ==========================================================================================
// reset_game (IM/:55-73): objects re-read (handle angles, 2 draws), start position (gauss
// pair, 2 draws), empty bag.  Keeps the error bits.
// ==========================================================================================
template <class R>
TG_HD void reset_env(const Level& L, Env& e, R& rng) {
  rng.reserve(4);
  e.f = (e.f & E_MASK) | L.init_flags | F_FACING;
  e.ang0 = ((L.init_flags >> (F_OBJ + 3)) & 1u) ? rng.uniform(0.85, 1.0) : rng.uniform(0, 0.15);
  e.ang1 = ((L.init_flags >> (F_OBJ + 4)) & 1u) ? rng.uniform(0.85, 1.0) : rng.uniform(0, 0.15);
  e.kx = L.key_cx;
  e.ky = L.key_cy;
  e.gx = L.gold_cx;
  e.gy = L.gold_cy;
  // player_initial_position (IM/:168-178) with Random.gauss's pair (gauss_next consumed)
  const double x2pi = rng.random() * (2.0 * 3.141592653589793);
  const double g2rad = sqrt(-2.0 * log(1.0 - rng.random()));
  const double zx = 0.0 + (cos(x2pi) * g2rad) * (S / 24.0);
  const double zy = fabs(0.0 + (sin(x2pi) * g2rad) * (S / 36.0));
  const double fx = fabs(zx) - floor(fabs(zx)), fy = zy - floor(zy);
  if ((fabs(zx) >= 0.5 && (fx < 1e-9 || fx > 1.0 - 1e-9)) || (zy >= 0.5 && (fy < 1e-9 || fy > 1.0 - 1e-9)))
    e.f |= E_NEARINT;
  e.px = L.start_x * S + S / 2 + (int)zx;
  e.py = L.start_y * S + (int)zy;
}

// Random.gauss's cached second value (CPython random.py gauss: gauss_next), for an env that
// draws from a shared Python-level stream (the N=1 drop-in's default, tg_reset1_py)
struct GaussNext {
  bool has;
  double v;
};
// z of Random.gauss (the caller applies mu + z * sigma): the cached value if there is one,
// else a fresh pair (2 draws) whose second value is cached
template <class R>
TG_HD double gauss_z(R& rng, GaussNext& g) {
  if (g.has) {
    g.has = false;
    return g.v;
  }
  const double x2pi = rng.random() * (2.0 * 3.141592653589793);
  const double g2rad = sqrt(-2.0 * log(1.0 - rng.random()));
  g.v = sin(x2pi) * g2rad;
  g.has = true;
  return cos(x2pi) * g2rad;
}
// reset_env with the stream's gauss_next carried in and out (reset_env assumes it unset, as
// after random.seed, and leaves it unset: the two gauss calls consume one pair)
template <class R>
TG_HD void reset_env_gauss(const Level& L, Env& e, R& rng, GaussNext& g) {
  e.f = (e.f & E_MASK) | L.init_flags | F_FACING;
  e.ang0 = ((L.init_flags >> (F_OBJ + 3)) & 1u) ? rng.uniform(0.85, 1.0) : rng.uniform(0, 0.15);
  e.ang1 = ((L.init_flags >> (F_OBJ + 4)) & 1u) ? rng.uniform(0.85, 1.0) : rng.uniform(0, 0.15);
  e.kx = L.key_cx;
  e.ky = L.key_cy;
  e.gx = L.gold_cx;
  e.gy = L.gold_cy;
  const double zx = 0.0 + gauss_z(rng, g) * (S / 24.0);
  const double zy = fabs(0.0 + gauss_z(rng, g) * (S / 36.0));
  const double fx = fabs(zx) - floor(fabs(zx)), fy = zy - floor(zy);
  if ((fabs(zx) >= 0.5 && (fx < 1e-9 || fx > 1.0 - 1e-9)) || (zy >= 0.5 && (fy < 1e-9 || fy > 1.0 - 1e-9)))
    e.f |= E_NEARINT;
  e.px = L.start_x * S + S / 2 + (int)zx;
  e.py = L.start_y * S + (int)zy;
}

}  // namespace tg
