// tg_state.h — one env's state and the level it plays: the game's constants, the primitive actions
// and options, the per-env flag word and error bits, `Level` (the kernel argument), `Env` (the
// registers), the st4 codec (the one place that knows the 16-B state word in HBM) and the integer
// helpers the tick loops share (floordiv, clampi, mul24, div48).  `__host__ __device__`; defines
// TG_HD.  Everything else of the per-env core (tg_core.h) builds on this header; the renderer and
// the handle (tg_render.h, tg_batch.h) need nothing more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TG_HD __host__ __device__ __forceinline__

namespace tg {

constexpr int S = 48;          // xscale == yscale (_scale.py:8-9)
constexpr int INCR = S / 10;   // x_incr / y_incr (IM/:46-47)
constexpr int HALFW = S / 4;   // player_width // 2 (IM/:49)
constexpr int MT_N = 624, MT_M = 397;
constexpr int TICK_CAP = 1 << 14;  // the reference has no cap (OP/:28-31); observed max 105
// random() draws a tick without INTERACT can take (a move or a jump: 1), with margin.  An
// INTERACT tick can take more: each handle flip is 1 draw plus one wiggle per handle change of
// its cascade, and since process_trigger clears previously_triggered on return (OB/:76-94) a
// cascade can change one handle several times.  Its bound depends on the level's trigger
// table: Level::interact_draws (tg_level.h interact_draw_bound), at most MAX_TICK_DRAWS.
constexpr uint32_t TICK_DRAWS = 8;
constexpr uint32_t MAX_TICK_DRAWS = 48;  // what a refilled code window always holds (tg_dev.h)
constexpr int PAD = 2;         // WALL cells around the grid in LDS (probes reach <= 60 px out)

// Cell bits in the LDS grid.  A door object's cell carries only its one-hot door bit: its type
// is 'D' or ' ' by the door's state (update_map overwrites whatever the file had there).
enum : uint32_t { B_OPEN = 1, B_LADDER = 2, B_WALL = 4, B_DOOR = 8, B_DOOROBJ = 16 /* << i */ };
// primitive actions (_actions.py:7-13)
enum : int { P_NOP = 0, P_UP, P_DOWN, P_LEFT, P_RIGHT, P_JUMP, P_INTERACT };
// options in create_options order (IM/:495)
enum : int { O_GO_LEFT = 0, O_GO_RIGHT, O_UP_LADDER, O_DOWN_LADDER, O_INTERACT, O_DOWN_LEFT,
             O_DOWN_RIGHT, O_JUMP_LEFT, O_JUMP_RIGHT, O_COUNT };

// ---- per-env flag word -------------------------------------------------------------------
// interactive object i (0..2 doors, 3..4 handles, 5 bolt) keeps its boolean at bit 6+i:
// door.closed, handle.up, bolt.locked.
constexpr uint32_t F_JT = 0x1Fu;          // jump_ticker (0..23)
constexpr uint32_t F_FACING = 1u << 5;    // facing_right (render only)
constexpr int F_OBJ = 6;                  // first interactive-object bit
constexpr int F_BAGLEN = 12;              // 3 bits: len(player_bag)
constexpr int F_BAGITEM = 15;             // 7 bits: item i is gold (1) or key (0)
constexpr uint32_t E_TICKCAP = 1u << 24;  // option exceeded TICK_CAP
constexpr uint32_t E_BAG = 1u << 25;      // bag overflow (unreachable in the default level)
constexpr uint32_t E_ACTION = 1u << 26;   // action outside [-9, 8] (reference: IndexError)
constexpr uint32_t E_NEARINT = 1u << 27;  // a reset's gauss landed within 1e-9 of an int()
                                          // boundary (device libm vs glibc watch)
constexpr uint32_t E_WINDOW = 1u << 29;   // a lane drew past its staged code window (a bug)
constexpr uint32_t E_MASK = 0xFF000000u;

// ---- level (kernel argument; the grid and the trigger table are staged in LDS) -------------
struct Level {
  int32_t W, H;              // cells (IM/:196-197)
  int32_t start_x, start_y;  // first non-WALL description cell (IM/:173-176)
  int8_t door_cx[3], door_cy[3];
  int8_t handle_cx[2], handle_cy[2];
  int8_t key_cx, key_cy, bolt_cx, bolt_cy, gold_cx, gold_cy;
  uint32_t init_flags;       // door/handle/bolt initial booleans at their F_OBJ bits
  uint32_t trig[6][2];       // trigger lists [object][polarity]: count(4b) + 7 x (target 3b, val 1b)
  uint32_t interact_draws;   // most random() draws one INTERACT tick can take (>= TICK_DRAWS)
  // go_left / go_right can_run and target per (cell, door state, key home?, gold home?)
  // (GoTable; device global memory, built at tg_create; null: computed directly)
  const uint32_t* gotab;
  // the level bitmasks (Map::mk; mk_words(W, H) words, device global memory, staged into LDS
  // by the kernels that use them; null: the level is too large, cell probes)
  const uint32_t* masks;
  // get_state's quotients (observe): obs_q[i] = (double)(Q_MIN + i) / (W * 48) for
  // i < qx_n, then obs_q[qx_n + i] = (double)(Q_MIN + i) / (H * 48) for i < qy_n, each the IEEE
  // quotient the division would give (built on the host, tg_level.h build_obs_q); null: divide
  const double* obs_q;
  int32_t qx_n, qy_n;
};
constexpr int Q_MIN = -2 * S;  // the smallest pixel coordinate the quotient table covers

// ---- per-env state (registers) -------------------------------------------------------------
struct Env {
  int px, py;            // playerx / playery (IM/:42)
  uint32_t f;            // flags above
  int kx, ky, gx, gy;    // key / goldcoin cell (OB/:34-38)
  double ang0, ang1;     // handle angles (OB/:111-114)
  uint32_t mti;          // MT state word: position ([0, MT_WORDS), even) | MT_STALE (see Rng)
};

// ---- the st4 codec ---------------------------------------------------------------------------
// An env's 16-B state word in HBM (Soa::st4, the worklist copies, tg_read_state / tg_write_state):
//   x = px | py << 16 (i16 pair), y = the flag word, z = kx, ky, gx, gy (i8 x 4), w = mti.
// The only code that knows the layout; st4_flags reads the flag word alone (one dword load).
TG_HD void unpack_st4(const uint4 s, Env& e) {
  e.px = (int)(int16_t)(s.x & 0xFFFFu);
  e.py = (int)(int16_t)(s.x >> 16);
  e.f = s.y;
  e.kx = (int)(int8_t)(s.z & 0xFF);
  e.ky = (int)(int8_t)((s.z >> 8) & 0xFF);
  e.gx = (int)(int8_t)((s.z >> 16) & 0xFF);
  e.gy = (int)(int8_t)(s.z >> 24);
  e.mti = s.w;
}
TG_HD void unpack(const uint4 s, const double2 a, Env& e) {
  unpack_st4(s, e);
  e.ang0 = a.x;
  e.ang1 = a.y;
}
TG_HD uint4 pack(const Env& e) {
  uint4 s;
  s.x = ((uint32_t)e.px & 0xFFFFu) | ((uint32_t)e.py << 16);
  s.y = e.f;
  s.z = ((uint32_t)e.kx & 0xFF) | (((uint32_t)e.ky & 0xFF) << 8) | (((uint32_t)e.gx & 0xFF) << 16) |
        ((uint32_t)e.gy << 24);
  s.w = e.mti;
  return s;
}
TG_HD uint32_t st4_flags(const uint4& s) { return s.y; }

TG_HD int floordiv(int a, int b) {  // Python // for b > 0
  int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
TG_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Pixel -> cell in the tick loops.  A 32-bit division by the constant 48 compiles to 32-bit
// magic-number multiplies (v_mul_hi_u32 / v_mul_lo_u32, slower VALU); 24-bit operands take
// the full-rate v_mul_u32_u24 instead.  v * 21846 >> 20 equals v / 48 for 0 <= v < 32,700
// (21846 / 2^20 - 1/48 = 6.4e-7; 6.4e-7 * 32,700 < 1/48) — levels are at most 124 cells
// (5,952 px) per side with the border.
static_assert(S == 48, "div48 constants");
TG_HD uint32_t mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(TG_NO_MUL24)
  return __umul24(a, b);
#else
  return a * b;
#endif
}
TG_HD int div48(int v) { return (int)(mul24((uint32_t)v, 21846u) >> 20); }  // 0 <= v < 32,700
TG_HD int floordiv48(int a) { return div48(a + 16 * S) - 16; }              // -768 <= a < 31,900

}  // namespace tg
