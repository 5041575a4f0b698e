// tg_walk.h — the plain phases' walk along one axis over staged draw codes: walk_ticks (the
// specification, one tick per draw), the multi-draw hops that take it several ticks at a time
// (hop_prefix, hop_dist, hop_ticks, walk_hops), and the index arithmetic of a rolling code window
// (ring_*; no kernel uses it now).  `__host__ __device__`; needs the draw codes and the ring's
// sizes (tg_mt.h) and nothing of the map or the rules (tests/native_walk builds it alone).
#pragma once
#include "tg_mt.h"

namespace tg {

// Plain ticks of a walk along one axis (the go / ladder loops' plain phases, run_option_k):
// while the coordinate x is inside its span (x <= lim moving in +, x >= lim moving in -), at
// least TICK_DRAWS draws are staged (rng.has) and fewer than `cap` ticks were taken, one draw
// moves x by its noisy step (IM/:361-366: +2..+4 or -4..-2).  Returns the ticks taken.  The
// device's RngCodes takes them by multi-draw hops (walk_hops below), with the same result.
template <int DIR, class R>
TG_HD int walk_ticks(R& rng, int& x, int lim, int cap) {
  int t = 0;
  while ((DIR > 0 ? x <= lim : x >= lim) && rng.has(TICK_DRAWS) && t < cap) {
    x += code_step(rng.code(), DIR < 0);
    ++t;
  }
  return t;
}

// Multi-draw hops of the plain phases: walk_ticks several ticks per step, from the staged code
// bytes themselves.  A tick's step is 2 + (c & CODE_POS) moving in + and the CODE_NEG_SHIFT
// field - 4 moving in -, so every step has the walk's sign and the distance covered grows with
// each tick.  hop_prefix sums a code dword's step fields by SWAR: byte j of the product is
// f_0 + .. + f_j (each field <= 3: no carry between bytes); hop_dist is the distance the first
// j ticks (0..4) of that dword cover.
TG_HD uint32_t hop_prefix(uint32_t w, bool neg) {
  return ((neg ? w >> CODE_NEG_SHIFT : w) & 0x03030303u) * 0x01010101u;
}
TG_HD int hop_dist(uint32_t p, int j, bool neg) {
  const int s = j ? (int)((p >> (8 * (j - 1))) & 0xFFu) : 0;
  return neg ? 4 * j - s : 2 * j + s;
}
// The hop: w holds the next m (1..4) staged codes from byte 0.  The distances are monotone, so
// all m ticks are plain (walk_ticks would take every one of them) exactly when the last of them
// still starts inside the span (x plus the first m - 1 steps), with TICK_DRAWS draws staged
// (left - (m - 1)) and under the cap (taken + m - 1).  Then x moves by all m steps at once and
// the caller advances its position by m; otherwise nothing changes and the walk ends inside
// these m codes, tick by tick.
template <int DIR>
TG_HD bool hop_ticks(uint32_t w, int m, int& x, int lim, uint32_t left, int taken, int cap) {
  const uint32_t p = hop_prefix(w, DIR < 0);
  const int d = DIR > 0 ? lim - x : x - lim;  // >= 0 inside the span
  if (!(hop_dist(p, m - 1, DIR < 0) <= d && left >= TICK_DRAWS + (uint32_t)(m - 1) &&
        taken + m - 1 < cap))
    return false;
  x += DIR * hop_dist(p, m, DIR < 0);
  return true;
}
// walk_ticks over a window of staged codes (the device's RngCodes, tg_dev.h; a flat array in
// tests/native_walk): win.rd is the next draw's index, win.left the draws staged from there,
// win.dword(i) the codes 4i .. 4i + 3 (read only where at least one of them is staged).
// A hop to the dword boundary, whole dwords while they are plain, then the last dword tick by
// tick; win.rd and win.left advance by the ticks taken, which are returned.
template <int DIR, class W>
TG_HD int walk_hops(W& win, int& x, int lim, int cap) {
  int taken = 0;
  bool whole = true;
  if (const int k = (int)(win.rd & 3u)) {
    const int m = 4 - k;
    whole = (DIR > 0 ? x <= lim : x >= lim) && win.left >= TICK_DRAWS &&
            hop_ticks<DIR>(win.dword(win.rd >> 2) >> (8 * k), m, x, lim, win.left, 0, cap);
    if (whole) taken = m, win.rd += (uint32_t)m, win.left -= (uint32_t)m;
  }
  if (whole) {
    // whole dwords, on the distance left in the span; the cap folded into the bound on left
    // (taken + 3 < cap), the next dword read while this one is tested
    int d = DIR > 0 ? lim - x : x - lim;  // < 0 outside the span: then nothing is read
    const int room = cap - 3 - taken;  // whole dwords while 4 * (dwords taken) < room
    uint32_t i = win.rd >> 2, left = win.left;
    const uint32_t left0 = left;
    const bool in = d >= 0;
    uint32_t w = in && left >= TICK_DRAWS + 3u ? win.dword(i) : 0u;
    while (in && left >= TICK_DRAWS + 3u && (int)(left0 - left) < room) {
      const uint32_t wn = win.dword(i + 1u);  // staged: left >= TICK_DRAWS here
      const uint32_t p = hop_prefix(w, DIR < 0);
      if (hop_dist(p, 3, DIR < 0) > d) break;
      d -= hop_dist(p, 4, DIR < 0);
      ++i;
      left -= 4u;
      w = wn;
    }
    x = DIR > 0 ? lim - d : lim + d;
    taken += (int)(left0 - left);
    win.rd = 4u * i;
    win.left = left;
  }
  // the dword the walk ends in: each tick checks the span, the staged draws and the cap at its
  // start, as walk_ticks
  if ((DIR > 0 ? x <= lim : x >= lim) && win.left >= TICK_DRAWS && taken < cap) {
    const uint32_t w = win.dword(win.rd >> 2);
    const int k = (int)(win.rd & 3u);
    int moved = 0;
    bool act = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int st = code_step((w >> (8 * i)) & 0xFFu, DIR < 0);
      act = act && (i >= k ? ((DIR > 0 ? x <= lim : x >= lim) &&
                              win.left - (uint32_t)moved >= TICK_DRAWS && taken + moved < cap)
                           : true);
      if (i >= k && act) {
        x += st;
        ++moved;
      }
    }
    taken += moved;
    win.rd += (uint32_t)moved;
    win.left -= (uint32_t)moved;
  }
  return taken;
}

// Index arithmetic of a rolling code window: the window of the device's RngCodes (tg_dev.h)
// refilled as a ring, unit by unit, instead of all at once.  No kernel uses it now: the form
// built on it measured slower than the blocking refill, and its device path was
// taken out again; these functions and their simulation over a flat code array
// (tests/native_walk, tests/test_walk_host.py) stay for the next form.  A lane's window is a
// ring of RING_SLOTS slots of RING_UNIT codes; rd counts the draws read since the last blocking
// fill plus the first one's offset in its unit (so rd % RING_UNIT is the offset in the unit),
// `staged` the draws staged from rd on, landed or in flight: they always end at a unit's end.
constexpr uint32_t RING_UNIT = 16, RING_SLOTS = 4, RING_DRAWS = RING_UNIT * RING_SLOTS;
constexpr uint32_t RING_UNITS = MT_CODES / RING_UNIT;  // code units per env
static_assert((MT_CODES / 2) % RING_UNIT == 0, "a half of the ring is whole units");
TG_HD uint32_t ring_slot(uint32_t rd) { return (rd / RING_UNIT) % RING_SLOTS; }
// slots that hold no staged, unread draw: the ones a new unit may land in
TG_HD uint32_t ring_free(uint32_t rd, uint32_t staged) {
  return RING_SLOTS - (rd % RING_UNIT + staged) / RING_UNIT;
}
// place of slot j in the order the free slots are filled (0: next), from the staged end
TG_HD uint32_t ring_order(uint32_t rd, uint32_t staged, uint32_t j) {
  return (j - (rd + staged) / RING_UNIT) % RING_SLOTS;
}
// the code unit k units past unit u (wrap at RING_UNITS)
TG_HD uint32_t ring_unit(uint32_t u, uint32_t k) {
  return u + k >= RING_UNITS ? u + k - RING_UNITS : u + k;
}
// the unit the next DMA fetches: the one after the staged end; cur = the next draw's code index
TG_HD uint32_t ring_next_unit(uint32_t cur, uint32_t staged) {
  return ((cur + staged) / RING_UNIT) % RING_UNITS;
}
// units a lane may fetch without the blocking path: its free slots, if all of those units lie
// in the half that holds pos (the word position of the last blocking fill), which is never
// stale and keeps sync()'s one-boundary assumption; else none (the blocking path refills)
TG_HD uint32_t ring_plan(uint32_t pos, uint32_t rd, uint32_t staged, uint32_t cur) {
  const uint32_t f = ring_free(rd, staged);
  if (!f) return 0u;
  const uint32_t u = ring_next_unit(cur, staged), per_half = RING_UNITS / 2u;
  const uint32_t h = pos >= (uint32_t)MT_HALF ? 1u : 0u;
  return (u / per_half == h && (u + f - 1u) / per_half == h) ? f : 0u;
}

}  // namespace tg
