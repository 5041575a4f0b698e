// walk_check.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host-only build of the plain phases' multi-draw hops (gym-treasure-game_amd/csrc/tg_walk.h:
// hop_ticks, walk_hops) over a flat array of code bytes, beside walk_ticks, which specifies them,
// over the same array.  tests/test_walk_host.py drives it.  Built by tests/native_walk/Makefile
// with hipcc --offload-host-only; the product library never contains or calls this.
#include <cstdint>
#include <cstring>

#include "../../gym-treasure-game_amd/csrc/tg_walk.h"

using namespace tg;

namespace {
// the staged window as walk_hops sees it: codes c[rd ..], `left` of them staged
struct FlatWin {
  const uint8_t* c;
  uint32_t rd, left;
  uint32_t dword(uint32_t i) const {
    uint32_t w;
    memcpy(&w, c + 4u * i, 4);
    return w;
  }
};
// the same window as walk_ticks sees it: one code per draw
struct FlatRng {
  const uint8_t* c;
  uint32_t rd, left;
  bool has(uint32_t k) const { return left >= k; }
  uint32_t code() {
    --left;
    return c[rd++];
  }
};
template <int DIR>
void ref_walk(const uint8_t* c, uint32_t rd, uint32_t left, int x, int lim, int cap, int32_t* out) {
  FlatRng r{c, rd, left};
  out[1] = walk_ticks<DIR>(r, x, lim, cap);
  out[0] = x;
  out[2] = (int32_t)(r.rd - rd);
  out[3] = (int32_t)r.left;
}
template <int DIR>
void hop_walk(const uint8_t* c, uint32_t rd, uint32_t left, int x, int lim, int cap, int32_t* out) {
  FlatWin w{c, rd, left};
  out[1] = walk_hops<DIR>(w, x, lim, cap);
  out[0] = x;
  out[2] = (int32_t)(w.rd - rd);
  out[3] = (int32_t)w.left;
}
}  // namespace

extern "C" {

int wk_tick_draws() { return (int)TICK_DRAWS; }

// one walk from code c[rd] with `left` staged: out = {x, ticks, draws consumed, left after};
// hops: walk_hops, else walk_ticks
void wk_walk(const uint8_t* c, int dir, int hops, uint32_t rd, uint32_t left, int x, int lim,
             int cap, int32_t* out) {
  if (hops) {
    if (dir > 0) hop_walk<1>(c, rd, left, x, lim, cap, out);
    else hop_walk<-1>(c, rd, left, x, lim, cap, out);
  } else {
    if (dir > 0) ref_walk<1>(c, rd, left, x, lim, cap, out);
    else ref_walk<-1>(c, rd, left, x, lim, cap, out);
  }
}

// hop_ticks on the m codes from c[rd]: out = {taken all m (0 / 1), x after}
void wk_hop(const uint8_t* c, int dir, uint32_t rd, int m, uint32_t left, int x, int lim, int taken,
            int cap, int32_t* out) {
  uint32_t w;
  memcpy(&w, c + rd, 4);
  out[0] = dir > 0 ? hop_ticks<1>(w, m, x, lim, left, taken, cap)
                   : hop_ticks<-1>(w, m, x, lim, left, taken, cap);
  out[1] = x;
}

// The whole grid of cases at unit `base` (a multiple of 16 codes) of the array: both directions,
// start offsets 0..15, distance to lim d0..d1, left l0..l1, cap c0..c1.  walk_hops against
// walk_ticks (coordinate, ticks, draws, left), and hop_ticks for m = 1..4 against walk_ticks
// capped at m ticks (all m taken or not; the coordinate when taken, untouched when not).
// Returns the cases run; *bad counts the mismatches and first[] describes the first one.
int64_t wk_sweep(const uint8_t* codes, uint32_t base, int d0, int d1, int l0, int l1, int c0,
                 int c1, int64_t* bad, int32_t* first) {
  int64_t cases = 0;
  *bad = 0;
  const uint8_t* const c = codes + base;
  const int x0 = 100;
  for (int dir = -1; dir <= 1; dir += 2)
    for (uint32_t off = 0; off < 16; ++off)
      for (int d = d0; d <= d1; ++d)
        for (int left = l0; left <= l1; ++left)
          for (int cap = c0; cap <= c1; ++cap) {
            const int lim = x0 + dir * d;
            int32_t a[4], b[4];
            wk_walk(c, dir, 0, off, (uint32_t)left, x0, lim, cap, a);
            wk_walk(c, dir, 1, off, (uint32_t)left, x0, lim, cap, b);
            bool ok = a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3] && a[1] == a[2];
            for (int m = 1; m <= 4 && ok; ++m) {
              int32_t h[2], t[4];
              wk_hop(c, dir, off, m, (uint32_t)left, x0, lim, 0, cap, h);
              wk_walk(c, dir, 0, off, (uint32_t)left, x0, lim, cap < m ? cap : m, t);
              ok = h[0] == (t[1] == m) && h[1] == (h[0] ? t[0] : x0);
            }
            ++cases;
            if (!ok && (*bad)++ == 0) {
              first[0] = dir, first[1] = (int32_t)off, first[2] = d, first[3] = left, first[4] = cap;
              for (int k = 0; k < 4; ++k) first[5 + k] = a[k], first[9 + k] = b[k];
            }
          }
  return cases;
}


// One lane's rolling code window over the flat array mc[MT_CODES]: the reserve / top-up / fill
// sequence of the form measured in DESIGN.md §3.3, written on tg_walk.h's ring_* functions: from
// draw index `start`, `total` draws in per-tick batches of 0..6 from a seeded generator, each
// tick behind reserve(TICK_DRAWS), now and then reserve(MAX_TICK_DRAWS).  A DMA's slot turns
// to garbage when it is issued and to its unit's codes when the lane waits for it, so a read
// of a unit not yet waited for, or of a slot refilled too early, shows as a wrong code.
// Returns 0, or a code for the first failure: 1 a draw read is not mc[(start + i) % MT_CODES],
// 2 a slot refilled while a staged, unread draw is in it, 3 reserve(k) left fewer than k.
// info: {failing draw, blocking refills, rolling DMAs}
int wk_ring(const uint8_t* mc, uint32_t start, int total, uint64_t seed, int32_t* info) {
  uint8_t ring[RING_DRAWS];
  int32_t pending[RING_SLOTS];  // unit in flight into the slot, or -1
  for (uint32_t j = 0; j < RING_SLOTS; ++j) pending[j] = -1;
  memset(ring, 0xEE, sizeof ring);
  uint32_t pos = 2u * start, n = 0, rd = 0, left = 0, infl = 0;
  int blocking = 0, rolled = 0, done = 0;
  auto land = [&]() {
    for (uint32_t j = 0; j < RING_SLOTS; ++j)
      if (pending[j] >= 0) memcpy(ring + j * RING_UNIT, mc + (uint32_t)pending[j] * RING_UNIT, RING_UNIT), pending[j] = -1;
    left += infl;
    infl = 0;
  };
  auto issue = [&](uint32_t j, uint32_t unit, bool check) -> bool {
    if (check)  // slot j must hold no staged, unread draw: rd .. rd + staged - 1
      for (uint32_t q = rd; q < rd + left + infl; ++q)
        if (ring_slot(q) == j) return false;
    memset(ring + j * RING_UNIT, 0xEE, RING_UNIT);
    pending[j] = (int32_t)unit;
    return true;
  };
  auto fill = [&]() {  // the blocking refill: fold the position, four units from it
    land();
    uint32_t e = (pos >> 1) + n;
    pos = 2u * (e >= (uint32_t)MT_CODES ? e - (uint32_t)MT_CODES : e);
    n = 0;
    const uint32_t d = pos >> 1, c0 = d / RING_UNIT;
    rd = d % RING_UNIT;
    left = 0, infl = 0;
    for (uint32_t j = 0; j < RING_SLOTS; ++j) issue(j, ring_unit(c0, j), false);
    infl = RING_DRAWS - rd;
    land();
    ++blocking;
  };
  auto reserve = [&](uint32_t k) -> int {
    uint32_t cur = (pos >> 1) + n;
    cur = cur >= (uint32_t)MT_CODES ? cur - (uint32_t)MT_CODES : cur;
    const uint32_t staged = left + infl;
    const uint32_t f = ring_plan(pos, rd, staged, cur);
    if (f != 0u && (staged < 32u || staged < k)) {
      const uint32_t u = ring_next_unit(cur, staged);
      for (uint32_t j = 0; j < RING_SLOTS; ++j) {
        const uint32_t o = ring_order(rd, staged, j);
        if (o < f) {
          if (!issue(j, ring_unit(u, o), true)) return 2;
          ++rolled;
        }
      }
      infl += f * RING_UNIT;
    }
    if (infl && left < (k > 16u ? k : 16u)) land();
    if (left < k) fill();
    return left >= k ? 0 : 3;
  };
  fill();
  blocking = 0;
  while (done < total) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t r = (uint32_t)(seed >> 33);
    const uint32_t k = r % 13u == 0u ? MAX_TICK_DRAWS : TICK_DRAWS;
    if (const int rc = reserve(k)) {
      info[0] = done, info[1] = blocking, info[2] = rolled;
      return rc;
    }
    const int batch = (int)((r >> 8) % 7u);
    for (int b = 0; b < batch && done < total; ++b) {
      const uint8_t c = ring[ring_slot(rd) * RING_UNIT + rd % RING_UNIT];
      if (c != mc[(start + (uint32_t)done) % (uint32_t)MT_CODES]) {
        info[0] = done, info[1] = blocking, info[2] = rolled;
        return 1;
      }
      ++rd, --left, ++n, ++done;
    }
  }
  info[0] = done, info[1] = blocking, info[2] = rolled;
  return 0;
}

}  // extern "C"
