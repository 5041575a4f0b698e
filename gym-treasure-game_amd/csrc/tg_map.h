// tg_map.h — the collision predicates on the 48-px cell grid: `Map` (the bordered grid's cell
// probes, the level bitmasks' layout Map::mk and their accessors), `AirCells` / `AirProbe` (an air
// tick's 2 x 3-cell window) and `LadMasks` (a ladder option's column masks).  `__host__
// __device__`; the grid is LDS on the device.  Reads `Env` and the constants of tg_state.h only.
#pragma once
#include "tg_state.h"

namespace tg {

// ==========================================================================================
// Map probes.  Every probe is a clamped index into the bordered grid plus one LDS byte read;
// predicates combine probes with bitwise &/| so their LDS reads issue back to back.
// ==========================================================================================
// The cells one air tick at (px, py) can probe, as two 6-bit masks (bit 2*ri + ci: row r0 + ri,
// column c0 + ci): every probe x of the tick lies in [px - 16, px + 16] (33 px: columns c0 =
// colx(px - 16) and c0 + 1), every probe y in [py - 4, py + 53] (58 px: rows r0 = rowy(py - 4)
// .. r0 + 2), the moved player's can_fall4 included (|x step| <= 4).  A probe's cell is then two
// compares against the column / row starts instead of a clamped pixel -> cell division and an
// LDS read; past the border the compares select the clamped cell, as colx / rowy do.
struct AirCells {
  // per window column (A: c0, B: c0 + 1) the rows r0 .. r0 + 2 (bits 0..2) that are OPEN /
  // hold a WALL or a closed door (can_go_side's blockers)
  uint32_t oA, oB, bA, bB;
  int bx, by1;   // first pixel of column c0 + 1 and of row r0 + 1
  uint32_t dc;   // the door state the masks were built for
  // still the window of (dc, px, py): colx(px - 16) == c0 and rowy(py - 4) == r0 (at a clamped
  // border this is false even right after a rebuild: the caller then takes the full tick)
  TG_HD bool holds(uint32_t d, int px, int py) const {
    return (d == dc) & (px - (HALFW + INCR) < bx) & (px - (HALFW + INCR) >= bx - S) &
           (py - INCR < by1) & (py - INCR >= by1 - S);
  }
};

// The air tick's predicates inside its window.  With s = bx - px and t = by1 - py the window
// holds iff s in (-16, 32] and t in [-3, 44], so a probe at px + o lies in column B iff o >= s,
// and one at py + o in row (o >= t) + (o >= t + 48): row 0 for o = -4, row 1 for o = 44, row 1 +
// (t <= 2) for o = 50; each predicate is a few compares and selects of 3-bit row masks
// (AirCells: every probe of the tick, the moved player's fall included, lies in the window).
struct AirProbe {
  const AirCells& ac;
  int s, t;
  TG_HD AirProbe(const AirCells& a, int px, int py) : ac(a), s(a.bx - px), t(a.by1 - py) {}
  static TG_HD uint32_t bit(uint32_t m, uint32_t r) { return (m >> r) & 1u; }
  TG_HD uint32_t open_col(int o) const { return o >= s ? ac.oB : ac.oA; }
  TG_HD uint32_t block_col(int o) const { return o >= s ? ac.bB : ac.bA; }
  TG_HD bool can_fall() const {  // can_fall_at: px -+ 10 at py and py + 50
    const uint32_t c = open_col(-(HALFW - 2)) & open_col(HALFW - 2);
    return (bit(c, (uint32_t)(t <= 0)) & bit(c, 1u + (uint32_t)(t <= 2))) != 0;
  }
  TG_HD bool side(int dir) const {  // can_go_side: px + 16 dir at py + 4 and py + 44
    const uint32_t c = block_col(dir * (HALFW + INCR));
    return (bit(c, (uint32_t)(t <= INCR)) | bit(c, 1u)) == 0;
  }
  TG_HD bool up_clear() const {  // px -+ 4 at py - 4 and py - 1
    const uint32_t c = open_col(-INCR) & open_col(INCR);
    return (bit(c, 0u) & bit(c, (uint32_t)(t <= -1))) != 0;
  }
  // the distance of a downward move of yd <= 4 px (IM/:341-348, Map::fall) after the player's
  // x moved to px2 (by <= 4: still in the window): the probes at py + k and py + 50 + k (k < 4)
  // enter their next row at k = t (if t > 0) / t - 2 (if t > 2); the others at >= 43
  TG_HD int fall(int px2, int yd) const {
    const int s2 = ac.bx - px2;
    const uint32_t c = (-(HALFW - 2) >= s2 ? ac.oB : ac.oA) & ((HALFW - 2) >= s2 ? ac.oB : ac.oA);
    if (!(bit(c, (uint32_t)(t <= 0)) & bit(c, 1u + (uint32_t)(t <= 2)))) return yd;
    int d = yd;
    if (!bit(c, (uint32_t)(t <= 3))) d = min(d, t > 0 ? t : t + S);
    if (!bit(c, 1u + (uint32_t)(t <= 5))) d = min(d, t > 2 ? t - 2 : t + S - 2);
    return d;
  }
};

// ---- level bitmasks (Map::mk) -------------------------------------------------------------------
// For levels of at most MK_DIM - 2 PAD cells a side (the default 14 x 13 is 18 x 17 bordered):
// per bordered column (index c + PAD) the rows holding a LADDER (bit r + PAD); per door state and
// column the OPEN rows; per door state and bordered row the OPEN columns and the WALL-or-closed-
// door columns (bit c + PAD).  Built on the host from the grid (tg_level.h build_masks) and
// staged with it; a predicate that would read several cells of one column or row reads one word
// and tests bits (the ladder and go loops' span limits).  Null: the cell probes.
constexpr int MK_DIM = 32;
constexpr int MK_MAX_WORDS = 25 * MK_DIM;  // 9 column tables + 16 row tables
TG_HD int mk_words(int W, int H) { return 9 * (W + 2 * PAD) + 16 * (H + 2 * PAD); }

struct Map {
  const uint8_t* g;  // LDS on device: (H + 2*PAD) rows of (W + 2*PAD) cells
  int W, H;
  const uint32_t* mk = nullptr;  // the level bitmasks (LDS on device), or null

  TG_HD int pw() const { return W + 2 * PAD; }
  TG_HD int ph() const { return H + 2 * PAD; }
  // mask words: c / r are clamped column / row indices (colx / rowy)
  TG_HD uint32_t mk_lad(int c) const { return mk[c + PAD]; }
  TG_HD uint32_t mk_colopen(uint32_t dc, int c) const { return mk[pw() * (1 + (int)dc) + c + PAD]; }
  TG_HD uint32_t mk_rowopen(uint32_t dc, int r) const { return mk[9 * pw() + ph() * (int)dc + r + PAD]; }
  TG_HD uint32_t mk_rowblk(uint32_t dc, int r) const {
    return mk[9 * pw() + ph() * (8 + (int)dc) + r + PAD];
  }
  TG_HD uint32_t rbit(int y) const { return (uint32_t)(rowy(y) + PAD); }  // row bit of pixel y
  // object_type_at_cell (IM/:227-230) as cell bits; anything outside the grid is WALL
  TG_HD uint32_t cellb(int cx, int cy) const {
    cx = clampi(cx, -PAD, W + PAD - 1);
    cy = clampi(cy, -PAD, H + PAD - 1);
    return g[mul24((uint32_t)(cy + PAD), (uint32_t)pw()) + cx + PAD];
  }
  // the cell column / row atb() probes for pixel x / y (clamped into the WALL border)
  TG_HD int colx(int x) const { return div48(clampi(x, -PAD * S, (W + PAD) * S - 1) + PAD * S) - PAD; }
  TG_HD int rowy(int y) const { return div48(clampi(y, -PAD * S, (H + PAD) * S - 1) + PAD * S) - PAD; }
  // object_type_at (IM/:218-225) as cell bits
  TG_HD uint32_t atb(int x, int y) const {
    x = clampi(x, -PAD * S, (W + PAD) * S - 1) + PAD * S;
    y = clampi(y, -PAD * S, (H + PAD) * S - 1) + PAD * S;
    return g[mul24((uint32_t)div48(y), (uint32_t)pw()) + div48(x)];
  }
  // door state -> type: `dc` = closed-door bits (f >> F_OBJ) & 7
  static TG_HD bool is_open(uint32_t c, uint32_t dc) {
    return ((c & B_OPEN) | ((c >> 4) & ~dc & 7u)) != 0;
  }
  static TG_HD bool is_ladder(uint32_t c) { return (c & B_LADDER) != 0; }
  static TG_HD bool is_wall(uint32_t c) { return (c & B_WALL) != 0; }
  static TG_HD bool is_door(uint32_t c, uint32_t dc) {
    return ((c & B_DOOR) | ((c >> 4) & dc)) != 0;
  }
  static TG_HD uint32_t dc_of(uint32_t f) { return (f >> F_OBJ) & 7u; }

  TG_HD bool open_at(uint32_t dc, int x, int y) const { return is_open(atb(x, y), dc); }
  TG_HD bool open_cell(uint32_t dc, int cx, int cy) const { return is_open(cellb(cx, cy), dc); }

  // up_clear (IM/:232-238): xs {px-4, px, px+4} x ys [py-4, py-1] all OPEN; the three xs
  // span at most two columns and the four ys at most two rows
  TG_HD bool up_clear(const Env& e) const {
    const uint32_t dc = dc_of(e.f);
    const int x0 = e.px - INCR, x1 = e.px + INCR, y0 = e.py - INCR, y1 = e.py - 1;
    return open_at(dc, x0, y0) & open_at(dc, x1, y0) & open_at(dc, x0, y1) & open_at(dc, x1, y1);
  }
  // can_go_up (IM/:240-250): ys {py-4, py, py+44} x xs {px-12, px+12}, any LADDER
  TG_HD bool can_go_up(const Env& e) const {
    const int xa = e.px - HALFW, xb = e.px + HALFW;
    const int y0 = e.py - INCR, y1 = e.py, y2 = e.py + S - INCR;
    const uint32_t any = atb(xa, y0) | atb(xb, y0) | atb(xa, y1) | atb(xb, y1) | atb(xa, y2) |
                         atb(xb, y2);
    return (e.py > 1) & is_ladder(any);
  }
  // can_go_down (IM/:252-257): ys [py, py+51] x xs {px-12, px+12}, any LADDER.  The 52 ys span
  // at most three rows; rows outside the grid are WALL, so probing the clamped rows
  // y, y+24, y+51 (every row of the span contains one of them) is exact.
  TG_HD bool can_go_down(const Env& e) const {
    const int xa = e.px - HALFW, xb = e.px + HALFW;
    const int y0 = e.py, y1 = e.py + S / 2, y2 = e.py + S + INCR - 1;
    const uint32_t any = atb(xa, y0) | atb(xb, y0) | atb(xa, y1) | atb(xb, y1) | atb(xa, y2) |
                         atb(xb, y2);
    return is_ladder(any);
  }
  // can_go_left / can_go_right (IM/:259-281): x = px -/+ 16 at ys {py+4, py+44}
  TG_HD bool can_go_side(const Env& e, int dir) const {
    const uint32_t dc = dc_of(e.f);
    const int x = e.px + dir * (HALFW + INCR);
    const uint32_t ta = atb(x, e.py + INCR), tb = atb(x, e.py + S - INCR);
    return !(is_wall(ta | tb) | is_door(ta, dc) | is_door(tb, dc));
  }
  // can_fall (IM/:283-288): xs {px-10, px+10} x ys {py, py+50} all OPEN
  TG_HD bool can_fall_at(uint32_t dc, int px, int py) const {
    const int xa = px - HALFW + 2, xb = px + HALFW - 2, ya = py, yb = py + S + 2;
    return open_at(dc, xa, ya) & open_at(dc, xa, yb) & open_at(dc, xb, ya) & open_at(dc, xb, yb);
  }
  TG_HD bool can_fall(const Env& e) const { return can_fall_at(dc_of(e.f), e.px, e.py); }
  // AirCells at (px, py): six LDS reads in one batch (rows and the second column clamped)
  TG_HD AirCells air_cells(uint32_t dc, int px, int py) const {
    const int c0 = colx(px - (HALFW + INCR)), r0 = rowy(py - INCR);
    const uint32_t x0 = (uint32_t)(c0 + PAD), x1 = (uint32_t)(c0 + 1 < W + PAD ? c0 + 1 + PAD : c0 + PAD);
    uint32_t oa = 0, ob = 0, ba = 0, bb = 0;
#pragma unroll
    for (int ri = 0; ri < 3; ++ri) {
      const int r = r0 + ri < H + PAD ? r0 + ri : H + PAD - 1;
      const uint8_t* const row = g + mul24((uint32_t)(r + PAD), (uint32_t)pw());
      const uint32_t ca = row[x0], cb = row[x1];
      oa |= (uint32_t)is_open(ca, dc) << ri;
      ob |= (uint32_t)is_open(cb, dc) << ri;
      ba |= (uint32_t)(is_wall(ca) | is_door(ca, dc)) << ri;
      bb |= (uint32_t)(is_wall(cb) | is_door(cb, dc)) << ri;
    }
    return AirCells{oa, ob, ba, bb, (c0 + 1) * S, (r0 + 1) * S, dc};
  }
  // integrate y on a downward move of yd <= 4 px (IM/:341-348): with can_fall at py the player
  // falls pixel by pixel while can_fall holds, so the distance is the first k in 1..yd-1 with
  // !can_fall(py + k), else yd.  The probes (px -+ 10 at py + k and py + 50 + k, k < 4) span at
  // most two rows each, entering the second at k = ka / kb: 8 lookups instead of 16, and the
  // first failing k in closed form (rows past the border clamp to the same WALL row, where
  // both lookups agree anyway)
  TG_HD int fall(uint32_t dc, int px, int py, int yd) const {
    const int ca = colx(px - HALFW + 2), cb = colx(px + HALFW - 2);
    const int ya = py, yb = py + S + 2;
    const int ra0 = rowy(ya), ra1 = rowy(ya + 3), rb0 = rowy(yb), rb1 = rowy(yb + 3);
    const bool a0 = is_open(cellb(ca, ra0), dc) & is_open(cellb(cb, ra0), dc);
    const bool a1 = is_open(cellb(ca, ra1), dc) & is_open(cellb(cb, ra1), dc);
    const bool b0 = is_open(cellb(ca, rb0), dc) & is_open(cellb(cb, rb0), dc);
    const bool b1 = is_open(cellb(ca, rb1), dc) & is_open(cellb(cb, rb1), dc);
    if (!(a0 & b0)) return yd;
    const int ka = S - (ya - floordiv48(ya) * S), kb = S - (yb - floordiv48(yb) * S);
    int d = yd;
    if (!a1) d = min(d, ka);
    if (!b1) d = min(d, kb);
    return d;
  }
};

// The ladder options' probes from the level bitmasks: px is fixed while a ladder option runs
// (its primitives UP / DOWN / NOP and the gravity move only py), and so are the door states, so
// the columns of every probe are: LADDER rows at px -+ 12 (can_go_up / can_go_down), OPEN rows at
// both px -+ 10 (can_fall) and at both px -+ 4 (up_clear, for a leftover jump ticker).
struct LadMasks {
  uint32_t lad, fall, up;
  TG_HD LadMasks(const Map& m, uint32_t dc, int px)
      : lad(m.mk_lad(m.colx(px - HALFW)) | m.mk_lad(m.colx(px + HALFW))),
        fall(m.mk_colopen(dc, m.colx(px - HALFW + 2)) & m.mk_colopen(dc, m.colx(px + HALFW - 2))),
        up(m.mk_colopen(dc, m.colx(px - INCR)) & m.mk_colopen(dc, m.colx(px + INCR))) {}
  // Map::can_go_up / can_go_down / can_fall_at / up_clear / fall at (px, py)
  TG_HD bool can_go_up(const Map& m, int py) const {
    return (py > 1) & ((((lad >> m.rbit(py - INCR)) | (lad >> m.rbit(py)) | (lad >> m.rbit(py + S - INCR))) & 1u) != 0);
  }
  TG_HD bool can_go_down(const Map& m, int py) const {
    return (((lad >> m.rbit(py)) | (lad >> m.rbit(py + S / 2)) | (lad >> m.rbit(py + S + INCR - 1))) & 1u) != 0;
  }
  TG_HD bool can_fall(const Map& m, int py) const {
    return ((fall >> m.rbit(py)) & (fall >> m.rbit(py + S + 2)) & 1u) != 0;
  }
  TG_HD bool up_clear(const Map& m, int py) const {
    return ((up >> m.rbit(py - INCR)) & (up >> m.rbit(py - 1)) & 1u) != 0;
  }
  TG_HD int fall_dist(const Map& m, int py, int yd) const {
    const int ya = py, yb = py + S + 2;
    if (!((fall >> m.rbit(ya)) & (fall >> m.rbit(yb)) & 1u)) return yd;
    const int ka = S - (ya - floordiv48(ya) * S), kb = S - (yb - floordiv48(yb) * S);
    int d = yd;
    if (!((fall >> m.rbit(ya + 3)) & 1u)) d = min(d, ka);
    if (!((fall >> m.rbit(yb + 3)) & 1u)) d = min(d, kb);
    return d;
  }
};

}  // namespace tg
