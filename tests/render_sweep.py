"""Synthesized env states for rendering sweeps against the oracle.  TEST INFRASTRUCTURE in the
style of tests/state_sweep.py (whose level reading, positions, bag states and flag packing it
uses); it does not import the product, and it is deterministic (fixed constants, a fixed
permutation, no clock).  Nothing is stepped: a case is a state written into a handle and drawn.

From a level directory it builds cases in the checkpoint format (tests/state_codec.py) far
outside what a seeded rollout stops on.  Four tiers, one ``RenderSweep`` per level:

``hero``    per cell that holds standing positions (all doors closed), py in {lowest, highest}
            of the cell and px the row's first 16 standing values (every residue of the 16-pixel
            period of the 16-byte chunks' three byte offsets) plus its last; one airborne
            position per open or ladder cell, the k-th with py % 48 nearest 7k mod 48 (the
            hero across two bands at many offsets).  Facing, door bits, handle bits, both angles,
            bolt and bag state are drawn per case from a fixed random.Random.
``door``    standing positions of the table with every door open that lie in a door's cell
            (same rows and columns), used only with that door open: the hero over the open
            door's tile.
``item``    all 448 combinations of door bits x handle bits x bolt x bag state, the hero at one
            fixed position that touches no object; angles drawn.
``handle``  per handle and range (down: [0, 0.15], up: [0.85, 1.0]): both ends, one angle
            inside every class of the integer end point (int(ex), int(ey)), and the two angles
            on either side of every integer crossing of ex or ey, each between 1e-7 px and 1e-5
            px from the integer (the product's guard, TG_ERR_RENDER, is 1e-9; a double cos at
            radius 36 errs by ~1e-14).  The crossings are found by bisection with the
            reference's formula (DR/:258-262) in Python's math.  Each angle gets three hero
            placements: away from the handle, standing over the knob, standing over the shaft
            next to the base.  The other handle's bit and angle are drawn.

A handle's bit and angle stay consistent (up: [0.85, 1.0], down: [0, 0.15]); other angles are
out of scope.  default and render_overlap take all tiers, corridor (thinned: CORRIDOR_CELLS),
cascade and narrow the hero and door tiers.  Bag states as in state_sweep (an item in the bag
lies in the bottom row).  Streams are any valid ones.
"""
import functools
import math
import os
import random

import numpy as np

import state_codec as sc
import state_sweep as ss

S = 48
DRAW_SEED = 0x5EED0F00    # random.Random(constant) of the drawn columns
PERM_SEED = 20261020      # the fixed permutation
NCOL = 16                 # standing px per row: one per residue of the chunk period
RANGES = ((0.0, 0.15), (0.85, 1.0))   # a handle's angles when down (bit 0) and up (bit 1)
NEAR_LO, NEAR_HI = 1e-7, 1e-5          # a crossing angle's distance from the integer, px
MIN_CLASSES = (13, 12)                 # end-point classes per range (down, up)
TIERS = ("hero", "door", "item", "handle")
KINDS = ("", "range end", "inside a class", "below a crossing", "above a crossing")
PLACES = ("", "away", "over the knob", "over the shaft")
LEVELS = {None: sc.DEFAULT_LEVEL}
for _n in ("render_overlap", "corridor", "cascade", "narrow"):
    LEVELS[_n] = os.path.join(sc.GOLDEN, "levels", _n)
ALL_TIERS = (None, "render_overlap")   # the other levels take the hero and door tiers


def corridor_cells(cx, cy):
    """corridor is 42 cells wide twice over: its object row (3) keeps cells 1..22 and 40..42,
    the other row cells 1, 21 and 42"""
    return (1 <= cx <= 22 or 40 <= cx <= 42) if cy == 3 else cx in (1, 21, 42)


CELL_FILTER = {"corridor": corridor_cells}


# ---- handle geometry (DR/:258-262) -------------------------------------------------------------
def end_point(cell, a):
    """the shaft's end point (ex, ey) before int(), for the handle on ``cell`` at angle ``a``"""
    th = ((math.pi / 2.0) * a) + math.pi / 4.0
    r = S * 0.75
    sx, sy = cell[0] * S + S / 2.0, float(cell[1] * S + S)
    return sx + (r * math.cos(th)), sy - (r * math.sin(th))


def crossings(cell, lo, hi):
    """[(a, axis, k, below, above)]: every angle a in (lo, hi) at which coordinate ``axis`` of
    the end point crosses the integer k (both coordinates are monotonic on either range), with
    the angles ``below`` / ``above`` that leave it NEAR_LO..NEAR_HI px under / over k"""
    out = []
    for axis in (0, 1):
        def c(a):
            return end_point(cell, a)[axis]
        c0, c1 = c(lo), c(hi)
        for k in range(int(math.floor(min(c0, c1))) + 1, int(math.ceil(max(c0, c1)))):
            under, over = (lo, hi) if c0 < c1 else (hi, lo)   # c(under) < k <= c(over)
            for _ in range(200):
                mid = 0.5 * (under + over)
                if mid == under or mid == over:
                    break
                if c(mid) < k:
                    under = mid
                else:
                    over = mid
            th = ((math.pi / 2.0) * over) + math.pi / 4.0
            slope = S * 0.75 * (math.pi / 2.0) * (math.sin(th) if axis == 0 else math.cos(th))
            da = 1e-6 / abs(slope) * (1.0 if c0 < c1 else -1.0)   # towards larger c
            below, above = over - da, over + da
            for a, sign in ((below, -1.0), (above, 1.0)):
                d = (c(a) - k) * sign
                assert NEAR_LO <= d <= NEAR_HI and lo < a < hi, (cell, axis, k, a, d)
                o = end_point(cell, a)[1 - axis]
                assert abs(o - round(o)) > NEAR_HI, (cell, axis, k, a, o)   # one crossing at a time
            assert int(c(below)) == k - 1 and int(c(above)) == k
            out.append((over, axis, k, below, above))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def handle_angles(cell, up):
    """[(angle, kind)] of the handle tier for one handle cell and range (kind: KINDS' index),
    and the number of end-point classes"""
    lo, hi = RANGES[up]
    cr = crossings(cell, lo, hi)
    cuts = [lo] + [c[0] for c in cr] + [hi]
    mids = [0.5 * (a + b) for a, b in zip(cuts, cuts[1:])]
    classes = set(tuple(int(v) for v in end_point(cell, a)) for a in mids)
    assert len(classes) == len(mids) >= MIN_CLASSES[up], (cell, up, len(classes), len(mids))
    angles = [(lo, 1), (hi, 1)] + [(a, 2) for a in mids]
    for c in cr:
        angles += [(c[3], 3), (c[4], 4)]
    return tuple(angles), len(classes)


def shaft_box(cell, a):
    """x0, x1, y0, y1 (half open) around the 5-px shaft and the knob of the handle on ``cell``"""
    x1, y1 = cell[0] * S + S // 2, cell[1] * S + S
    x2, y2 = (int(v) for v in end_point(cell, a))
    return (min(min(x1, x2) - 2, x2 - 4), max(max(x1, x2) + 3, x2 + 5),
            min(min(y1, y2) - 2, y2 - 4), max(max(y1, y2) + 3, y2 + 5))


def hero_box(px, py):
    return px - S // 2, px + S // 2, py, py + S


def overlaps(a, b):
    return a[0] < b[1] and a[1] > b[0] and a[2] < b[3] and a[3] > b[2]


def cell_box(cx, cy):
    return cx * S, cx * S + S, cy * S, cy * S + S


# ---- positions ---------------------------------------------------------------------------------
def by_cell(mask):
    """{(cx, cy): [(px, py)]} of a position table (the cell as state_sweep counts it)"""
    cells = {}
    ys, xs = np.nonzero(mask)
    for x, y in zip(xs.tolist(), ys.tolist()):
        cells.setdefault((x // S, (y + S // 2) // S), []).append((x, y))
    return cells


def rows_and_columns(pts):
    """of one cell's positions: py in {lowest, highest}, px the row's first NCOL and its last"""
    sel = []
    pys = sorted(set(y for _, y in pts))
    for y in sorted({pys[0], pys[-1]}):
        row = sorted(x for x, yy in pts if yy == y)
        sel += [(x, y) for x in sorted(set(row[:NCOL] + row[-1:]))]
    return sel


def hero_positions(name):
    """(ground [(px, py)], airborne [(px, py)], cells with ground positions)"""
    level_dir = LEVELS[name]
    lv = ss.read_level(level_dir)
    ground, air = ss.positions(level_dir)
    keep = CELL_FILTER.get(name, lambda cx, cy: True)
    cells = by_cell(ground)
    sel = []
    for cell, pts in sorted(cells.items()):
        if keep(*cell):
            sel += rows_and_columns(pts)
    airborne = []
    k = 0
    for (cx, cy), pts in sorted(by_cell(air).items()):
        if lv["rows"][cy][cx] == "/":
            continue
        want = 7 * k % S
        k += 1
        airborne.append(min(pts, key=lambda p: (min((p[1] - want) % S, (want - p[1]) % S),
                                                abs(p[0] - (cx * S + S // 2)), p)))
    return sel, airborne, sorted(cells)


def door_positions(name):
    """[(door, px, py)]: standing positions with every door open that lie in a door's cell"""
    level_dir = LEVELS[name]
    lv = ss.read_level(level_dir)
    cells = by_cell(ss.positions(level_dir, 0)[0])
    out = []
    for d, (cx, cy, _) in enumerate(lv["door"]):
        out += [(d, x, y) for x, y in rows_and_columns(cells.get((cx, cy), []))]
    return out


def object_boxes(lv):
    """{name: box} of every object's home cell"""
    out = {}
    for kind in ("door", "handle", "bolt", "key", "gold"):
        for i, o in enumerate(lv[kind]):
            out["%s %d" % (kind, i)] = cell_box(o[0], o[1])
    return out


def away_position(name):
    """the first standing position (row-major) whose hero box touches no object's cell, no bag
    slot and neither handle's reach (the hull of its shaft boxes over both ranges)"""
    level_dir = LEVELS[name]
    lv = ss.read_level(level_dir)
    boxes = list(object_boxes(lv).values())
    boxes += [cell_box(lv["W"] - 1 - slot, lv["H"] - 1) for slot in range(2)]
    for h in lv["handle"]:
        cx, cy = h[0] * S + S // 2, h[1] * S + S
        boxes.append((cx - 32, cx + 33, cy - 42, cy + 3))
    ys, xs = np.nonzero(ss.positions(level_dir)[0])
    for x, y in zip(xs.tolist(), ys.tolist()):
        if not any(overlaps(hero_box(x, y), b) for b in boxes):
            return x, y
    raise AssertionError("level %s: no standing position away from every object" % name)


# ---- the sweep ---------------------------------------------------------------------------------
class RenderSweep:
    """n cases: the columns below and ``states(lo, hi)``.  In the handle tier ``which`` is the
    handle whose angle is chosen, ``kind`` what the angle is (KINDS) and ``place`` where the hero
    stands (PLACES); elsewhere they are -1, 0 and 0."""
    COLS = ("px", "py", "doors", "handles", "bolt", "bag", "facing", "tier", "kind", "place", "which")

    def __init__(self, name, rows):
        self.name, self.level_dir = name or "default", LEVELS[name]
        self.lv = ss.read_level(self.level_dir)
        n = self.n = len(rows)
        perm = np.random.RandomState(PERM_SEED).permutation(n)
        for j, k in enumerate(self.COLS):
            setattr(self, k, np.ascontiguousarray(np.array([r[j] for r in rows], np.int32)[perm]))
        self.ang = np.ascontiguousarray(np.array([r[-2:] for r in rows], np.float64)[perm])
        self.objs = ss.bag_objs(self.lv, self.bag)
        self.flags = np.ascontiguousarray(
            ss.pack_flags(self.facing, self.doors, self.handles, self.bolt, self.bag), np.uint32)
        self.pos = np.ascontiguousarray(np.stack([self.px, self.py], 1), np.int32)

    def states(self, lo=0, hi=None, mt=True):
        """cases [lo, hi) as one batch state (write_state's argument); mt False: no streams"""
        hi = self.n if hi is None else hi
        st = {"pos": self.pos[lo:hi], "flags": self.flags[lo:hi], "objs": self.objs[lo:hi],
              "ang": self.ang[lo:hi], "ep": np.zeros((hi - lo, 2), np.int32)}
        if mt:   # any valid words do (all zero would be MT19937's fixed point)
            st["mt"], st["mt_pos"] = np.zeros((hi - lo, 624), np.uint32), np.zeros(hi - lo, np.uint32)
            st["mt"][:, 0] = 0x80000000
        return st

    def tier_cases(self, *tiers):
        return np.flatnonzero(np.isin(self.tier, [TIERS.index(t) for t in tiers]))

    def describe(self, i):
        extra = ""
        if self.tier[i] == TIERS.index("handle"):
            extra = ", handle %d %s, hero %s" % (self.which[i], KINDS[self.kind[i]],
                                                 PLACES[self.place[i]])
        return ("level %s case %d (%s tier%s): px %d py %d (px %% 16 = %d, py %% 48 = %d) doors %s "
                "handles %s angles %r %r bolt %d bag %s facing %d"
                % (self.name, i, TIERS[self.tier[i]], extra, self.px[i], self.py[i],
                   self.px[i] % 16, self.py[i] % S, format(int(self.doors[i]), "03b"),
                   format(int(self.handles[i]), "02b"), float(self.ang[i, 0]),
                   float(self.ang[i, 1]), self.bolt[i], ss.BAG_NAMES[self.bag[i]], self.facing[i]))


def _place(cands, j, what):
    assert cands, what
    return cands[7 * j % len(cands)]


@functools.lru_cache(maxsize=None)
def sweep(name=None):
    lv = ss.read_level(LEVELS[name])
    rnd = random.Random(DRAW_SEED)
    rows = []

    def add(tier, px, py, kind=0, place=0, **fixed):
        """one case: the given columns, the others drawn (always in the same order)"""
        d = {"facing": rnd.getrandbits(1), "doors": rnd.getrandbits(3), "handles": rnd.getrandbits(2),
             "bolt": rnd.getrandbits(1), "bag": rnd.randrange(7)}
        handle_fix = fixed.pop("handle", None)   # (index, bit, angle)
        open_door = fixed.pop("open_door", None)
        d.update(fixed)
        if open_door is not None:
            d["doors"] &= ~(1 << open_door)
        if handle_fix is not None:
            d["handles"] = d["handles"] & ~(1 << handle_fix[0]) | handle_fix[1] << handle_fix[0]
        ang = [rnd.uniform(*RANGES[d["handles"] >> h & 1]) for h in (0, 1)]
        if handle_fix is not None:
            ang[handle_fix[0]] = handle_fix[2]
        rows.append((px, py, d["doors"], d["handles"], d["bolt"], d["bag"], d["facing"],
                     TIERS.index(tier), kind, place, -1 if handle_fix is None else handle_fix[0],
                     ang[0], ang[1]))

    ground, airborne, _ = hero_positions(name)
    for x, y in ground + airborne:
        add("hero", x, y)
    for door, x, y in door_positions(name):
        add("door", x, y, open_door=door)
    if name in ALL_TIERS:
        ax, ay = away_position(name)
        for doors in range(8):
            for handles in range(4):
                for bolt in range(2):
                    for bag in range(7):
                        add("item", ax, ay, doors=doors, handles=handles, bolt=bolt, bag=bag)
        standing = [p for pts in by_cell(ss.positions(LEVELS[name])[0]).values() for p in pts]
        standing.sort()
        for h, (hx, hy, _) in enumerate(lv["handle"]):
            base = (hx * S + S // 2 - 3, hx * S + S // 2 + 4, hy * S + S - 10, hy * S + S - 1)
            at_base = [p for p in standing if overlaps(hero_box(*p), base)]
            for up in (0, 1):
                for j, (a, kind) in enumerate(handle_angles((hx, hy), up)[0]):
                    ex, ey = (int(v) for v in end_point((hx, hy), a))
                    knob = (ex - 4, ex + 5, ey - 4, ey + 5)
                    at_knob = [p for p in standing if overlaps(hero_box(*p), knob)]
                    what = "level %s handle %d" % (name, h)
                    spots = ((ax, ay), _place(at_knob, j, what), _place(at_base, j, what))
                    for place, (x, y) in enumerate(spots, 1):
                        add("handle", x, y, kind, place, handle=(h, up, a))
    return RenderSweep(name, rows)


# ---- comparison --------------------------------------------------------------------------------
def compare_frames(sw, cases, got, want, what):
    """frames ``got`` against ``want`` [k, h, w, c] of the sweep's cases ``cases`` [k], exactly.
    The message names the first differing case and its first differing pixel."""
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    if len(bad):
        i = int(bad[0])
        px = np.argwhere((got[i] != want[i]).any(-1))
        y, x = (int(v) for v in px[0])
        raise AssertionError("%s: %d of %d frames differ; first: %s; %d pixels differ, first at "
                             "(y, x) = (%d, %d): got %s, oracle %s"
                             % (what, len(bad), len(want), sw.describe(int(cases[i])), len(px), y, x,
                                got[i, y, x].tolist(), want[i, y, x].tolist()))
