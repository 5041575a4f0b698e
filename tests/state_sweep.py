"""Synthesized env states for one-step sweeps against the oracle.  TEST INFRASTRUCTURE; it does
not import the product, and it is deterministic (fixed constants, no clock).

From a level directory it builds ``(states, actions)`` in the checkpoint format (tests/
state_codec.py, include/tg_amd.h at tg_read_state), far outside what a seeded constructor and a
policy reach: every standing position of the level, every door pattern, every bag, both sides
of the options' thresholds.

Positions (evaluated with the oracle's predicate table, all doors closed): the body probes at
px +- 16, py + 4 and py + 44 are neither WALL nor a closed door (can_go_left and can_go_right
hold) and can_fall is false.  Ladder positions are among them.

``mask_tier``: every such position x all door patterns x {key at home, in the bag, used} x
{gold at home, in the bag}.  Only available_mask is compared; no option runs.

``step_tier``: per cell that holds positions, py in {lowest, middle, highest} of the cell's
values and px in {lowest, centre - 5, - 4, - 3, centre, centre + 3, + 4, + 5, highest} clipped
to the cell's positions on that row (close_x's threshold of 4 on both sides), x all door
patterns x all 9 actions x LEVEL_DRAWS fixed draws of (handle bits, bolt, bag state, facing).  Cells
within one cell of a handle, the bolt, the key or the gold add the full cross handle bits x
bolt x bag state per action (door pattern and facing drawn).  One airborne position per open
cell (can_fall, body clear, jump_ticker 0) adds 9 actions x LEVEL_DRAWS draws.

Bag states: '', K, G, KG, GK, '' with the key used, G with the key used; an item lies at home,
in the bottom-row slot of its pick-up order (W - 1 - slot, H - 1), or at (-1, -1).  Handle
angles are 0.9 (up) and 0.1 (down).

Case i (after a fixed permutation, so neighbouring lanes differ in option and position) takes
the stream random.Random(STREAM_BASE + i), advanced so that its index cycles through 0 (the
successor form), 2, 310, 312, 620, 622, 624 (oracle.stream_states): the draw-code windows start
at both ends of a generation.
"""
import functools
import os
import random

import numpy as np

import state_codec as sc

S = 48
DRAWS = 4                 # fixed draws of (handle bits, bolt, bag, facing) per (position, doors, action)
# ... on the default level; the other levels take 2 (every position, door pattern and action
# stays): with 4 the host sweep of all four levels took 60 s of the CPU suite on 8 cores
LEVEL_DRAWS = {None: DRAWS, "corridor": 2, "exit": 2, "cascade": 2}
DRAW_SEED = 0x5EED5EED    # random.Random(constant) of those draws
PERM_SEED = 20260131      # the fixed permutation
STREAM_BASE = 770000      # case i's stream is random.Random(STREAM_BASE + i)
TICK_CAP = 1 << 14        # include/tg_amd.h TG_ERR_TICKCAP
E_TICKCAP = 1 << 24
OPTIONS = ("go_left", "go_right", "up_ladder", "down_ladder", "interact", "down_left",
           "down_right", "jump_left", "jump_right")
BAGS = ("", "K", "G", "KG", "GK", "", "G")   # states 5 and 6: the key used
BAG_NAMES = ("''", "K", "G", "KG", "GK", "'' key used", "G key used")
LEVELS = {None: sc.DEFAULT_LEVEL}
for _n in ("corridor", "exit", "cascade"):
    LEVELS[_n] = os.path.join(sc.GOLDEN, "levels", _n)


def read_level(level_dir):
    """the level text: rows, W, H and the objects' cells in objects-file order"""
    with open(os.path.join(level_dir, "domain.txt")) as fh:
        rows = [ln.strip() for ln in fh.read().split("\n")]
    while rows and not rows[-1]:
        rows.pop()
    lv = {"rows": rows, "W": len(rows[0]), "H": len(rows), "door": [], "handle": [], "bolt": [],
          "key": [], "gold": []}
    with open(os.path.join(level_dir, "domain-objects.txt")) as fh:
        for line in fh:
            w = line.split()
            if w:
                kind = next(k for k in ("door", "handle", "bolt", "key", "gold") if line.startswith(k))
                lv[kind].append((int(w[1]), int(w[2]), len(w) > 3 and w[3] == "True"))
    assert len(lv["door"]) == 3 and len(lv["handle"]) == 2
    assert len(lv["bolt"]) == len(lv["key"]) == len(lv["gold"]) == 1
    return lv


def positions(level_dir, door_bits=7):
    """(ground [H*48, W*48] bool, air likewise): the standing and the airborne positions with
    the doors of ``door_bits`` closed (all of them unless said otherwise)"""
    import oracle
    lv = read_level(level_dir)
    env = oracle.OracleEnv(0, level_dir)
    t = env.predicate_table(0, lv["W"] * S, 0, lv["H"] * S, door_bits)
    body = (t & 0x18) == 0x18                      # can_go_left and can_go_right
    fall = (t & 0x20) != 0
    return body & ~fall, body & fall


def item_cells(lv, bag):
    """key cx, cy, gold cx, cy of bag state ``bag`` (index into BAGS)"""
    W, H = lv["W"], lv["H"]
    key, gold = lv["key"][0][:2], lv["gold"][0][:2]
    s = BAGS[bag]
    if bag >= 5:
        key = (-1, -1)
    for slot, item in enumerate(s):
        if item == "K":
            key = (W - 1 - slot, H - 1)
        else:
            gold = (W - 1 - slot, H - 1)
    return key + gold


def bag_objs(lv, bag):
    """objs [n, 4] (key cx, cy, gold cx, cy) of the bag states ``bag`` [n]"""
    cells = np.array([item_cells(lv, b) for b in range(7)], np.int32)
    return np.ascontiguousarray(cells[np.asarray(bag)])


def pack_flags(facing, doors, handles, bolt, bag):
    """the checkpoint format's flag words [n] of the given columns (jump_ticker 0)"""
    def as_u32(a):
        return np.asarray(a).astype(np.uint32)

    bag = np.asarray(bag)
    baglen = np.array([len(b) for b in BAGS], np.uint32)
    items = np.array([sum((c == "G") << j for j, c in enumerate(b)) for b in BAGS], np.uint32)
    return (as_u32(facing) << sc.F_FACING | as_u32(doors) << sc.F_OBJ
            | as_u32(handles) << (sc.F_OBJ + 3) | as_u32(bolt) << (sc.F_OBJ + 5)
            | baglen[bag] << sc.F_BAGLEN | items[bag] << sc.F_BAGITEM)


class Sweep:
    """n cases: the columns below, and ``states(lo, hi)`` / ``actions``"""
    COLS = ("px", "py", "doors", "handles", "bolt", "bag", "facing", "action")

    def __init__(self, name, level_dir, tier, cols):
        self.name, self.level_dir, self.tier = name or "default", level_dir, tier
        self.lv = read_level(level_dir)
        n = len(cols["px"])
        perm = np.random.RandomState(PERM_SEED).permutation(n)
        for k in self.COLS:
            setattr(self, k, np.ascontiguousarray(np.asarray(cols[k], np.int32)[perm]))
        self.n = n
        self.cx = self.px // S
        self.cy = (self.py + S // 2) // S
        self.objs = bag_objs(self.lv, self.bag)
        f = pack_flags(self.facing, self.doors, self.handles, self.bolt, self.bag)
        self.flags = np.ascontiguousarray(f, np.uint32)   # jump_ticker 0
        self.pos = np.ascontiguousarray(np.stack([self.px, self.py], 1), np.int32)
        up = np.stack([self.handles & 1, self.handles >> 1 & 1], 1)
        self.ang = np.ascontiguousarray(np.where(up == 1, 0.9, 0.1), np.float64)
        self.actions = self.action

    def states(self, lo=0, hi=None, mt=True):
        """cases [lo, hi) as one batch state (write_state's argument); mt False: no streams"""
        hi = self.n if hi is None else hi
        st = {"pos": self.pos[lo:hi], "flags": self.flags[lo:hi], "objs": self.objs[lo:hi],
              "ang": self.ang[lo:hi], "ep": np.zeros((hi - lo, 2), np.int32)}
        if mt:
            import oracle
            st["mt"], st["mt_pos"] = oracle.stream_states(STREAM_BASE, lo, hi - lo)
        return st

    def describe(self, i):
        return ("level %s case %d: px %d py %d cell (%d, %d) doors %s handles %s bolt %d bag %s "
                "facing %d action %d (%s)"
                % (self.name, i, self.px[i], self.py[i], self.cx[i], self.cy[i],
                   format(int(self.doors[i]), "03b"), format(int(self.handles[i]), "02b"),
                   self.bolt[i], BAG_NAMES[self.bag[i]], self.facing[i], self.action[i],
                   OPTIONS[self.action[i]]))


def _cols():
    return {k: [] for k in Sweep.COLS}


def _add(c, **kw):
    """append the broadcast of the given columns (arrays of one shape, or scalars)"""
    arrs = np.broadcast_arrays(*[np.asarray(kw[k]) for k in Sweep.COLS])
    for k, a in zip(Sweep.COLS, arrs):
        c[k].append(a.ravel())


def _finish(name, level_dir, tier, c):
    return Sweep(name, level_dir, tier, {k: np.concatenate(v) for k, v in c.items()})


@functools.lru_cache(maxsize=None)
def mask_tier(name=None):
    level_dir = LEVELS[name]
    lv = read_level(level_dir)
    ground, _ = positions(level_dir)
    ys, xs = np.nonzero(ground)
    doors = np.arange(8)
    bags = np.array([0, 1, 5, 2, 3, 6])   # key home / in bag / used x gold home / in bag
    h0 = sum(int(h[2]) << i for i, h in enumerate(lv["handle"]))
    c = _cols()
    _add(c, px=xs[:, None, None], py=ys[:, None, None], doors=doors[None, :, None],
         handles=h0, bolt=int(lv["bolt"][0][2]), bag=bags[None, None, :], facing=1, action=0)
    return _finish(name, level_dir, "mask", c)


def step_positions(level_dir):
    """(selected standing positions [(px, py)], cells near an object, airborne [(px, py)])"""
    lv = read_level(level_dir)
    ground, air = positions(level_dir)
    sel = []
    ys, xs = np.nonzero(ground)
    cell = {}
    for x, y in zip(xs.tolist(), ys.tolist()):
        cell.setdefault((x // S, (y + S // 2) // S), []).append((x, y))
    for (cx, cy), pts in sorted(cell.items()):
        pys = sorted(set(y for _, y in pts))
        have = set(pts)
        seen = set()
        for y in (pys[0], pys[len(pys) // 2], pys[-1]):
            row = sorted(x for x, yy in pts if yy == y)
            c = cx * S + S // 2
            for x in (row[0], c - 5, c - 4, c - 3, c, c + 3, c + 4, c + 5, row[-1]):
                x = min(max(x, row[0]), row[-1])
                if (x, y) in have and (x, y) not in seen:
                    seen.add((x, y))
                    sel.append((x, y))
    homes = [o[:2] for k in ("handle", "bolt", "key", "gold") for o in lv[k]]
    near = set(c for c in cell if any(abs(c[0] - hx) <= 1 and abs(c[1] - hy) <= 1 for hx, hy in homes))
    airborne = []
    ays, axs = np.nonzero(air)
    acell = {}
    for x, y in zip(axs.tolist(), ays.tolist()):
        acell.setdefault((x // S, (y + S // 2) // S), []).append((x, y))
    for (cx, cy), pts in sorted(acell.items()):
        if lv["rows"][cy][cx] != " ":
            continue
        want = (cx * S + S // 2, cy * S)   # the middle of the cell, or the cell's nearest to it
        airborne.append(min(pts, key=lambda p: (abs(p[0] - want[0]) + abs(p[1] - want[1]), p)))
    return sel, near, airborne


@functools.lru_cache(maxsize=None)
def step_tier(name=None, draws=None):
    level_dir = LEVELS[name]
    draws = LEVEL_DRAWS[name] if draws is None else draws
    sel, near, airborne = step_positions(level_dir)
    rnd = random.Random(DRAW_SEED)

    def bits(shape):
        k = int(np.prod(shape))
        b = np.frombuffer(rnd.getrandbits(32 * k).to_bytes(4 * k, "little"), np.uint32)
        return b.reshape(shape).astype(np.int64)

    doors = np.arange(8)[:, None, None]
    acts = np.arange(9)[None, :, None]
    c = _cols()
    for x, y in sel:
        b = bits((8, 9, draws))
        _add(c, px=x, py=y, doors=doors, handles=b & 3, bolt=b >> 2 & 1, bag=(b >> 8 & 0xFFFF) % 7,
             facing=b >> 3 & 1, action=acts)
        if (x // S, (y + S // 2) // S) in near:
            b = bits((4, 2, 7, 9))
            _add(c, px=x, py=y, doors=b >> 4 & 7, handles=np.arange(4)[:, None, None, None],
                 bolt=np.arange(2)[None, :, None, None], bag=np.arange(7)[None, None, :, None],
                 facing=b >> 3 & 1, action=np.arange(9)[None, None, None, :])
    for x, y in airborne:
        b = bits((9, draws))
        _add(c, px=x, py=y, doors=b >> 4 & 7, handles=b & 3, bolt=b >> 2 & 1, bag=(b >> 8 & 0xFFFF) % 7,
             facing=b >> 3 & 1, action=np.arange(9)[:, None])
    return _finish(name, level_dir, "step", c)


# ---- streams ------------------------------------------------------------------------------------
def twist(mt):
    """the generations after mt [k, 624] (genrand_uint32's twist, column by column)"""
    mt = np.array(mt, np.uint32)
    for kk in range(624):
        y = (mt[:, kk] & np.uint32(0x80000000)) | (mt[:, (kk + 1) % 624] & np.uint32(0x7FFFFFFF))
        mt[:, kk] = mt[:, (kk + 397) % 624] ^ (y >> np.uint32(1)) ^ np.where(
            y & np.uint32(1), np.uint32(0x9908B0DF), np.uint32(0))
    return mt


def successor_form(mt, pos):
    """(mt, pos) with every (generation, 624) as (successor generation, 0): the same streams"""
    mt, pos = np.array(mt, np.uint32), np.array(pos, np.uint32)
    at_end = pos == 624
    if at_end.any():
        mt[at_end] = twist(mt[at_end])
        pos[at_end] = 0
    return mt, pos


def streams_differ(got_mt, got_pos, ref_mt, ref_pos):
    """indices of the cases whose (mt, index) pairs do not continue as the same stream
    (state_codec.same_stream decides; equal tuples and equal successor forms are the same
    stream, so only the others are replayed)"""
    got_pos, ref_pos = np.asarray(got_pos), np.asarray(ref_pos)
    cand = np.flatnonzero((got_pos != ref_pos) | (got_mt != ref_mt).any(axis=1))
    if len(cand):
        a, ap = successor_form(got_mt[cand], got_pos[cand])
        b, bp = successor_form(ref_mt[cand], ref_pos[cand])
        cand = cand[(ap != bp) | (a != b).any(axis=1)]
    return [int(i) for i in cand
            if not sc.same_stream((got_mt[i], got_pos[i]), (ref_mt[i], ref_pos[i]))]


# ---- comparison ---------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def compare(sw, lo, got, ref, what, fields=None):
    """``got`` (the product's outputs for cases [lo, lo + k)) against ``ref`` (oracle.step_states
    of the same cases), exactly.  A capped case is compared only in that E_TICKCAP is set; no
    other case may carry an error bit.  The message names the first differing case and field."""
    k = len(ref["mask"])
    capped = ref["capped"].astype(bool) if "capped" in ref else np.zeros(k, bool)
    live = ~capped
    bad = {}   # case -> first differing field

    def note(idx, field):
        for i in np.atleast_1d(idx).tolist():
            bad.setdefault(int(i), field)

    if "mask" in got:
        note(np.flatnonzero(np.asarray(got["mask"]).astype(np.int64) & 0x1FF != ref["mask"]), "mask")
    if "flags" in got:
        err = np.asarray(got["flags"], np.uint32) >> 24
        note(np.flatnonzero(capped & (err != E_TICKCAP >> 24)), "errors (E_TICKCAP alone expected)")
        note(np.flatnonzero(live & (err != 0)), "errors")
    for f in fields or ("obs", "reward", "valid", "done", "pos", "flags", "objs", "ang",
                        "ticks", "draws"):
        if f not in got:
            continue
        g, r = np.asarray(got[f]), ref[f]
        if f in ("obs", "ang"):
            g, r = _bits(g), _bits(r)
        if f == "flags":
            g = g & np.uint32(0x00FFFFFF)
        d = g.astype(np.int64) != r.astype(np.int64) if g.dtype != np.uint64 else g != r
        if d.ndim > 1:
            d = d.any(axis=1)
        note(np.flatnonzero(d & live), f)
    if "mt" in got and "mt" in ref:
        for j in streams_differ(got["mt"], got["mt_pos"], ref["mt"], ref["mt_pos"]):
            if live[j]:
                note(j, "stream")
    if bad:
        i = min(bad)
        f = bad[i]
        detail = ""
        if f in got and f in ref:
            detail = ": got %s, oracle %s" % (np.asarray(got[f])[i].tolist(), ref[f][i].tolist())
        elif f.startswith("errors"):
            detail = ": flags %#x, oracle capped %d" % (int(got["flags"][i]), int(capped[i]))
        raise AssertionError("%s: %d of %d cases differ; first: %s; field %s%s"
                             % (what, len(bad), k, sw.describe(lo + i), f, detail))
