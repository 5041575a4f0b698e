"""The plain phases' multi-draw hops (csrc/tg_core.h: hop_prefix, hop_dist, hop_ticks, walk_hops)
on the CPU: their host-only build (tests/native_walk) against walk_ticks, which specifies them,
and against a tick-by-tick walk written here, over one flat array of code bytes.

The array holds the four codes a draw can have (tg_core.h code_of_top27: r < 0.25, < 0.75,
<= 0.8, > 0.8), drawn with their probabilities from a fixed seed, so every step field takes
every value it can: +2, +3, +4 moving in +, -4, -3, -2 moving in -.

A walk must give the same coordinate, ticks taken and draws consumed for both directions, every
start offset 0..15 inside a 16-code unit, every distance to the span's limit from -1 (outside:
no tick) to 70 px (farther than 16 ticks of the shortest step reach: the cap or the staged draws
end those), `left` from TICK_DRAWS - 1 to 64 and `cap` from 0 to 20."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LOW, MID, HIGH_FLIP, HIGH = 0x20, 0x35, 0x3A, 0x1A  # tg_core.h code_of_top27's four codes
NCODES = 4096
PAD = 16 + 64 + 8  # a sweep reads at most offset 15 + 64 staged codes (+ the dword they end in)


@pytest.fixture(scope="module")
def walk():
    d = os.path.join(ROOT, "tests", "native_walk")
    subprocess.check_call(["make", "-s", "-C", d])
    L = ctypes.CDLL(os.path.join(d, "libtg_walkcheck.so"))
    P, i32, u32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64
    L.wk_tick_draws.restype = i32
    L.wk_walk.argtypes = [P, i32, i32, u32, u32, i32, i32, i32, P]
    L.wk_hop.argtypes = [P, i32, u32, i32, u32, i32, i32, i32, i32, P]
    L.wk_sweep.restype = i64
    L.wk_sweep.argtypes = [P, u32, i32, i32, i32, i32, i32, i32, P, P]
    L.wk_ring.restype = i32
    L.wk_ring.argtypes = [P, u32, i32, ctypes.c_uint64, P]
    return L


@pytest.fixture(scope="module")
def codes():
    r = np.random.RandomState(20261019).random_sample(NCODES + PAD)
    c = np.where(r < 0.25, LOW, np.where(r < 0.75, MID, np.where(r <= 0.8, HIGH_FLIP, HIGH)))
    c = np.ascontiguousarray(c, dtype=np.uint8)
    assert set(np.unique(c)) == {LOW, MID, HIGH_FLIP, HIGH}
    return c


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def py_walk(c, dir_, rd, left, x, lim, cap, tick_draws):
    """walk_ticks, written out: (x, ticks, draws, left)"""
    t = 0
    while (x <= lim if dir_ > 0 else x >= lim) and left >= tick_draws and t < cap:
        b = int(c[rd])
        x += (b & 3) + 2 if dir_ > 0 else ((b >> 2) & 3) - 4
        rd += 1
        left -= 1
        t += 1
    return x, t, t, left


def test_sweep_hops_equal_walk_ticks(walk, codes):
    """the whole grid, at several places of the array (so that the codes differ)"""
    td = walk.wk_tick_draws()
    bad = ctypes.c_int64(0)
    first = np.zeros(13, np.int32)
    total = 0
    for base in (0, 16, 1008, 2048, NCODES - 16):
        n = walk.wk_sweep(_p(codes), base, -1, 70, td - 1, 64, 0, 20, ctypes.byref(bad), _p(first))
        assert bad.value == 0, "base %d: %d of %d differ; first (dir, offset, dist, left, cap) = %s: " \
            "walk_ticks (x, ticks, draws, left) = %s, walk_hops = %s" % (
                base, bad.value, n, first[:5].tolist(), first[5:9].tolist(), first[9:13].tolist())
        total += n
    assert total == 5 * 2 * 16 * 72 * (64 - td + 2) * 21


def test_walks_equal_python_reference(walk, codes):
    """walk_ticks and walk_hops against the walk written in this file, on a sample of the grid
    (the sweep ties the two native forms together over all of it)"""
    td = walk.wk_tick_draws()
    rng = np.random.RandomState(7)
    out = np.zeros(4, np.int32)
    for _ in range(4000):
        base = 16 * int(rng.randint(0, NCODES // 16))
        off = int(rng.randint(0, 16))
        dir_ = 1 if rng.randint(0, 2) else -1
        dist = int(rng.randint(-1, 71))
        left = int(rng.randint(td - 1, 65))
        cap = int(rng.randint(0, 21))
        x0 = int(rng.randint(-50, 700))
        want = py_walk(codes, dir_, base + off, left, x0, x0 + dir_ * dist, cap, td)
        for hops in (0, 1):
            walk.wk_walk(_p(codes[base:]), dir_, hops, off, left, x0, x0 + dir_ * dist, cap, _p(out))
            assert tuple(out.tolist()) == want, (hops, base, off, dir_, dist, left, cap, x0)


def test_hop_takes_all_or_nothing(walk, codes):
    """hop_ticks: all m ticks exactly when the m-th still starts inside the span, with
    TICK_DRAWS staged and under the cap; otherwise the coordinate is untouched"""
    td = walk.wk_tick_draws()
    out = np.zeros(2, np.int32)
    for rd in range(0, 40):
        for m in (1, 2, 3, 4):
            for dir_ in (1, -1):
                steps = [((int(b) & 3) + 2) if dir_ > 0 else (((int(b) >> 2) & 3) - 4)
                         for b in codes[rd:rd + m]]
                before_last = abs(sum(steps[:m - 1]))
                for dist in range(-1, 14):
                    for left, taken, cap in ((64, 0, 20), (td + m - 1, 0, 20), (td + m - 2, 0, 20),
                                             (64, 5, 5 + m), (64, 5, 4 + m), (64, 0, 0)):
                        walk.wk_hop(_p(codes), dir_, rd, m, left, 100, 100 + dir_ * dist, taken, cap, _p(out))
                        want = before_last <= dist and left - (m - 1) >= td and taken + m - 1 < cap
                        assert bool(out[0]) == want, (rd, m, dir_, dist, left, taken, cap)
                        assert out[1] == (100 + sum(steps) if want else 100)


MT_CODES = 2 * 8 * 312  # tg_core.h: one code per draw of an env's ring of 2 x 8 generations


def test_rolling_window_indices(walk):
    """the rolling window's index functions (tg_core.h ring_*) in the refill sequence that
    tests/native_walk simulates (no kernel uses them now: DESIGN.md 3.3), over a
    flat code array whose every byte differs from its neighbours' units (so a read from the
    wrong unit or slot shows): from every start position of the ring, 400 draws in random
    per-tick batches of 0..6 (the wrap at MT_CODES, more than six ring turns).  Every draw read
    is mc[(start + i) % MT_CODES], no slot is refilled while a staged unread draw is in it, and
    reserve(MAX_TICK_DRAWS) always holds; and the window does roll: away from the half
    boundaries the DMAs are the rolling ones, not blocking refills."""
    mc = (np.arange(MT_CODES, dtype=np.uint64) * 2654435761 >> 7).astype(np.uint8)
    mc[mc == 0xEE] = 0x11  # 0xEE marks a slot whose DMA has not landed
    mc = np.ascontiguousarray(mc)
    info = np.zeros(3, np.int32)
    why = {1: "a draw read is not the stream's", 2: "a slot refilled over a staged unread draw",
           3: "reserve(k) left fewer than k draws"}
    for start in range(MT_CODES):
        rc = walk.wk_ring(_p(mc), start, 400, 0x9E3779B97F4A7C15 ^ start, _p(info))
        assert rc == 0, "start %d, draw %d: %s" % (start, info[0], why[rc])
        assert info[0] == 400
        # a run that stays inside one half of the ring (its 400 draws and the 64 staged beyond
        # them) never takes the blocking path: all it reads after the first fill came rolling
        if start % (MT_CODES // 2) + 400 + 64 < MT_CODES // 2:
            assert info[1] == 0 and info[2] >= 400 // 16 - 4, (start, info.tolist())
