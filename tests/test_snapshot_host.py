"""The snapshot slot's code (csrc/tg_snapshot.h) on the CPU: its host-only build
(tests/native_snapshot) against CPython's ``random`` and tests/state_codec.py.  The gather of the
generation holding an env's position from every generation of the ring, the per-lane rebuild of
a ring from a slot, the slot codec on reference fixture rows, and the header's stand-alone
compile.  No GPU."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import state_codec as sc
from conftest import ROOT

MT_N, GENS = 624, 16
MT_STALE, MT_LISTED = 1 << 31, 1 << 30
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_host = None


def hostlib():
    """tests/native_snapshot's library (built on first use)"""
    global _host
    if _host is None:
        d = os.path.join(ROOT, "tests", "native_snapshot")
        subprocess.check_call(["make", "-s", "-C", d])
        L = ctypes.CDLL(os.path.join(d, "libtg_hostcheck_snapshot.so"))
        P, u32, i64, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64
        L.hs_init.argtypes = [u64, P, P]
        L.hs_init.restype = None
        L.hs_draw.argtypes = [P, P, ctypes.POINTER(u32), i64, P]
        L.hs_draw.restype = None
        L.hs_gather.argtypes = [P, u32, P]
        L.hs_gather.restype = u32
        L.hs_rebuild.argtypes = [P, P, P]
        L.hs_rebuild.restype = None
        L.hs_save.argtypes = [P, u32, P, u32, P, u32, P, P]
        L.hs_save.restype = None
        L.hs_load.argtypes = [P, P, u32, ctypes.c_int, P, ctypes.POINTER(u32), P, ctypes.POINTER(u32), P]
        L.hs_load.restype = None
        _host = L
    return _host


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Ring:
    """one env's ring in host memory: random.seed(seed), then ``draw(k)`` random() calls"""

    def __init__(self, seed=None):
        L = hostlib()
        self.mt = np.zeros(L.hs_ring_words(), np.uint32)
        self.mc = np.zeros(L.hs_ring_codes(), np.uint8)
        self.state = ctypes.c_uint32(0)
        if seed is not None:
            L.hs_init(seed, _p(self.mt), _p(self.mc))

    def draw(self, k):
        out = np.zeros(k, np.uint64)
        hostlib().hs_draw(_p(self.mt), _p(self.mc), ctypes.byref(self.state), k, _p(out))
        return out

    def gather(self):
        gen = np.zeros(MT_N, np.uint32)
        index = hostlib().hs_gather(_p(self.mt), self.state.value, _p(gen))
        return gen, index

    @classmethod
    def rebuilt(cls, gen, index):
        r = cls()
        hostlib().hs_rebuild(_p(r.mt), _p(r.mc), _p(np.ascontiguousarray(gen, np.uint32)))
        r.state.value = index
        return r


def py_bits(rng, k):
    return np.array([rng.random() for _ in range(k)], np.float64).view(np.uint64)


# draws that put the position in every generation of the ring, at index 0, 2, an inner one and
# 622, and past a whole lap of the ring (generations 16..19: both halves regenerated once)
INDICES = (0, 2, 300, 622)
CASES = [(g, i) for g in range(GENS + 4) for i in INDICES]


def test_layout():
    L = hostlib()
    assert L.hs_slot_bytes() == 2536 == 16 + 16 + 8 + 4 * MT_N
    assert L.hs_ring_words() == 8 * MT_N and L.hs_ring_codes() == GENS * MT_N // 2
    # coverage of CASES, from the numbers alone: every ring generation, both halves, odd and even
    gens = {g % GENS for g, _ in CASES}
    assert gens == set(range(GENS)) and {i for _, i in CASES} >= {0, 2, 622}
    assert any(g >= GENS for g, _ in CASES)


@pytest.mark.parametrize("seed", [0, 12345, 2**40 + 17])
def test_gather_is_cpythons_generation(seed):
    ring = Ring(seed)
    ref = random.Random(seed)
    drawn = 0
    for g, i in CASES:
        d = g * (MT_N // 2) + i // 2
        got = ring.draw(d - drawn)
        assert np.array_equal(got, py_bits(ref, d - drawn)), (seed, g, i)
        drawn = d
        pos = ring.state.value & 0xFFFF
        assert pos == (2 * d) % (GENS * MT_N) and pos // MT_N == g % GENS and pos % MT_N == i
        gen, index = ring.gather()
        assert index == i
        want = ref.getstate()[1]
        assert sc.same_stream((gen, index), (want[:MT_N], want[MT_N])), (seed, g, i)
        assert int(sc.ref_index(d)) == want[MT_N]
        if want[MT_N] != MT_N:  # (CPython holds (generation, 624) where the ring says (successor, 0))
            assert index == want[MT_N] and gen.tolist() == list(want[:MT_N]), (seed, g, i)
        else:
            assert index == 0
    # a stale half was left behind on the way and never showed
    assert ring.state.value & MT_STALE


@pytest.mark.parametrize("seed", [7, 99991])
def test_rebuild_continues_the_stream(seed):
    ring = Ring(seed)
    ref = random.Random(seed)
    # the first generation at index 0: the rebuilt ring is the seeded ring, word for word
    gen, index = ring.gather()
    again = Ring.rebuilt(gen, index)
    assert np.array_equal(again.mt, ring.mt) and np.array_equal(again.mc, ring.mc)
    drawn = 0
    for g, i in CASES[::3]:
        d = g * (MT_N // 2) + i // 2
        ring.draw(d - drawn)
        for _ in range(d - drawn):
            ref.random()
        drawn = d
        gen, index = ring.gather()
        fork = Ring.rebuilt(gen, index)
        cont = random.Random()
        cont.setstate(ref.getstate())
        # 2,000 draws: through six generations of the rebuilt ring, codes and words alike
        assert np.array_equal(fork.draw(2000), py_bits(cont, 2000)), (seed, g, i)
    # CPython's own (generation, 624): position 624 of the rebuilt ring is the successor's word 0
    r = random.Random(seed)
    st = r.getstate()[1]
    assert st[MT_N] == MT_N
    fork = Ring.rebuilt(np.array(st[:MT_N], np.uint32), MT_N)
    assert np.array_equal(fork.draw(700), py_bits(r, 700))


def test_slot_codec_round_trips_reference_rows():
    L = hostlib()
    z = sc.load("traj_autoreset.npz")
    rows = [(g, t) for g in range(8) for t in (0, 1, 629, 630, 1500, 2290)]
    assert {str(z["bag"][g, t]) for g, t in rows} >= {"", "K"}
    tstep = 5000
    for n, (g, t) in enumerate(rows):
        st = sc.row_state(z, g, t, mt=False)
        ret, length = (int(x) for x in st["ep"])
        ring_gen, index = n % GENS, (2 * n) % MT_N
        mti = (ring_gen * MT_N + index) | (MT_STALE if n % 2 else 0) | (MT_LISTED if n % 4 == 1 else 0)
        pos = np.ascontiguousarray(st["pos"], np.int32)
        objs = np.ascontiguousarray(st["objs"], np.int32)
        ep = np.array([ret, tstep - length], np.int32)  # Soa::ep: (return, start step)
        s4, sep = np.zeros(4, np.uint32), np.zeros(2, np.int32)
        L.hs_save(_p(pos), int(st["flags"]), _p(objs), mti, _p(ep), tstep, _p(s4), _p(sep))
        assert int(s4[3]) == index and sep.tolist() == [ret, length], (g, t)
        for reseed in (0, 1):
            later = (tstep + 12345) if n % 2 else 2**32 - 3  # (the step counter wraps)
            lpos, lobjs, lep = np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros(2, np.int32)
            f, m = ctypes.c_uint32(), ctypes.c_uint32()
            L.hs_load(_p(s4), _p(sep), later % 2**32, reseed, _p(lpos), ctypes.byref(f), _p(lobjs),
                      ctypes.byref(m), _p(lep))
            back = {"pos": lpos, "flags": np.uint32(f.value), "objs": lobjs}
            assert sc.decode(back) == sc.decode(st), (g, t)
            assert m.value == (0 if reseed else index)
            assert int(lep[0]) == ret and (later - int(np.uint32(lep[1]))) % 2**32 == length


def test_header_compiles_alone(tmp_path):
    unit = tmp_path / "tg_snapshot_unit.hip"
    unit.write_text('#include "%s"\n' % os.path.join(ROOT, "gym-treasure-game_amd", "csrc",
                                                      "tg_snapshot.h"))
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-fsyntax-only", "-std=c++17",
                    "-Wno-unused-command-line-argument", str(unit)], check=True)
