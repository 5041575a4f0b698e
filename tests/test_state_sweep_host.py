"""The product's per-env core (host build, tests/native) stepped once from every synthesized
state of tests/state_sweep.py, against the C oracle, exactly: the mask tier and the full step
tier on the default level, the step tier on corridor, exit and cascade, each with the go-target
table and the level bitmasks on and off (hc_set_gotab x hc_set_masks).  The reference-only
conditions of the state set are checked first."""
import ctypes
import functools
import os

import numpy as np
import pytest

import state_sweep as ss

CHUNK = 1 << 15
THREADS = min(16, os.cpu_count() or 1)
SETTINGS = [(1, 1), (0, 1), (1, 0), (0, 0)]   # (gotab, masks); the device's setting first


def level_texts(sw):
    if sw.name == "default":
        return None, None, None   # the built-in level
    return tuple(open(os.path.join(sw.level_dir, f), "rb").read()
                 for f in ("domain.txt", "domain-objects.txt", "domain-interactions.txt"))


def hc_step_states(lib, sw, states, actions=None):
    P = ctypes.c_void_p
    lib.hc_step_states.restype = ctypes.c_int
    lib.hc_step_states.argtypes = [P, P, P, ctypes.c_int64] + [P] * 20 + [ctypes.c_int]
    lib.hc_set_masks.argtypes = [ctypes.c_int]
    n = len(states["pos"])
    out = {"mask": np.zeros(n, np.uint16)}
    if actions is not None:
        out.update(obs=np.zeros((n, 9), np.float64), reward=np.zeros(n, np.int32),
                   valid=np.zeros(n, np.uint8), done=np.zeros(n, np.uint8),
                   pos=np.zeros((n, 2), np.int32), flags=np.zeros(n, np.uint32),
                   objs=np.zeros((n, 4), np.int32), ang=np.zeros((n, 2), np.float64),
                   mt=np.zeros((n, 624), np.uint32), mt_pos=np.zeros(n, np.uint32),
                   ticks=np.zeros(n, np.int64), draws=np.zeros(n, np.int64))

    def p(a):
        return None if a is None else np.ascontiguousarray(a).ctypes.data_as(P)

    ins = [np.ascontiguousarray(states[k]) for k in ("pos", "flags", "objs", "ang")]
    ins += [np.ascontiguousarray(states[k]) if k in states else None for k in ("mt", "mt_pos")]
    ins.append(None if actions is None else np.ascontiguousarray(actions, np.int32))
    g = out.get
    rc = lib.hc_step_states(*level_texts(sw), n,
                            *[p(a) for a in ins], p(g("obs")), p(g("reward")), p(g("valid")),
                            p(g("done")), p(out["mask"]), p(g("pos")), p(g("flags")), p(g("objs")),
                            p(g("ang")), p(g("mt")), p(g("mt_pos")), p(g("ticks")), p(g("draws")),
                            THREADS)
    assert rc == 0
    return out


def each_setting(lib):
    for gotab, masks in SETTINGS:
        try:
            lib.hc_set_gotab(gotab)
            lib.hc_set_masks(masks)
            yield "gotab %d masks %d" % (gotab, masks)
        finally:
            lib.hc_set_gotab(1)
            lib.hc_set_masks(1)


@functools.lru_cache(maxsize=None)
def reference_summary(name):
    """oracle.step_states over a whole step tier, the stream words left out"""
    import oracle
    sw = ss.step_tier(name)
    parts = []
    for lo in range(0, sw.n, CHUNK):
        hi = min(lo + CHUNK, sw.n)
        r = oracle.step_states(sw.states(lo, hi), sw.actions[lo:hi], level_dir=sw.level_dir,
                               mt_out=False)
        parts.append({k: r[k] for k in ("valid", "capped", "mask", "ticks")})
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def test_state_set_is_deterministic_and_sized(oracle):
    sw = ss.step_tier()
    print("default level: step tier %d cases, mask tier %d cases" % (sw.n, ss.mask_tier().n))
    assert 200_000 <= sw.n <= 1_000_000
    ss.step_tier.cache_clear()
    again = ss.step_tier()
    for k in ss.Sweep.COLS + ("flags", "objs"):
        assert np.array_equal(getattr(sw, k), getattr(again, k)), k
    ground, _ = ss.positions(sw.level_dir)
    ys, xs = np.nonzero(ground)
    assert len(xs) == 28884 and len(set(zip((xs // 48).tolist(), ((ys + 24) // 48).tolist()))) == 70
    assert ss.mask_tier().n == 28884 * 8 * 6
    # close_x's threshold on both sides, in every door pattern, for every action
    off = sw.px - (sw.cx * 48 + 24)
    for d in (-5, -4, -3, 0, 3, 4, 5):
        sel = off == d
        assert len(set(zip(sw.doors[sel].tolist(), sw.action[sel].tolist()))) == 72, d
    for name in ("corridor", "exit", "cascade"):
        other = ss.step_tier(name)
        print("%s: step tier %d cases" % (name, other.n))
        assert other.n >= 100_000


def test_state_set_reference_conditions(oracle):
    """from the oracle alone, on the default level's step tier: at most 5 % of the cases hit
    the tick limit, at least 15 % run an option, every option runs from at least 1,000 cases,
    and every (door pattern, bag state) pair occurs"""
    sw = ss.step_tier()
    r = reference_summary(None)
    capped, ran = r["capped"].astype(bool), r["valid"].astype(bool)
    per_option = np.bincount(sw.action[ran], minlength=9)
    print("step tier %d: capped %d (%.2f %%), ran %d (%.1f %%), per option %s"
          % (sw.n, capped.sum(), 100.0 * capped.mean(), ran.sum(), 100.0 * ran.mean(),
             per_option.tolist()))
    assert capped.mean() <= 0.05
    assert ran.mean() >= 0.15
    assert per_option.min() >= 1000, per_option.tolist()
    assert len(set(zip(sw.doors.tolist(), sw.bag.tolist()))) == 8 * 7
    assert len(set(zip(sw.doors[ran].tolist(), sw.bag[ran].tolist()))) == 8 * 7
    assert (r["ticks"][capped] == ss.TICK_CAP).all() and (r["ticks"][~capped] < ss.TICK_CAP).all()


def test_mask_tier_default(hostcheck, oracle):
    sw = ss.mask_tier()
    st = sw.states(mt=False)
    ref = oracle.step_states(st, level_dir=sw.level_dir)
    for k in range(9):   # every option can run from some of the states and not from others
        assert 0 < int((ref["mask"] >> k & 1).sum()) < sw.n, k
    for setting in each_setting(hostcheck):
        ss.compare(sw, 0, hc_step_states(hostcheck, sw, st), ref, "mask tier, " + setting)


@pytest.mark.parametrize("name", [None, "corridor", "exit", "cascade"])
def test_step_tier(hostcheck, oracle, name):
    sw = ss.step_tier(name)
    ncap = 0
    for lo in range(0, sw.n, CHUNK):
        hi = min(lo + CHUNK, sw.n)
        st, act = sw.states(lo, hi), sw.actions[lo:hi]
        ref = oracle.step_states(st, act, level_dir=sw.level_dir)
        ncap += int(ref["capped"].sum())
        for setting in each_setting(hostcheck):
            ss.compare(sw, lo, hc_step_states(hostcheck, sw, st, act), ref,
                       "step tier, " + setting)
    assert ncap > 0 or name == "corridor"   # the tick limit is met: E_TICKCAP is compared
