"""The step kernels stepped once from every synthesized state of tests/state_sweep.py, against
the C oracle, exactly: write_state(states), available_mask(), one step (tg_step in the compact
and direct modes; rollout(1) with both synthetic policies in the flow mode, and once in the
compact mode), read_state(mt=True), errors().  The mask tier and the step tier of the default
level, the step tier of corridor, exit and cascade, in parts of 64 Ki cases (one handle per
level; the last part overlaps the one before it, so every part has the handle's size).

Compared per case: mask, obs bits, reward, valid, done, the state after (pos, flags without
the error bits, objs, angle bits), the stream after; per part the tick and draw totals
(tg_stats).  A case the oracle stops at the tick limit must carry TG_ERR_TICKCAP and nothing
else (its other outputs are not compared); no other case may carry an error bit.  The oracle
side is pinned on the CPU by test_oracle_state.py, the state set by test_state_sweep_host.py."""
import functools

import numpy as np
import pytest
import torch

import state_sweep as ss

pytestmark = pytest.mark.gpu

PART = 1 << 16
MASK_PART = 1 << 18
A0 = 0x5EED0007
TICKCAP = 1 << 24
# the step tiers' case counts: the part lists are built from them at collection, without the
# builder (which needs the oracle built); test_part_lists_cover_the_tiers holds them to it
STEP_TIERS = ((None, 626580), ("corridor", 464616), ("exit", 209952), ("cascade", 209952))
MASK_TIER = 1386432
KINDS = ("compact", "direct", "flow-uniform", "flow-masked")


def part_bounds(n, size, part):
    lo = min(part * size, max(n - size, 0))
    return lo, min(lo + size, n)


def nparts(n, size):
    return (n + size - 1) // size


_VEC = {}


def get_vec(tg, name, n):
    """the one live handle: n envs on level ``name``, no auto-reset"""
    key = (name, n)
    if _VEC.get("key") != key:
        if "vec" in _VEC:
            _VEC.pop("vec").close()
        _VEC["vec"] = tg.TreasureGameVec(n, seed=1, autoreset=False, level_dir=ss.LEVELS[name])
        _VEC["key"] = key
    return _VEC["vec"]


@pytest.fixture(scope="module", autouse=True)
def _close_handle():
    yield
    if "vec" in _VEC:
        _VEC.pop("vec").close()
    _VEC.clear()


@functools.lru_cache(maxsize=1)
def part_states(name, part):
    sw = ss.step_tier(name)
    lo, hi = part_bounds(sw.n, PART, part)
    return sw, lo, hi, sw.states(lo, hi)


@functools.lru_cache(maxsize=1)
def part_reference(name, part):
    """oracle.step_states of the part with the sweep's own actions (the threaded oracle, once
    for the modes that share it)"""
    import oracle
    sw, lo, hi, st = part_states(name, part)
    return oracle.step_states(st, sw.actions[lo:hi], level_dir=sw.level_dir)


def after_step(vec, out_obs, reward, valid, done, mask):
    got = dict(vec.read_state(mt=True))
    got.update(mask=mask, obs=out_obs.cpu().numpy(), reward=reward.cpu().numpy(),
               valid=valid.cpu().numpy(), done=done.cpu().numpy())
    return got


def check_errors(vec, got, ref):
    err = vec.errors()
    assert err & ~TICKCAP == 0, hex(err)
    if ref["capped"].any():
        assert err & TICKCAP


STEP_CASES = [(name, part, kind) for name, n in STEP_TIERS
              for part in range(nparts(n, PART)) for kind in KINDS]
STEP_CASES += [(None, 0, "compact-uniform"), (None, 0, "compact-masked")]


def test_part_lists_cover_the_tiers(oracle):
    for name, n in STEP_TIERS:
        assert ss.step_tier(name).n == n, name
    assert ss.mask_tier().n == MASK_TIER


@pytest.mark.parametrize("name,part,kind", STEP_CASES,
                         ids=["%s-%d-%s" % (n or "default", p, k) for n, p, k in STEP_CASES])
def test_step_tier(tg, oracle, name, part, kind):
    sw, lo, hi, st = part_states(name, part)
    n = hi - lo
    mode, _, policy = kind.partition("-")
    vec = get_vec(tg, name, n)
    vec.set_mode(mode)
    vec.write_state(st)
    mask = vec.available_mask().cpu().numpy().copy()
    what = "step tier, %s, part %d" % (kind, part)
    if not policy:
        ref = part_reference(name, part)
        vec.stats_reset()
        o, r, v, d, _ = vec.step(torch.as_tensor(sw.actions[lo:hi]))
        got = after_step(vec, o, r, v, d, mask)
        ss.compare(sw, lo, got, ref, what)
        s = vec.stats()
        assert s["steps"] == n and s["valid_steps"] == int(ref["valid"].sum()), what
        assert s["ticks"] == int(ref["ticks"].sum()), what
        assert s["draws"] == int(ref["draws"].sum()), what
    else:
        # the step is the rollout's: its action is the hash's, from the mask where masked
        masks = oracle.step_states(st, level_dir=sw.level_dir)["mask"]
        act = np.array([oracle.pick_action(A0, g, part, policy == "masked", int(masks[g]))
                        for g in range(n)], np.int32)
        ref = oracle.step_states(st, act, level_dir=sw.level_dir)
        out = vec.rollout(1, t0=part, action_seed=A0, policy=policy)
        a = out["actions"][0].cpu().numpy()
        bad = np.flatnonzero(a != act)
        assert len(bad) == 0, "%s: action %d, reference %d: %s" % (
            what, a[bad[0]], act[bad[0]], sw.describe(lo + int(bad[0])))
        got = after_step(vec, out["obs"][0], out["reward"][0], out["valid"][0], out["done"][0], mask)
        ss.compare(sw, lo, got, ref, what)
    check_errors(vec, got, ref)


MASK_PARTS = list(range(nparts(MASK_TIER, MASK_PART)))


@pytest.mark.parametrize("part", MASK_PARTS)
def test_mask_tier(tg, oracle, part):
    """available_mask alone (no option runs; the streams are any valid ones)"""
    sw = ss.mask_tier()
    lo, hi = part_bounds(sw.n, MASK_PART, part)
    st = sw.states(lo, hi, mt=False)
    ref = oracle.step_states(st, level_dir=sw.level_dir)
    st["mt"], st["mt_pos"] = np.zeros((hi - lo, 624), np.uint32), np.zeros(hi - lo, np.uint32)
    st["mt"][:, 0] = 0x80000000   # (any words do; all zero would be MT19937's fixed point)
    vec = get_vec(tg, None, hi - lo)
    vec.set_mode("compact")
    vec.write_state(st)
    got = {"mask": vec.available_mask().cpu().numpy()}
    ss.compare(sw, lo, got, ref, "mask tier, part %d" % part)
    assert vec.errors() == 0
