"""Options that outlast the staged code window, through the product API against the oracle.

The plain phases of the go and ladder options take their ticks by multi-draw hops over the
window's code dwords (tg_core.h walk_hops, RngCodes::walk) and the step's epilogue no longer
waits behind its own result stores (RngCodes::drain / finish).  Both sit on paths that only long
options exercise: a walk that runs into the window's end, a refill in the middle of a span, a
half boundary of the MT ring crossed inside an option.  So every case first shows, from the
oracle's own run on the CPU (the first PROBE envs stepped one by one), that its run contains
such options, and then compares every env of the batch: the trajectory hash (per-step API:
compact and direct modes) or every output row (flow rollouts), each env's draw count through
its MT position, and the launch counters' draws and ticks.

Sizes: 192 (one partly filled workgroup), 1,000 (ragged), 4,096 on the default level.  Levels:
the default one (options of up to ~105 draws: more than one 64-draw window, never more than
two, so its cases cannot show an option of more than 128 draws and assert the other two
properties) and tests/golden/levels/corridor (~650 draws per option: ten windows).  Both
policies, auto-reset on, 300 steps, every step mode (all three run the changed walk; compact
and direct the changed epilogue)."""
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import run_gpu

pytestmark = pytest.mark.gpu

CORRIDOR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels", "corridor")
STEPS, A0, SEED = 300, 0x77, 1000  # (the oracle has no tick cap: a seed whose corridor options all end)
PROBE = 32
WINDOW = 64            # draws a filled window stages (tg_dev.h WIN_DRAWS)
HALF_DRAWS = 8 * 312   # draws per half of an env's MT ring (tg_core.h MT_HALF / 2)

CASES = [(None, 192), (None, 1000), (None, 4096), ("corridor", 192), ("corridor", 1000)]


def option_draws(oracle, level_dir, masked):
    """(draws before, draws of the option) of every step of the run's first PROBE envs, from
    oracle envs stepped one at a time with the run's actions (the reset's draws not included)"""
    out = []
    for g in range(PROBE):
        e = oracle.OracleEnv(SEED + g, level_dir=level_dir)
        for t in range(STEPS):
            a = oracle.pick_action(A0, g, t, masked, e.mask() if masked else 0)
            d0 = e.draws()
            _, _, done, _ = e.step(a)
            out.append((d0, e.draws() - d0))
            if done:
                e.reset()
    return np.array(out, np.int64)


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's run and the probe of its options per (level, n, policy): computed once,
    shared by the modes, never written to"""
    cache = {}

    def get(level, n, policy):
        key = (level, n, policy)
        if key not in cache:
            ld = CORRIDOR if level else None
            pk = (level, policy)
            if pk not in cache:
                cache[pk] = option_draws(oracle, ld, bool(policy))
            r = oracle.run(SEED, 0, n, STEPS, A0, policy, True, level_dir=ld)
            r.pop("final_obs", None)
            cache[key] = (r, cache[pk])
        return cache[key]

    return get


def assert_run_outlasts_windows(probe, level):
    d0, d = probe[:, 0], probe[:, 1]
    assert (d > WINDOW).any(), "no option of more than one window"
    if level:  # the default level's longest option is ~105 draws (module docstring)
        assert (d > 2 * WINDOW).any(), "no option of more than two windows"
    # a half boundary strictly inside an option: draws on both sides of it
    inside = (d0 // HALF_DRAWS != (d0 + d - 1) // HALF_DRAWS) & (d > 1) & (d0 % HALF_DRAWS != 0)
    assert inside.any(), "no env crosses an MT half boundary inside an option"


@pytest.mark.parametrize("mode", ["compact", "direct", "flow"])
@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("level,n", CASES)
def test_long_options_vs_oracle(tg, refs, level, n, policy, mode):
    r, probe = refs(level, n, policy)
    assert_run_outlasts_windows(probe, level)
    ld = CORRIDOR if level else None
    if mode == "flow":
        vec = tg.TreasureGameVec(n, seed=SEED, autoreset=True, level_dir=ld)
        vec.set_mode("flow")
        obs0 = vec.reset().cpu().numpy()
        assert np.array_equal(obs0.view(np.uint64), r["obs"][:, 0].view(np.uint64))
        for t0 in range(0, STEPS, 100):
            o = vec.rollout(100, t0=t0, action_seed=A0, policy="masked" if policy else "uniform",
                            actions=False)
            got = o["obs"].cpu().numpy().transpose(1, 0, 2)
            bad = np.flatnonzero((got.view(np.uint64) != r["obs"][:, t0 + 1:t0 + 101].view(np.uint64))
                                 .any(axis=(1, 2)))
            assert len(bad) == 0, "obs from step %d: %d envs differ, first %s" % (t0, len(bad), bad[:8].tolist())
            for key in ("reward", "valid", "done"):
                assert np.array_equal(o[key].cpu().numpy().T, r[key][:, t0 + 1:t0 + 101]), (key, t0)
        stats, errors = vec.stats(), vec.errors()
    else:
        g = run_gpu(tg, SEED, 0, n, STEPS, A0, policy, True, hash_only=True, mode=mode, level_dir=ld)
        bad = np.flatnonzero(g["hash"] != r["hash"])
        assert len(bad) == 0, "%d envs differ, first %s" % (len(bad), bad[:8].tolist())
        vec, stats, errors = g["vec"], g["stats"], g["errors"]
    # each env's draws, through its position in the MT generation (624 words, two per draw)
    pos = np.asarray(vec.read_state(mt=True)["mt_pos"]).astype(np.int64)
    bad = np.flatnonzero(pos % 624 != (2 * r["draws"]) % 624)
    assert len(bad) == 0, "draws: %d envs differ, first %s" % (len(bad), bad[:8].tolist())
    assert stats["draws"] == int(r["draws"].sum()) - 8 * n  # minus construct + reset
    assert stats["ticks"] == int(r["ticks"].sum())
    assert errors == 0
    vec.close()
