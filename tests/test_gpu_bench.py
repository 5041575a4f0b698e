"""bench.py's own surface: what ``--dump-outputs`` writes is what the last timed step returned
(checked against the oracle's replay of the run), its sample is the same for every array and
from call to call, and a plain run leaves the ``--full`` legs out of its line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WARM, BURN, STEPS = 4096, 2, 30, 12


def _measured(tg, policy, extra=()):
    import bench
    import gym_treasure_game_amd.dist as D
    args = bench.parse(["--envs", str(N), "--policy", policy, "--steps", str(STEPS), "--warmup",
                        str(WARM), "--burn-in", str(BURN)] + list(extra))
    run = bench.Runner(tg, D, args, policy, N, 0, 1, torch.device("cuda", 0), keep_log=True)
    run.measure(WARM, BURN, STEPS)
    return bench, run


@pytest.fixture(scope="module")
def replay(oracle):
    """the oracle's replay of the run, per policy (computed once)"""
    import bench
    return {pol: oracle.run(0, 0, N, WARM + BURN + STEPS, bench.ACTION_SEED, k, True)
            for k, pol in enumerate(("uniform", "masked"))}


@pytest.mark.parametrize("policy", ["uniform", "masked"])
def test_outputs_are_the_last_timed_step(tg, replay, policy):
    """Runner.outputs() after measure(): obs f64, reward f64, valid / done f32 of every env ==
    the oracle's step WARM + BURN + STEPS (uniform: the actions pre-generated before the timed
    region; masked: generated in the loop)."""
    bench, run = _measured(tg, policy)
    out = run.outputs()
    ref = replay[policy]
    assert sorted(out) == ["done", "env_index", "obs", "reward", "valid"]
    assert [out[k].dtype for k in sorted(out)] == [np.float32, np.float64, np.float64, np.float64,
                                                   np.float32]
    assert np.array_equal(out["env_index"], np.arange(N))
    assert_bits(out["obs"], ref["obs"][:, -1], "obs")
    for k in ("reward", "valid", "done"):
        assert np.array_equal(out[k], ref[k][:, -1].astype(out[k].dtype)), k
    assert run.vec.errors() == 0
    run.vec.close()


def test_outputs_sample_is_fixed_and_shared(tg, replay, monkeypatch):
    """Past the byte limit every array holds the same seeded choice of envs (sorted, distinct,
    global indices), the same from call to call, and the arrays stay within the limit."""
    bench, run = _measured(tg, "masked")
    monkeypatch.setattr(bench, "DUMP_BYTES", 96 * 1000 + 50)
    a, b = run.outputs(), run.outputs()
    idx = a["env_index"].astype(np.int64)
    assert len(idx) == 1000 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < N
    assert 0 < np.count_nonzero(np.diff(idx) > 1)  # a choice over the batch, not a leading block
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    ref = replay["masked"]
    assert_bits(a["obs"], ref["obs"][idx, -1], "obs")
    for k in ("reward", "valid", "done"):
        assert np.array_equal(a[k], ref[k][idx, -1].astype(a[k].dtype)), k
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    run.vec.close()


def test_rollout_outputs_are_its_last_row(tg, replay):
    """--rollout K: the last row of the last tg_rollout call (a shorter one: 12 steps = 8 + 4)."""
    bench, run = _measured(tg, "masked", ["--rollout", "8"])
    out = run.outputs()
    assert sorted(out) == ["done", "env_index", "reward", "valid"] and run.roll_k == 4
    for k in ("reward", "valid", "done"):
        assert np.array_equal(out[k], replay["masked"][k][:, -1].astype(out[k].dtype)), k
    run.vec.close()


def test_plain_run_line_and_dump(tmp_path):
    """bench.py as a command: --steps sets the timed steps, the line carries ms_per_step, a
    plain run has none of the --full legs, and --dump-outputs writes float arrays."""
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "7", "--warmup", "2", "--envs", str(N), "--burn-in", "20",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["unit"] == "env-steps/s"
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - N / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["episodes_gathered"] == line["episodes"] - line["episodes_dropped"]
    for k in ("cpu_baseline", "parity_check", "episode_check", "masked_policy", "dropin_n1"):
        assert k not in line, k
    assert line["roofline"]["step"]["region_probe"] is None
    assert sorted(os.listdir(d)) == ["done.npy", "env_index.npy", "obs.npy", "reward.npy",
                                     "valid.npy"]
    for f in os.listdir(d):
        a = np.load(d / f)
        assert a.dtype in (np.float32, np.float64) and len(a) == N, f
