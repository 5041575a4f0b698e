"""k_run's quiet drain: a stale MT half whose env cannot run its option in the step that lists it
(a quiet env) is regenerated inside that step's k_run, by its waves without a chunk, instead of
by k_regen up to 16 steps later.  Which kernel writes a half must not show anywhere: rows,
states, MT generations and counters are compared bit for bit with the direct mode (which has
neither list), with the oracle, and between per-step and rollout runs.  No tolerances.

Set-up shared by the cases: masked steps first (an option every step, ~37 draws per env-step:
they carry the envs' positions across the ring), then uniform steps (~4 in 5 envs quiet per
step), which produce crossings followed by quiet steps."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CORRIDOR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels", "corridor")
SEED, A0 = 6, 0x51E7
MT_N, HALF_WORDS, HALF_GENS = 624, 8 * 624, 8  # words per generation / per half of the ring
COUNTERS = ("steps", "valid_steps", "ticks", "draws", "episodes")


def sm64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def rec_hash(h, obs, rew, valid, done):
    """tests/golden/make_golden.py:rec_hash over envs (as test_gpu_parity.py)"""
    bits = np.ascontiguousarray(obs).view(np.uint64)
    for k in range(9):
        h = sm64(h ^ bits[:, k])
    w = (rew.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)) | \
        (valid.astype(np.uint64) << np.uint64(32)) | (done.astype(np.uint64) << np.uint64(40))
    return sm64(h ^ w)


def run_hash(rows):
    n = rows["obs"].shape[0]
    z = np.zeros(n, np.uint8)
    with np.errstate(over="ignore"):
        h = rec_hash(np.arange(n, dtype=np.uint64), rows["obs"][:, 0], np.zeros(n, np.int32), z, z)
        for t in range(1, rows["obs"].shape[1]):
            h = rec_hash(h, rows["final_obs"][:, t], rows["reward"][:, t], rows["valid"][:, t],
                         rows["done"][:, t])
    return h


def step_rows(vec, t, policy):
    """one step; its rows as device tensors (views of the batch's buffers: use before the next)"""
    o, r, v, d, info = vec.step(vec.policy_actions(t, A0, policy))
    return {"obs": o.view(torch.int64), "reward": r, "valid": v, "done": d,
            "final_obs": info["final_obs"].view(torch.int64)}


def blank_rows(n, steps):
    return {"obs": np.zeros((n, steps + 1, 9)), "final_obs": np.zeros((n, steps + 1, 9)),
            "reward": np.zeros((n, steps + 1), np.int32), "valid": np.zeros((n, steps + 1), np.uint8),
            "done": np.zeros((n, steps + 1), np.uint8)}


def keep_rows(rows, t, r):
    for k in rows:
        x = r[k].cpu().numpy()
        rows[k][:, t] = x.view(np.float64) if k in ("obs", "final_obs") else x


@functools.lru_cache(maxsize=None)
def mode_pair(n, level, pre, uni, keep):
    """The batch stepped in compact and in direct mode side by side, `pre` masked then `uni`
    uniform steps, every step's rows compared on the device as they are written.  Returns the
    compact side's rows (keep), whether the final states are equal, both sides' counters, and the compact side's
    counters over the uniform part.  Computed once per case and shared; nothing changes it.

    A half left stale by a step is listed by the next step's k_classify only, so after the states
    are read the compact side takes one more step (rows unused) and drains: then every crossing
    of the compared steps is regenerated exactly once on both sides, and regens is comparable."""
    import gym_treasure_game_amd as tg
    ld = CORRIDOR if level == "corridor" else None
    vecs = [tg.TreasureGameVec(n, seed=SEED, autoreset=True, mode=m, level_dir=ld)
            for m in ("compact", "direct")]
    obs0 = [v.reset().clone() for v in vecs]
    assert torch.equal(obs0[0], obs0[1])
    rows = blank_rows(n, pre + uni) if keep else None
    if keep:
        rows["obs"][:, 0] = rows["final_obs"][:, 0] = obs0[0].cpu().numpy()
    at_pre = None
    for t in range(pre + uni):
        if t == pre:  # the masked part's deferred entries are not the uniform part's
            vecs[0].regenerate()
            at_pre = vecs[0].stats()
        a, b = (step_rows(v, t, "masked" if t < pre else "uniform") for v in vecs)
        for k in a:
            assert torch.equal(a[k], b[k]), "step %d: %s differs between compact and direct" % (t, k)
        if keep:
            keep_rows(rows, t + 1, a)
    vecs[0].regenerate()
    torch.cuda.synchronize()
    sc, sd = (v.read_state(mt=True) for v in vecs)
    states = {k: bool(np.array_equal(sc[k], sd[k])) for k in sc}  # (the states themselves: 160 MB)
    del sc, sd
    stats = [v.stats() for v in vecs]
    errors = [v.errors() for v in vecs]
    step_rows(vecs[0], pre + uni, "uniform")  # lists the halves the last compared step left
    vecs[0].regenerate()
    regens = [v.stats()["regens"] for v in vecs]
    for v in vecs:
        v.close()
    at_pre = at_pre or stats[0]
    return {"rows": rows, "states": states, "stats": stats, "regens": regens, "errors": errors,
            "uniform": {k: stats[0][k] - at_pre[k] for k in ("regens", "regens_quiet")}}


def assert_sides_equal(r):
    tc, td = r["stats"]
    for k, same in r["states"].items():
        assert same, "read_state(mt=True): %s differs between compact and direct" % k
    for k in COUNTERS:
        assert tc[k] == td[k], k
    assert r["regens"][0] == r["regens"][1], "a half regenerated twice, or not at all"


def oracle_rows(O, n, pre, uni):
    """the same run by the oracle, one env at a time (oracle.run drives one policy throughout)"""
    rows = blank_rows(n, pre + uni)
    for g in range(n):
        e = O.OracleEnv(SEED + g)
        rows["obs"][g, 0] = rows["final_obs"][g, 0] = e.obs
        for t in range(pre + uni):
            masked = t < pre
            o, r, done, _ = e.step(O.pick_action(A0, g, t, masked, e.mask() if masked else 0))
            rows["final_obs"][g, t + 1] = o
            rows["obs"][g, t + 1] = e.reset() if done else o
            rows["reward"][g, t + 1] = 0 if r is None else r
            rows["valid"][g, t + 1] = r is not None
            rows["done"][g, t + 1] = done
    return rows


# 192: a 4-workgroup k_run grid (most shards' lists have no wave of their own XCD); 1000: no
# multiple of 64; 65,536: hundreds of chunk-less workgroups
@pytest.mark.parametrize("n", [192, 1000, 1 << 16])
def test_exact_across_writers(tg, oracle, n):
    r = mode_pair(n, None, 80, 200, n <= 1000)
    assert_sides_equal(r)
    assert r["errors"] == [0, 0]
    if n <= 1000:
        want = oracle_rows(oracle, n, 80, 200)
        for k in want:
            x, y = r["rows"][k], want[k]
            if x.dtype == np.float64:
                x, y = x.view(np.uint64), y.view(np.uint64)
            np.testing.assert_array_equal(x, y, err_msg=k)
        np.testing.assert_array_equal(run_hash(r["rows"]), run_hash(want))


@pytest.mark.parametrize("n", [192, 1000, 1 << 16])
def test_the_drain_takes_the_quiet_share(tg, n):
    """over the uniform part ~4 in 5 listed halves are quiet; at least half of all regenerated
    generations must be the drain's, so that a silent fallback to k_regen cannot pass"""
    u = mode_pair(n, None, 80, 200, n <= 1000)["uniform"]
    print("n %d: regens %d regens_quiet %d" % (n, u["regens"], u["regens_quiet"]))
    assert u["regens_quiet"] > 0
    assert 2 * u["regens_quiet"] >= u["regens"]


def test_every_quiet_half_is_drained_in_its_step(tg):
    """15 uniform steps with no k_regen launch: the drain alone regenerates, and it must have
    regenerated exactly the halves listed while their env was quiet, each once.

    tg_read_state reports the position inside its generation and not the state word's
    MT_STALE / MT_LISTED bits, so which envs were listed, and when, is worked out here from the
    positions: an env's ring position is the running sum of its steps' position advances (a step
    of the default level draws < 312 times, so an advance mod 624 is the advance), a half goes
    stale in the step whose advance crosses a half boundary, and the next step's k_classify
    lists it: on the quiet list iff that step's valid row is 0 (auto-reset is on from the start,
    so no env enters a step done)."""
    n, pre, win = 4096, 80, 15
    vec = tg.TreasureGameVec(n, seed=SEED, autoreset=True)
    vec.reset()
    last = vec.read_state()["mt_pos"].astype(np.int64)
    pos = last.copy()  # (generation 0 after the constructor's and the reset's draws)
    crossed = np.zeros(n, bool)
    want_quiet = want_listed = 0
    for t in range(pre + win):
        if t == pre:
            vec.regenerate()
            vec.stats_reset()
        o, r, v, d, info = vec.step(vec.policy_actions(t, A0, "masked" if t < pre else "uniform"))
        valid = v.cpu().numpy().astype(bool)
        if t >= pre:  # this step's k_classify listed the halves the previous step left
            want_quiet += int((crossed & ~valid).sum())
            want_listed += int((crossed & valid).sum())
        now = vec.read_state()["mt_pos"].astype(np.int64)
        new = pos + (now - last) % MT_N
        crossed = new // HALF_WORDS != pos // HALF_WORDS
        pos, last = new, now
    st = vec.stats()
    print("quiet halves %d, deferred %d; regens %d regens_quiet %d"
          % (want_quiet, want_listed, st["regens"], st["regens_quiet"]))
    assert want_quiet > 0 and want_listed > 0  # the window holds both classes
    assert st["regen_launches"] == 0
    assert st["regens_quiet"] == HALF_GENS * want_quiet
    assert st["regens"] == st["regens_quiet"]  # (no lane reaches a stale half on this level)
    vec.regenerate()  # the listed envs' entries are k_regen's, as before
    st = vec.stats()
    assert st["regen_launches"] == 1
    assert st["regens"] == HALF_GENS * (want_quiet + want_listed)
    assert vec.errors() == 0
    vec.close()


def test_masked_policy_has_no_quiet_entries(tg):
    r = mode_pair(1000, None, 64, 0, False)
    assert_sides_equal(r)
    assert r["stats"][0]["regens_quiet"] == 0
    assert r["errors"] == [0, 0]


# tg_set_groups takes batches of at least 4,096 envs per group only: one group at 1,000 envs is
# the handle's own stepper (no call), two groups at the smallest batch it accepts that is no
# multiple of 64 (groups of 4,352 and 3,944 envs, each with lists and counters of its own)
@pytest.mark.parametrize("n,groups", [(1000, 1), (8296, 2)])
def test_rollout_and_groups(tg, n, groups):
    """rollout(40, policy="uniform") after the preamble equals the per-step run: rows, states,
    counters, regens and regens_quiet"""
    pre, k = 80, 40
    sides = []
    for roll in (False, True):
        vec = tg.TreasureGameVec(n, seed=SEED, autoreset=True)
        vec.reset()
        for t in range(pre):
            vec.step(vec.policy_actions(t, A0, "masked"))
        if roll:
            if groups > 1:
                vec.set_groups(groups)
            out = vec.rollout(k, t0=pre, action_seed=A0, policy="uniform")
            rows = {x: out[x].clone() for x in ("obs", "reward", "valid", "done")}
        else:
            rows = {x: [] for x in ("obs", "reward", "valid", "done")}
            for s in range(k):
                a = step_rows(vec, pre + s, "uniform")
                for x in rows:
                    rows[x].append(a[x].clone())
            rows = {x: torch.stack(rows[x]) for x in rows}
        vec.regenerate()
        torch.cuda.synchronize()
        sides.append((rows, vec.read_state(mt=True), vec.stats(), vec.errors()))
        vec.close()
    (ra, sa, ta, ea), (rb, sb, tb, eb) = sides
    for x in ra:
        b = rb[x].view(torch.int64) if x == "obs" else rb[x]
        assert torch.equal(ra[x], b), x
    for x in sa:
        assert np.array_equal(sa[x], sb[x]), x
    for x in COUNTERS + ("regens",):
        assert ta[x] == tb[x], x
    assert ta["regens_quiet"] == tb["regens_quiet"] > 0
    assert ea == eb == 0


def test_corridor_lanes_and_the_drain_share_the_halves(tg):
    """~650 draws per go step: lanes reach still-stale halves and regenerate them themselves,
    beside the drain and k_regen.  Identical to direct mode, and regens equal: no half twice."""
    r = mode_pair(192, "corridor", 40, 40, False)
    print("corridor: regens %s regens_quiet %d" % (r["regens"], r["stats"][0]["regens_quiet"]))
    assert_sides_equal(r)
    assert r["errors"][0] == r["errors"][1]
