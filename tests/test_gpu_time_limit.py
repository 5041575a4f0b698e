"""The step limit on the device (tg_set_time_limit, k_timelimit): every step path against the
oracle driven as the reference's env with a TimeLimit would be (step; reset on done or on
len >= limit), the rollouts against the per-step loop, the device limit against the host-side
path it replaces (tg_step + tg_reset(mask)) across k_regen launches and env groups, and the
edges: no auto-reset, lengths restored from a checkpoint, lowering and clearing the limit,
invalid limits, the episode queue's bound, and the vector env's device_time_limit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import state_codec as sc
from test_policy_mlp_host import seeded_params

pytestmark = pytest.mark.gpu

LEVELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels")
EXIT = os.path.join(LEVELS, "exit")
N, SEED, A0, STEPS = 200, 5, 0x3C, 60  # three waves plus 8 lanes


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(t).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[t.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def sorted_rows(e):
    e = e.cpu().numpy() if isinstance(e, torch.Tensor) else np.asarray(e, np.int64).reshape(-1, 4)
    return e[np.lexsort(tuple(e[:, c] for c in range(e.shape[1] - 1, -1, -1)))] if len(e) else e


# ---- the oracle driven with a TimeLimit: computed once per (level, n, limit), never changed -----
_ref = {}


def oracle_ref(oracle, level_dir, n, limit, steps=STEPS, seed=SEED, a0=A0):
    key = (level_dir, n, limit, steps)
    if key in _ref:
        return _ref[key]
    envs = [oracle.OracleEnv(seed + g, level_dir) for g in range(n)]
    d0 = sum(e.draws() for e in envs)
    r = {"obs0": np.stack([e.obs for e in envs]),
         "actions": np.zeros((steps, n), np.int32), "obs": np.zeros((steps, n, 9)),
         "final": np.zeros((steps, n, 9)), "reward": np.zeros((steps, n), np.int32),
         "valid": np.zeros((steps, n), np.uint8), "done": np.zeros((steps, n), np.uint8)}
    lens, rets, eps = [0] * n, [0] * n, []
    term = trunc = term_at_limit = 0
    for t in range(steps):
        for g, e in enumerate(envs):
            a = oracle.pick_action(a0, g, t, True, e.mask())
            o, rew, d, _ = e.step(a)
            lens[g] += 1
            rets[g] += rew or 0
            tr = (not d) and lens[g] >= limit
            r["actions"][t, g], r["final"][t, g] = a, o
            r["reward"][t, g], r["valid"][t, g] = rew or 0, rew is not None
            r["done"][t, g] = 1 if d else 2 if tr else 0
            term += d
            trunc += tr
            term_at_limit += d and lens[g] == limit
            if d or tr:
                eps.append((g, rets[g], lens[g], int(tr)))
                o = e.reset()
                lens[g] = rets[g] = 0
            r["obs"][t, g] = o
    r["state"] = [e.get_state() for e in envs]
    r["ep"] = np.array([[rets[g], lens[g]] for g in range(n)], np.int32)
    r["episodes"] = sorted_rows(np.array(eps, np.int64).reshape(-1, 4))
    r["draws"] = sum(e.draws() for e in envs) - d0
    r["counts"] = (int(term), int(trunc), int(term_at_limit))
    _ref[key] = r
    return r


def check_state(vec, ref):
    """read_state(mt=True) against the oracle envs' get_state(): CPython's (generation, 624) is
    the device's (successor generation, 0)"""
    st = vec.read_state(mt=True)
    assert np.array_equal(st["ep"], ref["ep"])
    for g, want in enumerate(ref["state"]):
        for k in ("pos", "objs"):
            assert np.array_equal(st[k][g], want[k]), (k, g)
        assert st["flags"][g] == want["flags"], g
        assert same(st["ang"][g], want["ang"]), g
        if int(want["mt_pos"]) != 624:
            assert st["mt_pos"][g] == want["mt_pos"] and np.array_equal(st["mt"][g], want["mt"]), g
        else:
            assert st["mt_pos"][g] == 0, g
            assert sc.same_stream((st["mt"][g], 0), (want["mt"], 624)), g


def check_against_oracle(tg, ref, n, limit, level_dir, mode, steps=STEPS):
    v = tg.TreasureGameVec(n, seed=SEED, autoreset=True, level_dir=level_dir, mode=mode,
                           max_episode_steps=limit)
    assert same(v.reset(), ref["obs0"])
    for t in range(steps):
        act = v.policy_actions(t, A0, "masked")
        assert np.array_equal(act.cpu().numpy(), ref["actions"][t]), t
        o, r, va, d, info = v.step(act)
        assert same(o, ref["obs"][t]), ("obs", t)
        assert same(info["final_obs"], ref["final"][t]), ("final_obs", t)
        assert np.array_equal(r.cpu().numpy(), ref["reward"][t]), ("reward", t)
        assert np.array_equal(va.cpu().numpy(), ref["valid"][t]), ("valid", t)
        assert np.array_equal(d.cpu().numpy(), ref["done"][t]), ("done", t)
    check_state(v, ref)
    assert np.array_equal(sorted_rows(v.episodes(cap=n * steps, truncated=True)), ref["episodes"])
    term, trunc, _ = ref["counts"]
    s = v.stats()
    assert (s["episodes"], s["episodes_truncated"]) == (term + trunc, trunc)
    assert s["draws"] == ref["draws"] and s["episodes_dropped"] == 0
    assert v.errors() == 0
    v.close()


# ---- 1. oracle parity, step by step -------------------------------------------------------------
@pytest.mark.parametrize("mode", ["compact", "direct", "flow"])
@pytest.mark.parametrize("limit", [7, 25])
def test_oracle_parity(tg, oracle, limit, mode):
    """level exit, where the masked policy both terminates and runs into the limit: limit 7 gives
    173 terminations, 1,496 truncations and 5 terminations at exactly length 7 (termination
    wins there); limit 25 gives 351, 221 and 5 (oracle alone, on the CPU)"""
    ref = oracle_ref(oracle, EXIT, N, limit)
    assert all(c > 0 for c in ref["counts"]), ref["counts"]
    check_against_oracle(tg, ref, N, limit, EXIT, mode)


# ---- 2. the default level ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1])
def test_default_level(tg, oracle, n):
    ref = oracle_ref(oracle, None, n, 3, steps=10)
    want = np.zeros((10, n), np.uint8)
    want[[2, 5, 8]] = 2  # every env truncates at steps 3, 6 and 9
    assert np.array_equal(ref["done"], want)
    check_against_oracle(tg, ref, n, 3, None, "compact", steps=10)


# ---- 3. rollouts ---------------------------------------------------------------------------------
ROW_KEYS = ("actions", "obs", "reward", "valid", "done")


def check_twins(a, b, outs_a, outs_b, keys):
    for key in keys:
        assert same(outs_a[key], outs_b[key]), key
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert np.array_equal(sorted_rows(a.episodes(cap=N * STEPS, truncated=True)),
                          sorted_rows(b.episodes(cap=N * STEPS, truncated=True)))
    sta, stb = a.stats(), b.stats()
    for key in ("steps", "valid_steps", "ticks", "draws", "episodes", "episodes_truncated",
                "episodes_dropped"):
        assert sta[key] == stb[key], key
    assert sta["episodes_truncated"] > 0 and sta["episodes"] > sta["episodes_truncated"]
    assert a.errors() == 0 and b.errors() == 0


def twins(tg):
    out = []
    for _ in range(2):
        v = tg.TreasureGameVec(N, seed=SEED, autoreset=True, level_dir=EXIT, max_episode_steps=7)
        v.reset()
        out.append(v)
    return out


def test_rollout_masked_in_chunks(tg):
    """rollout(60) as (7, 1, 52) against 60 x (policy_actions + step), the same limit on both;
    between the chunks a flow-mode rollout is refused and leaves the step count alone"""
    a, b = twins(tg)
    parts, t0 = [], 0
    for c in (7, 1, 52):
        if c == 52:
            a.set_mode("flow")
            with pytest.raises(tg.TgError):
                a.rollout(4, t0=t0, action_seed=A0, policy="masked")
            buf = torch.zeros(4 * N, dtype=torch.int32, device=a.device)
            p = ctypes.c_void_p(buf.data_ptr())
            assert a._L.tg_rollout(a.handle, 4, A0, t0, 1, 1, None, None, p, p, p, None) == -1
            assert a._L.tg_rollout(a.handle, 0, A0, t0, 1, 1, None, None, p, p, p, None) == -1
            a.set_mode("compact")
        parts.append(a.rollout(c, t0=t0, action_seed=A0, policy="masked"))
        t0 += c
    outs_a = {k: torch.cat([p[k] for p in parts]) for k in ROW_KEYS}
    rows = []
    for t in range(STEPS):
        act = b.policy_actions(t, A0, "masked").clone()
        o, r, va, d, _ = b.step(act)
        rows.append({"actions": act, "obs": o.clone(), "reward": r.clone(), "valid": va.clone(),
                     "done": d.clone()})
    outs_b = {k: torch.stack([r[k] for r in rows]) for k in ROW_KEYS}
    assert set(np.unique(outs_a["done"].cpu().numpy())) == {0, 1, 2}
    check_twins(a, b, outs_a, outs_b, ROW_KEYS)
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["compact", "direct"])
def test_rollout_mlp(tg, mode):
    a, b = twins(tg)
    packed = tg.pack_mlp_params(seeded_params(32, 332))
    for v in (a, b):
        v.set_policy_mlp(packed, act="relu", masked=True)
    a.set_mode(mode)
    outs_a = a.rollout(STEPS, t0=0, action_seed=A0, policy="mlp")
    rows = []
    for t in range(STEPS):
        act, lp, val = (x.clone() for x in b.policy_mlp(t, A0))
        o, r, va, d, _ = b.step(act)
        rows.append({"actions": act, "logp": lp, "value": val, "obs": o.clone(),
                     "reward": r.clone(), "valid": va.clone(), "done": d.clone()})
    keys = ROW_KEYS + ("logp", "value")
    outs_b = {k: torch.stack([r[k] for r in rows]) for k in keys}
    check_twins(a, b, outs_a, outs_b, keys)
    a.close()
    b.close()


# ---- 4. against the host-side path, across k_regen and groups ----------------------------------
def test_equals_step_plus_masked_reset(tg):
    """n = 12,288 (3 groups of 4,096), uniform policy, limit 5: 5 plain steps, rollouts of 10, 3
    and 27 steps in 3 staggered groups (k_regen runs every 16 compact steps), 6 plain steps;
    against a handle without a limit stepped with tg_step + tg_reset(mask) where len >= 5"""
    n, limit, a0 = 12288, 5, 0xA5A5
    a = tg.TreasureGameVec(n, seed=11, autoreset=True, max_episode_steps=limit)
    b = tg.TreasureGameVec(n, seed=11, autoreset=True)
    a.reset()
    b.reset()
    got = {k: [] for k in ("obs", "reward", "valid", "done")}

    def plain(t):
        o, r, va, d, _ = a.step(a.policy_actions(t, a0, "uniform"))
        for k, x in zip(("obs", "reward", "valid", "done"), (o, r, va, d)):
            got[k].append(x.clone()[None])

    for t in range(5):
        plain(t)
    a.set_groups(3, stagger=True)
    t0 = 5
    for c in (10, 3, 27):
        out = a.rollout(c, t0=t0, action_seed=a0, policy="uniform")
        for k in got:
            got[k].append(out[k])
        t0 += c
    for t in range(45, 51):
        plain(t)
    got = {k: torch.cat(v) for k, v in got.items()}
    ln = torch.zeros(n, dtype=torch.int32, device=b.device)
    truncs = 0
    for t in range(51):
        o, r, va, d, _ = b.step(b.policy_actions(t, a0, "uniform"))
        ln += 1
        ln.masked_fill_(d.bool(), 0)
        tr = ln >= limit
        ln.masked_fill_(tr, 0)
        o = b.reset(tr)
        truncs += int(tr.sum())
        assert same(got["obs"][t], o), ("obs", t)
        assert torch.equal(got["reward"][t], r) and torch.equal(got["valid"][t], va), t
        assert torch.equal(got["done"][t], d | (tr.to(torch.uint8) * 2)), ("done", t)
    assert truncs > 9 * n
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    sta, stb = a.stats(), b.stats()
    assert sta["episodes_truncated"] == truncs and stb["episodes_truncated"] == 0
    assert sta["episodes"] - truncs == stb["episodes"]
    assert sta["regen_launches"] >= 3 and sta["draws"] == stb["draws"] + 4 * truncs
    assert a.errors() == 0 and b.errors() == 0
    a.close()
    b.close()


# ---- 5. without auto-reset -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["compact", "direct"])
def test_without_autoreset_only_flags(tg, mode):
    n, limit = 130, 4
    a = tg.TreasureGameVec(n, seed=3, mode=mode, max_episode_steps=limit)
    b = tg.TreasureGameVec(n, seed=3, mode=mode)
    assert same(a.reset(), b.reset())
    for t in range(8):
        ra = a.step(a.policy_actions(t, A0, "masked"))
        rb = b.step(b.policy_actions(t, A0, "masked"))
        assert same(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2]), t
        assert torch.equal(ra[3], rb[3] | (2 if t + 1 >= limit else 0)), t
        assert bool((ra[3] & 2).all()) == (t + 1 >= limit)
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert np.array_equal(sa["ep"][:, 1], np.full(n, 8))
    assert len(a.episodes(truncated=True)) == 0
    sta = a.stats()
    assert sta["episodes"] == 0 and sta["episodes_truncated"] == 0
    assert sta["draws"] == b.stats()["draws"]
    a.close()
    b.close()


# ---- 6. lengths from a checkpoint -----------------------------------------------------------------
def test_lengths_from_a_checkpoint(tg):
    n, limit = 130, 10
    v = tg.TreasureGameVec(n, seed=9, autoreset=True, max_episode_steps=limit)
    v.reset()
    for t in range(2):
        v.step(v.policy_actions(t, A0, "masked"))
    st = v.read_state(mt=True)
    assert np.array_equal(st["ep"][:, 1], np.full(n, 2))
    chosen = {3: limit - 1, 64: limit, 129: limit + 3}
    for g, ln in chosen.items():
        st["ep"][g, 1] = ln
    v.write_state(st)
    o, r, va, d, _ = v.step(v.policy_actions(2, A0, "masked"))
    d, r = d.cpu().numpy(), r.cpu().numpy()
    want = np.zeros(n, np.uint8)
    want[list(chosen)] = 2
    assert np.array_equal(d, want)
    e = sorted_rows(v.episodes(truncated=True))
    assert e.tolist() == [[g, int(st["ep"][g, 0]) + int(r[g]), ln + 1, 1] for g, ln in chosen.items()]
    ep = v.read_state()["ep"]
    assert all(ep[g].tolist() == [0, 0] for g in chosen)
    assert np.array_equal(np.delete(ep[:, 1], list(chosen)), np.full(n - 3, 3))
    v.close()


# ---- 7. lowering and clearing the limit ----------------------------------------------------------
def test_lowering_and_clearing(tg):
    n = 130
    a = tg.TreasureGameVec(n, seed=4, autoreset=True, max_episode_steps=50)
    b = tg.TreasureGameVec(n, seed=4, autoreset=True)
    a.reset()
    b.reset()

    def both(t):
        ra = a.step(a.policy_actions(t, A0, "masked"))
        rb = b.step(b.policy_actions(t, A0, "masked"))
        assert torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2]), t
        assert same(ra[4]["final_obs"], rb[4]["final_obs"]), t
        return ra, rb

    for t in range(6):
        ra, rb = both(t)
        assert same(ra[0], rb[0]) and torch.equal(ra[3], rb[3]), t
    a.set_time_limit(4)  # every episode is already longer: all truncate at the next step
    assert a.max_episode_steps == 4
    ra, rb = both(6)
    assert bool((rb[3] == 0).all()), "the default level's masked policy does not terminate here"
    assert bool((ra[3] == 2).all())
    assert same(ra[0], b.reset())
    for clear in (0, None):
        a.set_time_limit(4)
        a.set_time_limit(clear)
        assert a.max_episode_steps is None
    for t in range(7, 17):
        ra, rb = both(t)
        assert same(ra[0], rb[0]) and torch.equal(ra[3], rb[3]), t
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.stats()["episodes_truncated"] == n
    a.close()
    b.close()


# ---- 8. invalid limits ----------------------------------------------------------------------------
def test_invalid_limits(tg):
    v = tg.TreasureGameVec(64, seed=1, autoreset=True)
    for bad in (-1, 2**30):
        with pytest.raises(tg.TgError):
            v.set_time_limit(bad)
        assert v._L.tg_set_time_limit(v.handle, bad) == -1  # TG_E_INVAL
        assert v.max_episode_steps is None
    with pytest.raises(tg.TgError):
        tg.TreasureGameVec(64, seed=1, max_episode_steps=-1)
    v.set_time_limit(2**30 - 1)
    v.reset()
    d = v.step(v.policy_actions(0, A0, "masked"))[3]
    assert bool((d == 0).all())
    v.close()


# ---- 9. the episode queue's bound -----------------------------------------------------------------
def test_episode_queue_bound(tg):
    n, cap = 256, 16
    v = tg.TreasureGameVec(n, seed=2, autoreset=True, max_episode_steps=1)
    v.set_episode_capacity(cap)
    v.reset()
    for t in range(5):
        d = v.step(v.policy_actions(t, A0, "masked"))[3]
        assert bool((d == 2).all())
    s = v.stats()
    kept = v.episodes(cap=4 * n, truncated=True).cpu().numpy()
    assert 0 < len(kept) <= cap
    assert s["episodes"] == 5 * n == s["episodes_truncated"]
    assert s["episodes_dropped"] + len(kept) == s["episodes"]
    assert np.array_equal(kept[:, 2:], np.ones((len(kept), 2), np.int64))
    assert v.errors() == 0
    v.close()


# ---- 10. the vector env ---------------------------------------------------------------------------
def test_vector_env_device_time_limit(tg):
    n, tmax = 48, 60
    ve = [tg.make_vec("treasure_game-v0", num_envs=n, seed=5, max_episode_steps=tmax, **kw)
          for kw in ({}, {"device_time_limit": True})]
    assert ve[1].env.max_episode_steps == tmax and ve[0].env.max_episode_steps is None
    o0, o1 = ve[0].reset()[0], ve[1].reset()[0]
    assert same(o0, o1)
    n_trunc = 0
    for t in range(100):
        act = ve[0].env.policy_actions(t, A0, "masked").clone()
        r0, r1 = ve[0].step(act), ve[1].step(act)
        assert same(r0[0], r1[0]), t
        for k in (1, 2, 3):
            assert r0[k].dtype == r1[k].dtype and torch.equal(r0[k], r1[k]), (k, t)
        assert same(r0[4]["final_obs"], r1[4]["final_obs"]), t
        assert torch.equal(r0[4]["valid"], r1[4]["valid"]), t
        n_trunc += int(r1[3].sum())
    assert n_trunc > 0
    e = ve[1].episodes(cap=4 * n, truncated=True).cpu().numpy()
    assert int(e[:, 3].sum()) == n_trunc and set(e[e[:, 3] == 1][:, 2]) == {tmax}
    for v in ve:
        v.close()
