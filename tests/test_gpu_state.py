"""The checkpoint format against the reference: tg_read_state / tg_write_state compared with
states built from the reference's fixture rows by tests/state_codec.py (pinned to the reference
on the CPU by test_state_codec.py), never with another device snapshot.  Bit for bit: there are
no tolerances.  Every test first asserts, from the fixture alone, that its rows hold what it
claims to cover."""
import functools
import random

import numpy as np
import pytest
import torch

import state_codec as sc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture(name):
    return sc.load(name)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_game_state(st, z, rows, what):
    """every field of a read_state() but the RNG against the fixture rows [(g, t)] (env i of
    the batch is rows[i]): the decoded flag word and cells against ``internal`` and ``bag``
    directly, then every array against row_state's"""
    want = sc.stack([sc.row_state(z, g, t, mt=False) for g, t in rows])
    for i, (g, t) in enumerate(rows):
        f = sc.flag_fields(st["flags"][i])
        assert f["errors"] == 0 and f["unused"] == 0, (what, i, hex(int(st["flags"][i])))
        row, bag = sc.decode({k: st[k][i] for k in ("pos", "flags", "objs")})
        assert row == z["internal"][g, t, :11].tolist(), (what, i, g, t, row)
        assert bag == str(z["bag"][g, t]) and f["bag_len"] == len(bag), (what, i, g, t, bag)
    for k in ("pos", "flags", "objs", "ep"):
        assert st[k].dtype == want[k].dtype and np.array_equal(st[k], want[k]), (what, k)
    assert np.array_equal(bits(st["ang"]), bits(want["ang"])), (what, "ang")


def check_rng(st, z, rows, what):
    """read_state(mt=True)'s (mt, mt_pos) against the rows' replayed streams: the same
    continuation, index 0..622 and even, and the same tuple where CPython's index is not 624
    (there the device reports the successor generation at 0)"""
    for i, (g, t) in enumerate(rows):
        want = sc.row_state(z, g, t)
        pos = int(st["mt_pos"][i])
        assert pos % 2 == 0 and 0 <= pos <= 622, (what, i, pos)
        assert sc.same_stream((st["mt"][i], pos), (want["mt"], want["mt_pos"])), (what, i, g, t)
        if int(want["mt_pos"]) != 624:
            assert pos == int(want["mt_pos"]), (what, i, g, t, pos)
            assert np.array_equal(st["mt"][i], want["mt"]), (what, i, g, t)
        else:
            assert pos == 0, (what, i, g, t, pos)


# ---- 1. read_state against reference rows ---------------------------------------------------------
@pytest.mark.parametrize("name,n,steps,bags", [
    ("traj_autoreset.npz", 8, 700, {"", "K", "G"}),
    ("traj_level_cascade_masked.npz", 16, 600, {"", "G", "GK"})])
def test_read_state_matches_reference_rows(tg, name, n, steps, bags):
    z = fixture(name)
    idx = sc.ref_index(z["draws"][:n, :steps + 1])
    # coverage, from the fixture alone
    assert set(z["bag"][:n, :steps + 1].ravel().tolist()) == bags
    if name == "traj_autoreset.npz":
        assert z["done"][2, 629] == 1 and z["done"][:n, :steps + 1].sum() == 1
    else:
        assert (z["bag"] == "GK").sum() == 643 and z["done"].sum() == 272
        assert sorted(set(z["internal"][:, :, 3].ravel().tolist())) == [0, 1, 2, 3]
    chosen = {0, 1, steps}
    for k in (622, 624, 2):
        ts = np.flatnonzero((idx == k).any(axis=0))
        assert len(ts) >= 3, k
        chosen.update(int(t) for t in ts[:3])
    done_ts = np.flatnonzero(z["done"][:n, :steps + 1].any(axis=0))
    chosen.update((int(done_ts[0]) - 1, int(done_ts[0])))
    assert 10 <= len(chosen) <= 16

    level = sc.level_dir_of(z) if "level" in z else None
    vec = tg.TreasureGameVec(n, seed=int(z["seed_base"]), autoreset=True, level_dir=level)
    obs = vec.reset().cpu().numpy()
    assert np.array_equal(bits(obs), bits(z["obs"][:n, 0]))
    for t in range(steps + 1):
        if t:
            o, r, v, d, _ = vec.step(torch.as_tensor(z["action"][:n, t].astype(np.int32)))
            assert np.array_equal(bits(o.cpu().numpy()), bits(z["obs"][:n, t])), t
            assert np.array_equal(d.cpu().numpy(), z["done"][:n, t]), t
        rows = [(g, t) for g in range(n)]
        st = vec.read_state(mt=t in chosen)
        check_game_state(st, z, rows, (name, t))
        if t in chosen:
            check_rng(st, z, rows, (name, t))
    assert vec.errors() == 0
    vec.close()


# ---- 2. write_state from reference rows -----------------------------------------------------------
N2, K2 = 333, 40


@functools.lru_cache(maxsize=None)
def restore_rows():
    """333 rows (g, t) of traj_autoreset.npz for test 2, selected in code, with their states
    and the states 40 steps later"""
    z = fixture("traj_autoreset.npz")
    n, t1 = z["valid"].shape
    last = t1 - 1 - K2  # the latest row with 40 rows after it
    idx = sc.ref_index(z["draws"])
    rows, seen = [], set()

    def take(cands, count):
        """``count`` of the candidates not taken yet, spread over them"""
        cands = [c for c in cands if 0 <= c[1] <= last and c not in seen]
        assert len(cands) >= count
        for j in sorted(set(np.linspace(0, len(cands) - 1, count).astype(int).tolist())):
            seen.add(cands[j])
            rows.append(cands[j])

    for k in (622, 624, 2):
        take([tuple(c) for c in np.argwhere(idx == k).tolist()], 10)
    for b in ("K", "G"):
        take([tuple(c) for c in np.argwhere(z["bag"] == b).tolist()], 10)
    jt = [tuple(c) for c in np.argwhere(z["internal"][:, :, 2] > 0).tolist()]
    assert len(jt) == 3
    take(jt, 3)
    dones = [tuple(c) for c in np.argwhere(z["done"] == 1).tolist()]
    assert len(dones) == 23
    before = [[(g, t - 3), (g, t - 2), (g, t - 1)] for g, t in dones[::3]]  # 8 dones, every env
    for three in before:
        take(three, len([c for c in three if c not in seen]))
    rest = N2 - len(rows)
    take([(i % n, int(t)) for i, t in enumerate(np.linspace(0, last, 2 * rest).astype(int))], rest)
    assert len(rows) == N2 and len(set(rows)) == N2
    # coverage, from the fixture alone
    got_idx = [int(idx[g, t]) for g, t in rows]
    assert all(got_idx.count(k) >= 8 for k in (622, 624, 2))
    assert all(sum(str(z["bag"][g, t]) == b for g, t in rows) >= 8 for b in ("K", "G"))
    assert sum(z["internal"][g, t, 2] > 0 for g, t in rows) >= 3
    assert sum(all(c in seen for c in three) for three in before) >= 6
    assert sum(bool(z["done"][g, t + 1:t + K2 + 1].any()) for g, t in rows) >= 6 * 3
    # the streams are replayed in (g, t) order: one pass per env
    order = sorted(set(rows) | {(g, t + K2) for g, t in rows})
    states = {gt: sc.row_state(z, *gt) for gt in order}
    return rows, [states[gt] for gt in rows]


@pytest.mark.parametrize("pre", [0, 5, 16, 17])
@pytest.mark.parametrize("mode", ["compact", "direct"])
def test_write_state_continues_reference_rows(tg, mode, pre):
    z = fixture("traj_autoreset.npz")
    rows, states = restore_rows()
    g_of = np.array([g for g, _ in rows])
    t_of = np.array([t for _, t in rows])
    vec = tg.TreasureGameVec(N2, seed=424242, autoreset=True, mode=mode)
    vec.reset()
    for t in range(pre):  # the rings and refill lists in every phase of the 16-step cadence
        vec.step(vec.policy_actions(t, 0xBEEF, "masked"))
    while len(vec.episodes()):  # (its own episodes, if any: not the restore's business)
        pass
    vec.write_state(sc.stack(states))
    check_game_state(vec.read_state(), z, rows, "read back")
    for k in range(1, K2 + 1):
        o, r, v, d, info = vec.step(torch.as_tensor(z["action"][g_of, t_of + k].astype(np.int32)))
        at = (mode, pre, k)
        assert np.array_equal(bits(o.cpu().numpy()), bits(z["obs"][g_of, t_of + k])), at
        assert np.array_equal(bits(info["final_obs"].cpu().numpy()),
                              bits(z["final_obs"][g_of, t_of + k])), at
        assert np.array_equal(r.cpu().numpy(), z["reward"][g_of, t_of + k]), at
        assert np.array_equal(v.cpu().numpy(), z["valid"][g_of, t_of + k]), at
        assert np.array_equal(d.cpu().numpy(), z["done"][g_of, t_of + k]), at
    end = [(g, t + K2) for g, t in rows]
    st = vec.read_state(mt=True)
    check_game_state(st, z, end, "after %d steps" % K2)
    check_rng(st, z, end, "after %d steps" % K2)
    # the episode records: return and length counted from before the restore (the ep input)
    want = []
    for i, (g, t) in enumerate(rows):
        for td in range(t + 1, t + K2 + 1):
            if z["done"][g, td]:
                ret, length = sc.row_state(z, g, td - 1, mt=False)["ep"]
                want.append((i, int(ret) + int(z["reward"][g, td]), int(length) + 1))
    assert len({i for i, _, _ in want}) >= 6
    assert sum(length > K2 for _, _, length in want) >= 6  # begun before the restore
    got = [tuple(int(x) for x in rec) for rec in vec.episodes(cap=4 * N2).cpu().numpy()]
    assert sorted(got) == sorted(want)
    assert vec.errors() == 0
    vec.close()


@pytest.mark.parametrize("pre", [5, 17])
def test_write_state_restarts_the_regeneration_cadence(tg, pre):
    """The restore discards the pending refill lists, so their 16-step cadence (tg_regenerate in
    include/tg_amd.h) starts over: in the compact mode the next k_regen comes with the 16th step
    after it, wherever in the cadence the batch was.  (Results never depend on when k_regen runs,
    so only this count shows whether the host's bookkeeping was reset with the lists.)"""
    z = fixture("traj_autoreset.npz")
    rows, states = restore_rows()
    g_of = np.array([g for g, _ in rows])
    t_of = np.array([t for _, t in rows])
    vec = tg.TreasureGameVec(N2, seed=424242, autoreset=True, mode="compact")
    vec.reset()
    for t in range(pre):
        vec.step(vec.policy_actions(t, 0xBEEF, "masked"))
    vec.write_state(sc.stack(states))
    regens = vec.stats()["regen_launches"]
    for k in range(1, 17):
        vec.step(torch.as_tensor(z["action"][g_of, t_of + k].astype(np.int32)))
        assert vec.stats()["regen_launches"] == regens + (1 if k == 16 else 0), (pre, k)
    assert vec.errors() == 0
    vec.close()


# ---- 3. restore, then the fused paths ---------------------------------------------------------------
def rollout_rows(tg, z, n, t0, k, mode, level=None):
    rows = [(g, t0) for g in range(n)]
    vec = tg.TreasureGameVec(n, seed=31337, global_offset=0, autoreset=True, mode=mode,
                             level_dir=level)
    vec.reset()
    vec.write_state(sc.stack([sc.row_state(z, g, t) for g, t in rows]))
    out = vec.rollout(k, t0=t0, action_seed=int(z["action_seed"]), policy="masked")
    sl = slice(t0 + 1, t0 + k + 1)
    at = (mode, t0)
    assert np.array_equal(out["actions"].cpu().numpy().T, z["action"][:n, sl]), at
    assert np.array_equal(bits(out["obs"].cpu().numpy().transpose(1, 0, 2)), bits(z["obs"][:n, sl])), at
    for key in ("reward", "valid", "done"):
        assert np.array_equal(out[key].cpu().numpy().T, z[key][:n, sl]), (at, key)
    end = [(g, t0 + k) for g in range(n)]
    st = vec.read_state(mt=True)
    check_game_state(st, z, end, at)
    check_rng(st, z, end, at)
    assert vec.errors() == 0
    vec.close()


@pytest.mark.parametrize("mode", ["compact", "direct", "flow"])
def test_restore_then_rollout(tg, mode):
    z = fixture("traj_autoreset.npz")
    assert int(z["masked"]) == 1 and z["done"][2, 629] == 1  # ends inside rows 601..640
    rollout_rows(tg, z, 8, 600, 40, mode)


@pytest.mark.parametrize("mode", ["compact", "direct", "flow"])
def test_restore_then_rollout_crosses_generations(tg, mode):
    """corridor: one option takes up to 682 draws, so the first option after the restore runs
    on into the successor generations that tg_write_state rebuilt"""
    z = fixture("traj_level_corridor_masked.npz")
    k = 8
    per_step = np.diff(z["draws"], axis=1)  # [g, t]: the draws of the step from row t
    crosses = 2 * per_step > 624 - sc.ref_index(z["draws"])[:, :-1]  # past the given generation
    ok = np.arange(per_step.shape[1]) <= z["valid"].shape[1] - 1 - k
    g_max, t_max = np.unravel_index(np.argmax(per_step * ok), per_step.shape)
    assert per_step[g_max, t_max] == 682 and 2 * 682 > 2 * 624  # past the successor too
    t_all = int(np.flatnonzero(crosses.all(axis=0) & ok)[0])  # every env crosses at once
    assert t_all != t_max and crosses[g_max, t_max]
    assert z["valid"][:, 1:].all()  # the fixture's options all ran and terminated
    for t0 in (int(t_max), t_all):
        rollout_rows(tg, z, 16, t0, k, mode, level=sc.level_dir_of(z))


# ---- 4. MT index 0 ------------------------------------------------------------------------------------
def test_write_state_mt_index_zero(tg):
    """(generation, 0): the index CPython's getstate() never reports but setstate() accepts"""
    import pyref
    z = fixture("traj_autoreset.npz")
    rows = [(g, 900 + 310 * g) for g in range(8)]
    states, refs = [], []
    for i, (g, t) in enumerate(rows):
        st = sc.row_state(z, g, t, mt=False)
        gen = random.Random(7000 + i).getstate()[1]
        st["mt"], st["mt_pos"] = np.array(gen[:624], np.uint32), np.uint32(0)
        states.append(st)
        env = pyref.Env(12345 + i)
        env.reset()
        sc.inject_pyref(env, st)
        assert env.rng.getstate()[1] == gen[:624] + (0,)
        refs.append(env)
    assert all(int(s["mt_pos"]) == 0 for s in states)
    vec = tg.TreasureGameVec(8, seed=99, autoreset=True)
    vec.reset()
    vec.write_state(sc.stack(states))
    a0 = 0x1D0
    for t in range(10):
        acts = [pyref.pick_action(a0, i, t, e.available_mask()) for i, e in enumerate(refs)]
        assert vec.policy_actions(t, a0, "masked").cpu().tolist() == acts, t
        o, r, v, d, info = vec.step(torch.as_tensor(np.array(acts, np.int32)))
        o, fo, r, v, d = (x.cpu().numpy() for x in (o, info["final_obs"], r, v, d))
        for i, e in enumerate(refs):
            ro, rr, rd, _ = e.step(acts[i])
            assert np.array_equal(bits(fo[i]), bits(ro)), (t, i)
            if rd:
                ro = e.reset()
            assert np.array_equal(bits(o[i]), bits(ro)), (t, i)
            assert (int(r[i]), bool(v[i]), bool(d[i])) == (rr or 0, rr is not None, rd), (t, i)
    st = vec.read_state(mt=True)
    for i, e in enumerate(refs):
        s = e.rng.getstate()[1]
        assert sc.same_stream((st["mt"][i], st["mt_pos"][i]), (s[:624], s[624])), i
        assert [int(st["pos"][i][0]), int(st["pos"][i][1])] == [e.game.px, e.game.py]
    assert vec.errors() == 0
    vec.close()


# ---- 5. a rejected write changes nothing --------------------------------------------------------------
def test_rejected_write_changes_nothing(tg):
    n, a0 = 100, 0xD00D
    a, b = (tg.TreasureGameVec(n, seed=5, autoreset=True) for _ in range(2))
    for v in (a, b):
        v.reset()
        for t in range(20):
            v.step(v.policy_actions(t, a0, "masked"))
    # a state the batch must not take on: other rows, the bad entry in the last env, so every
    # env before it has passed the checks when the call fails
    z = fixture("traj_autoreset.npz")
    good = sc.stack([sc.row_state(z, i % 8, 2000 + 3 * i) for i in range(n)])

    def bad(key, value=None, shape=None):
        s = {k: v.copy() for k, v in good.items()}
        if shape is not None:
            s[key] = np.zeros(shape, s[key].dtype)
        elif value is None:
            del s[key]
        else:
            s[key].reshape(n, -1)[n - 1, -1] = value
        return s

    for state, exc in ((bad("mt_pos", 311), tg.TgError), (bad("mt_pos", 626), tg.TgError),
                       (bad("pos", 40000), tg.TgError), (bad("objs", 200), tg.TgError),
                       (bad("mt"), KeyError), (bad("flags", shape=(n + 1,)), ValueError),
                       (bad("mt", shape=(n, 623)), ValueError)):
        with pytest.raises(exc):
            b.write_state(state)
    for t in range(20, 40):
        ra = a.step(a.policy_actions(t, a0, "masked"))
        rb = b.step(b.policy_actions(t, a0, "masked"))
        for x, y in zip(ra[:4] + (ra[4]["final_obs"],), rb[:4] + (rb[4]["final_obs"],)):
            assert torch.equal(x, y), t
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert torch.equal(a.episodes(cap=4 * n), b.episodes(cap=4 * n))
    assert a.errors() == 0 and b.errors() == 0
    a.close()
    b.close()


# ---- 6. restore under a resident N = 1 server ---------------------------------------------------------
def test_write_state_under_the_resident_server(tg, monkeypatch):
    """A 1-env handle whose server is resident (idle limit 1 s, stepped microseconds ago) takes a
    fixture row and continues it through the server.  The write must stop the server itself and
    change the state only then: it returns long before the idle limit (a write that did not stop
    the server would wait, in its device synchronisation, for the server to leave by itself), and
    the env continues from the written state, not from the copy the server held."""
    import time
    idle_s = 1.0
    monkeypatch.setenv("TG_SERVE_IDLE_US", str(int(idle_s * 1e6)))  # read at tg_create
    z = fixture("traj_autoreset.npz")
    g, t0, k = 2, 610, 30
    assert z["done"][g, 629] == 1  # the episode ends inside the window
    state = sc.stack([sc.row_state(z, g, t0)])  # before the served steps: nothing slow after them
    env = tg.TreasureGame(seed=77)
    env._vec.set_serve(True)
    env.reset()
    for t in range(12):  # the server is resident and holds the env's state
        env.step(t % 9)
    t_w = time.perf_counter()
    env._vec.write_state(state)
    t_w = time.perf_counter() - t_w
    # stopping a server and writing one env takes milliseconds; the limit is a quarter of the time
    # a server left alone would stay
    assert t_w < idle_s / 4, "write_state took %.3f s: it waited for the server to leave" % t_w
    for t in range(t0 + 1, t0 + k + 1):
        st, r, d, _ = env.step(int(z["action"][g, t]))
        assert np.array_equal(bits(st), bits(z["final_obs"][g, t])), t
        assert (0 if r is None else r, r is not None, d) == (
            int(z["reward"][g, t]), bool(z["valid"][g, t]), bool(z["done"][g, t])), t
        if d:
            st = env.reset()
        assert np.array_equal(bits(st), bits(z["obs"][g, t])), t
    end = env._vec.read_state(mt=True)
    check_game_state(end, z, [(g, t0 + k)], "served")
    check_rng(end, z, [(g, t0 + k)], "served")
    assert env._vec.errors() == 0
    env.close()
