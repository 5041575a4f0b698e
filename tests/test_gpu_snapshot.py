"""Device-resident snapshots (tg_snap_*: Snapshot, TreasureGameVec.fork) against the reference:
``save`` is checked on rows the device produced by following a fixture, ``load`` on rows the
device never produced (written with ``Snapshot.write`` from tests/state_codec.py's states), both
against the reference's fixture rows, never against another device snapshot.  Bit for bit: there
are no tolerances.  Every test first asserts, from the fixture alone, that its rows hold what it
claims to cover."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import state_codec as sc

pytestmark = pytest.mark.gpu

GENS = 16  # ring generations (tg_mt_layout: 9,984 ring words of 624)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return sc.load(name)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dev(x):
    return torch.as_tensor(np.asarray(x, np.int64), device="cuda")


def rows_of(st, idx):
    return {k: v[idx] for k, v in st.items()}


def check_game_state(st, z, rows, what):
    """every field of a read_state()-style dict but the RNG against the fixture rows [(g, t)]
    (record i is rows[i]): the decoded flag word and cells against ``internal`` and ``bag``
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
    """(mt, mt_pos) against the rows' replayed streams: the same continuation, index 0..622 and
    even, and the same tuple where CPython's index is not 624 (there the device holds the
    successor generation at 0)"""
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


def same_state(a, b, what, idx=None):
    for k in a:
        x, y = (a[k], b[k]) if idx is None else (a[k][idx], b[k][idx])
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y), (what, k)


# ---- 1. save against reference rows ---------------------------------------------------------------
def ring_gen(draws):
    """ring generation of an env ``draws`` random() calls after its seeding"""
    return (2 * np.asarray(draws, np.int64) // 624) % GENS


@pytest.mark.parametrize("name,n,windows,total", [
    ("traj_level_corridor_masked.npz", 16, [(0, 20)], 20),
    # (rows 0..130; then the rows around the only done of these envs' first 700, row 629 of env 2)
    ("traj_autoreset.npz", 8, [(0, 130), (600, 650)], 650)])
def test_save_matches_reference_rows(tg, name, n, windows, total):
    z = fixture(name)
    saved = [(g, t) for a, b in windows for t in range(a, b + 1) for g in range(n)]
    # coverage, from the fixture alone
    gens = ring_gen([z["draws"][g, t] for g, t in saved])
    assert set(gens.tolist()) == set(range(GENS))
    assert (gens < GENS // 2).sum() >= 8 and (gens >= GENS // 2).sum() >= 8
    assert (gens % 2 == 1).sum() >= 8 and (gens % 2 == 0).sum() >= 8
    if name == "traj_autoreset.npz":
        assert z["done"][2, 629] == 1 and (2, 629) in saved and (2, 628) in saved
        assert max(int(sc.row_state(z, g, t, mt=False)["ep"][1]) for g, t in saved) >= 600
    perm = np.random.RandomState(3).permutation(n)
    level = sc.level_dir_of(z) if "level" in z else None
    vec = tg.TreasureGameVec(n, seed=int(z["seed_base"]), autoreset=bool(z["autoreset"]),
                             level_dir=level)
    snap = vec.snapshot(len(saved) + n)
    assert len(snap) == len(saved) + n
    envs = dev(np.arange(n))
    slot_of = {gt: i for i, gt in enumerate(saved)}
    obs = vec.reset().cpu().numpy()
    assert np.array_equal(bits(obs), bits(z["obs"][:n, 0]))
    for t in range(total + 1):
        if t:
            o, r, v, d, _ = vec.step(torch.as_tensor(z["action"][:n, t].astype(np.int32)))
            assert np.array_equal(bits(o.cpu().numpy()), bits(z["obs"][:n, t])), t
            assert np.array_equal(r.cpu().numpy(), z["reward"][:n, t]), t
            assert np.array_equal(d.cpu().numpy(), z["done"][:n, t]), t
        if (0, t) in slot_of:
            snap.save(envs, dev([slot_of[(g, t)] for g in range(n)]))
    snap.save(envs, dev(len(saved) + perm))  # the last rows again, into permuted slots
    st = snap.read()
    check_game_state(rows_of(st, slice(0, len(saved))), z, saved, (name, "saved"))
    check_rng(rows_of(st, slice(0, len(saved))), z, saved, (name, "saved"))
    last = [None] * n
    for g in range(n):
        last[perm[g]] = (g, total)
    tail = rows_of(st, slice(len(saved), len(saved) + n))
    check_game_state(tail, z, last, (name, "permuted"))
    check_rng(tail, z, last, (name, "permuted"))
    # saving changed nothing: the envs are the fixture's to the end
    end = vec.read_state(mt=True)
    check_game_state(end, z, [(g, total) for g in range(n)], (name, "envs"))
    check_rng(end, z, [(g, total) for g in range(n)], (name, "envs"))
    assert vec.errors() == 0
    snap.close()
    vec.close()


# ---- 2. load continues reference rows ---------------------------------------------------------------
N2, K2, NB, FAN = 333, 40, 700, 64


@functools.lru_cache(maxsize=None)
def restore_rows():
    """333 rows (g, t) of traj_autoreset.npz, selected in code as tests/test_gpu_state.py selects
    its own: MT indices 622, 624 and 2, both one-item bags, every row with a running jump, the
    three rows before 8 dones, the rest spread over the fixture; with their states"""
    z = fixture("traj_autoreset.npz")
    n, t1 = z["valid"].shape
    last = t1 - 1 - K2  # the latest row with 40 rows after it
    idx = sc.ref_index(z["draws"])
    rows, seen = [], set()

    def take(cands, count):
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
    before = [[(g, t - 3), (g, t - 2), (g, t - 1)] for g, t in dones[::3]]
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
    order = sorted(set(rows) | {(g, t + K2) for g, t in rows})  # one replay pass per env
    states = {gt: sc.row_state(z, *gt) for gt in order}
    return rows, [states[gt] for gt in rows]


@functools.lru_cache(maxsize=None)
def load_plan():
    """the call's 397 entries: slot k into env perm[k], 64 of the slots into a second env each,
    in a fixed shuffled order; (slots, envs) and the envs not named"""
    perm = np.random.RandomState(11).permutation(NB)
    slots = np.concatenate([np.arange(N2), np.arange(N2)[::5][:FAN]])
    envs = perm[:N2 + FAN]
    order = np.random.RandomState(12).permutation(N2 + FAN)
    assert len(slots) == 397 and 397 % 64 != 0 and 397 > 256 and len(set(envs.tolist())) == 397
    return slots[order], envs[order], np.sort(perm[N2 + FAN:])


@pytest.mark.parametrize("pre", [0, 5, 17])
@pytest.mark.parametrize("mode", ["compact", "direct"])
def test_load_continues_reference_rows(tg, mode, pre):
    z = fixture("traj_autoreset.npz")
    rows, states = restore_rows()
    slots, envs, others = load_plan()
    g_of = np.array([rows[s][0] for s in slots])
    t_of = np.array([rows[s][1] for s in slots])
    a0 = 0xBEEF
    vec, twin = (tg.TreasureGameVec(NB, seed=424242, autoreset=True, mode=mode) for _ in range(2))
    for v in (vec, twin):
        v.reset()
        for t in range(pre):  # the rings and refill lists in every phase of the 16-step cadence
            v.step(v.policy_actions(t, a0, "masked"))
    while len(vec.episodes()):  # (its own episodes so far: not the load's business)
        pass
    snap = vec.snapshot(N2)
    snap.write(sc.stack(states))
    back = snap.read()
    for k, want in sc.stack(states).items():  # a written record is read back verbatim, 624 too
        assert np.array_equal(back[k].view(np.uint64) if k == "ang" else back[k],
                              want.view(np.uint64) if k == "ang" else want), k
    assert (back["mt_pos"] == 624).sum() >= 8
    d_envs = dev(envs)
    snap.load(dev(slots), d_envs)
    loaded = [rows[s] for s in slots]
    check_game_state(rows_of(vec.read_state(), envs), z, loaded, "read back")
    for k in range(1, K2 + 1):
        acts = vec.policy_actions(pre + k, a0, "masked").clone()
        acts[d_envs] = torch.as_tensor(z["action"][g_of, t_of + k].astype(np.int32), device="cuda")
        o, r, v, d, info = vec.step(acts)
        o2, r2, v2, d2, info2 = twin.step(twin.policy_actions(pre + k, a0, "masked"))
        at = (mode, pre, k)
        for x, y in ((o, o2), (r, r2), (v, v2), (d, d2), (info["final_obs"], info2["final_obs"])):
            assert torch.equal(x[others], y[others]), at
        o, fo, r, v, d = (x.cpu().numpy()[envs] for x in (o, info["final_obs"], r, v, d))
        assert np.array_equal(bits(o), bits(z["obs"][g_of, t_of + k])), at
        assert np.array_equal(bits(fo), bits(z["final_obs"][g_of, t_of + k])), at
        assert np.array_equal(r, z["reward"][g_of, t_of + k]), at
        assert np.array_equal(v, z["valid"][g_of, t_of + k]), at
        assert np.array_equal(d, z["done"][g_of, t_of + k]), at
    end = [(g, t + K2) for g, t in loaded]
    st, st2 = vec.read_state(mt=True), twin.read_state(mt=True)
    check_game_state(rows_of(st, envs), z, end, "after %d steps" % K2)
    check_rng(rows_of(st, envs), z, end, "after %d steps" % K2)
    same_state(st, st2, "the envs not named", others)
    # the cadence is not restarted: k_regen ran exactly when the twin's did
    assert vec.stats()["regen_launches"] == twin.stats()["regen_launches"]
    # the episode records: return and length counted from before the save (the slot's ep)
    want = []
    for env, (g, t) in zip(envs.tolist(), loaded):
        for td in range(t + 1, t + K2 + 1):
            if z["done"][g, td]:
                ret, length = sc.row_state(z, g, td - 1, mt=False)["ep"]
                want.append((env, int(ret) + int(z["reward"][g, td]), int(length) + 1))
    assert len({e for e, _, _ in want}) >= 6
    assert sum(length > K2 for _, _, length in want) >= 6  # begun before the save
    named = set(envs.tolist())
    got = [tuple(int(x) for x in rec) for rec in vec.episodes(cap=4 * NB).cpu().numpy()]
    assert sorted(rec for rec in got if rec[0] in named) == sorted(want)
    assert vec.errors() == 0 and twin.errors() == 0
    vec.close()  # (with the snapshot open)
    twin.close()


# ---- 3. reseeding ---------------------------------------------------------------------------------------
def test_load_with_seeds(tg):
    import pyref
    n, a0 = 130, 0x1D0
    z = fixture("traj_autoreset.npz")
    g, t = 3, 1210
    assert str(z["bag"][g, t]) == "K" and not z["done"][g, t]  # a state no fresh env is in
    slot = sc.row_state(z, g, t)
    vec = tg.TreasureGameVec(n, seed=99, autoreset=True)
    vec.reset()
    for k in range(3):
        vec.step(vec.policy_actions(k, a0, "masked"))
    snap = vec.snapshot(4)
    snap.write(sc.stack([slot]), first=2)
    envs = dev(np.arange(n))
    seeds = [9000 + k for k in range(n)]
    snap.load(dev([2] * n), envs, seeds=torch.as_tensor(np.array(seeds, np.int64), device="cuda"))
    st = vec.read_state(mt=True)
    check_game_state(st, z, [(g, t)] * n, "reseeded")
    refs = []
    for k in range(n):
        s = random.Random(seeds[k]).getstate()[1]
        assert s[624] == 624
        assert int(st["mt_pos"][k]) == 0, k
        assert sc.same_stream((st["mt"][k], 0), (s[:624], 624)), k
        one = dict(slot, mt=np.array(s[:624], np.uint32), mt_pos=np.uint32(624))
        env = pyref.Env(12345 + k)
        env.reset()
        sc.inject_pyref(env, one)
        refs.append(env)
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
    assert len({tuple(p) for p in st["pos"].tolist()}) > 1  # the streams differ: so do the envs
    # without seeds: one stream, so the envs stay identical under identical actions
    snap.load(dev([2] * n), envs)
    for t in range(10):
        a = int(vec.policy_actions(t, a0, "masked")[0])
        o, r, v, d, info = vec.step(torch.full((n,), a, dtype=torch.int32, device="cuda"))
        for x in (o, r, v, d, info["final_obs"]):
            assert torch.equal(x, x[:1].expand_as(x)), t
    st = vec.read_state(mt=True)
    for k in st:
        assert (st[k] == st[k][:1]).all(), k
    assert vec.errors() == 0
    vec.close()


# ---- 4. fork ----------------------------------------------------------------------------------------------
def test_fork_with_overlap_and_fan_out(tg):
    n, a0 = 301, 0xF0
    vec = tg.TreasureGameVec(n, seed=7, autoreset=True)
    vec.reset()
    for t in range(25):
        vec.step(vec.policy_actions(t, a0, "masked"))
    st0 = vec.read_state(mt=True)
    assert len({tuple(st0["pos"][i].tolist()) + (int(st0["mt_pos"][i]),) for i in range(4)}) == 4
    src, dst = [0, 1, 2, 3], [1, 2, 3, 0]
    vec.fork(src, dst)  # every source is read before any destination is written
    st1 = vec.read_state(mt=True)
    for k in st0:
        want = st0[k].copy()
        want[dst] = st0[k][src]
        assert np.array_equal(want.view(np.uint64) if k == "ang" else want,
                              st1[k].view(np.uint64) if k == "ang" else st1[k]), k
    rest = [i for i in range(n) if i != 5]
    vec.fork([5] * 300, rest)  # 1 -> 300 (the scratch snapshot grows)
    st2 = vec.read_state(mt=True)
    for k in st2:
        assert (st2[k] == st1[k][5:6]).all(), k
    for t in range(8):
        a = int(vec.policy_actions(t, a0, "masked")[5])
        o, r, v, d, info = vec.step(torch.full((n,), a, dtype=torch.int32, device="cuda"))
        for x in (o, r, v, d, info["final_obs"]):
            assert torch.equal(x, x[:1].expand_as(x)), t
    # with seeds the copies part ways
    vec.fork([5] * 300, rest, seeds=np.arange(300, dtype=np.uint64) + 2**63)
    st3 = vec.read_state(mt=True)
    for k in ("pos", "flags", "objs", "ep"):
        assert (st3[k] == st3[k][5:6]).all(), k
    for i in (0, 299):
        s = random.Random(2**63 + i).getstate()[1]
        assert sc.same_stream((st3["mt"][rest[i]], st3["mt_pos"][rest[i]]), (s[:624], s[624])), i
    assert vec.errors() == 0
    vec.close()


# ---- 5. the step limit counts the slot's length -------------------------------------------------------------
def test_loaded_length_counts_toward_the_step_limit(tg):
    z = fixture("traj_autoreset.npz")
    g, t0, limit, n, env = 1, 40, 50, 70, 66
    assert not z["done"][g, t0:t0 + 4].any()
    slot = sc.row_state(z, g, t0)
    slot["ep"] = np.array([7, limit - 3], np.int32)
    vec = tg.TreasureGameVec(n, seed=5, autoreset=True, max_episode_steps=limit)
    vec.reset()
    for t in range(6):
        vec.step(vec.policy_actions(t, 1, "masked"))
    while len(vec.episodes()):
        pass
    snap = vec.snapshot(1)
    snap.write(sc.stack([slot]))
    snap.load(dev([0]), dev([env]))
    for k in range(1, 4):
        acts = vec.policy_actions(6 + k, 1, "masked").clone()
        acts[env] = int(z["action"][g, t0 + k])
        o, r, v, d, info = vec.step(acts)
        assert int(r[env]) == int(z["reward"][g, t0 + k])
        assert np.array_equal(bits(info["final_obs"][env].cpu().numpy()), bits(z["final_obs"][g, t0 + k]))
        assert int(d[env]) == (tg.DONE_TRUNCATED if k == 3 else 0), k
    recs = [rec for rec in vec.episodes(cap=4 * n, truncated=True).cpu().tolist() if rec[0] == env]
    assert recs == [[env, 7 + int(z["reward"][g, t0 + 1:t0 + 4].sum()), limit, 1]]
    st = vec.read_state()
    assert st["ep"][env].tolist() == [0, 0]  # reset by the truncation
    assert vec.errors() == 0
    vec.close()


# ---- 6. bad indices and arguments -----------------------------------------------------------------------------
def test_bad_indices_and_arguments(tg):
    n, a0, slots = 100, 0xD00D, 10
    z = fixture("traj_autoreset.npz")
    vec, twin = (tg.TreasureGameVec(n, seed=5, autoreset=True) for _ in range(2))
    for v in (vec, twin):
        v.reset()
        for t in range(20):
            v.step(v.policy_actions(t, a0, "masked"))
    snap = vec.snapshot(slots)
    recs = [sc.row_state(z, i % 8, 2000 + 3 * i) for i in range(slots)]
    snap.write(sc.stack(recs))
    before = snap.read()
    L, h, s = vec._L, vec.handle, snap.handle
    ok_e, ok_s = dev([1, 2]), dev([0, 1])
    other = twin.snapshot(2)
    inval = [L.tg_snap_save(None, s, ok_e.data_ptr(), ok_s.data_ptr(), 2, None),
             L.tg_snap_save(h, None, ok_e.data_ptr(), ok_s.data_ptr(), 2, None),
             L.tg_snap_save(h, s, None, ok_s.data_ptr(), 2, None),
             L.tg_snap_save(h, s, ok_e.data_ptr(), None, 2, None),
             L.tg_snap_save(h, s, ok_e.data_ptr(), ok_s.data_ptr(), -1, None),
             L.tg_snap_save(h, other.handle, ok_e.data_ptr(), ok_s.data_ptr(), 2, None),
             L.tg_snap_load(None, s, ok_s.data_ptr(), ok_e.data_ptr(), None, 2, None),
             L.tg_snap_load(h, None, ok_s.data_ptr(), ok_e.data_ptr(), None, 2, None),
             L.tg_snap_load(h, s, None, ok_e.data_ptr(), None, 2, None),
             L.tg_snap_load(h, s, ok_s.data_ptr(), None, None, 2, None),
             L.tg_snap_load(h, s, ok_s.data_ptr(), ok_e.data_ptr(), None, -1, None),
             L.tg_snap_load(h, other.handle, ok_s.data_ptr(), ok_e.data_ptr(), None, 2, None)]
    assert inval == [tg._lib.TG_E_INVAL] * len(inval)
    out = ctypes.c_void_p()
    for bad_slots in (0, -3):
        assert L.tg_snap_create(h, bad_slots, ctypes.byref(out)) == tg._lib.TG_E_INVAL
    assert L.tg_snap_save(h, s, ok_e.data_ptr(), ok_s.data_ptr(), 0, None) == 0  # count 0: nothing
    assert L.tg_snap_load(h, s, ok_s.data_ptr(), ok_e.data_ptr(), None, 0, None) == 0
    # a rejected write (the bad entry in the last record) changes nothing
    worse = sc.stack([sc.row_state(z, i % 8, 100 + i) for i in range(slots)])
    for key, val in (("mt_pos", 311), ("mt_pos", 626), ("pos", 40000), ("objs", 200)):
        bad = {k: v.copy() for k, v in worse.items()}
        bad[key].reshape(slots, -1)[slots - 1, -1] = val
        with pytest.raises(tg.TgError):
            snap.write(bad)
    with pytest.raises(ValueError):
        snap.write(worse, first=1)
    same_state(snap.read(), before, "after the rejected calls")
    same_state(vec.read_state(mt=True), twin.read_state(mt=True), "after the rejected calls")
    assert vec.errors() == 0
    # bad entries among valid ones: env N, env -1 and slot `slots`
    l_slots, l_envs = [0, 1, 2, 3, slots, 4], [3, n, 7, -1, 20, 9]
    snap.load(dev(l_slots), dev(l_envs))
    assert vec.errors() == tg.TG_ERR_INDEX
    st, st2 = vec.read_state(mt=True), twin.read_state(mt=True)
    good = {3: 0, 7: 2, 9: 4}
    for env, k in good.items():
        for key in ("pos", "flags", "objs", "ep"):
            assert np.array_equal(st[key][env], recs[k][key]), (env, key)
        assert np.array_equal(bits(st["ang"][env]), bits(recs[k]["ang"]))
        assert sc.same_stream((st["mt"][env], st["mt_pos"][env]), (recs[k]["mt"], recs[k]["mt_pos"]))
    same_state(st, st2, "envs not named", [i for i in range(n) if i not in good])
    # the same in a save: env N into slot 5, env 2 into slot `slots`, and env 2 into slot 6
    snap.save(dev([n, 2, 2, -1]), dev([5, slots, 6, 7]))
    after = snap.read()
    keep = [i for i in range(slots) if i != 6]
    same_state(after, before, "slots not named", keep)
    for key in ("pos", "flags", "objs", "ang", "mt", "mt_pos", "ep"):
        assert np.array_equal(after[key][6], st[key][2]), key
    assert vec.errors() == tg.TG_ERR_INDEX and twin.errors() == 0
    # the flag is the handle's: no env's flag word has it, and the envs step on as the twin's
    assert not (vec.read_state()["flags"] >> 24).any()
    for t in range(20, 30):
        ra = vec.step(vec.policy_actions(t, a0, "masked"))
        rb = twin.step(twin.policy_actions(t, a0, "masked"))
        rest = [i for i in range(n) if i not in good]
        for x, y in zip(ra[:4], rb[:4]):
            assert torch.equal(x[rest], y[rest]), t
    other.close()
    vec.close()
    twin.close()


# ---- 7. lifecycle --------------------------------------------------------------------------------------------
def test_snapshots_are_counted_and_freed(tg):
    L = tg._lib.load()
    base = L.tg_live_resources()
    vec = tg.TreasureGameVec(50, seed=1)
    vec.reset()
    live = L.tg_live_resources()
    snap = vec.snapshot(5)
    assert len(snap) == 5 and L.tg_live_resources() == live + 4
    snap.close()
    assert L.tg_live_resources() == live
    snap.close()  # (idempotent)
    left = vec.snapshot(9)
    vec.fork([1], [2])  # (and the scratch snapshot)
    assert L.tg_live_resources() == live + 8
    raw = ctypes.c_void_p()  # one the Python object does not know of: tg_destroy's to free
    assert L.tg_snap_create(vec.handle, 3, ctypes.byref(raw)) == 0 and L.tg_snap_slots(raw) == 3
    assert L.tg_live_resources() == live + 12
    vec.close()  # with all three open
    assert L.tg_live_resources() == base
    with pytest.raises(tg.TgError):
        left.read()


def test_save_and_load_under_the_resident_server(tg, monkeypatch):
    """A 1-env handle whose server is resident: save and load stop it themselves, and the env
    continues from the loaded state, not from the copy the server held."""
    monkeypatch.setenv("TG_SERVE_IDLE_US", "200000")  # resident between this test's calls
    acts = [1, 4, 0, 3, 1, 6, 2, 8, 5, 7, 1, 0]

    def run(env):
        out = []
        for a in acts:
            st, r, d, _ = env.step(a)
            out.append((bits(st).tolist(), r, d))
        return out

    # (everything that launches or synchronises outside the two envs' own calls comes first: a
    # device-wide wait behind a resident server lasts until its idle limit)
    zero = dev([0])
    env = tg.TreasureGame(seed=77)
    env2 = tg.TreasureGame(seed=78)
    env2._vec.read_state()  # (its server, if any, stopped)
    env._vec.set_serve(True)
    env.reset()
    for t in range(9):
        env.step(t % 9)
    snap = env._vec.snapshot(1)  # the server is resident: every snapshot call stops it itself
    for t in range(3):
        env.step(t)
    snap.save(zero, zero)
    rec = snap.read()
    first = run(env)
    assert len({tuple(o) for o, _, _ in first}) > 1  # the env moved on
    snap.load(zero, zero)
    again = run(env)
    assert again == first
    end = env._vec.read_state(mt=True)
    # the same 12 steps from the saved record through the checkpoint path
    env2._vec.write_state(rec)
    assert run(env2) == first
    end2 = env2._vec.read_state(mt=True)
    for k in ("pos", "flags", "objs", "ang", "ep"):
        assert np.array_equal(end[k], end2[k]), k
    assert sc.same_stream((end["mt"][0], end["mt_pos"][0]), (end2["mt"][0], end2["mt_pos"][0]))
    assert env._vec.errors() == 0 and env2._vec.errors() == 0
    env.close()
    env2.close()
