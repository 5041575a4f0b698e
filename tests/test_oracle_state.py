"""State injection on the C oracle (tgo_env_set_state / tgo_env_get_state, the tick-limited
step, the threaded oracle.step_states and oracle.render_states), pinned on the CPU before the
sweeps rely on it:
against the reference's recorded fixtures, and against the Python restatement (oracle/pyref.py
through state_codec.inject_pyref) on synthesized states under the same tick limit."""
import glob
import os
import random

import numpy as np
import pytest

import state_codec as sc
import state_sweep as ss

TRAJ = sorted(os.path.basename(p) for p in glob.glob(os.path.join(sc.GOLDEN, "traj_*.npz")))
K = 24


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", TRAJ)
def test_injected_rows_continue_the_fixture(oracle, name):
    """rows of every fixture (3 envs x 3 time points), each injected into an OracleEnv built
    from another seed, continue the fixture for 24 steps bit for bit (obs, final obs, reward,
    valid, done), arrive at the fixture's row, and end on its stream"""
    z = sc.load(name)
    ld = sc.level_dir_of(z)
    n, t1 = z["valid"].shape
    autoreset = bool(z["autoreset"])
    steps = 0
    for g in (0, n // 2, n - 1):
        for t0 in (0, t1 // 3, t1 - 1 - K):
            env = oracle.OracleEnv(424242 + 31 * g + t0, ld)
            start = sc.row_state(z, g, t0)
            env.set_state(start)
            back = env.get_state()
            for k in ("pos", "flags", "objs", "mt", "mt_pos"):
                assert np.array_equal(back[k], start[k]), (g, t0, k)
            assert np.array_equal(bits(back["ang"]), bits(start["ang"])), (g, t0)
            for t in range(t0 + 1, t0 + K + 1):
                fo, r, d, _ = env.step(int(z["action"][g, t]))
                o = env.reset() if (d and autoreset) else fo
                assert np.array_equal(bits(fo), bits(z["final_obs"][g, t])), (g, t)
                assert np.array_equal(bits(o), bits(z["obs"][g, t])), (g, t)
                assert (0 if r is None else r) == z["reward"][g, t], (g, t)
                assert (r is not None) == bool(z["valid"][g, t]) and d == bool(z["done"][g, t]), (g, t)
                steps += 1
            want, got = sc.row_state(z, g, t0 + K), env.get_state()
            for k in ("pos", "flags", "objs", "mt", "mt_pos"):  # CPython's own index, 624 included
                assert np.array_equal(got[k], want[k]), (g, t0, k)
            assert np.array_equal(bits(got["ang"]), bits(want["ang"])), (g, t0)
    assert steps == 9 * K


def test_set_state_rejects_what_the_format_does_not_admit(oracle):
    env = oracle.OracleEnv(1)
    st = env.get_state()
    for flags, pos in ((1 << 22, 0), (1 << 24, 0), (1 << 15, 0), (0, 626)):
        bad = dict(st, flags=np.uint32(int(st["flags"]) | flags), mt_pos=np.uint32(pos or st["mt_pos"]))
        with pytest.raises(ValueError):
            env.set_state(bad)


def test_stream_states_are_cpython_getstate(oracle):
    """oracle.stream_states (the sweeps' streams) against random.Random itself: words, index,
    and the successor form as the same stream; the index cycle"""
    mt, pos = oracle.stream_states(ss.STREAM_BASE, 35, 28)
    assert pos.tolist() == [0, 2, 310, 312, 620, 622, 624] * 4
    draws = (312, 1, 155, 156, 310, 311, 312)
    for k in range(28):
        r = random.Random(ss.STREAM_BASE + 35 + k)
        for _ in range(draws[k % 7]):
            r.random()
        want = r.getstate()[1]
        if k % 7:
            assert want[624] == pos[k] and list(want[:624]) == mt[k].tolist(), k
        else:
            assert want[624] == 624 and sc.same_stream((mt[k], 0), (want[:624], 624)), k
    # successor_form (the comparison's normalisation) is CPython's twist
    a, ap = ss.successor_form(mt[6::7], pos[6::7])
    assert ap.tolist() == [0] * 4
    for k in range(4):
        assert sc.same_stream((a[k], 0), (mt[6 + 7 * k], 624))
        assert not sc.same_stream((a[k], 2), (mt[6 + 7 * k], 624))


def test_single_env_step_under_the_limit_is_the_batch_entry(oracle):
    """OracleEnv.set_state + step_cap + get_state against oracle.step_states, on cases that
    finish, cases that cannot run and cases that hit the limit"""
    cap, count = 2048, 400
    sw = ss.step_tier()
    st = sw.states(0, count)
    ref = oracle.step_states(st, sw.actions[:count], cap=cap)
    assert ref["capped"].sum() >= 2 and 0 < ref["valid"].sum() < count
    env = oracle.OracleEnv(77)
    for i in range(count):
        env.set_state({k: st[k][i] for k in st})
        assert env.mask() == ref["mask"][i], sw.describe(i)
        d0, t0 = env.draws(), env.ticks()
        o, r, d, capped = env.step_cap(int(sw.actions[i]), cap)
        assert capped == bool(ref["capped"][i]), sw.describe(i)
        assert np.array_equal(bits(o), bits(ref["obs"][i])), sw.describe(i)
        assert (0 if r is None else r) == ref["reward"][i] and d == bool(ref["done"][i])
        assert (r is not None) == bool(ref["valid"][i]), sw.describe(i)
        assert env.draws() - d0 == ref["draws"][i] and env.ticks() - t0 == ref["ticks"][i]
        after = env.get_state()
        for k in ("pos", "flags", "objs", "mt", "mt_pos"):
            assert np.array_equal(after[k], ref[k][i]), (k, sw.describe(i))
        assert np.array_equal(bits(after["ang"]), bits(ref["ang"][i])), sw.describe(i)


def pyref_step(env, a, cap):
    """env.step(a) of the restatement, its option loop (OP/:20-36) under the tick limit"""
    o = env.options[a]
    ticks, capped, r = 0, False, None
    if o.can_run():
        o.done = False
        r = 0
        while not o.done:
            r += env.game.tick(o.policy_step())
            ticks += 1
            if ticks >= cap:
                capped = True
                break
    g = env.game
    return g.get_state(), r, bool(g.got("gold") and g.cell()[1] == 0), ticks, capped


@pytest.mark.parametrize("name,count", [(None, 2000), ("cascade", 600)])
def test_step_states_match_the_restatement(oracle, name, count):
    """the first ``count`` cases of the (permuted) step tier: oracle.step_states against pyref
    through inject_pyref under the same tick limit: mask, outputs, state after, stream after,
    ticks and the capped verdict"""
    import pyref
    cap = 2048
    sw = ss.step_tier(name)
    st = sw.states(0, count)
    ref = oracle.step_states(st, sw.actions[:count], cap=cap, level_dir=sw.level_dir)
    level = pyref.read_level(sw.level_dir)
    env = pyref.Env(5, level)
    ran = ncap = 0
    for i in range(count):
        what = sw.describe(i)
        env.reset()
        sc.inject_pyref(env, {k: st[k][i] for k in st})
        mask = sum(b << k for k, b in enumerate(env.available_mask()))
        assert mask == ref["mask"][i], what
        o, r, d, ticks, capped = pyref_step(env, int(sw.actions[i]), cap)
        assert capped == bool(ref["capped"][i]) and ticks == ref["ticks"][i], what
        assert np.array_equal(bits(o), bits(ref["obs"][i])), what
        assert (0 if r is None else r) == ref["reward"][i], what
        assert (r is not None) == bool(ref["valid"][i]) and d == bool(ref["done"][i]), what
        g = env.game
        row = [g.px, g.py, g.jump_ticker, sum(int(x.closed) << j for j, x in enumerate(g.doors)),
               sum(int(x.up) << j for j, x in enumerate(g.handles)), int(g.bolts[0].locked)]
        key = next(x for x in g.objects if x.kind == "key")
        gold = next(x for x in g.objects if x.kind == "gold")
        row += [key.cx, key.cy, gold.cx, gold.cy, int(g.facing_right)]
        bag = "".join("K" if x is key else "G" for x in g.bag)
        after = {k: ref[k][i] for k in ("pos", "flags", "objs")}
        assert (row, bag) == sc.decode(after), what
        assert [h.angle for h in g.handles] == ref["ang"][i].tolist(), what
        assert env.rng.getstate() == sc.pystate(ref["mt"][i], ref["mt_pos"][i]), what
        ran += r is not None
        ncap += capped
    assert ran >= count // 10 and ncap >= 1   # the sample runs options, and meets the limit


def _sprites(seed):
    from gym_treasure_game_amd import render as R
    return R.synthetic_sprites(seed=seed)


@pytest.mark.parametrize("name", [None, "render_overlap", "narrow"])
def test_render_states_is_set_state_then_render(oracle, name):
    """the threaded oracle.render_states against OracleEnv.set_state + render, frame by frame,
    on the first 40 cases of the (permuted) render sweep"""
    import render_sweep as rs
    sw = rs.sweep(name)
    sprites = _sprites(17)
    st = sw.states(0, 40, mt=False)
    frames = oracle.render_states(st, sprites, level_dir=sw.level_dir)
    assert frames.shape == (40, sw.lv["H"] * 48, sw.lv["W"] * 48, 3) and frames.dtype == np.uint8
    env = oracle.OracleEnv(99, sw.level_dir)
    for i in range(40):
        env.set_state({k: st[k][i] for k in ("pos", "flags", "objs", "ang")})
        assert np.array_equal(env.render(sprites), frames[i]), sw.describe(i)
    assert len({f.tobytes() for f in frames}) == 40
    one = oracle.render_states(st, sprites, level_dir=sw.level_dir, nthreads=1)
    assert np.array_equal(one, frames)


@pytest.mark.parametrize("name,policy,autoreset,a0", [(None, 1, True, 0x51), ("corridor", 1, True, 9),
                                                      ("render_overlap", 1, True, 5),
                                                      (None, 0, False, 0x52)])
def test_render_states_of_replayed_envs_is_run_render(oracle, name, policy, autoreset, a0):
    """envs replayed as run_render replays them (seed base 0, the run() action stream):
    render_states(get_state()) is run_render's frame, at a few step counts; this ties the new
    entry point to every pin of run_render"""
    import render_sweep as rs
    level_dir = rs.LEVELS[name] if name else None
    sprites = _sprites(23)
    envs = np.arange(6) * 5
    for steps in (0, 7, 33):
        rows = []
        for g in envs.tolist():
            env = oracle.OracleEnv(g, level_dir)
            for t in range(steps):
                m = env.mask() if policy else 0
                _, _, d, _ = env.step(oracle.pick_action(a0, g, t, bool(policy), m))
                if d and autoreset:
                    env.reset()
            rows.append(env.get_state())
        st = {k: np.stack([r[k] for r in rows]) for k in ("pos", "flags", "objs", "ang")}
        got = oracle.render_states(st, sprites, level_dir=level_dir)
        want = oracle.run_render(0, envs, steps, a0, policy, autoreset, sprites, level_dir=level_dir)
        assert np.array_equal(got, want), (name, steps)
