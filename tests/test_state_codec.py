"""tests/state_codec.py against the reference's fixtures, on the CPU: the helper that the GPU
checkpoint tests (test_gpu_state.py) use as their reference side reproduces every fixture row
and, injected into the Python restatement of the reference, continues the fixture exactly.  A
failure there then points at the product, not at the helper."""
import glob
import os

import numpy as np
import pytest

import state_codec as sc

TRAJ = sorted(os.path.basename(p) for p in glob.glob(os.path.join(sc.GOLDEN, "traj_*.npz")))


def test_fixture_list():
    assert "traj_autoreset.npz" in TRAJ and "traj_level_cascade_masked.npz" in TRAJ
    assert len(TRAJ) >= 15


def test_handle_columns():
    """the default level lists its handles fourth and fifth: obs columns 2 and 3; the exit
    level's lie after three doors too"""
    assert sc.handle_columns(sc.DEFAULT_LEVEL) == [2, 3]
    for name in ("corridor", "gen1", "gen2", "gen3", "exit", "cascade"):
        cols = sc.handle_columns(os.path.join(sc.GOLDEN, "levels", name))
        assert len(cols) == 2 and cols[0] < cols[1] < 9, (name, cols)


LEVELS = ("corridor", "gen1", "gen2", "gen3", "exit", "cascade")


@pytest.mark.parametrize("name", [None] + list(LEVELS))
def test_handle_columns_match_get_state(name):
    """the columns against the restatement's own get_state: the slots its Handle objects fill"""
    import random
    import pyref
    ld = os.path.join(sc.GOLDEN, "levels", name) if name else sc.DEFAULT_LEVEL
    game = pyref.Game(pyref.read_level(ld), random.Random(3))
    cols, c = [], 2
    for o in game.objects:
        if o.kind == "handle":
            cols.append(c)
        c += len(o.state())
    assert c == 9 and sc.handle_columns(ld) == cols
    for i, h in enumerate(game.handles):
        h.angle = 0.123 + i
    s = game.get_state()
    assert [s[k] for k in cols] == [0.123, 1.123]


@pytest.mark.parametrize("name", ["traj_level_cascade_masked.npz", "traj_level_corridor_masked.npz",
                                  "traj_level_gen2_masked.npz"])
def test_injected_level_rows_continue_the_fixture(name):
    """rows of level fixtures (other objects files, so other angle columns) injected into pyref
    continue their fixtures: 4 envs x 2 time points x 12 steps each"""
    import pyref
    z = sc.load(name)
    level = pyref.read_level(sc.level_dir_of(z))
    for g in (0, 5, 10, 15):
        for t0 in (150, 570):
            env = pyref.Env(777 + g, level)
            env.reset()
            sc.inject_pyref(env, sc.row_state(z, g, t0))
            for t in range(t0 + 1, t0 + 13):
                o, r, d, _ = env.step(int(z["action"][g, t]))
                assert np.array_equal(np.array(o).view(np.uint64), z["final_obs"][g, t].view(np.uint64)), (g, t)
                if d:
                    o = env.reset()
                assert np.array_equal(np.array(o).view(np.uint64), z["obs"][g, t].view(np.uint64)), (g, t)
                assert (0 if r is None else r) == z["reward"][g, t] and d == bool(z["done"][g, t]), (g, t)
            want = sc.row_state(z, g, t0 + 12)
            assert env.rng.getstate() == sc.pystate(want["mt"], want["mt_pos"])


@pytest.mark.parametrize("name", TRAJ)
def test_decode_reproduces_every_row(name):
    z = sc.load(name)
    n, t1 = z["valid"].shape
    internal, bags = z["internal"], z["bag"]
    for g in range(n):
        for t in range(t1):
            st = sc.row_state(z, g, t, mt=False)
            row, bag = sc.decode(st)
            assert row == internal[g, t, :11].tolist() and bag == str(bags[g, t]), (g, t)
            assert st["pos"].dtype == np.int32 and st["objs"].dtype == np.int32
            assert st["flags"].dtype == np.uint32 and st["ang"].dtype == np.float64
            assert st["ep"].dtype == np.int32


def test_rng_part_is_getstate():
    """mt / mt_pos of a row: the dtypes, an even index in 2..624 (CPython never reports 0),
    and the stream the counted draws give"""
    import random
    z = sc.load("traj_autoreset.npz")
    for g, t in ((0, 0), (3, 17), (7, 4000), (2, 629), (2, 630)):
        st = sc.row_state(z, g, t)
        assert st["mt"].dtype == np.uint32 and st["mt"].shape == (624,)
        assert st["mt_pos"].dtype == np.uint32
        assert 2 <= int(st["mt_pos"]) <= 624 and int(st["mt_pos"]) % 2 == 0
        r = random.Random(int(z["seed_base"]) + g)
        for _ in range(int(z["draws"][g, t])):
            r.random()
        assert sc.pystate(st["mt"], st["mt_pos"]) == r.getstate()
    # ref_index: the index the GPU tests select their rows by, against CPython over two twists
    r = random.Random(11)
    for d in range(700):
        assert r.getstate()[1][624] == sc.ref_index(d), d
        r.random()
    assert [(sc.ref_index(z["draws"]) == k).sum() for k in (622, 624, 2)] == [103, 103, 81]
    # (generation, 624) and (successor, 0) are one stream; a shifted index is another
    r = random.Random(5)
    for _ in range(312):
        r.random()
    a = r.getstate()[1]
    assert a[624] == 624
    r.getrandbits(32)
    b = r.getstate()[1]
    assert b[624] == 1
    assert sc.same_stream((a[:624], 624), (b[:624], 0))
    assert not sc.same_stream((a[:624], 624), (b[:624], 2))
    assert not sc.same_stream((a[:624], 624), (a[:624], 0))


def test_ep_is_the_unfinished_episode():
    """ep against a direct count on the fixture: return and length since the last done row"""
    z = sc.load("traj_autoreset.npz")
    done = z["done"]
    assert done[2, 629] == 1 and done[2, :629].sum() == 0
    assert sc.row_state(z, 2, 629, mt=False)["ep"].tolist() == [0, 0]
    assert sc.row_state(z, 2, 628, mt=False)["ep"].tolist() == [int(z["reward"][2, 1:629].sum()), 628]
    assert sc.row_state(z, 2, 640, mt=False)["ep"].tolist() == [int(z["reward"][2, 630:641].sum()), 11]
    assert sc.row_state(z, 0, 0, mt=False)["ep"].tolist() == [0, 0]
    assert (z["reward"][z["valid"] == 0] == 0).all()
    u = sc.load("traj_masked.npz")  # recorded without auto-reset: since row 0
    assert sc.row_state(u, 1, 1500, mt=False)["ep"].tolist() == [int(u["reward"][1].sum()), 1500]


def test_injected_rows_continue_the_fixture():
    """8 envs x 6 time points of traj_autoreset.npz, each injected into a pyref Env built from
    another seed, continue the fixture for 40 steps: obs bits, reward, done (1,920 steps)"""
    import pyref
    z = sc.load("traj_autoreset.npz")
    level = pyref.read_level()
    points = (0, 613, 1200, 2047, 3100, 3960)
    assert z["done"][2, 614:654].any()  # an episode ends inside a window (env 2, row 629)
    steps = 0
    for g in range(8):
        for t0 in points:
            env = pyref.Env(9000 + 17 * g + t0, level)
            env.reset()
            sc.inject_pyref(env, sc.row_state(z, g, t0))
            for t in range(t0 + 1, t0 + 41):
                o, r, d, _ = env.step(int(z["action"][g, t]))
                fo = np.array(o)
                if d:
                    o = env.reset()
                assert np.array_equal(fo.view(np.uint64), z["final_obs"][g, t].view(np.uint64)), (g, t)
                assert np.array_equal(np.array(o).view(np.uint64), z["obs"][g, t].view(np.uint64)), (g, t)
                assert (0 if r is None else r) == z["reward"][g, t], (g, t)
                assert (r is not None) == bool(z["valid"][g, t]) and d == bool(z["done"][g, t]), (g, t)
                steps += 1
            # and the state it arrives at is the fixture's row, RNG included
            want = sc.row_state(z, g, t0 + 40)
            assert env.rng.getstate() == sc.pystate(want["mt"], want["mt_pos"])
            assert env.game.px == want["pos"][0] and env.game.py == want["pos"][1]
    assert steps == 1920
