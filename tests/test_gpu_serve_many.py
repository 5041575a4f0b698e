"""The N = 1 drop-in's resident server (k_serve1) the way the reference env is used: several envs
alive in one process (each handle with a server of its own, more servers than the process has
hardware queues), several envs drawing from Python's one global ``random``, torch work and a
batched handle between the served steps, the handle's other entry points between them,
out-of-range actions through the C ABI, and two handles whose servers ask for different amounts
of dynamic LDS.  Everything is compared bit for bit with the oracle (private streams) or with
oracle/pyref.py over one shared ``Random`` (shared streams), served and launch-per-call.

No single env call here may take longer than MAX_CALL_S of wall time: about 500 x the worst wait
the design allows (a 500-us idle limit x at most 4 servers ahead on a queue, plus a relaunch) and
20 x below the 20 s after which the library gives up, so it catches starvation whatever the box's
speed.  Mean times per step() are printed (pytest -s), never asserted."""
import ctypes
import gc
import os
import random
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_CALL_S = 1.0
HERE = os.path.dirname(os.path.abspath(__file__))
COUNTERS = ("steps", "valid_steps", "ticks", "draws")


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def mask_bits(ref):
    return [(ref.mask() >> k) & 1 for k in range(9)]


def live(tg):
    return tg._lib.load().tg_live_resources()


class Clock:
    """Runs the env calls of one test: every call under MAX_CALL_S; step() times summed by key"""

    def __init__(self):
        self.sum, self.n = {}, {}

    def __call__(self, fn, *args, key=None):
        t0 = time.perf_counter()
        out = fn(*args)
        dt = time.perf_counter() - t0
        assert dt < MAX_CALL_S, "%s took %.3f s" % (getattr(fn, "__name__", fn), dt)
        if key is not None:
            self.sum[key] = self.sum.get(key, 0.0) + dt
            self.n[key] = self.n.get(key, 0) + 1
        return out

    def us(self, key):
        return 1e6 * self.sum[key] / self.n[key] if self.n.get(key) else float("nan")


def private_env_vs_oracle(tg, oracle, seed, serve, steps, clock, key, between=None):
    """One TreasureGame(seed) against its OracleEnv: masked actions, a reset on done and every
    37th step, the mask read before each step; between(t) runs before step t.  Returns the
    trajectory."""
    env = tg.TreasureGame(seed=seed)
    env._vec.set_serve(serve)
    ref = oracle.OracleEnv(seed)
    assert np.array_equal(bits(clock(env.reset)), bits(ref.obs))
    out = []
    for t in range(steps):
        if between is not None:
            between(t)
        assert clock(lambda: env.available_mask).tolist() == mask_bits(ref), (serve, t)
        a = oracle.pick_action(0xA5, seed, t, True, ref.mask())
        st, r, d, _ = clock(env.step, a, key=key)
        rs, rr, rd, _ = ref.step(a)
        assert np.array_equal(bits(st), bits(rs)) and (r, d) == (rr, rd), (serve, t)
        out.append((tuple(bits(st).tolist()), r, d))
        if d or t % 37 == 36:
            assert np.array_equal(bits(clock(env.reset)), bits(ref.reset())), (serve, t)
    assert env._vec.errors() == 0
    env.close()
    return out


@pytest.fixture(scope="module")
def single_us(tg, oracle):
    """us per step() of one env alone in the process's GPU work, served and launch-per-call:
    the figure the patterns below are printed beside"""
    clock = Clock()
    for serve in (True, False):
        private_env_vs_oracle(tg, oracle, 41, serve, 120, clock, serve)
    return {True: clock.us(True), False: clock.us(False)}


def report(what, clock, single_us):
    parts = ["%s %.1f us" % ("served" if k else "launch-per-call", clock.us(k))
             for k in (True, False) if clock.n.get(k)]
    print("\n[serve_many] %s: mean per step() %s (one env alone: served %.1f us, launch-per-call "
          "%.1f us)" % (what, ", ".join(parts), single_us[True], single_us[False]))


# ---- 1. several private-stream envs, round-robin ------------------------------------------------
# (K, visiting order, env closed in the middle, order of the closes at the end)
ROBIN = [(2, "forward", False, "creation"), (5, "forward", False, "reverse"),
         (5, "reversed", False, "creation"), (5, "forward", True, "reverse")]


@pytest.mark.parametrize("serving", ["on", "off", "mixed"])
@pytest.mark.parametrize("k,order,close_mid,close_order", ROBIN)
def test_private_envs_round_robin(tg, oracle, single_us, k, order, close_mid, close_order, serving):
    """K envs with distinct seeds alive at once (K = 5: one more server than the process's 4
    hardware queues), stepped in turn for 120 steps each, every one against its own OracleEnv;
    visited forwards or backwards, one env closed at step 60 while the others go on; served, not
    served, and serving off on every second env.  At the end every handle's errors() is 0; the
    envs are then closed in creation or in reverse order, with serving on after one more served
    mask read, so their servers are resident at close(); tg_live_resources() returns to its value
    at the start."""
    gc.collect()
    base = live(tg)
    clock = Clock()
    seeds = [100 + 17 * i for i in range(k)]
    serve = [serving == "on" or (serving == "mixed" and i % 2 == 0) for i in range(k)]
    envs = [tg.TreasureGame(seed=s) for s in seeds]
    refs = [oracle.OracleEnv(s) for s in seeds]
    for e, sv, r in zip(envs, serve, refs):
        e._vec.set_serve(sv)
        assert np.array_equal(bits(clock(e.reset)), bits(r.obs))
    visit = list(range(k)) if order == "forward" else list(reversed(range(k)))
    alive = [True] * k
    for t in range(120):
        for i in visit:
            if not alive[i]:
                continue
            e, r = envs[i], refs[i]
            assert clock(lambda: e.available_mask).tolist() == mask_bits(r), (i, t)
            a = oracle.pick_action(0xA5 + i, seeds[i], t, True, r.mask())
            st, rew, d, _ = clock(e.step, a, key=serve[i])
            rs, rr, rd, _ = r.step(a)
            assert np.array_equal(bits(st), bits(rs)) and (rew, d) == (rr, rd), (i, t)
            if d or t % 37 == 36:
                assert np.array_equal(bits(clock(e.reset)), bits(r.reset())), (i, t)
            if close_mid and t == 60 and i == 2:
                assert e._vec.errors() == 0
                e.close()
                alive[i] = False
    for i in range(k):
        if alive[i]:
            assert envs[i]._vec.errors() == 0  # (stops the server)
    for i in range(k):
        if alive[i] and serve[i]:  # a server again, resident at close()
            assert clock(lambda: envs[i].available_mask).tolist() == mask_bits(refs[i])
    for i in (range(k) if close_order == "creation" else reversed(range(k))):
        envs[i].close()
    report("%d envs round-robin %s%s" % (k, order, ", one closed midway" if close_mid else ""),
           clock, single_us)
    del envs
    gc.collect()
    assert live(tg) == base


# ---- 2. several shared-stream envs on Python's global random ------------------------------------
_SHARED_REF = {}


def shared_reference(nenvs, seed=53):
    """The script of test 2 and what the reference answers: `nenvs` pyref envs over ONE
    Random(seed), built in order (each constructor draws 4 values), then stepped from a seeded
    schedule: runs of one env, the user's own random() / getrandbits(32) (an odd index) / gauss
    draws, resets, mask reads, and one stretch of 25 steps of env 0 around a 3-ms sleep, after
    which env 1 goes on.  Entries: (op, env, argument, the call's return, getstate() after it).
    Computed once per nenvs and shared by the four (serving, words) runs."""
    if nenvs in _SHARED_REF:
        return _SHARED_REF[nenvs]
    import pyref
    rng = random.Random(seed)
    level = pyref.read_level()
    envs, script = [], []

    def rec(op, i, arg, ret):
        script.append((op, i, arg, ret, rng.getstate()))

    for i in range(nenvs):
        e = pyref.Env.__new__(pyref.Env)
        e.rng = rng
        e.game = pyref.Game(level, rng)
        e.options = [pyref.Option(e.game, j) for j in range(9)]
        envs.append(e)
        rec("new", i, None, None)
    for i in range(nenvs):
        rec("reset", i, None, envs[i].reset())
    u = random.Random(seed + 7)  # the schedule's own generator

    def step(i):
        m = envs[i].available_mask()
        can = [j for j in range(9) if m[j]]
        a = u.choice(can) if can and u.random() < 0.85 else u.randrange(-9, 9)
        st, r, d, _ = envs[i].step(a)
        rec("step", i, a, (list(st), r, d))
        if d:
            rec("reset", i, None, envs[i].reset())

    for block in range(60):
        i = u.randrange(nenvs)
        for _ in range(u.choice((1, 1, 1, 2, 3))):
            step(i)
        x = u.randrange(12)
        if x == 0:
            rec("random", None, None, rng.random())
        elif x == 1:
            rec("bits", None, None, rng.getrandbits(32))
        elif x == 2:
            rec("gauss", None, None, rng.gauss(0, 1))
        elif x == 3:
            rec("reset", i, None, envs[i].reset())
        elif x == 4:
            j = u.randrange(nenvs)
            rec("mask", j, None, list(envs[j].available_mask()))
        if block == 30:  # env 1's server idles out while env 0 steps on; then env 1 continues
            step(1)
            for n in range(25):
                if n == 12:
                    rec("sleep", None, None, None)
                step(0)
            step(1)
            step(1)
    for i in range(nenvs):
        rec("mask", i, None, list(envs[i].available_mask()))
    _SHARED_REF[nenvs] = script
    return script


@pytest.mark.parametrize("words", [True, False])
@pytest.mark.parametrize("serve", [True, False])
@pytest.mark.parametrize("nenvs", [2, 3])
def test_shared_stream_envs_interleaved(tg, nenvs, serve, words):
    """Two and three TreasureGame() on the global random after random.seed(s), interleaved with
    each other and with the user's own draws: every return and random.getstate() after every
    call equal pyref envs sharing one Random(s).  An env's server keeps the stream's ring in LDS
    and its handle the last state it returned; another env's draws must make its next call cold
    (the ring rebuilt from the caller's state), with its server still resident and with a new
    server after the old one idled out (which must not load the ring the old one left on the
    device).  In place on the global Random's words (tg_step1_pywords) and through a tg_pystate
    (tg_step1_py), served and launch-per-call: one reference for all four."""
    script = shared_reference(nenvs)
    gc.collect()
    base = live(tg)
    clock = Clock()
    saved = random.getstate()
    try:
        random.seed(53)
        envs = []
        for n, (op, i, arg, want, state) in enumerate(script):
            e = envs[i] if i is not None and i < len(envs) else None
            if op == "new":
                e = tg.TreasureGame()  # (not timed: the process's first also initialises HIP)
                e._vec.set_serve(serve)
                if words:
                    assert e._pywords is not None
                else:
                    e._pywords = None
                envs.append(e)
            elif op == "reset":
                assert clock(e.reset) == want, n
            elif op == "step":
                st, r, d, _ = clock(e.step, arg)
                assert (st, r, d) == want, (n, i, arg)
            elif op == "mask":
                assert clock(lambda: e.available_mask).tolist() == want, n
            elif op == "random":
                assert random.random() == want, n
            elif op == "bits":
                assert random.getrandbits(32) == want, n
            elif op == "gauss":
                assert random.gauss(0, 1) == want, n
            elif op == "sleep":
                time.sleep(0.003)
            assert random.getstate() == state, (n, op, i)
        for e in envs:
            assert e._vec.errors() == 0
        if serve:  # servers resident at close()
            for i, e in enumerate(envs):
                assert clock(lambda: e.available_mask).tolist() == script[len(script) - nenvs + i][3]
        for e in (envs if words else reversed(envs)):
            e.close()
    finally:
        random.setstate(saved)
    del envs, e
    gc.collect()
    assert live(tg) == base


# ---- 3. other GPU work between served steps -----------------------------------------------------
_VEC_REF = {}
_OTHER_WORK = {}


@pytest.mark.parametrize("serve", [True, False])
@pytest.mark.parametrize("work", ["torch_current_stream", "torch_new_stream", "device_synchronize",
                                  "batched_env"])
def test_other_gpu_work_between_steps(tg, oracle, single_us, work, serve):
    """One TreasureGame(seed) against the oracle for 150 steps with, between the steps: a small
    torch kernel on the current stream and .item(); the same on a torch.cuda.Stream created for
    it; torch.cuda.synchronize() (which waits for a resident server to leave); a 4,096-env
    TreasureGameVec stepped with its on-device masked policy, itself checked against oracle.run
    at the end (the last obs, done and valid rows, every env's return, the tick count).  Served
    and launch-per-call give the same trajectory."""
    clock = Clock()
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.arange(256, dtype=torch.float32, device=dev)
    n, a0, steps = 4096, 0xBEEF, 150
    vec = ret = None
    if work == "batched_env":
        vec = tg.TreasureGameVec(n, seed=7, autoreset=True)
        vec.reset()
        ret = torch.zeros(n, dtype=torch.int64, device=dev)
    side = [None]

    def between(t):
        if work == "torch_current_stream":
            assert (x * t).sum().item() == 32640.0 * t
        elif work == "torch_new_stream":
            if t % 10 == 0:
                side[0] = torch.cuda.Stream(dev)
                side[0].wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side[0]):
                assert (x * t).sum().item() == 32640.0 * t
        elif work == "device_synchronize":
            torch.cuda.synchronize()
        else:
            _, r, _, _, _ = vec.step(vec.policy_actions(t, a0, "masked"))
            ret.add_(r)

    got = private_env_vs_oracle(tg, oracle, 29, serve, steps, clock, serve, between)
    assert _OTHER_WORK.setdefault(work, got) == got
    if vec is not None:
        if "ref" not in _VEC_REF:
            _VEC_REF["ref"] = oracle.run(7, 0, n, steps, a0, 1, True)
        ref = _VEC_REF["ref"]
        assert np.array_equal(vec._obs.cpu().numpy().view(np.uint64), ref["obs"][:, -1].view(np.uint64))
        assert np.array_equal(vec._done.cpu().numpy(), ref["done"][:, -1])
        assert np.array_equal(vec._valid.cpu().numpy(), ref["valid"][:, -1])
        assert np.array_equal(ret.cpu().numpy(), ref["reward"][:, 1:].sum(1, dtype=np.int64))
        assert vec.stats()["ticks"] == int(ref["ticks"].sum())
        assert vec.errors() == 0
        vec.close()
    report("one env, between steps: %s" % work, clock, single_us)


# ---- 4. other calls on the handle between served steps ------------------------------------------
def test_other_calls_on_the_handle_between_served_steps(tg, oracle):
    """Two 1-env handles with one seed and one action stream, one served and one not; every 5th
    step one of the handle's other entry points runs on both: observe, read_state(mt=True),
    errors, stats, render, the batch available_mask, a batch step of one action, rollout(3),
    write_state(read_state).  Each stops the server, which must first write back what it holds in
    LDS (the env's state words, its angles, its episode, the Python stream's ring): after every
    such call and at the end the handles agree on the rows, the whole read_state and the
    counters, and both equal the oracle."""
    seed, a0, ra0 = 19, 0x4C, 0x7777
    on, off = tg.TreasureGame(seed=seed), tg.TreasureGame(seed=seed)
    off._vec.set_serve(False)
    ref = oracle.OracleEnv(seed)
    sprites = tg.synthetic_sprites(seed=7)
    clock = Clock()
    for e in (on, off):
        e._vec.render_init(sprites)
        assert np.array_equal(bits(clock(e.reset)), bits(ref.obs))
    dev = on._vec.device

    def agree(where):
        sa, sb = on._vec.read_state(mt=True), off._vec.read_state(mt=True)
        assert sorted(sa) == sorted(sb)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (where, key)
        ca, cb = on._vec.stats(), off._vec.stats()
        assert [ca[c] for c in COUNTERS] == [cb[c] for c in COUNTERS], where
        for e in (on, off):
            assert np.array_equal(e._vec.observe().cpu().numpy()[0].view(np.uint64), bits(ref.obs)), where

    def reset_all():
        want = ref.reset()
        for e in (on, off):
            assert np.array_equal(bits(clock(e.reset)), bits(want))

    def other(kind, t):
        """entry point `kind` on both handles; True if it left the episode done"""
        done = False
        if kind == "step":
            a = oracle.pick_action(a0 + 1, seed, t, True, ref.mask())
            rs, rr, rd, _ = ref.step(a)
            done = rd
        elif kind == "rollout":
            want = [ref.step(oracle.pick_action(ra0, 0, t + s, False, 0)) for s in range(3)]
            done = want[-1][2]
        for e in (on, off):
            v = e._vec
            if kind == "observe":
                assert np.array_equal(v.observe().cpu().numpy()[0].view(np.uint64), bits(ref.obs))
            elif kind == "read_state":
                assert v.read_state(mt=True)["mt"].shape == (1, 624)
            elif kind == "errors":
                assert v.errors() == 0
            elif kind == "stats":
                assert v.stats()["steps"] > 0
            elif kind == "render":
                assert np.array_equal(v.render().cpu().numpy()[0], ref.render(sprites))
            elif kind == "mask":
                assert int(v.available_mask().cpu()[0]) & 0x1FF == ref.mask()
            elif kind == "step":
                o, r, va, d, _ = v.step(torch.tensor([a], dtype=torch.int32, device=dev))
                assert np.array_equal(o.cpu().numpy()[0].view(np.uint64), bits(rs))
                assert (int(r[0]) if int(va[0]) else None, bool(d[0])) == (rr, rd)
            elif kind == "rollout":
                out = v.rollout(3, t0=t, action_seed=ra0, policy="uniform")
                for s, (rs, rr, rd, _) in enumerate(want):
                    assert np.array_equal(out["obs"][s, 0].cpu().numpy().view(np.uint64), bits(rs)), s
                    assert (int(out["reward"][s, 0]) if int(out["valid"][s, 0]) else None,
                            bool(out["done"][s, 0])) == (rr, rd), s
            elif kind == "write_state":
                v.write_state(v.read_state(mt=True))
        return done

    kinds = ["observe", "read_state", "errors", "stats", "render", "mask", "step", "rollout",
             "write_state"]
    for t in range(135):
        assert clock(lambda: on.available_mask).tolist() == mask_bits(ref), t
        a = oracle.pick_action(a0, seed, t, True, ref.mask())
        rs, rr, rd, _ = ref.step(a)
        for e in (on, off):
            st, r, d, _ = clock(e.step, a)
            assert np.array_equal(bits(st), bits(rs)) and (r, d) == (rr, rd), (t, e is on)
        if rd:
            reset_all()
        if t % 5 == 4:  # (the served handle's server is resident here)
            kind = kinds[(t // 5) % len(kinds)]
            done = other(kind, t)
            agree((t, kind))
            if done:
                reset_all()
    agree("end")
    for e in (on, off):
        assert e._vec.errors() == 0
        e.close()


# ---- 5. out-of-range actions through the C ABI --------------------------------------------------
BAD_ACTIONS = [-10, 9, 23, 25, 40, -41, 2**31 - 1, -2**31]
_CONTINUE_REF = {}


def continue_reference(oracle, fn, seed, state):
    """40 in-range steps of an env that never saw a bad action: its actions, rows and (the
    Python-stream calls) the stream's words and index after each.  Once per entry point."""
    if fn in _CONTINUE_REF:
        return _CONTINUE_REF[fn]
    u = random.Random(99)
    out = []
    if fn == "tg_step1":
        ref = oracle.OracleEnv(seed)
        for t in range(40):
            can = [k for k in range(9) if (ref.mask() >> k) & 1]
            a = u.choice(can) - (9 if t % 4 == 3 else 0)  # (negative indexing too)
            rs, rr, rd, _ = ref.step(a)
            out.append((a, tuple(bits(rs).tolist()), rr, rd, None))
    else:
        import pyref
        e = pyref.Env.__new__(pyref.Env)
        e.rng = random.Random()
        e.rng.setstate(state)
        e.game = pyref.Game(pyref.read_level(), e.rng)  # the constructor's build: 4 draws
        e.options = [pyref.Option(e.game, j) for j in range(9)]
        first = e.rng.getstate()[1]
        for t in range(40):
            m = e.available_mask()
            can = [k for k in range(9) if m[k]]
            a = u.choice(can) - (9 if t % 4 == 3 else 0)
            rs, rr, rd, _ = e.step(a)
            out.append((a, tuple(bits(list(rs)).tolist()), rr, rd, e.rng.getstate()[1]))
        out = [first] + out
    _CONTINUE_REF[fn] = out
    return out


@pytest.mark.parametrize("fn", ["tg_step1", "tg_step1_py", "tg_step1_pywords"])
def test_out_of_range_actions_through_the_c_abi(tg, oracle, fn):
    """An action outside [-9, 8] through tg_step1 / tg_step1_py / tg_step1_pywords on a 1-env
    handle, served and not (the Python surface raises IndexError before the call, so only a C
    caller gets here): valid == 0, the obs row is the env's current one, TG_ERR_ACTION is raised,
    the caller's stream state comes back untouched and no draw is counted; then 40 in-range
    steps equal an env that never saw the bad action, and the served and the launch-per-call
    handle agree on every row, the final read_state, the counters and the error word.  A fresh
    handle per action (the error bit is sticky).  Before the command word's codec was fixed the
    served path failed here: the 5-bit field aliased 25 to -7 and 40 to 8, and the option ran."""
    from gym_treasure_game_amd import _lib
    L = _lib.load()
    seed = 23
    r0 = random.Random(5)
    for _ in range(3):
        r0.random()
    r0.getrandbits(32)  # an odd index
    state = r0.getstate()
    assert state[1][624] % 2 == 1
    want = continue_reference(oracle, fn, seed, state)
    obs = np.zeros(9)
    rew, va, dn, m = ctypes.c_int32(), ctypes.c_uint8(), ctypes.c_uint8(), ctypes.c_uint16()
    outs = (obs.ctypes.data, ctypes.byref(rew), ctypes.byref(va), ctypes.byref(dn), None)
    for bad in BAD_ACTIONS:
        runs = {}
        for serve in (True, False):
            v = tg.TreasureGameVec(1, seed=seed)
            v.set_serve(serve)
            h = v.handle
            ps = _lib.PyState()
            idx = ctypes.c_int32()

            def call(a):
                t0 = time.perf_counter()
                if fn == "tg_step1":
                    rc = L.tg_step1(h, a, *outs)
                elif fn == "tg_step1_py":
                    rc = L.tg_step1_py(h, a, ctypes.byref(ps), *outs)
                else:
                    idx.value = ps.index
                    rc = L.tg_step1_pywords(h, a, ps.mt, ctypes.byref(idx), *outs)
                    ps.index = idx.value
                _lib.check(rc, fn)
                assert time.perf_counter() - t0 < MAX_CALL_S
                return tuple(bits(obs).tolist()), (rew.value if va.value else None), bool(dn.value)

            if fn == "tg_step1":
                _lib.check(L.tg_reset1(h, obs.ctypes.data, None), "tg_reset1")
            else:
                for j in range(624):
                    ps.mt[j] = state[1][j]
                ps.index, ps.has_gauss, ps.gauss_next = state[1][624], 0, 0.0
                _lib.check(L.tg_reset1_py(h, ctypes.byref(ps), obs.ctypes.data, None), "tg_reset1_py")
                assert tuple(ps.mt) + (ps.index,) == want[0]
            now = tuple(v.observe().cpu().numpy()[0].view(np.uint64).tolist())
            assert v.errors() == 0
            draws = v.stats()["draws"]
            # (a served mask read: with serving on the bad action goes to a resident server)
            _lib.check(L.tg_available_mask1(h, ctypes.byref(m), None), "tg_available_mask1")
            before = bytes(ps)
            row = call(bad)
            assert row == (now, None, False), (bad, serve, row)
            assert bytes(ps) == before, (bad, serve)
            assert v.stats()["draws"] == draws, (bad, serve)
            assert v.errors() & _lib.TG_ERR_ACTION, (bad, serve)
            assert tuple(v.observe().cpu().numpy()[0].view(np.uint64).tolist()) == now
            rows = []
            for t, (a, o, r, d, words) in enumerate(want[0 if fn == "tg_step1" else 1:]):
                got = call(a)
                assert got == (o, r, d), (bad, serve, t)
                if words is not None:
                    assert tuple(ps.mt) + (ps.index,) == words, (bad, serve, t)
                rows.append(got)
            st = v.stats()
            runs[serve] = (rows, {k: a.tolist() for k, a in v.read_state(mt=True).items()},
                           [st[c] for c in COUNTERS], v.errors())
            v.close()
        assert runs[True] == runs[False], bad


# ---- 6. the kernel's dynamic-LDS limit across handles -------------------------------------------
def wide_level(tmp_path, cells):
    src = os.path.join(HERE, "golden", "levels", "gen1")
    rows = [r.rstrip("\n") for r in open(os.path.join(src, "domain.txt")) if r.strip()]
    extra = cells - len(rows[0])
    wide = [r[:-1] + ("/" if y % 2 == 0 else " ") * extra + r[-1] for y, r in enumerate(rows)]
    ld = tmp_path / ("gen1_%d" % cells)
    ld.mkdir()
    (ld / "domain.txt").write_text("\n".join(wide) + "\n")
    for f in ("domain-objects.txt", "domain-interactions.txt"):
        (ld / f).write_text(open(os.path.join(src, f)).read())
    return str(ld)


@pytest.mark.parametrize("first", ["wide_first", "narrow_first"])
def test_dynamic_lds_limit_is_the_kernels_not_a_handles(tg, oracle, tmp_path, monkeypatch, capfd, first):
    """Two served envs whose GoTables both exceed 64 KB: gen1 widened to 80 cells (80 x 11 x 32
    x 4 B = 112,640 B) and to 60 (84,480 B).  A server keeps its table in dynamic LDS beside
    k_serve1's static LDS: .group_segment_fixed_size = 17,328 B in the gfx950 code object's
    metadata, so 129,968 B and 101,808 B of the CU's 163,840: both tables are staged, and each
    needs hipFuncAttributeMaxDynamicSharedMemorySize raised for the kernel.  That attribute is
    the kernel's: the 80-cell env steps, the 60-cell env steps (its launch must not lower the
    limit), the first one's server idles out (3 ms), and its relaunch asks for 112,640 B again.
    Both equal their oracle throughout and no call fails; in either creation order.  That the
    wider table really is staged (a table that did not fit would fall back to global memory and
    leave nothing to test) is read from TG_SERVE_TRACE's summary of a third env."""
    clock = Clock()
    dirs = {"A": wide_level(tmp_path, 80), "B": wide_level(tmp_path, 60)}
    names = ["A", "B"] if first == "wide_first" else ["B", "A"]
    envs, refs = {}, {}
    for nm in names:
        envs[nm] = tg.TreasureGame(seed=5, level_dir=dirs[nm])
        refs[nm] = oracle.OracleEnv(5, level_dir=dirs[nm])
    t_of = {"A": 0, "B": 0}

    def steps(nm, count):
        e, r = envs[nm], refs[nm]
        for _ in range(count):
            t = t_of[nm]
            t_of[nm] += 1
            assert clock(lambda: e.available_mask).tolist() == mask_bits(r), (nm, t)
            a = oracle.pick_action(0x99, 5, t, True, r.mask())
            st, rew, d, _ = clock(e.step, a)
            rs, rr, rd, _ = r.step(a)
            assert np.array_equal(bits(st), bits(rs)) and (rew, d) == (rr, rd), (nm, t)
            if d:
                assert np.array_equal(bits(clock(e.reset)), bits(r.reset()))

    for nm in ("A", "B"):
        assert np.array_equal(bits(clock(envs[nm].reset)), bits(refs[nm].obs))
    steps("A", 10)
    steps("B", 10)
    time.sleep(0.003)  # A's server has left
    steps("A", 30)
    steps("B", 30)
    for nm in names:
        assert envs[nm]._vec.errors() == 0
        envs[nm].close()
    capfd.readouterr()
    monkeypatch.setenv("TG_SERVE_TRACE", "1")
    env = tg.TreasureGame(seed=5, level_dir=dirs["A"])
    for t in range(4):
        env.step(t)
    env.close()
    assert "GoTable in LDS: 1, 112640 B" in capfd.readouterr().err
