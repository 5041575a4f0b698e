"""The learned actor on the device (k_policy_mlp; tg_policy_mlp, tg_rollout_mlp) against the host
restatement of csrc/tg_policy_mlp.h (tests/native_policy) run on observe()'s rows and
available_mask()'s bits: logits and value bit for bit for ReLU nets, within a measured
tolerance for tanh nets, the action rules of tests/test_policy_mlp_host.py, the rollout against
the per-step loop and the oracle, sharding, env groups, weights refreshed on the stream, errors
and determinism.  N = 333 leaves a partial wave and a partial workgroup; the states are varied
by 12 masked synthetic steps with auto-reset."""
import ctypes

import numpy as np
import pytest
import torch

from test_policy_mlp_host import (A0, DELTA, INSIDE_CAP, allowed_bits, check_sampled, greedy64,
                                  host_forward, host_select, host_uniform, seeded_params)

pytestmark = pytest.mark.gpu

N, SEED, PRE = 333, 21, 12
STEP_SEED = 0xA5A5
TS = (12, 13, 14, 15)


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(t).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[t.dtype.itemsize])


def make_vec(tg, n=N, global_offset=0, pre=PRE, **kw):
    v = tg.TreasureGameVec(n, seed=SEED, global_offset=global_offset, autoreset=True, **kw)
    v.reset()
    for t in range(pre):
        v.step(v.policy_actions(t, STEP_SEED, "masked"))
    return v


@pytest.fixture(scope="module")
def vec(tg):
    v = make_vec(tg)
    yield v
    v.close()


@pytest.fixture(scope="module")
def state(vec):
    """the rows the actor reads: observe()'s f64 [N, 9] and available_mask()'s bits (unchanged
    by the tests: policy_mlp only reads the state)"""
    return vec.observe().cpu().numpy().copy(), vec.available_mask().cpu().numpy().copy()


_packed = {}


def packed_of(tg, h):
    if h not in _packed:
        _packed[h] = tg.pack_mlp_params(seeded_params(h, 300 + h))
    return _packed[h]


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("h", [16, 64, 128])
def test_relu_bit_exact(tg, vec, state, h, masked):
    obs, avail = state
    packed = packed_of(tg, h)
    vec.set_policy_mlp(packed, act="relu", masked=bool(masked))
    want_lg, want_v = host_forward(packed, h, 0, obs)
    A = allowed_bits(masked, avail)
    a, lp, v, lg = [x.cpu().numpy().copy() for x in vec.policy_mlp(TS[0], A0, greedy=True, logits=True)]
    assert np.array_equal(bits(lg), bits(want_lg)), "logits differ from the host restatement"
    assert np.array_equal(bits(v), bits(want_v)), "value differs from the host restatement"
    h_a, h_lp = host_select(want_lg, avail, masked, 1, A0, 0, TS[0])
    assert np.array_equal(a, h_a), "greedy actions differ"
    assert np.all((A >> a) & 1 == 1)
    assert np.all(np.abs(lp - h_lp) <= 2.0 ** -20 * np.maximum(1, np.abs(lp)))
    inside = same = 0
    for t in TS:
        a, lp, v2, lg2 = [x.cpu().numpy().copy() for x in vec.policy_mlp(t, A0, logits=True)]
        assert np.array_equal(bits(lg2), bits(want_lg)) and np.array_equal(bits(v2), bits(want_v))
        assert np.all((A >> a) & 1 == 1), "an action outside the mask"
        u = host_uniform(A0, 0, t, N)
        inside += check_sampled(a, want_lg.astype(np.float64), A, u, what="H=%d t=%d" % (h, t))
        h_a, h_lp = host_select(want_lg, avail, masked, 0, A0, 0, t)
        eq = a == h_a
        same += int(eq.sum())
        assert np.all(np.abs(lp - h_lp)[eq] <= (2.0 ** -20 * np.maximum(1, np.abs(lp)))[eq])
    assert inside <= INSIDE_CAP * N * len(TS), inside
    assert same >= (1 - INSIDE_CAP) * N * len(TS), same


@pytest.mark.parametrize("h", [16, 64])
def test_tanh_within_measured_tolerance(tg, vec, state, h):
    """D = the largest difference in any logit or value between the host restatement with tanhf
    and with (float)tanh((double)z): the outputs' sensitivity to activations that differ in the
    last place.  The device lies within 8 * D of the tanhf restatement; greedy actions by the
    gap rule at 2 * 8 * D, sampled ones by the delta rule widened by 8 * D (a logit change of e
    moves a normalised CDF boundary by at most e / 2).
    Measured on an MI355X: see DESIGN.md §11."""
    obs, avail = state
    packed = packed_of(tg, h)
    lg_f, v_f = host_forward(packed, h, 1, obs)
    lg_d, v_d = host_forward(packed, h, 2, obs)
    D = float(max(np.abs(lg_f - lg_d).max(), np.abs(v_f - v_d).max()))
    assert D > 0
    vec.set_policy_mlp(packed, act="tanh", masked=True)
    A = allowed_bits(1, avail)
    a, lp, v, lg = [x.cpu().numpy().copy() for x in vec.policy_mlp(TS[0], A0, greedy=True, logits=True)]
    dev = float(max(np.abs(lg - lg_f).max(), np.abs(v - v_f).max()))
    print("tanh H=%d: D = %.3e, device deviation = %.3e (%.2f D)" % (h, D, dev, dev / D))
    assert dev <= 8 * D
    want, gap = greedy64(lg_f.astype(np.float64), A)
    decided = gap > 2 * 8 * D
    assert decided.any() and np.array_equal(a[decided], want[decided])
    assert np.all((A >> a) & 1 == 1)
    inside = 0
    for t in TS:
        a = vec.policy_mlp(t, A0)[0].cpu().numpy()
        assert np.all((A >> a) & 1 == 1)
        inside += check_sampled(a, lg_f.astype(np.float64), A, host_uniform(A0, 0, t, N),
                                near=DELTA + 8 * D, what="tanh H=%d t=%d" % (h, t))
    assert inside <= INSIDE_CAP * N * len(TS), inside


@pytest.mark.parametrize("policy", ["mlp", "mlp_greedy"])
def test_rollout_equals_the_loop_and_the_oracle(tg, oracle, policy):
    k, h = 6, 32
    packed = packed_of(tg, h)
    greedy = policy == "mlp_greedy"
    a = tg.TreasureGameVec(N, seed=SEED, autoreset=True)
    a.reset()
    a.set_policy_mlp(packed)  # tanh, masked
    out = {key: val.cpu().numpy() for key, val in a.rollout(k, t0=0, action_seed=A0, policy=policy).items()}
    assert set(out) == {"reward", "valid", "done", "obs", "actions", "logp", "value"}
    b = tg.TreasureGameVec(N, seed=SEED, autoreset=True)
    b.reset()
    b.set_policy_mlp(packed)
    for s in range(k):
        act, lp, v = b.policy_mlp(s, A0, greedy=greedy)
        row = {"actions": act.cpu().numpy().copy(), "logp": lp.cpu().numpy().copy(),
               "value": v.cpu().numpy().copy()}
        o, r, va, d, _ = b.step(act)
        row.update(obs=o.cpu().numpy(), reward=r.cpu().numpy(), valid=va.cpu().numpy(),
                   done=d.cpu().numpy())
        for key, val in row.items():
            assert np.array_equal(bits(out[key][s]), bits(val)), (key, s)
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.errors() == 0 and b.errors() == 0
    a.close()
    b.close()
    for g in range(32):
        e = oracle.OracleEnv(SEED + g)
        for s in range(k):
            o, r, d, _ = e.step(int(out["actions"][s, g]))
            if d:
                o = e.reset()
            assert np.array_equal(o.view(np.uint64), out["obs"][s, g].view(np.uint64)), (g, s)
            assert r == (int(out["reward"][s, g]) if out["valid"][s, g] else None), (g, s)
            assert d == bool(out["done"][s, g]), (g, s)


def test_sharding(tg, vec):
    """envs 100..149 as a handle of their own (global_offset=100) after the same history"""
    packed = packed_of(tg, 32)
    sh = make_vec(tg, 50, global_offset=100)
    for v in (vec, sh):
        v.set_policy_mlp(packed, act="tanh", masked=True)
    for greedy in (False, True):
        full = [x.cpu().numpy().copy() for x in vec.policy_mlp(TS[1], A0, greedy=greedy, logits=True)]
        part = [x.cpu().numpy().copy() for x in sh.policy_mlp(TS[1], A0, greedy=greedy, logits=True)]
        for f, p, name in zip(full, part, ("actions", "logp", "value", "logits")):
            assert np.array_equal(bits(f[100:150]), bits(p)), name
    sh.close()


def test_env_groups(tg):
    n, k, h = 8200, 3, 16
    packed = packed_of(tg, h)
    outs = []
    for groups in (1, 2):
        v = make_vec(tg, n, pre=3)
        v.set_policy_mlp(packed, act="relu", masked=True)
        if groups > 1:
            v.set_groups(groups)
        o = v.rollout(k, t0=3, action_seed=A0, policy="mlp")
        o2 = v.rollout(2, t0=3 + k, action_seed=A0, policy="mlp", actions=False, obs=False)
        torch.cuda.synchronize()
        outs.append(({key: val.cpu().numpy() for key, val in o.items()},
                     {key: val.cpu().numpy() for key, val in o2.items()}, v.read_state(mt=True)))
        assert v.errors() == 0
        v.close()
    (a, a2, sa), (b, b2, sb) = outs
    assert set(a2) == {"reward", "valid", "done", "logp", "value"}
    for x, y in ((a, b), (a2, b2)):
        for key in x:
            assert np.array_equal(bits(x[key]), bits(y[key])), key
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key


def test_weights_refreshed_on_the_stream(tg, vec, state):
    """load A, evaluate, load B, evaluate with no host synchronisation in between: each result
    matches its own parameter set"""
    obs, _ = state
    h = 64
    pa, pb = packed_of(tg, h), tg.pack_mlp_params(seeded_params(h, 999))
    da, db = (torch.from_numpy(p).to(vec.device) for p in (pa, pb))
    oa = {"logits": torch.empty((N, 9), dtype=torch.float32, device=vec.device),
          "value": torch.empty(N, dtype=torch.float32, device=vec.device)}
    ob = {key: torch.empty_like(val) for key, val in oa.items()}
    torch.cuda.synchronize()
    vec.set_policy_mlp(da, act="relu", masked=False)
    vec.policy_mlp(TS[0], A0, logits=True, out=oa)
    vec.set_policy_mlp(db, act="relu", masked=False)
    vec.policy_mlp(TS[0], A0, logits=True, out=ob)
    torch.cuda.synchronize()
    for p, o in ((pa, oa), (pb, ob)):
        lg, v = host_forward(p, h, 0, obs)
        assert np.array_equal(bits(o["logits"]), bits(lg)) and np.array_equal(bits(o["value"]), bits(v))
    assert not np.array_equal(bits(oa["logits"]), bits(ob["logits"]))


def test_params_from_a_modules_tensors(tg, vec, state):
    """a dict of device tensors (a torch module's, [1, H] value head) is packed on the device and
    gives the logits of the same dict packed on the host"""
    obs, _ = state
    h = 32
    p = seeded_params(h, 77)
    d = {k: torch.from_numpy(v).to(vec.device).requires_grad_(True) for k, v in p.items()}
    d["wv"] = d["wv"].reshape(1, h)
    vec.set_policy_mlp(d, act="relu", masked=True)
    lg = vec.policy_mlp(TS[0], A0, logits=True)[3]
    want, _ = host_forward(tg.pack_mlp_params(p), h, 0, obs)
    assert np.array_equal(bits(lg), bits(want))
    d["w1"] = d["w1"].reshape(9, h)
    with pytest.raises(ValueError):
        vec.set_policy_mlp(d)


def test_errors(tg):
    v = tg.TreasureGameVec(64, seed=1)
    v.reset()
    with pytest.raises(tg.TgError, match=r"\(-5\)"):  # TG_E_STATE
        v.policy_mlp(0)
    with pytest.raises(tg.TgError, match=r"\(-5\)"):
        v.rollout(2, policy="mlp")
    lib = tg._lib.load()
    dev = torch.from_numpy(packed_of(tg, 16)).to(v.device)
    ptr = ctypes.c_void_p(dev.data_ptr())
    assert lib.tg_policy_mlp_load(v.handle, 48, 0, 1, ptr, None) == -1  # TG_E_INVAL
    assert lib.tg_policy_mlp_load(v.handle, 16, 2, 1, ptr, None) == -1
    assert lib.tg_policy_mlp_load(v.handle, 16, 0, 1, None, None) == -1
    with pytest.raises(tg.TgError, match=r"\(-5\)"):  # the failed loads left no network
        v.policy_mlp(0)
    with pytest.raises(ValueError):
        v.set_policy_mlp(np.zeros(100, np.float32))
    with pytest.raises(ValueError):
        v.set_policy_mlp(packed_of(tg, 16).astype(np.float64))
    with pytest.raises(KeyError):
        v.set_policy_mlp(packed_of(tg, 16), act="gelu")
    v.set_policy_mlp(packed_of(tg, 16), act="relu")
    assert lib.tg_policy_mlp(v.handle, A0, 0, 2, ptr, None, None, None, None) == -1  # bad mode
    assert lib.tg_policy_mlp(v.handle, A0, 0, 0, None, None, None, None, None) == -1  # no actions
    for key, shape, dt in (("actions", (63,), torch.int32), ("logp", (64, 1), torch.float32),
                           ("value", (64,), torch.float64), ("logits", (64, 8), torch.float32)):
        with pytest.raises(ValueError):
            v.policy_mlp(0, logits=True, out={key: torch.empty(shape, dtype=dt, device=v.device)})
    with pytest.raises(ValueError):
        v.policy_mlp(0, out={"actions": torch.empty(64, dtype=torch.int32)})  # a host tensor
    v.set_mode("flow")
    with pytest.raises(tg.TgError):
        v.rollout(2, policy="mlp")
    one = torch.empty(2 * 64, dtype=torch.int32, device=v.device)
    u8 = torch.empty(2 * 64, dtype=torch.uint8, device=v.device)
    rc = lib.tg_rollout_mlp(v.handle, 2, A0, 0, 0, 0, None, None, ctypes.c_void_p(one.data_ptr()),
                            ctypes.c_void_p(u8.data_ptr()), ctypes.c_void_p(u8.data_ptr()), None,
                            None, None)
    assert rc == -1 and b"TG_MODE_FLOW" in lib.tg_last_error()
    v.set_mode("direct")
    out = v.rollout(2, policy="mlp_greedy")
    assert out["logp"].shape == (2, 64) and v.errors() == 0
    v.close()


def test_determinism(tg, vec):
    vec.set_policy_mlp(packed_of(tg, 128), act="tanh", masked=True)
    runs = []
    for _ in range(2):
        runs.append([x.cpu().numpy().copy() for x in vec.policy_mlp(TS[2], A0, logits=True)])
    for x, y in zip(*runs):
        assert np.array_equal(bits(x), bits(y))
