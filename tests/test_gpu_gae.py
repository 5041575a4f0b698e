"""Advantages on the device (tg_gae, tg_rollout_mlp_gae): k_gae against the host
build of csrc/tg_gae.h bit for bit, the rollout's adv / ret / vnext against the host build fed
the rollout's own rows, the truncated envs' values and vboot against a twin handle that
evaluates them with policy_mlp on the pre-reset states, the rollout's other outputs and final
state undisturbed, env groups, no auto-reset, and the rejected arguments.

Set-up (tests/test_gpu_time_limit.py's): level exit, 200 envs (three waves plus 8 lanes), seed
5, limit 7, auto-reset, where the actor seeded_params(32, 332) both terminates and truncates
within 60 steps."""
import ctypes

import numpy as np
import pytest
import torch

from test_gae_host import TERMINATED, TRUNCATED, host_gae, random_rows
from test_gpu_time_limit import A0, EXIT, N, SEED, STEPS, ROW_KEYS, bits, check_twins, same
from test_policy_mlp_host import host_forward, seeded_params

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95
GAE_KEYS = ("adv", "ret", "vnext", "vboot")
MLP_KEYS = ROW_KEYS + ("logp", "value")


def make(tg, limit=7, autoreset=True, hidden=32, act="relu", n=N, seed=SEED, level=EXIT, **kw):
    v = tg.TreasureGameVec(n, seed=seed, autoreset=autoreset, level_dir=level,
                           max_episode_steps=limit, **kw)
    v.reset()
    v.set_policy_mlp(tg.pack_mlp_params(seeded_params(hidden, 300 + hidden)), act=act, masked=True)
    return v


def cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def host_of(o, given):
    """the host build on a rollout's own rows; given: its truncated-alone vnext entries"""
    vn = None
    if given:
        vn = np.where(o["done"] == TRUNCATED, o["vnext"], np.float32(0)).astype(np.float32)
    return host_gae(o["reward"], o["done"], o["value"], o["vboot"], GAMMA, LAM, vn)


def check_host(o, given):
    adv, ret, vnext = host_of(o, given)
    for key, want in (("adv", adv), ("ret", ret), ("vnext", vnext)):
        assert np.array_equal(bits(o[key]), bits(want)), key


# ---- 1. k_gae alone ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain333(tg):
    v = tg.TreasureGameVec(333, seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("given", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 8, 17])  # the unrolled loop alone, its tail alone, both
def test_k_gae_equals_the_host_build(plain333, k, given):
    v = plain333
    d = random_rows(k, 333, 7 * k + given)
    assert k < 8 or set(np.unique(d["done"])) == {0, 1, 2, 3}
    t = {key: torch.from_numpy(x).to(v.device) for key, x in d.items()}
    out = cpu(v.gae(t["reward"], t["done"], t["value"], t["vboot"], GAMMA, LAM,
                    vnext=t["vnext"] if given else None))
    adv, ret, vnext = host_gae(d["reward"], d["done"], d["value"], d["vboot"], GAMMA, LAM,
                               d["vnext"] if given else None)
    for key, want in (("adv", adv), ("ret", ret), ("vnext", vnext)):
        assert np.array_equal(bits(out[key]), bits(want)), key
    if given:
        assert same(t["vnext"], vnext)  # completed in place


def test_gae_of_no_steps(plain333):
    v = plain333
    e = lambda dt: torch.empty((0, 333), dtype=dt, device=v.device)
    out = v.gae(e(torch.int32), e(torch.uint8), e(torch.float32),
                torch.zeros(333, device=v.device), GAMMA, LAM)
    assert out["adv"].shape == (0, 333)


# ---- 2. the rollout, in chunks ---------------------------------------------------------------------
def test_rollout_chunks_equal_the_host_build(tg):
    a = make(tg)
    t0, dones = 0, []
    for c in (7, 1, 52):
        o = cpu(a.rollout(c, t0=t0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM)))
        t0 += c
        check_host(o, given=True)
        after = np.concatenate([o["value"][1:], o["vboot"][None]])
        live = o["done"] == 0
        assert np.array_equal(bits(o["vnext"][live]), bits(after[live]))
        assert (o["vnext"][(o["done"] & TERMINATED) != 0] == 0).all()
        dones.append(o["done"])
    assert set(np.unique(np.concatenate(dones))) == {0, 1, 2}
    assert a.errors() == 0
    a.close()


# ---- 3. the truncated values and vboot, independently -----------------------------------------------
@pytest.mark.parametrize("hidden,act,steps,limit", [(32, "relu", STEPS, 7), (128, "relu", 8, 7),
                                                     (16, "tanh", STEPS, 7), (32, "relu", 9, 1)])
def test_truncated_values_and_vboot_against_a_twin(tg, hidden, act, steps, limit):
    """The twin has no limit: per step policy_mlp + step, then policy_mlp's value row of the
    states the step left, then reset(mask = the envs the first handle truncated), which the
    header guarantees equals the device limit bit for bit.  ReLU: equal bits.  tanh: within
    8 D of each other, D being the outputs' sensitivity to activations that differ in the last
    place (tests/test_gpu_policy_mlp.py), over the rows compared.
    The saved states' list holds 4 x limit steps: 60 steps at limit 7 run the value kernel over
    it after steps 28, 56 and 60; at limit 1 every env is listed in every step and the list is
    full after 4."""
    a = make(tg, limit=limit, hidden=hidden, act=act)
    b = make(tg, limit=None, hidden=hidden, act=act)
    o = cpu(a.rollout(steps, t0=0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM)))
    assert set(np.unique(o["done"])) >= ({0, 1, 2} if steps == STEPS else {2} if limit == 1 else {0, 2})
    got, want, rows = [], [], []
    for t in range(steps):
        act_t = b.policy_mlp(t, A0)[0].clone()
        assert np.array_equal(act_t.cpu().numpy(), o["actions"][t]), t
        b.step(act_t)
        tr = o["done"][t] == TRUNCATED
        got.append(o["vnext"][t][tr])
        want.append(b.policy_mlp(t, A0)[2].cpu().numpy()[tr])
        rows.append(b.observe().cpu().numpy()[tr])
        b.reset(torch.from_numpy(tr.astype(np.uint8)).to(b.device))
    got.append(o["vboot"])
    want.append(b.policy_mlp(steps, A0)[2].cpu().numpy())
    rows.append(b.observe().cpu().numpy())
    got, want, rows = np.concatenate(got), np.concatenate(want), np.concatenate(rows)
    assert len(got) > N
    if act == "relu":
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got), bits(host_forward(a_packed(tg, hidden), hidden, 0, rows)[1]))
    else:
        packed = a_packed(tg, hidden)
        D = float(np.abs(host_forward(packed, hidden, 1, rows)[1] -
                         host_forward(packed, hidden, 2, rows)[1]).max())
        dev = float(np.abs(got - want).max())
        print("tanh H=%d: D = %.3e, value kernel vs actor kernel = %.3e" % (hidden, D, dev))
        assert D > 0 and dev <= 8 * D
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        if key != "ep":  # (the twin counts no lengths to reset)
            assert np.array_equal(sa[key], sb[key]), key
    a.close()
    b.close()


def a_packed(tg, hidden):
    return tg.pack_mlp_params(seeded_params(hidden, 300 + hidden))


# ---- 4. undisturbed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["compact", "direct"])
def test_rollout_is_undisturbed(tg, mode):
    a, b = make(tg, mode=mode), make(tg, mode=mode)
    oa = a.rollout(STEPS, t0=0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM))
    ob = b.rollout(STEPS, t0=0, action_seed=A0, policy="mlp")
    assert set(ob) == set(MLP_KEYS) and set(oa) == set(MLP_KEYS + GAE_KEYS)
    assert set(np.unique(oa["done"].cpu().numpy())) == {0, 1, 2}
    check_twins(a, b, oa, ob, MLP_KEYS)
    check_host(cpu(oa), given=True)
    a.close()
    b.close()


# ---- 5. groups ------------------------------------------------------------------------------------------
def test_groups_equal_the_ungrouped_handle(tg):
    n, k = 12288, 20
    a, b = make(tg, limit=5, n=n, seed=11), make(tg, limit=5, n=n, seed=11)
    a.set_groups(3, stagger=True)
    oa = a.rollout(k, t0=0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM))
    ob = b.rollout(k, t0=0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM))
    for key in MLP_KEYS + GAE_KEYS:
        assert same(oa[key], ob[key]), key
    o = cpu(oa)
    assert set(np.unique(o["done"])) == {0, 1, 2}
    check_host(o, given=True)
    sa, sb = a.read_state(mt=True), b.read_state(mt=True)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.errors() == 0 and b.errors() == 0
    a.close()
    b.close()


# ---- 6. without auto-reset ------------------------------------------------------------------------------
def test_without_autoreset_the_next_state_is_used(tg):
    a = make(tg, autoreset=False)
    o = cpu(a.rollout(20, t0=0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM)))
    tr = o["done"] == TRUNCATED
    assert tr.any()
    after = np.concatenate([o["value"][1:], o["vboot"][None]])
    assert tr[-1].any() and np.array_equal(bits(o["vnext"][tr]), bits(after[tr]))
    check_host(o, given=False)
    a.close()


# ---- 7. rejected arguments ---------------------------------------------------------------------------------
def _raw(v, k, bufs, gamma=GAMMA, lam=LAM, null=()):
    p = lambda key: None if key in null else ctypes.c_void_p(bufs[key].data_ptr())
    return v._L.tg_rollout_mlp_gae(v.handle, k, A0, 0, 0, 1 if v.autoreset else 0, p("actions"),
                                   p("obs"), p("reward"), p("valid"), p("done"), p("logp"),
                                   p("value"), gamma, lam, p("adv"), p("ret"), p("vnext"),
                                   p("vboot"), None)


def _bufs(v, k):
    n, dev = v.num_envs, v.device
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    return {"actions": torch.zeros((k, n), dtype=torch.int32, device=dev),
            "obs": torch.zeros((k, n, 9), dtype=torch.float64, device=dev),
            "reward": torch.zeros((k, n), dtype=torch.int32, device=dev),
            "valid": torch.zeros((k, n), dtype=torch.uint8, device=dev),
            "done": torch.zeros((k, n), dtype=torch.uint8, device=dev),
            "logp": f(k, n), "value": f(k, n), "adv": f(k, n), "ret": f(k, n), "vnext": f(k, n),
            "vboot": f(n)}


def test_rejected_arguments_change_nothing(tg):
    base = tg._lib.load().tg_live_resources()
    a, b = make(tg), make(tg)
    k = 3
    bufs = _bufs(a, k)
    t0 = 0

    def still_twins():
        nonlocal t0
        oa = a.rollout(k, t0=t0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM))
        ob = b.rollout(k, t0=t0, action_seed=A0, policy="mlp", gae=(GAMMA, LAM))
        t0 += k
        for key in MLP_KEYS + GAE_KEYS:
            assert same(oa[key], ob[key]), key
        sa, sb = a.read_state(mt=True), b.read_state(mt=True)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), key

    bad = [dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(lam=float("inf")),
           dict(lam=-1.0), dict(null=("adv",)), dict(null=("ret",)), dict(null=("value",)),
           dict(null=("vnext",))]
    live = tg._lib.load().tg_live_resources
    for kw in bad:
        held = live()  # (the first is rejected before the handle has allocated its lists)
        assert _raw(a, k, bufs, **kw) == tg._lib.TG_E_INVAL, kw
        assert live() == held, kw
        still_twins()
    a.set_mode("flow")
    held = live()
    assert _raw(a, k, bufs) == tg._lib.TG_E_INVAL
    assert live() == held
    a.set_mode("compact")
    still_twins()
    assert _raw(a, 0, bufs) == 0  # no steps
    still_twins()
    # tg_gae's own
    g = lambda gamma, lam, null=(), given=0: a._L.tg_gae(
        a.handle, k, gamma, lam, *[None if key in null else ctypes.c_void_p(bufs[key].data_ptr())
                                   for key in ("reward", "done", "value", "vnext", "vboot")],
        given, *[None if key in null else ctypes.c_void_p(bufs[key].data_ptr())
                 for key in ("adv", "ret")], None)
    assert g(GAMMA, LAM) == 0 and g(GAMMA, LAM, null=("vnext",)) == 0
    for rc in (g(1.01, LAM), g(GAMMA, float("nan")), g(GAMMA, LAM, null=("adv",)),
               g(GAMMA, LAM, null=("ret",)), g(GAMMA, LAM, null=("value",)),
               g(GAMMA, LAM, null=("vnext",), given=1)):
        assert rc == tg._lib.TG_E_INVAL
    with pytest.raises(tg.TgError):
        a.rollout(k, t0=t0, action_seed=A0, policy="masked", gae=(GAMMA, LAM))
    still_twins()
    assert a.errors() == 0 and b.errors() == 0
    a.close()
    b.close()
    # no limit: vnext may be NULL (not stored), and vboot too (the handle's scratch)
    c = make(tg, limit=None)
    bufs = _bufs(c, k)
    assert _raw(c, k, bufs, null=("vnext", "vboot")) == 0
    o = cpu(bufs)
    o["vboot"] = c.policy_mlp(k, A0)[2].cpu().numpy()
    check_host({**o, "vnext": host_of(o, given=False)[2]}, given=False)
    c.close()
    assert tg._lib.load().tg_live_resources() == base
