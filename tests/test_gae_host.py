"""The advantage scan (csrc/tg_gae.h) on the CPU: its host-only build (tests/native_gae) against
an independent float64 numpy scan written here, with a derived running error bound, cases that
are exact in binary, and the header's stand-alone compile.  Also the helpers the GPU tests share
(tests/test_gpu_gae.py imports them).

Bound.  One step of the scan makes three f32 roundings (u = 2^-24): the fma gamma * nv + r, the
subtraction of value[s], and the fma gl * carry + delta.  Each is at most u times the magnitude
of its exact result, and the carried advantage's error enters scaled by gl where it is carried:
    b_s = u * (|gamma * nv + r| + |delta| + |A_s|) + gl * b_{s+1}        (b_K = 0)
ret = A_s + value[s] adds one more rounding: u * |ret|.  gamma and gl enter the float64 scan as
the f32 values widened, so they carry no error of their own.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

U = 2.0 ** -24
TERMINATED, TRUNCATED = 1, 2

_host = None


def hostlib():
    """tests/native_gae's library (built on first use)"""
    global _host
    if _host is None:
        d = os.path.join(ROOT, "tests", "native_gae")
        subprocess.check_call(["make", "-s", "-C", d])
        L = ctypes.CDLL(os.path.join(d, "libtg_hostcheck_gae.so"))
        P, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        L.hg_gae.restype = i32
        L.hg_gae.argtypes = [i32, i64, f32, f32, P, P, P, P, P, i32, P, P]
        _host = L
    return _host


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_gae(reward, done, value, vboot, gamma, lam, vnext=None):
    """the host restatement: (adv, ret, vnext) f32 [K, N].  vnext given: a copy is completed
    (its truncated-alone entries are read as the pre-reset values); None: vnext_given = 0"""
    reward = np.ascontiguousarray(reward, np.int32)
    done = np.ascontiguousarray(done, np.uint8)
    value = np.ascontiguousarray(value, np.float32)
    vboot = np.ascontiguousarray(vboot, np.float32)
    k, n = reward.shape
    assert done.shape == (k, n) and value.shape == (k, n) and vboot.shape == (n,)
    given = vnext is not None
    vn = np.array(vnext, np.float32, copy=True, order="C") if given else np.zeros((k, n), np.float32)
    assert vn.shape == (k, n)
    adv = np.zeros((k, n), np.float32)
    ret = np.zeros((k, n), np.float32)
    assert hostlib().hg_gae(k, n, gamma, lam, _p(reward), _p(done), _p(value), _p(vn), _p(vboot),
                            1 if given else 0, _p(adv), _p(ret)) == 0
    return adv, ret, vn


def f64_gae(reward, done, value, vboot, gamma, lam, vnext=None):
    """the definition in float64, written independently of tg_gae.h: (adv, ret, vnext, bound)"""
    g = float(np.float32(gamma))
    gl = float(np.float32(gamma) * np.float32(lam))  # the one f32 product, widened
    r = np.asarray(reward, np.float64)
    v = np.asarray(value, np.float64)
    k, n = r.shape
    adv, nvs, bound = np.zeros((k, n)), np.zeros((k, n)), np.zeros((k, n))
    a_next, b_next = np.zeros(n), np.zeros(n)
    for s in reversed(range(k)):
        term = (done[s] & TERMINATED) != 0
        trunc = (done[s] & TRUNCATED) != 0
        after = np.asarray(vboot, np.float64) if s == k - 1 else v[s + 1]
        nv = after.copy()
        if vnext is not None:
            nv = np.where(trunc, np.asarray(vnext[s], np.float64), nv)
        nv = np.where(term, 0.0, nv)
        target = g * nv + r[s]
        delta = target - v[s]
        kept = done[s] == 0
        a = gl * np.where(kept, a_next, 0.0) + delta
        b = U * (np.abs(target) + np.abs(delta) + np.abs(a)) + gl * np.where(kept, b_next, 0.0)
        adv[s], nvs[s], bound[s] = a, nv, b
        a_next, b_next = a, b
    return adv, adv + v, nvs, bound


def random_rows(k, n, seed):
    """done bytes from {0, 1, 2, 3}, rewards in [-5, 5], values in [-3, 3]"""
    r = np.random.RandomState(seed)
    return {"reward": r.randint(-5, 6, size=(k, n)).astype(np.int32),
            "done": r.randint(0, 4, size=(k, n)).astype(np.uint8),
            "value": r.uniform(-3, 3, size=(k, n)).astype(np.float32),
            "vboot": r.uniform(-3, 3, size=n).astype(np.float32),
            "vnext": r.uniform(-3, 3, size=(k, n)).astype(np.float32)}


# ---- against the float64 scan -----------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 17])
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_host_scan_within_the_running_bound(k, given, gamma, lam):
    d = random_rows(k, 67, 100 + k)
    vn = d["vnext"] if given else None
    adv, ret, vnext = host_gae(d["reward"], d["done"], d["value"], d["vboot"], gamma, lam, vn)
    wa, wr, wn, b = f64_gae(d["reward"], d["done"], d["value"], d["vboot"], gamma, lam, vn)
    assert set(np.unique(d["done"])) == {0, 1, 2, 3} or k < 17
    assert np.array_equal(vnext.astype(np.float64), wn)  # nv is a copy or 0: exact
    ea = np.abs(adv.astype(np.float64) - wa)
    assert (ea <= b).all(), (ea - b).max()
    er = np.abs(ret.astype(np.float64) - wr)
    assert (er <= b + U * np.abs(wr)).all(), (er - b - U * np.abs(wr)).max()
    assert ea.max() > 0.0 or k == 1  # f32 does round here: the bound is not met vacuously


# ---- exact cases: gamma = lambda = 1/2, small integers, K = 3, one env ------------------------
R3 = np.array([[1], [2], [3]], np.int32)
V3 = np.array([[2], [4], [8]], np.float32)
VB, VT = np.array([16], np.float32), 32.0


def _exact(done, vnext_at=None):
    """(adv, ret, vnext) columns of the host build, checked equal to the float64 scan's"""
    done = np.array(done, np.uint8).reshape(3, 1)
    vn = None
    if vnext_at is not None:
        vn = np.full((3, 1), -99.0, np.float32)  # (an entry that must not be read stands out)
        vn[vnext_at, 0] = VT
    adv, ret, vnext = host_gae(R3, done, V3, VB, 0.5, 0.5, vn)
    wa, wr, wn, _ = f64_gae(R3, done, V3, VB, 0.5, 0.5, vn)
    assert np.array_equal(adv.astype(np.float64), wa)
    assert np.array_equal(ret.astype(np.float64), wr)
    assert np.array_equal(vnext.astype(np.float64), wn)
    return adv[:, 0].tolist(), ret[:, 0].tolist(), vnext[:, 0].tolist()


def test_exact_no_done():
    adv, ret, vnext = _exact([0, 0, 0])
    # s=2: 8 + 3 - 8 = 3;  s=1: 4 + 2 - 4 + 3/4 = 2.75;  s=0: 2 + 1 - 2 + 2.75/4 = 1.6875
    assert adv == [1.6875, 2.75, 3.0]
    assert ret == [3.6875, 6.75, 11.0]
    assert vnext == [4.0, 8.0, 16.0]


def test_exact_terminated_mid():
    adv, ret, vnext = _exact([0, TERMINATED, 0])
    # s=1: nv = 0, delta = 2 - 4 = -2, carry cut;  s=0: 1 + (-2)/4 = 0.5
    assert adv == [0.5, -2.0, 3.0]
    assert vnext == [4.0, 0.0, 16.0]


def test_exact_truncated_mid_with_vnext():
    adv, ret, vnext = _exact([0, TRUNCATED, 0], vnext_at=1)
    # s=1: nv = 32, delta = 16 + 2 - 4 = 14, carry cut;  s=0: 1 + 14/4 = 4.5
    assert adv == [4.5, 14.0, 3.0]
    assert vnext == [4.0, 32.0, 16.0]


def test_exact_truncated_mid_without_vnext():
    adv, ret, vnext = _exact([0, TRUNCATED, 0])
    # s=1: nv = value[2] = 8, delta = 2, carry cut;  s=0: 1 + 2/4 = 1.5
    assert adv == [1.5, 2.0, 3.0]
    assert vnext == [4.0, 8.0, 16.0]


def test_exact_terminated_last_ignores_vboot():
    adv, ret, vnext = _exact([0, 0, TERMINATED])
    # s=2: nv = 0, delta = 3 - 8 = -5;  s=1: 2 - 5/4 = 0.75;  s=0: 1 + 0.75/4 = 1.1875
    assert adv == [1.1875, 0.75, -5.0]
    assert vnext == [4.0, 8.0, 0.0]


def test_exact_truncated_last_uses_vnext_not_vboot():
    adv, ret, vnext = _exact([0, 0, TRUNCATED], vnext_at=2)
    # s=2: nv = 32, delta = 16 + 3 - 8 = 11;  s=1: 2 + 11/4 = 4.75;  s=0: 1 + 4.75/4 = 2.1875
    assert adv == [2.1875, 4.75, 11.0]
    assert vnext == [4.0, 8.0, 32.0]


def test_exact_both_bits_terminated_wins():
    adv, ret, vnext = _exact([0, TERMINATED | TRUNCATED, 0], vnext_at=1)
    assert adv == [0.5, -2.0, 3.0]
    assert vnext == [4.0, 0.0, 16.0]


def test_sum_case():
    """gamma = lambda = 1, no done: ret[0] == sum of rewards + vboot exactly (small integers)"""
    r = np.random.RandomState(3)
    k, n = 17, 67
    reward = r.randint(-5, 6, size=(k, n)).astype(np.int32)
    value = r.randint(-3, 4, size=(k, n)).astype(np.float32)
    vboot = r.randint(-3, 4, size=n).astype(np.float32)
    adv, ret, vnext = host_gae(reward, np.zeros((k, n), np.uint8), value, vboot, 1.0, 1.0)
    assert np.array_equal(ret[0], (reward.sum(0) + vboot).astype(np.float32))
    assert np.array_equal(vnext[:-1], value[1:]) and np.array_equal(vnext[-1], vboot)


def test_rejects_what_tg_gae_rejects():
    d = random_rows(2, 5, 1)
    a = np.zeros((2, 5), np.float32)
    L = hostlib()
    for gamma, lam in ((-0.1, 0.5), (1.5, 0.5), (0.5, float("nan")), (float("inf"), 0.5)):
        assert L.hg_gae(2, 5, gamma, lam, _p(d["reward"]), _p(d["done"]), _p(d["value"]), None,
                        _p(d["vboot"]), 0, _p(a), _p(a)) == -1
    assert L.hg_gae(2, 5, 0.5, 0.5, _p(d["reward"]), _p(d["done"]), _p(d["value"]), None,
                    _p(d["vboot"]), 1, _p(a), _p(a)) == -1


# ---- the header ---------------------------------------------------------------------------------
def test_header_compiles_alone_on_the_host(tmp_path):
    from test_headers_host import CSRC, HOST
    unit = tmp_path / "tg_gae_unit.hip"
    unit.write_text('#include "%s"\n' % os.path.join(CSRC, "tg_gae.h"))
    p = subprocess.run(HOST + [str(unit)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
