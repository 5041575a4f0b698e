"""GPU: both renderers on every synthesized state of tests/render_sweep.py, against the C
oracle, byte for byte.  Per level one handle and parts of 256 cases (the last part overlaps the
one before it, so every part has the handle's size); per part: write_state(states), then

  render()                      (k_render)         against oracle.render_states,
  render(scale=s, gray=g)       (k_render_scaled)  against the pooled oracle frames, for every
                                                   divisor of 48 and both channel counts,
  tg_render_scaled at scale 1 through the C ABI, both channel counts (render() takes
  tg_render's path for scale 1 rgb),

and errors() == 0 (TG_ERR_RENDER: a handle end point within 1e-9 of an integer; the handle
tier's crossing angles stay 1e-7 px away).  The oracle's frames are computed once per part,
moved to the device and pooled there (test_render_sweep_host.pool_fast, held to the numpy
definition on the CPU and below).  The narrow level (8 cells wide) fills k_render_scaled's LDS
queue past SQCAP at scales 1 and 2, so its part runs the inline-compose branch; the host check
counts the declined boxes with the kernel's span arithmetic.  The state set is held to its
conditions on the CPU by test_render_sweep_host.py, which also runs the host composition."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import render_sweep as rs
from test_render_scaled_host import SCALES, hostscaled, pool  # noqa: F401 (hostscaled: a fixture)
from test_render_sweep_host import COUNTS, pool_fast, span_queue_max, sprites_of

pytestmark = pytest.mark.gpu

PART = 256
# the case counts are test_render_sweep_host.COUNTS': the part lists are built from them at
# collection, without the builder (which needs the oracle built);
# test_part_lists_cover_the_sweeps holds them to it
TOTALS = {name: sum(c) for name, c in COUNTS.items()}


def part_bounds(n, size, part):
    lo = min(part * size, max(n - size, 0))
    return lo, min(lo + size, n)


def nparts(n, size):
    return (n + size - 1) // size


_VEC = {}


def get_vec(tg, name, n):
    """the one live handle: n envs on level ``name`` with its sprite sheet, no auto-reset"""
    key = (name, n)
    if _VEC.get("key") != key:
        if "vec" in _VEC:
            _VEC.pop("vec").close()
        _VEC["vec"] = tg.TreasureGameVec(n, seed=1, autoreset=False, level_dir=rs.LEVELS[name])
        _VEC["vec"].render_init(sprites_of(name))
        _VEC["key"] = key
    return _VEC["vec"]


@pytest.fixture(scope="module", autouse=True)
def _close_handle():
    yield
    if "vec" in _VEC:
        _VEC.pop("vec").close()
    _VEC.clear()
    part_reference.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=1)
def part_reference(name, part):
    """(sweep, lo, hi, states, the oracle's frames on the device) of one part, computed once"""
    import oracle
    sw = rs.sweep(name)
    lo, hi = part_bounds(sw.n, PART, part)
    st = sw.states(lo, hi)
    full = oracle.render_states(st, sprites_of(name), level_dir=sw.level_dir)
    return sw, lo, hi, st, torch.from_numpy(full).cuda()


def abi_render(tg, vec, count, s, channels):
    """tg_render_scaled called directly, into a buffer of 0xA5"""
    h, w, _ = vec.frame_shape_scaled(s)
    out = torch.full((count, h, w, channels), 0xA5, dtype=torch.uint8, device=vec.device)
    tg._lib.check(vec._L.tg_render_scaled(vec.handle, 0, count, s, channels,
                                          ctypes.c_void_p(out.data_ptr()), vec._stream()),
                  "tg_render_scaled")
    return out


def same_frames(sw, lo, got, want, what):
    """device tensors, exactly; a failure names the case and its first differing pixel"""
    assert got.shape == want.shape and got.dtype == torch.uint8, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        rs.compare_frames(sw, np.arange(lo, lo + len(want)), got.cpu().numpy(), want.cpu().numpy(),
                          "level %s, %s" % (sw.name, what))


def check_part(tg, name, part):
    sw, lo, hi, st, full = part_reference(name, part)
    n = hi - lo
    vec = get_vec(tg, name, n)
    vec.write_state(st)
    same_frames(sw, lo, vec.render(), full, "part %d, full size" % part)
    for s in SCALES:
        rgb = pool_fast(full, s, False)
        for gray in (False, True):
            want = pool_fast(rgb, 1, True) if gray else rgb   # the gray frame: the pooled one's luma
            what = "part %d, scale %d gray %s" % (part, s, gray)
            same_frames(sw, lo, vec.render(scale=s, gray=gray), want, what)
            if s == 1:   # k_render_scaled itself at scale 1
                same_frames(sw, lo, abi_render(tg, vec, n, 1, 1 if gray else 3), want,
                            what + " (C ABI)")
    assert vec.errors() == 0, "level %s part %d: errors %#x" % (sw.name, part, vec.errors())
    return sw, st, full


CASES = [(name, part) for name, n in TOTALS.items() for part in range(nparts(n, PART))]


def test_part_lists_cover_the_sweeps(oracle):
    for name, n in TOTALS.items():
        assert rs.sweep(name).n == n, name


def test_device_pooling_is_the_definition(oracle):
    """pool_fast on the device against the numpy definition, on a part's first 12 oracle frames"""
    _, _, _, _, full = part_reference(None, 0)
    for s in SCALES:
        for gray in (False, True):
            assert np.array_equal(pool_fast(full[:12], s, gray).cpu().numpy(),
                                  pool(full[:12].cpu().numpy(), s, gray)), (s, gray)


@pytest.mark.parametrize("name,part", CASES, ids=["%s-%d" % (n or "default", p) for n, p in CASES])
def test_render_sweep(tg, oracle, name, part):
    check_part(tg, name, part)


def test_narrow_level_composes_inline(tg, oracle, hostscaled):  # noqa: F811
    """the narrow level's whole sweep in one call: at scales 1 and 2 the host check counts more
    than SQCAP declined boxes in a span of exactly these states in this order, so k_render_scaled
    composes the excess inline; every scale and both channel counts, and scale 1
    through the C ABI, against the pooled oracle frames"""
    assert nparts(TOTALS["narrow"], PART) == 1   # one call renders all of it, as counted
    sw, st, _ = check_part(tg, "narrow", 0)
    for s in (1, 2):
        count, sqcap = span_queue_max(hostscaled, "narrow", st, s)
        print("narrow level, scale %d: %d declined boxes in the worst span, SQCAP %d"
              % (s, count, sqcap))
        assert count > sqcap, (s, count, sqcap)
