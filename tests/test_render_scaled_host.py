"""Downscaled / grayscale frames on the CPU: the product's per-output-pixel code
(csrc/tg_render_scaled.h, host-only build in tests/native_scaled) against ``pool`` — the
definition in include/tg_amd.h, restated in numpy — applied to the oracle's full frames.  Every
comparison is byte-exact; the fast paths (pooled static layer, pooled tiles) are also checked
against the general path (every box composed at full resolution)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gym_treasure_game_amd import render as R

SCALES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 48)
LEVELS = os.path.join(ROOT, "tests", "golden", "levels")
OVERLAP = os.path.join(LEVELS, "render_overlap")
CORRIDOR = os.path.join(LEVELS, "corridor")


def pool(frames, s, gray):
    """The definition: [n, Hpx, Wpx, 3] u8 full frames -> [n, Hpx/s, Wpx/s, 3 or 1] u8."""
    f = np.ascontiguousarray(frames, np.uint8)
    n, hp, wp, _ = f.shape
    assert hp % s == 0 and wp % s == 0
    sums = f.reshape(n, hp // s, s, wp // s, s, 3).sum(axis=(2, 4), dtype=np.uint32)
    out = ((2 * sums + s * s) // (2 * s * s)).astype(np.uint8)
    return luma(out) if gray else out


def luma(rgb):
    """[..., 3] u8 averaged RGB -> [..., 1] u8 gray."""
    c = rgb.astype(np.uint32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8)[..., None].astype(np.uint8)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def level_texts(level_dir):
    if level_dir is None:
        return None, None, None
    return tuple(open(os.path.join(level_dir, f), "rb").read()
                 for f in ("domain.txt", "domain-objects.txt", "domain-interactions.txt"))


def full_shape(level_dir):
    if level_dir is None:
        return 624, 672
    rows = [r.strip() for r in open(os.path.join(level_dir, "domain.txt")).read().split("\n")]
    rows = [r for r in rows if r]
    return len(rows) * 48, len(rows[0]) * 48


@pytest.fixture(scope="module")
def hostscaled():
    """Host-only build of the scaled renderer's per-pixel code (tests/native_scaled)."""
    d = os.path.join(ROOT, "tests", "native_scaled")
    subprocess.check_call(["make", "-s", "-C", d])
    L = ctypes.CDLL(os.path.join(d, "libtg_hostcheck_scaled.so"))
    P = ctypes.c_void_p
    L.hcs_render_run.restype = ctypes.c_int
    L.hcs_render_run.argtypes = [P, P, P, ctypes.c_uint64, P, ctypes.c_int64, ctypes.c_int,
                                 ctypes.c_uint64, ctypes.c_int, ctypes.c_int, P, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    return L


def hcs_frames(lib, envs, steps, a0, policy, autoreset, sprites, s, gray, fast=1, level_dir=None,
               states=None, angs=None):
    envs = np.ascontiguousarray(envs, np.int64)
    hp, wp = full_shape(level_dir)
    out = np.full((len(envs), hp // s, wp // s, 1 if gray else 3), 0xA5, np.uint8)
    rc = lib.hcs_render_run(*level_texts(level_dir), 0, _p(envs), len(envs), steps, a0, policy,
                            int(autoreset), _p(sprites), sprites.shape[2], sprites.shape[1], s,
                            1 if gray else 3, fast, _p(out),
                            None if states is None else _p(states),
                            None if angs is None else _p(angs))
    assert rc == 0
    return out


def check_all(lib, want_full, envs, steps, a0, policy, autoreset, sprites, scales, level_dir=None):
    for s in scales:
        for gray in (False, True):
            want = pool(want_full, s, gray)
            for fast in (1, 0):
                got = hcs_frames(lib, envs, steps, a0, policy, autoreset, sprites, s, gray, fast,
                                 level_dir)
                assert got.shape == want.shape
                np.testing.assert_array_equal(
                    got, want, err_msg="scale %d gray %s fast %d step %d" % (s, gray, fast, steps))


def test_pool_is_the_definition():
    """pool on a frame with known sums: halves round up, gray from the averaged bytes."""
    f = np.zeros((1, 2, 4, 3), np.uint8)
    f[0, :, :2] = [[[1, 0, 255], [2, 0, 255]], [[0, 0, 255], [0, 1, 254]]]  # sums 3, 1, 1019
    got = pool(f, 2, False)
    assert got.shape == (1, 1, 2, 3)
    assert got[0, 0, 0].tolist() == [1, 0, 255]  # 0.75 -> 1, 0.25 -> 0, 254.75 -> 255
    f[0, :, 2:] = [[[1, 1, 1], [0, 0, 0]], [[1, 1, 1], [0, 0, 0]]]  # 0.5 rounds up
    assert pool(f, 2, False)[0, 0, 1].tolist() == [1, 1, 1]
    assert pool(f, 2, True)[0, 0].ravel().tolist() == [(77 * 1 + 29 * 255 + 128) >> 8, 1]
    assert np.array_equal(pool(f, 1, False), f)


def test_header_and_exports(tg):
    src = open(os.path.join(ROOT, "include", "tg_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("tg_frame_shape_scaled", "tg_render_scaled"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in tg._lib.EXPORTS
    assert re.search(r"#define\s+TG_FRAME_RGB\s+3\b", code)
    assert re.search(r"#define\s+TG_FRAME_GRAY\s+1\b", code)
    out = subprocess.check_output(["nm", "-D", "--defined-only", tg._lib.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"tg_frame_shape_scaled", "tg_render_scaled"} <= exported


@pytest.mark.parametrize("steps", [0, 7, 60])
def test_default_level_every_scale(hostscaled, oracle, steps):
    """24 envs, masked auto-reset policy: every scale x {rgb, gray}, fast and general paths."""
    sprites = R.synthetic_sprites(seed=steps + 1)
    envs = np.arange(24) * 37
    a0 = 0x52
    want = oracle.run_render(0, envs, steps, a0, 1, True, sprites)
    check_all(hostscaled, want, envs, steps, a0, 1, True, sprites, SCALES)


@pytest.mark.parametrize("steps", [0, 20, 80])
def test_overlapping_items(hostscaled, oracle, steps):
    """Two items on one cell (key on the bolt) and a shaft crossing a later item's cell."""
    sprites = R.synthetic_sprites(seed=3)
    envs = np.arange(16)
    want = oracle.run_render(0, envs, steps, 5, 1, True, sprites, level_dir=OVERLAP)
    check_all(hostscaled, want, envs, steps, 5, 1, True, sprites, (3, 4, 8), OVERLAP)


def test_other_level_size(hostscaled, oracle):
    """The 44 x 5-cell corridor (full frames 240 x 2,112)."""
    sprites = R.synthetic_sprites(seed=4, size=24)
    envs = np.arange(12)
    want = oracle.run_render(0, envs, 6, 9, 1, True, sprites, level_dir=CORRIDOR)
    assert want.shape == (12, 240, 2112, 3)
    check_all(hostscaled, want, envs, 6, 9, 1, True, sprites, (8, 48), CORRIDOR)
    assert hcs_frames(hostscaled, envs, 6, 9, 1, True, sprites, 48, True,
                      level_dir=CORRIDOR).shape == (12, 5, 44, 1)


def test_covers_every_item(hostscaled, oracle):
    """64 envs x 150 masked steps without auto-reset at scale 8.  The states the frames were
    rendered from are read back and must cover: each door open and closed, the bolt open and
    locked, each handle up and down at many shaft angles, the key on the map and taken, and the
    hero facing both ways.  (The gold is never taken by this stream: it is drawn on its cell in
    every frame.)"""
    sprites = R.synthetic_sprites(seed=99)
    envs = np.arange(64)
    want = oracle.run_render(0, envs, 150, 0xBEEF, 1, False, sprites)
    check_all(hostscaled, want, envs, 150, 0xBEEF, 1, False, sprites, (8,))
    assert len({g.tobytes() for g in pool(want, 8, False)}) > 32
    states, angs = np.zeros((64, 4), np.uint32), np.zeros((64, 2), np.float64)
    hcs_frames(hostscaled, envs, 150, 0xBEEF, 1, False, sprites, 8, False, states=states, angs=angs)
    facing, obj = ctypes.c_uint32(), ctypes.c_int()
    hostscaled.hcs_flag_bits(ctypes.byref(facing), ctypes.byref(obj))
    flags = states[:, 1]
    assert set(np.unique(flags & facing.value)) == {0, facing.value}, "hero facing"
    for b, name in enumerate(("door 0", "door 1", "door 2", "handle 0", "handle 1", "bolt")):
        assert set(np.unique((flags >> (obj.value + b)) & 1)) == {0, 1}, name
    key_x = (states[:, 2] & 0xFF).astype(np.int8)
    assert (key_x < 0).any() and (key_x >= 0).any(), "key on the map and taken"
    assert len(np.unique(angs[:, 0])) > 16 and len(np.unique(angs[:, 1])) > 16, "shaft angles"


def test_bad_scale_is_rejected(hostscaled):
    sprites = R.synthetic_sprites(seed=1)
    envs = np.zeros(1, np.int64)
    out = np.zeros(1 << 16, np.uint8)
    for s, ch in ((0, 3), (5, 3), (96, 3), (8, 2)):
        assert hostscaled.hcs_render_run(None, None, None, 0, _p(envs), 1, 0, 0, 1, 1, _p(sprites),
                                         32, 32, s, ch, 1, _p(out), None, None) == -2
