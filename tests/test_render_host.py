"""render('rgb_array') on the CPU: the oracle's pygame/SDL restatement (oracle/tg_oracle.c,
"Renderer") against Python's own random for the background choices, and against the product's
frame composition (csrc/tg_render.h, host-only build in tests/native, driven band by band and
chunk by chunk as k_render's lanes are).  The renderer's parity with the reference itself is
UNPINNED: pygame is absent from this image."""
import ctypes
import os
import random

import numpy as np
import pytest

from gym_treasure_game_amd import render as R


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


OVERLAP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels",
                       "render_overlap")


def level_texts(level_dir):
    if level_dir is None:
        return None, None, None
    return tuple(open(os.path.join(level_dir, f), "rb").read()
                 for f in ("domain.txt", "domain-objects.txt", "domain-interactions.txt"))


CORRIDOR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels",
                        "corridor")


def frame_shape(level_dir):
    if level_dir is None:
        return 624, 672
    rows = [r.strip() for r in open(os.path.join(level_dir, "domain.txt")).read().split("\n")]
    rows = [r for r in rows if r]
    return len(rows) * 48, len(rows[0]) * 48


def hc_frames(lib, envs, steps, a0, policy, autoreset, sprites, seed_base=0, level_dir=None):
    envs = np.ascontiguousarray(envs, np.int64)
    out = np.zeros((len(envs),) + frame_shape(level_dir) + (3,), np.uint8)
    rc = lib.hc_render_run(*level_texts(level_dir), seed_base, _p(envs), len(envs), steps, a0, policy,
                           int(autoreset), _p(sprites), sprites.shape[2], sprites.shape[1], _p(out))
    assert rc == 0
    return out


def test_background_choices_vs_cpython(oracle):
    """draw_domain's Random(12).choice sequence (DR/:83-86, 137) == CPython's."""
    r = random.Random(12)
    want = [r.choice(range(5)) for _ in range(2000)]
    assert list(oracle.choice_seq(12, 5, 2000)) == want
    for n in (1, 2, 3, 7, 8, 9):
        r = random.Random(3)
        assert list(oracle.choice_seq(3, n, 300)) == [r.choice(range(n)) for _ in range(300)]


@pytest.mark.parametrize("policy,autoreset,steps", [(1, True, 0), (1, True, 7), (0, False, 25),
                                                    (1, True, 60)])
def test_composition_vs_oracle(hostcheck, oracle, policy, autoreset, steps):
    sprites = R.synthetic_sprites(seed=steps + 1)
    envs = np.arange(24) * 37
    a0 = 0x51 + policy
    got = hc_frames(hostcheck, envs, steps, a0, policy, autoreset, sprites)
    want = oracle.run_render(0, envs, steps, a0, policy, autoreset, sprites)
    for i in range(len(envs)):
        np.testing.assert_array_equal(got[i], want[i], err_msg="env %d" % envs[i])


def test_composition_vs_oracle_sprite_sizes(hostcheck, oracle):
    """Sheets of other source sizes (scale up, down and 1:1)."""
    envs = np.arange(6)
    for size in (16, 48, 50, 64):
        sprites = R.synthetic_sprites(seed=size, size=size)
        got = hc_frames(hostcheck, envs, 12, 7, 1, True, sprites)
        want = oracle.run_render(0, envs, 12, 7, 1, True, sprites)
        np.testing.assert_array_equal(got, want, err_msg="size %d" % size)


def test_composition_covers_every_item(hostcheck, oracle):
    """Masked rollouts long enough that keys, gold, bolts, handles and doors all change and
    the hero faces both ways; each frame matches and differs from the static layer."""
    sprites = R.synthetic_sprites(seed=99)
    envs = np.arange(64)
    got = hc_frames(hostcheck, envs, 150, 0xBEEF, 1, False, sprites)
    want = oracle.run_render(0, envs, 150, 0xBEEF, 1, False, sprites)
    np.testing.assert_array_equal(got, want)
    assert len({g.tobytes() for g in got}) > 32


@pytest.mark.parametrize("steps", [0, 20, 80])
def test_composition_vs_oracle_overlapping_items(hostcheck, oracle, steps):
    """Two items on one cell (key on the bolt) and a shaft crossing a later item's cell."""
    sprites = R.synthetic_sprites(seed=3)
    envs = np.arange(16)
    got = hc_frames(hostcheck, envs, steps, 5, 1, True, sprites, level_dir=OVERLAP)
    want = oracle.run_render(0, envs, steps, 5, 1, True, sprites, level_dir=OVERLAP)
    np.testing.assert_array_equal(got, want)


def test_composition_vs_oracle_other_level_size(hostcheck, oracle):
    """A 44 x 5-cell level (frames 240 x 2,112): other row lengths and band counts."""
    sprites = R.synthetic_sprites(seed=4, size=24)
    envs = np.arange(12)
    got = hc_frames(hostcheck, envs, 6, 9, 1, True, sprites, level_dir=CORRIDOR)
    want = oracle.run_render(0, envs, 6, 9, 1, True, sprites, level_dir=CORRIDOR)
    assert got.shape == (12, 240, 2112, 3)
    np.testing.assert_array_equal(got, want)


SPRITES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sprites")


def test_real_sprites_if_present(hostcheck, oracle):
    """The reference's own sprite sheet: its 24 PNGs are stored under tests/golden/sprites
    (their licences: attribution.txt there), in the layout load_sprites reads."""
    sprites = R.load_sprites(SPRITES)
    assert sprites.shape == (R.SPRITE_COUNT, 32, 32, 4) and sprites.dtype == np.uint8
    envs = np.arange(8)
    got = hc_frames(hostcheck, envs, 40, 3, 1, True, sprites)
    want = oracle.run_render(0, envs, 40, 3, 1, True, sprites)
    np.testing.assert_array_equal(got, want)
