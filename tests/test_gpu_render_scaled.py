"""GPU: downscaled / grayscale frames (k_render_scaled through tg_render_scaled) against
``pool`` — the definition in include/tg_amd.h, in numpy — of the oracle's full frames, byte
for byte.  Sprite sheets are synthetic (every blend case: alpha 0, 255 and in between)."""
import ctypes

import numpy as np
import pytest
import torch

from test_render_scaled_host import CORRIDOR, OVERLAP, SCALES, luma, pool

pytestmark = pytest.mark.gpu


def _check(oracle, got, envs, steps, a0, policy, autoreset, sprites, s, gray, level_dir=None):
    full = oracle.run_render(0, envs, steps, a0, policy, autoreset, sprites, level_dir=level_dir)
    _check_pooled(got, full, envs, steps, s, gray)


def _check_pooled(got, full, envs, steps, s, gray, want=None):
    want = pool(full, s, gray) if want is None else want
    assert got.shape == want.shape and got.dtype == np.uint8
    for i, g in enumerate(envs):
        if not np.array_equal(got[i], want[i]):
            bad = np.argwhere((got[i] != want[i]).any(-1))
            raise AssertionError("env %d step %d scale %d gray %s: %d pixels differ, first at "
                                 "(y, x) = %s" % (g, steps, s, gray, len(bad), tuple(bad[0])))


def _stepped(tg, n, steps, a0, policy, sprites, **kw):
    vec = tg.TreasureGameVec(n, seed=0, autoreset=True, **kw)
    vec.render_init(sprites)
    vec.reset()
    for t in range(steps):
        vec.step(vec.policy_actions(t, a0, policy))
    return vec


def _abi_render(tg, vec, first, count, s, channels):
    """tg_render_scaled called directly: ``vec.render(scale=1, gray=False)`` takes tg_render's
    path, so k_render_scaled at scale 1 rgb is reached only through the C ABI."""
    h, w, _ = vec.frame_shape_scaled(s)
    out = torch.full((count, h, w, channels), 0xA5, dtype=torch.uint8, device=vec.device)
    tg._lib.check(vec._L.tg_render_scaled(vec.handle, first, count, s, channels,
                                          ctypes.c_void_p(out.data_ptr()), vec._stream()),
                  "tg_render_scaled")
    return out


def test_every_scale_and_channel(tg, oracle):
    """37 envs (not a multiple of the 4-env group), masked auto-reset, after 12 steps."""
    n, steps, a0 = 37, 12, 0x61
    sprites = tg.synthetic_sprites(seed=31)
    vec = _stepped(tg, n, steps, a0, "masked", sprites)
    envs = np.arange(n)
    full = oracle.run_render(0, envs, steps, a0, 1, True, sprites)
    for s in SCALES:
        for gray in (False, True):
            assert vec.frame_shape_scaled(s, gray) == (624 // s, 672 // s, 1 if gray else 3)
            got = vec.render(scale=s, gray=gray)
            assert tuple(got.shape) == (n,) + vec.frame_shape_scaled(s, gray)
            _check_pooled(got.cpu().numpy(), full, envs, steps, s, gray)
    # scale 1 rgb through k_render_scaled itself (render() above took tg_render's path for it)
    got = _abi_render(tg, vec, 0, n, 1, tg._lib.TG_FRAME_RGB)
    _check_pooled(got.cpu().numpy(), full, envs, steps, 1, False)
    assert vec.errors() == 0
    vec.close()


@pytest.mark.parametrize("lo,hi", [(0, 14), (14, 28), (28, 41)])
def test_every_step(tg, oracle, lo, hi):
    """48 envs x 40 masked steps at scale 8, both channel counts, every frame (the frames after
    steps lo .. hi-1 per case: the oracle's full-size CPU render is what takes the time)."""
    n, a0 = 48, 0x77
    sprites = tg.synthetic_sprites(seed=5)
    vec = tg.TreasureGameVec(n, seed=0, autoreset=True)
    vec.render_init(sprites)
    vec.reset()
    envs = np.arange(n)
    for t in range(hi):
        if t:
            vec.step(vec.policy_actions(t - 1, a0, "masked"))
        if t < lo:
            continue
        full = oracle.run_render(0, envs, t, a0, 1, True, sprites)
        rgb = pool(full, 8, False)  # pooled once per step; the gray frame is its luma
        for gray in (False, True):
            _check_pooled(vec.render(scale=8, gray=gray).cpu().numpy(), full, envs, t, 8, gray,
                          want=luma(rgb) if gray else rgb)
    assert vec.errors() == 0
    vec.close()


def test_subranges_and_guard_bytes(tg):
    n = 301
    vec = tg.TreasureGameVec(n, seed=9, autoreset=True)
    vec.render_init(tg.synthetic_sprites(seed=1, size=16))
    for t in range(15):
        vec.step(vec.policy_actions(t, 3, "uniform"))
    full = vec.render(scale=8).clone()
    assert torch.equal(vec.render(first=37, count=99, scale=8), full[37:136])
    buf = torch.empty((5,) + vec.frame_shape_scaled(8), dtype=torch.uint8, device=vec.device)
    assert vec.render(first=n - 5, count=5, out=buf, scale=8).data_ptr() == buf.data_ptr()
    assert torch.equal(buf, full[n - 5:])
    pad = 256
    for s, fb in ((8, 6552), (48, 182)):  # frames that are no multiple of 16 B
        h, w, c = vec.frame_shape_scaled(s, True)
        assert h * w * c == fb
        whole = vec.render(scale=s, gray=True).clone()
        for first, count in ((37, 99), (n - 5, 5), (0, 1)):
            big = torch.full((pad + count * fb + pad,), 0xA5, dtype=torch.uint8, device=vec.device)
            view = big[pad:pad + count * fb].view(count, h, w, c)
            assert view.data_ptr() % 16 == 0
            vec.render(first=first, count=count, out=view, scale=s, gray=True)
            assert torch.equal(view, whole[first:first + count])
            assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + count * fb:] == 0xA5).all())
    for bad in (0, 5, 96):
        with pytest.raises(tg.TgError):
            vec.render(scale=bad)
        with pytest.raises(tg.TgError):
            vec.frame_shape_scaled(bad)
    with pytest.raises(tg.TgError):
        vec.render(first=n - 4, count=5, scale=8)
    with pytest.raises(tg.TgError):  # a channel count that is neither RGB nor gray
        tg._lib.check(vec._L.tg_render_scaled(vec.handle, 0, 5, 8, 2,
                                              ctypes.c_void_p(buf.data_ptr()), None),
                      "tg_render_scaled")
    with pytest.raises(ValueError):
        vec.render(first=0, count=4, out=buf, scale=8)
    with pytest.raises(ValueError):
        vec.render(first=0, count=5, out=buf, scale=8, gray=True)
    assert vec.errors() == 0
    vec.close()


def test_scale_one(tg):
    n = 21
    vec = _stepped(tg, n, 9, 0x11, "masked", tg.synthetic_sprites(seed=2))
    full = vec.render().clone()
    assert torch.equal(vec.render(scale=1), full)  # the Python default: tg_render's own path
    # k_render_scaled at scale 1 with 3 channels == k_render, byte for byte (whole batch, and a
    # sub-range whose 5 frames end a 4-env group early)
    assert torch.equal(_abi_render(tg, vec, 0, n, 1, tg._lib.TG_FRAME_RGB), full)
    assert torch.equal(_abi_render(tg, vec, 3, 5, 1, tg._lib.TG_FRAME_RGB), full[3:8])
    assert torch.equal(_abi_render(tg, vec, 0, n, 1, tg._lib.TG_FRAME_GRAY),
                       vec.render(scale=1, gray=True))
    assert np.array_equal(vec.render(scale=1, gray=True).cpu().numpy(),
                          pool(full.cpu().numpy(), 1, True))
    assert vec.errors() == 0
    vec.close()


def test_other_levels(tg, oracle):
    sprites = tg.synthetic_sprites(seed=21, size=40)
    n, a0 = 40, 0x3C
    vec = _stepped(tg, n, 8, a0, "masked", sprites, level_dir=CORRIDOR)
    full = oracle.run_render(0, np.arange(n), 8, a0, 1, True, sprites, level_dir=CORRIDOR)
    for s in (8, 48):
        for gray in (False, True):
            assert vec.frame_shape_scaled(s, gray)[:2] == (240 // s, 2112 // s)
            _check_pooled(vec.render(scale=s, gray=gray).cpu().numpy(), full, np.arange(n), 8, s,
                          gray)
    assert vec.errors() == 0
    vec.close()
    sprites = tg.synthetic_sprites(seed=3)
    for steps in (0, 20):
        vec = _stepped(tg, 16, steps, 5, "masked", sprites, level_dir=OVERLAP)
        for gray in (False, True):
            _check(oracle, vec.render(scale=4, gray=gray).cpu().numpy(), np.arange(16), steps, 5,
                   1, True, sprites, 4, gray, level_dir=OVERLAP)
        assert vec.errors() == 0
        vec.close()


def test_64_bit_addressing(tg, oracle):
    """16,384 envs at scale 2 rgb: 314,496 B per frame, a 5.15-GB buffer that crosses 4 GiB at
    env 13,656, in one launch."""
    n, steps, a0, s = 16384, 10, 0x64, 2
    sprites = tg.synthetic_sprites(seed=64)
    vec = _stepped(tg, n, steps, a0, "uniform", sprites)
    frames = vec.render(scale=s)
    fb = frames[0].numel()
    assert fb == 314496 and n * fb > 1 << 32
    edge = (1 << 32) // fb
    assert edge == 13656
    envs = np.concatenate([np.arange(32), np.arange(edge - 32, edge + 32), np.arange(n - 32, n)])
    for k in range(0, len(envs), 64):
        chunk = envs[k:k + 64]
        got = frames.index_select(0, torch.as_tensor(chunk, device=vec.device)).cpu().numpy()
        _check(oracle, got, chunk, steps, a0, 0, True, sprites, s, False)
    sums = frames.view(n, -1).view(torch.int64).sum(1)  # per-frame checksum (wrapping)
    again = vec.render(out=frames, scale=s)
    assert torch.equal(again.view(n, -1).view(torch.int64).sum(1), sums)
    assert vec.errors() == 0
    del frames, again
    vec.close()
    torch.cuda.empty_cache()


def test_batch_of_65536(tg, oracle):
    """65,536 envs at scale 8 rgb after 25 uniform steps: 512 spread envs vs the oracle."""
    n, steps, a0 = 65536, 25, 0xC5
    sprites = tg.synthetic_sprites(seed=55)
    vec = _stepped(tg, n, steps, a0, "uniform", sprites)
    frames = vec.render(scale=8)
    assert tuple(frames.shape) == (n, 78, 84, 3)
    envs = np.unique(np.concatenate([np.arange(64), np.linspace(0, n - 1, 448).astype(np.int64)]))
    for k in range(0, len(envs), 64):
        chunk = envs[k:k + 64]
        got = frames.index_select(0, torch.as_tensor(chunk, device=vec.device)).cpu().numpy()
        _check(oracle, got, chunk, steps, a0, 0, True, sprites, 8, False)
    assert vec.errors() == 0
    del frames
    vec.close()


def test_wrappers(tg, oracle):
    n, a0 = 32, 0x99
    sprites = tg.synthetic_sprites(seed=12)
    w = tg.ObservationWrapper(tg.TreasureGameVec(n, seed=0, autoreset=True), sprites=sprites,
                              scale=8, gray=True)
    frames = w.reset()
    assert tuple(frames.shape) == (n, 78, 84, 1)
    _check(oracle, frames.cpu().numpy(), np.arange(n), 0, a0, 1, True, sprites, 8, True)
    for t in range(6):
        frames, rew, valid, done, info = w.step(w.env.policy_actions(t, a0, "masked"))
        assert tuple(frames.shape) == (n, 78, 84, 1) and info["world_state"].shape == (n, 9)
    _check(oracle, frames.cpu().numpy(), np.arange(n), 6, a0, 1, True, sprites, 8, True)
    assert w.env.errors() == 0
    w.close()

    w = tg.ObservationWrapper(tg.make("treasure_game-v0", seed=4), sprites=sprites, scale=4)
    e = oracle.OracleEnv(4)
    first = w.reset()
    assert isinstance(first, np.ndarray) and first.shape == (156, 168, 3)
    np.testing.assert_array_equal(first, pool(e.render(sprites)[None], 4, False)[0])
    for t in range(10):
        a = oracle.pick_action(1, 4, t, True, e.mask())
        screen, r, d, info = w.step(a)
        o, r2, d2, _ = e.step(a)
        assert screen.shape == (156, 168, 3) and screen.dtype == np.uint8
        np.testing.assert_array_equal(screen, pool(e.render(sprites)[None], 4, False)[0])
        assert (r, d) == (r2, d2)
        assert np.array_equal(np.array(info["world_state"]).view(np.uint64), o.view(np.uint64))
    g = w.env.render("rgb_array", scale=8, gray=True)
    assert g.shape == (78, 84, 1)
    np.testing.assert_array_equal(g, pool(e.render(sprites)[None], 8, True)[0])
    np.testing.assert_array_equal(w.env.render("rgb_array"), e.render(sprites))
    assert w.env._vec.errors() == 0
    w.close()
