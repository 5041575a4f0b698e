"""GPU: agent-centred windows (k_render_view through tg_render_view) against the definition: the
zero-padded crop, at the hero's cell minus the radius, of the downscaled / grayscale frame.  The
crop is taken on the device from the product's own whole frames and, per test, from the pooled
oracle frames (test_render_view_host.crop0 / test_render_scaled_host.pool), so the check does not
rest on the product's renderer; everything is byte-exact.  Origins are held to read_state's and
the oracle's positions."""
import ctypes

import numpy as np
import pytest
import torch

import render_sweep as rs
from test_render_scaled_host import luma, pool
from test_render_sweep_host import luma_fast, pool_fast
from test_render_view_host import (RADII, SYNTH_SPRITES, crop0, hcv_states, hostview,  # noqa: F401
                                   leaves, oracle_positions, origins, side, synth_states)

pytestmark = pytest.mark.gpu


def crop_dev(frames, org, r, s):
    """crop0 on the device: [n, h, w, c] u8 frames at scale s, origins [n, 2] (cells, a tensor)
    -> [n, k, k, c], zero outside the frame"""
    n, h, w, c = frames.shape
    k, cs = side(r, s), 48 // s
    ar = torch.arange(k, device=frames.device)
    ys = (org[:, 1].long() * cs)[:, None] + ar
    xs = (org[:, 0].long() * cs)[:, None] + ar
    inside = ((ys >= 0) & (ys < h))[:, :, None] & ((xs >= 0) & (xs < w))[:, None, :]
    idx = torch.arange(n, device=frames.device)[:, None, None]
    got = frames[idx, ys.clamp(0, h - 1)[:, :, None], xs.clamp(0, w - 1)[:, None, :]]
    return got * inside[..., None].to(torch.uint8)


def read_origins(vec, r):
    return origins(vec.read_state()["pos"], r)


def _stepped(tg, n, steps, a0, sprites, autoreset=True, **kw):
    vec = tg.TreasureGameVec(n, seed=0, autoreset=autoreset, **kw)
    vec.render_init(sprites)
    vec.reset()
    for t in range(steps):
        vec.step(vec.policy_actions(t, a0, "masked"))
    return vec


def view_and_origin(vec, r, s, gray, first=0, count=None):
    count = vec.num_envs - first if count is None else count
    org = torch.full((count, 2), -9999, dtype=torch.int32, device=vec.device)
    got = vec.render(first=first, count=count, scale=s, gray=gray, view=r, origin=org)
    return got, org


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == torch.uint8, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).flatten(1).any(1)).flatten()
        i = int(bad[0])
        px = torch.nonzero((got[i] != want[i]).any(-1))
        raise AssertionError("%s: %d of %d windows differ; first: env %d, %d pixels, first at "
                             "(y, x) = %s" % (what, len(bad), len(want), i, len(px), px[0].tolist()))


def test_crop_identity_and_origins(tg, oracle):
    """37 envs (a short last group at every group size) after 12 masked steps: every r x s x
    channel count against the crop of the product's whole frame, one (r, s) per channel count
    also against the crop of the pooled oracle frames, the origins against read_state"""
    n, steps, a0 = 37, 12, 0x61
    sprites = tg.synthetic_sprites(seed=31)
    vec = _stepped(tg, n, steps, a0, sprites)
    full = oracle.run_render(0, np.arange(n), steps, a0, 1, True, sprites)
    pos = oracle_positions(oracle, n, steps, a0, 1, True)[:, steps]
    assert np.array_equal(vec.read_state()["pos"], pos)
    for r in RADII:
        want_org = read_origins(vec, r)
        for s in (1, 8, 48):
            for gray in (False, True):
                assert vec.frame_shape_view(r, s, gray) == (side(r, s), side(r, s), 1 if gray else 3)
                got, org = view_and_origin(vec, r, s, gray)
                assert np.array_equal(org.cpu().numpy(), want_org), (r, s)
                whole = vec.render(scale=s, gray=gray)
                what = "r %d scale %d gray %s" % (r, s, gray)
                same(got, crop_dev(whole, org, r, s), what)
                if (r, s, gray) in ((2, 8, False), (1, 1, True)):
                    want = crop0(pool(full, s, gray), origins(pos, r), r, s)
                    assert np.array_equal(got.cpu().numpy(), want), what + " (oracle)"
                    # and the device crop is the numpy one
                    assert np.array_equal(crop_dev(whole, org, r, s).cpu().numpy(),
                                          crop0(whole.cpu().numpy(), origins(pos, r), r, s))
    assert vec.errors() == 0
    vec.close()


ROLL_N, ROLL_T0, ROLL_T, ROLL_A0 = 48, 60, 40, 0x5A


@pytest.mark.parametrize("lo,hi", [(60, 74), (74, 88), (88, 101)])
@pytest.mark.parametrize("autoreset", [False, True])
def test_every_frame_of_a_rollout(tg, oracle, autoreset, lo, hi):
    """48 envs x 40 masked steps (steps 60..100 of the rollout: before step 20 no hero of these
    48 has come down to the rows from which a window leaves at the bottom) at r = 2, scale 4,
    both channel counts, every frame, against the crop of the oracle frames pooled on the device
    (pool_fast, held to the numpy definition by tests/test_render_sweep_host.py); the frames
    after steps lo .. hi-1 per case.  First, from the oracle's positions alone: the 48 x 41
    windows hold some leaving the frame on each of the four sides and some wholly inside it."""
    n, r, s = ROLL_N, 2, 4
    pos = oracle_positions(oracle, n, ROLL_T0 + ROLL_T, ROLL_A0, 1, autoreset)
    where = leaves(origins(pos[:, ROLL_T0:].reshape(-1, 2), r), r, (624, 672))
    counts = {b: int((where & b != 0).sum()) for b in (1, 2, 4, 8)}
    print("windows of %d leaving: left %d right %d top %d bottom %d, inside %d"
          % (len(where), counts[1], counts[2], counts[4], counts[8], int((where == 0).sum())))
    assert len(where) == 48 * 41 and all(counts.values()) and (where == 0).any()
    sprites = tg.synthetic_sprites(seed=5)
    vec = tg.TreasureGameVec(n, seed=0, autoreset=autoreset)
    vec.render_init(sprites)
    vec.reset()
    envs = np.arange(n)
    for t in range(hi):
        if t:
            vec.step(vec.policy_actions(t - 1, ROLL_A0, "masked"))
        if t < lo:
            continue
        full = torch.from_numpy(oracle.run_render(0, envs, t, ROLL_A0, 1, autoreset, sprites)).cuda()
        rgb = pool_fast(full, s, False)   # pooled once per step; the gray frame is its luma
        want_org = torch.as_tensor(origins(pos[:, t], r), device=vec.device)
        for gray in (False, True):
            got, org = view_and_origin(vec, r, s, gray)
            assert torch.equal(org, want_org), t
            same(got, crop_dev(luma_fast(rgb) if gray else rgb, want_org, r, s),
                 "step %d gray %s" % (t, gray))
    assert vec.errors() == 0
    vec.close()


def test_guarded_subranges(tg):
    """sub-ranges whose first and count are no multiples of the group size into 0xA5-guarded
    buffers, at 324-B, 9-B (an odd byte count with 5 envs) and 62,208-B frames"""
    n = 61
    vec = _stepped(tg, n, 15, 3, tg.synthetic_sprites(seed=1, size=16))
    pad = 256
    for r, s, gray, fb in ((1, 8, True, 324), (1, 48, True, 9), (1, 1, False, 62208)):
        shape = vec.frame_shape_view(r, s, gray)
        assert shape[0] * shape[1] * shape[2] == fb
        whole = vec.render(scale=s, gray=gray, view=r).clone()
        orgs = torch.as_tensor(read_origins(vec, r), device=vec.device)
        same(whole, crop_dev(vec.render(scale=s, gray=gray), orgs, r, s), "whole batch, %d B" % fb)
        for first, count in ((37, 19), (n - 5, 5), (0, 1), (3, 13), (0, n)):
            big = torch.full((pad + count * fb + pad,), 0xA5, dtype=torch.uint8, device=vec.device)
            view = big[pad:pad + count * fb].view((count,) + shape)
            assert view.data_ptr() % 16 == 0
            org = torch.full((count + 2, 2), -9999, dtype=torch.int32, device=vec.device)
            vec.render(first=first, count=count, out=view, scale=s, gray=gray, view=r, origin=org[1:-1])
            assert torch.equal(view, whole[first:first + count]), (fb, first, count)
            assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + count * fb:] == 0xA5).all())
            assert torch.equal(org[1:-1], orgs[first:first + count])
            assert bool((org[0] == -9999).all()) and bool((org[-1] == -9999).all())
    assert vec.errors() == 0
    vec.close()


def test_synthesized_states(tg, oracle, hostview):  # noqa: F811
    """the host test's synthesized states (the hero on, across and far off every edge, a window
    wholly outside the frame) written with write_state: every r x s x channel count against the
    crop of the pooled oracle frames; errors() is what the host check predicts"""
    st, labels = synth_states(mt=True)
    n = len(labels)
    sprites = tg.synthetic_sprites(seed=SYNTH_SPRITES)
    full = oracle.render_states(st, sprites)
    vec = tg.TreasureGameVec(n, seed=1, autoreset=False)
    vec.render_init(sprites)
    vec.write_state(st)
    predicted = 0
    for r in RADII:
        want_org = origins(st["pos"], r)
        for s in (1, 8, 48):
            rgb = pool(full, s, False)
            for gray in (False, True):
                got, org = view_and_origin(vec, r, s, gray)
                assert np.array_equal(org.cpu().numpy(), want_org), (r, s)
                want = crop0(luma(rgb) if gray else rgb, want_org, r, s)
                g = got.cpu().numpy()
                bad = np.flatnonzero((g != want).reshape(n, -1).any(1))
                assert not len(bad), "r %d scale %d gray %s: %d windows differ; first: %s" % (
                    r, s, gray, len(bad), labels[int(bad[0])])
        predicted |= hcv_states(hostview, None, st, sprites, r, 48, True)[2]
    assert vec.errors() == predicted == 0
    vec.close()


def test_crossing_4_gib(tg, oracle):
    """2,800 envs at r = 7, scale 1, rgb: 1,555,200 B per frame, a 4.35-GB buffer that crosses
    4 GiB inside env 2,761, in one launch"""
    n, steps, a0, r = 2800, 10, 0x64, 7
    sprites = tg.synthetic_sprites(seed=64)
    vec = _stepped(tg, n, steps, a0, sprites)
    frames, org = view_and_origin(vec, r, 1, False)
    fb = frames[0].numel()
    assert fb == 1555200 and n * fb > 1 << 32
    edge = (1 << 32) // fb
    assert edge == 2761
    envs = np.concatenate([np.arange(4), np.arange(edge - 4, edge + 5), np.arange(n - 4, n)])
    full = oracle.run_render(0, envs, steps, a0, 1, True, sprites)
    pos = oracle_positions(oracle, n, steps, a0, 1, True)[envs, steps]
    assert np.array_equal(org.cpu().numpy()[envs], origins(pos, r))
    got = frames.index_select(0, torch.as_tensor(envs, device=vec.device)).cpu().numpy()
    assert np.array_equal(got, crop0(full, origins(pos, r), r, 1))
    assert vec.errors() == 0
    del frames
    vec.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,r,s", [("render_overlap", 1, 4), ("corridor", 3, 8),
                                      ("narrow", 2, 1), ("cascade", 7, 48)])
def test_other_levels(tg, oracle, name, r, s):
    level_dir = rs.LEVELS[name]
    n, steps, a0 = 21, 8, 0x3C
    sprites = tg.synthetic_sprites(seed=21, size=40)
    vec = _stepped(tg, n, steps, a0, sprites, level_dir=level_dir)
    full = oracle.run_render(0, np.arange(n), steps, a0, 1, True, sprites, level_dir=level_dir)
    pos = oracle_positions(oracle, n, steps, a0, 1, True, level_dir)[:, steps]
    for gray in (False, True):
        got, org = view_and_origin(vec, r, s, gray)
        assert np.array_equal(org.cpu().numpy(), origins(pos, r))
        assert np.array_equal(got.cpu().numpy(), crop0(pool(full, s, gray), origins(pos, r), r, s)), gray
    assert vec.errors() == 0
    vec.close()


def test_argument_errors_and_cache_warming(tg):
    L, lib = tg._lib.load(), tg._lib
    n = 9
    vec = tg.TreasureGameVec(n, seed=2, autoreset=True)
    out = torch.zeros(n * 62208 + 16, dtype=torch.uint8, device=vec.device)
    p, h, w = ctypes.c_void_p(out.data_ptr()), ctypes.c_int32(), ctypes.c_int32()

    def view(first, count, r, s, ch, ptr=p):
        return L.tg_render_view(vec.handle, first, count, r, s, ch, ptr, None, None)

    assert view(0, n, 1, 8, 1) == lib.TG_E_STATE   # before tg_render_init
    vec.render_init(tg.synthetic_sprites(seed=8))
    for r, s, ch in ((0, 8, 1), (8, 8, 1), (-1, 8, 3), (1, 5, 1), (1, 0, 1), (1, 96, 3), (1, 8, 2),
                     (1, 8, 0)):
        assert view(0, n, r, s, ch) == lib.TG_E_INVAL, (r, s, ch)
    for first, count in ((-1, 2), (0, n + 1), (n - 1, 2), (0, -1)):
        assert view(first, count, 1, 8, 1) == lib.TG_E_INVAL, (first, count)
    assert view(0, n, 1, 8, 1, ctypes.c_void_p(out.data_ptr() + 4)) == lib.TG_E_INVAL   # misaligned
    assert view(0, n, 1, 8, 1, None) == lib.TG_E_INVAL
    for r, s in ((0, 8), (8, 8), (1, 7)):
        assert L.tg_frame_shape_view(vec.handle, r, s, ctypes.byref(h), ctypes.byref(w)) == lib.TG_E_INVAL
    assert L.tg_frame_shape_view(vec.handle, 7, 1, ctypes.byref(h), ctypes.byref(w)) == 0
    assert (h.value, w.value) == (720, 720)
    with pytest.raises(tg.TgError):
        vec.render(view=0)
    with pytest.raises(ValueError):
        vec.render(view=1, out=torch.zeros((n, 18, 18, 1), dtype=torch.uint8, device=vec.device))
    with pytest.raises(ValueError):
        vec.render(view=1, origin=torch.zeros((n, 2), dtype=torch.int64, device=vec.device))
    with pytest.raises(ValueError):
        vec.render(origin=torch.zeros((n, 2), dtype=torch.int32, device=vec.device))
    assert vec.errors() == 0
    # the shared table cache, in both orders: the window call first at scale 8, the whole frame
    # first at scale 4; either way the window is the crop of the whole frame
    for s, view_first in ((8, True), (4, False)):
        if view_first:
            got, org = view_and_origin(vec, 1, s, True)
            whole = vec.render(scale=s, gray=True)
        else:
            whole = vec.render(scale=s, gray=True)
            got, org = view_and_origin(vec, 1, s, True)
        same(got, crop_dev(whole, org, 1, s), "scale %d" % s)
    assert vec.errors() == 0
    vec.close()


def test_python_surface(tg, oracle):
    n, a0 = 32, 0x99
    sprites = tg.synthetic_sprites(seed=12)
    w = tg.ObservationWrapper(tg.TreasureGameVec(n, seed=0, autoreset=True), sprites=sprites,
                              scale=8, gray=True, view=1)
    frames = w.reset()
    assert tuple(frames.shape) == (n, 18, 18, 1)
    for t in range(6):
        frames, rew, valid, done, info = w.step(w.env.policy_actions(t, a0, "masked"))
        assert tuple(frames.shape) == (n, 18, 18, 1) and info["world_state"].shape == (n, 9)
    assert torch.equal(frames, w.env.render(scale=8, gray=True, view=1))
    full = oracle.run_render(0, np.arange(n), 6, a0, 1, True, sprites)
    pos = oracle_positions(oracle, n, 6, a0, 1, True)[:, 6]
    assert np.array_equal(frames.cpu().numpy(), crop0(pool(full, 8, True), origins(pos, 1), 1, 8))
    assert w.env.errors() == 0
    w.close()

    vec = tg.TreasureGameVec(1, seed=3, autoreset=True)
    vec.render_init(sprites)
    vec.reset()
    env = tg.TreasureGame(seed=3)
    env._sprites = sprites
    env.reset()
    one = env.render("rgb_array", view=1)
    assert isinstance(one, np.ndarray) and one.shape == (144, 144, 3)
    np.testing.assert_array_equal(one, vec.render(view=1).cpu().numpy()[0])
    e = oracle.OracleEnv(3)
    np.testing.assert_array_equal(one, crop0(e.render(sprites)[None], origins(
        oracle_positions(oracle, 4, 0, 0, 1, True)[3:4, 0], 1), 1, 1)[0])
    ow = tg.ObservationWrapper(env, sprites=sprites, scale=8, gray=True, view=1)
    first = ow.reset()
    assert first.shape == (18, 18, 1) and first.dtype == np.uint8
    screen, r, d, info = ow.step(1)
    assert screen.shape == (18, 18, 1) and "world_state" in info
    ow.close()
    vec.close()
