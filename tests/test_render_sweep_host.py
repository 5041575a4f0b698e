"""The synthesized render states of tests/render_sweep.py on the CPU: the builder held to its
conditions (counts, every chunk residue, every item combination, every end-point class and
crossing, a hero over every object cell and shaft), then the product's frame composition
(csrc/tg_render.h through hc_render_states, driven as k_render's lanes are) and its scaled
per-pixel code (csrc/tg_render_scaled.h through hcs_render_states) on every case against
``oracle.render_states``, byte for byte, and the host count of k_render_scaled's queue on the
narrow level (hcs_span_queue_max)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import render_sweep as rs
import state_sweep as ss
from gym_treasure_game_amd import render as R
from test_render_scaled_host import hostscaled, pool  # noqa: F401 (hostscaled: a fixture)

CHUNK = 256
THREADS = min(16, os.cpu_count() or 1)
# cases per level (hero, door, item, handle tiers), recorded; the GPU sweep builds its part
# lists from the totals
COUNTS = {None: (2236, 102, 448, 468), "render_overlap": (2236, 102, 448, 468),
          "corridor": (846, 102, 0, 0), "cascade": (636, 102, 0, 0), "narrow": (102, 102, 0, 0)}
SPRITE_SEED = {None: 41, "render_overlap": 42, "corridor": 43, "cascade": 44, "narrow": 45}
HOST_SCALES = (2, 3, 8, 48)   # and 1 on the handle and item tiers
SCALED_EVERY = 5              # the scaled host sweep's thinning (scaled_cases)
P = ctypes.c_void_p


def _p(a):
    return None if a is None else a.ctypes.data_as(P)


def level_texts(name):
    if name is None:
        return None, None, None   # the built-in level
    return tuple(open(os.path.join(rs.LEVELS[name], f), "rb").read()
                 for f in ("domain.txt", "domain-objects.txt", "domain-interactions.txt"))


def sprites_of(name):
    return R.synthetic_sprites(seed=SPRITE_SEED[name])


def frame_shape(sw):
    return sw.lv["H"] * 48, sw.lv["W"] * 48


def _ins(st):
    return [np.ascontiguousarray(st["pos"], np.int32), np.ascontiguousarray(st["flags"], np.uint32),
            np.ascontiguousarray(st["objs"], np.int32), np.ascontiguousarray(st["ang"], np.float64)]


def hc_render_states(lib, name, st, sprites, shape):
    """frames of the states by the host composition; the TG_ERR_RENDER bit must be clear"""
    lib.hc_render_states.restype = ctypes.c_int
    lib.hc_render_states.argtypes = [P, P, P, ctypes.c_int64] + [P] * 5 + [ctypes.c_int] * 2 + [
        P, ctypes.c_int]
    ins = _ins(st)
    out = np.full((len(ins[0]),) + shape + (3,), 0xA5, np.uint8)
    rc = lib.hc_render_states(*level_texts(name), len(ins[0]), *[_p(a) for a in ins], _p(sprites),
                              sprites.shape[2], sprites.shape[1], _p(out), THREADS)
    assert rc == 0, "hc_render_states: %#x (TG_ERR_RENDER set, or a bad level)" % rc
    return out


def hcs_render_states(lib, name, st, sprites, shape, s, gray, fast=1):
    lib.hcs_render_states.restype = ctypes.c_int
    lib.hcs_render_states.argtypes = [P, P, P, ctypes.c_int64] + [P] * 5 + [ctypes.c_int] * 5 + [
        P, ctypes.c_int]
    ins = _ins(st)
    out = np.full((len(ins[0]), shape[0] // s, shape[1] // s, 1 if gray else 3), 0xA5, np.uint8)
    rc = lib.hcs_render_states(*level_texts(name), len(ins[0]), *[_p(a) for a in ins], _p(sprites),
                               sprites.shape[2], sprites.shape[1], s, 1 if gray else 3, fast,
                               _p(out), THREADS)
    assert rc == 0, "hcs_render_states: %#x (TG_ERR_RENDER set, or a bad level or scale)" % rc
    return out


def span_queue_max(lib, name, st, s):
    """(the most pixels scaled_lookup declines in one span of the states rendered in one call
    at scale s, SQCAP)"""
    lib.hcs_span_queue_max.restype = ctypes.c_int64
    lib.hcs_span_queue_max.argtypes = [P, P, P, ctypes.c_int64] + [P] * 4 + [ctypes.c_int, P]
    ins = _ins(st)
    cap = ctypes.c_int(0)
    n = lib.hcs_span_queue_max(*level_texts(name), len(ins[0]), *[_p(a) for a in ins], s,
                               ctypes.byref(cap))
    assert n >= 0
    return int(n), cap.value


def pool_fast(frames, s, gray):
    """``pool`` (the definition, test_render_scaled_host) in torch's integer arithmetic, on the
    device that holds ``frames`` (a uint8 tensor, or an array: then on the CPU): the sweeps pool
    hundreds of full frames per comparison, which numpy's strided sum takes seconds for.
    test_pool_fast_is_pool holds it to ``pool``."""
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
    n, hp, wp, _ = f.shape
    assert f.dtype == torch.uint8 and hp % s == 0 and wp % s == 0
    if s == 1:   # the mean of one pixel
        out = f
    else:
        sums = f.view(n, hp // s, s, wp // s, s, 3).sum((2, 4), dtype=torch.int32)
        out = ((2 * sums + s * s) // (2 * s * s)).to(torch.uint8)
    return luma_fast(out) if gray else out


def luma_fast(rgb):
    """[..., 3] uint8 averaged RGB -> [..., 1] uint8 gray (test_render_scaled_host.luma)"""
    c = rgb.to(torch.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8)[..., None].to(torch.uint8)


def select(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


# ---- the builder -------------------------------------------------------------------------------
def test_counts_and_determinism(oracle):
    for name, counts in COUNTS.items():
        sw = rs.sweep(name)
        got = tuple(int((sw.tier == t).sum()) for t in range(4))
        print("%s: %d cases %s" % (sw.name, sw.n, got))
        assert got == counts, name
    sw = rs.sweep()
    cols = {k: getattr(sw, k).copy() for k in rs.RenderSweep.COLS + ("flags", "objs", "ang")}
    rs.sweep.cache_clear()
    again = rs.sweep()
    for k, v in cols.items():
        assert np.array_equal(v, getattr(again, k)), k
    ground, air, cells = rs.hero_positions(None)
    assert (len(ground), len(air), len(cells)) == (2191, 45, 70)
    assert tuple(len(rs.hero_positions(n)[2]) for n in ("corridor", "cascade")) == (81, 19)
    # the narrow level's door cells hold positions only with their doors open
    closed, opened = (int(ss.positions(rs.LEVELS["narrow"], b)[0].sum()) for b in (7, 0))
    assert (closed, opened) == (896, 2048)


@pytest.mark.parametrize("name", list(COUNTS))
def test_hero_tier_conditions(oracle, name):
    sw = rs.sweep(name)
    hero = sw.tier_cases("hero")
    assert set((sw.px[hero] % 16).tolist()) == set(range(16))
    # (the hero's edges px - 24 and px + 24 share px's residue + 8: every residue of the 16-pixel
    # period of the chunks' byte offsets, on both edges)
    assert set(sw.facing[hero].tolist()) == {0, 1}
    assert set(sw.bag[hero].tolist()) == set(range(7)) and set(sw.doors[hero].tolist()) == set(range(8))
    up = np.stack([sw.handles & 1, sw.handles >> 1 & 1], 1)
    lo, hi = np.where(up == 1, 0.85, 0.0), np.where(up == 1, 1.0, 0.15)
    assert ((sw.ang >= lo) & (sw.ang <= hi)).all()   # bits and angles agree, in every tier
    door = sw.tier_cases("door")
    for d, (cx, cy, _) in enumerate(sw.lv["door"]):   # the hero in an open door's cell
        mine = door[(sw.px[door] // 48 == cx) & ((sw.py[door] + 24) // 48 == cy)]
        assert len(mine) >= 17 and (sw.doors[mine] >> d & 1 == 0).all(), (name, d)
        assert len(set((sw.px[mine] % 16).tolist())) == 16, (name, d)
    assert len(door) == sum(len(door[(sw.px[door] // 48 == cx) & ((sw.py[door] + 24) // 48 == cy)])
                            for cx, cy, _ in sw.lv["door"])
    if name is None:
        residues = set((sw.py[hero] % 48).tolist())   # standing rows, and the airborne spread
        assert {0, 3, 23, 24, 44, 46, 47} <= residues and len(residues) >= 24, sorted(residues)


@pytest.mark.parametrize("name", rs.ALL_TIERS)
def test_hero_covers_every_object_and_shaft(oracle, name):
    """hero and door tiers: the hero's box over every object's home cell, and over each handle's
    shaft box (at the case's own angle) with the handle up and down"""
    sw = rs.sweep(name)
    idx = sw.tier_cases("hero", "door")
    boxes = [rs.hero_box(int(sw.px[i]), int(sw.py[i])) for i in idx]
    for what, cell in rs.object_boxes(sw.lv).items():
        n = sum(rs.overlaps(b, cell) for b in boxes)
        print("%s: hero over %s in %d cases" % (sw.name, what, n))
        assert n >= 15, (name, what, n)
    for h, (hx, hy, _) in enumerate(sw.lv["handle"]):
        over = [int(sw.handles[i] >> h & 1) for i, b in zip(idx, boxes)
                if rs.overlaps(b, rs.shaft_box((hx, hy), float(sw.ang[i, h])))]
        print("%s: hero over handle %d's shaft in %d cases" % (sw.name, h, len(over)))
        assert len(over) >= 30 and over.count(0) >= 8 and over.count(1) >= 8, (name, h, len(over))


@pytest.mark.parametrize("name", rs.ALL_TIERS)
def test_item_tier_holds_every_combination(oracle, name):
    sw = rs.sweep(name)
    item = sw.tier_cases("item")
    combos = set(zip(sw.doors[item].tolist(), sw.handles[item].tolist(), sw.bolt[item].tolist(),
                     sw.bag[item].tolist()))
    assert len(item) == len(combos) == 8 * 4 * 2 * 7
    ax, ay = rs.away_position(name)
    assert (sw.px[item] == ax).all() and (sw.py[item] == ay).all()
    hero = rs.hero_box(ax, ay)
    assert not any(rs.overlaps(hero, b) for b in rs.object_boxes(sw.lv).values())
    for h, (hx, hy, _) in enumerate(sw.lv["handle"]):
        for a in (0.0, 0.15, 0.85, 1.0):
            assert not rs.overlaps(hero, rs.shaft_box((hx, hy), a))


@pytest.mark.parametrize("name", rs.ALL_TIERS)
def test_handle_tier_classes_and_crossings(oracle, name):
    """against a grid of 150,001 angles per range: the builder's classes are all of the grid's,
    each crossing pair sits astride a change of int(ex) or int(ey) at 1e-7..1e-5 px, and each
    angle has its three hero placements, over the knob and over the shaft where it says so"""
    sw = rs.sweep(name)
    tier = sw.tier_cases("handle")
    for h, (hx, hy, _) in enumerate(sw.lv["handle"]):
        cell = (hx, hy)
        for up, (lo, hi) in enumerate(rs.RANGES):
            angles, nclass = rs.handle_angles(cell, up)
            grid = set()
            for k in range(150001):
                ex, ey = rs.end_point(cell, lo + (hi - lo) * k / 150000.0)
                grid.add((int(ex), int(ey)))
            mine = set(tuple(int(v) for v in rs.end_point(cell, a)) for a, kind in angles if kind == 2)
            assert grid <= mine and nclass == len(mine) >= rs.MIN_CLASSES[up], (name, h, up)
            sides = [a for a, kind in angles if kind in (3, 4)]
            assert len(sides) == 2 * (nclass - 1)
            for below, above in zip(sides[::2], sides[1::2]):
                pb, pa = rs.end_point(cell, below), rs.end_point(cell, above)
                moved = [ax for ax in (0, 1) if int(pb[ax]) != int(pa[ax])]
                assert len(moved) == 1, (name, h, below, above)
                k = max(int(pb[moved[0]]), int(pa[moved[0]]))
                for v in (pb[moved[0]], pa[moved[0]]):
                    assert rs.NEAR_LO <= abs(v - k) <= rs.NEAR_HI, (name, h, below, above, v)
            assert {lo, hi} <= set(a for a, kind in angles if kind == 1)
            # drawline's axis tie |dx| == |dy| (make_layer's major_x) lies at the up range's end:
            # there the line is the exact diagonal, the same pixels whichever axis is major
            ties = [a for a, _ in angles
                    if abs(int(rs.end_point(cell, a)[0]) - (hx * 48 + 24))
                    == abs(int(rs.end_point(cell, a)[1]) - (hy * 48 + 48))]
            assert (1.0 in ties and len(ties) >= 3) if up else not ties, (name, h, up, ties)
            sel = tier[(sw.which[tier] == h) & (sw.handles[tier] >> h & 1 == up)]
            assert len(sel) == 3 * len(angles)
            for a, kind in angles:
                cases = sel[(sw.ang[sel, h] == a) & (sw.kind[sel] == kind)]
                cases = cases[np.argsort(sw.place[cases])]
                assert sw.place[cases].tolist() == [1, 2, 3], (name, h, up, a)
                ex, ey = (int(v) for v in rs.end_point(cell, a))
                away, knob, shaft = (rs.hero_box(int(sw.px[i]), int(sw.py[i])) for i in cases)
                assert not rs.overlaps(away, rs.shaft_box(cell, a))
                assert rs.overlaps(knob, (ex - 4, ex + 5, ey - 4, ey + 5))
                assert rs.overlaps(shaft, (hx * 48 + 21, hx * 48 + 28, hy * 48 + 38, hy * 48 + 47))


# ---- the product's host composition ------------------------------------------------------------
@pytest.mark.parametrize("name", list(COUNTS))
def test_full_size_composition(hostcheck, oracle, name):
    """every case: hc_render_states against oracle.render_states, byte for byte"""
    sw = rs.sweep(name)
    sprites = sprites_of(name)
    for lo in range(0, sw.n, CHUNK):
        hi = min(lo + CHUNK, sw.n)
        st = sw.states(lo, hi, mt=False)
        want = oracle.render_states(st, sprites, level_dir=sw.level_dir)
        got = hc_render_states(hostcheck, name, st, sprites, frame_shape(sw))
        rs.compare_frames(sw, np.arange(lo, hi), got, want, "full size")


def scaled_cases(sw):
    """(the cases of the scaled host sweep at scales 2, 3, 8 and 48, those at scale 1).  The
    first is thinned to every fifth case of the permuted sweep: at every case numpy's pooling of
    the full frames alone took the CPU suite ten minutes; the full-size sweep
    above and the GPU sweep take every case."""
    return np.arange(0, sw.n, SCALED_EVERY), sw.tier_cases("handle", "item")


@pytest.mark.parametrize("name", list(COUNTS))
def test_scaled_composition(hostscaled, oracle, name):  # noqa: F811
    """every fifth case at scales 2, 3, 8 and 48, and the whole handle and item tiers at scale
    1, both channel counts, fast = 1 (the kernel's three paths): against the pooled oracle frames"""
    sw = rs.sweep(name)
    sprites = sprites_of(name)
    whole = sw.states(mt=False)
    for cases, scales in zip(scaled_cases(sw), (HOST_SCALES, (1,))):
        for lo in range(0, len(cases), CHUNK):
            idx = cases[lo:lo + CHUNK]
            st = select(whole, idx)
            full = oracle.render_states(st, sprites, level_dir=sw.level_dir)
            for s in scales:
                rgb = pool_fast(full, s, False)   # pooled once; the gray frame is its luma
                for gray in (False, True):
                    got = hcs_render_states(hostscaled, name, st, sprites, frame_shape(sw), s, gray)
                    rs.compare_frames(sw, idx, got, (luma_fast(rgb) if gray else rgb).numpy(),
                                      "scale %d gray %s" % (s, gray))


def test_pool_fast_is_pool(oracle):
    """the sweeps' pooling (torch, on whichever device holds the frames) against the definition
    in numpy (test_render_scaled_host.pool) on oracle frames: every scale, both channel counts"""
    sw = rs.sweep("cascade")
    st = sw.states(0, 6, mt=False)
    full = oracle.render_states(st, sprites_of("cascade"), level_dir=sw.level_dir)
    for s in (1, 2, 3, 4, 6, 8, 12, 16, 24, 48):
        for gray in (False, True):
            got = pool_fast(full, s, gray)
            assert got.dtype == torch.uint8
            assert np.array_equal(got.numpy(), pool(full, s, gray)), (s, gray)


def test_general_path_on_the_handle_tier(hostscaled, oracle):  # noqa: F811
    """fast = 0 (every box composed at full resolution, what k_render_scaled's inline branch
    runs) on the default level's handle tier at scales 1 and 3"""
    sw = rs.sweep()
    sprites = sprites_of(None)
    idx = sw.tier_cases("handle")[:96]
    st = select(sw.states(mt=False), idx)
    full = oracle.render_states(st, sprites, level_dir=sw.level_dir)
    for s in (1, 3):
        got = hcs_render_states(hostscaled, None, st, sprites, frame_shape(sw), s, False, fast=0)
        rs.compare_frames(sw, idx, got, pool_fast(full, s, False).numpy(), "general path, scale %d" % s)


def narrow_queue_maxima(lib):
    """{scale: hcs_span_queue_max} of the narrow level's sweep rendered in one call"""
    sw = rs.sweep("narrow")
    st = sw.states(mt=False)
    out = {}
    for s in (1, 2, 3, 4, 6, 8, 12, 16, 24, 48):
        out[s], cap = span_queue_max(lib, "narrow", st, s)
        assert cap == 1024
    return out


def test_narrow_level_overflows_the_queue(hostscaled):  # noqa: F811
    """the narrow level's cases, rendered in one call, leave more than SQCAP declined boxes in
    some span at scales 1 and 2 (k_render_scaled composes the excess inline); the default level
    stays below it"""
    got = narrow_queue_maxima(hostscaled)
    print("narrow level, declined boxes in the worst span per scale: %s" % got)
    assert got[1] > 1024 and got[2] > 1024, got
    sw = rs.sweep()
    st = sw.states(0, 512, mt=False)
    for s in (1, 2, 8):
        n, _ = span_queue_max(hostscaled, None, st, s)
        assert 0 < n < 1024, (s, n)
