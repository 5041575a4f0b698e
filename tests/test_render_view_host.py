"""Agent-centred windows on the CPU: the product's per-pixel window code
(csrc/tg_render_view.h, host-only build in tests/native_view) against ``crop0(pool(F))`` — the
definition in include/tg_amd.h restated in numpy: the zero-padded crop, at the window's origin, of
the pooled oracle frame.  Every comparison is byte-exact, with the fast paths (pooled static
layer, pooled tiles) on and off; the origins are held to the oracle's positions.  The host build
asserts that every table index it forms lies inside its table (a call returns -3 otherwise), and
the same source runs as a stand-alone program under the host AddressSanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import render_sweep as rs
import state_sweep as ss
from conftest import ROOT
from gym_treasure_game_amd import render as R
from test_render_scaled_host import full_shape, level_texts, pool

RADII = (1, 2, 3, 7)
CSRC = os.path.join(ROOT, "gym-treasure-game_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
THREADS = min(16, os.cpu_count() or 1)
P = ctypes.c_void_p


def _p(a):
    return None if a is None else a.ctypes.data_as(P)


def side(r, s):
    return 48 * (2 * r + 1) // s


def origins(pos, r):
    """[n, 2] (ox, oy) in cells of positions [n, 2]: the definition, with floor division"""
    pos = np.asarray(pos, np.int64)
    return np.stack([pos[:, 0] // 48 - r, (pos[:, 1] + 24) // 48 - r], 1).astype(np.int32)


def crop0(frames, org, r, s):
    """The definition: [n, h, w, c] frames pooled at scale s and each one's window origin
    [n, 2] in cells -> [n, side, side, c], zero outside the frame."""
    n, h, w, c = frames.shape
    k, cs = side(r, s), 48 // s
    out = np.zeros((n, k, k, c), np.uint8)
    for i in range(n):
        x0, y0 = int(org[i, 0]) * cs, int(org[i, 1]) * cs
        xa, xb, ya, yb = max(x0, 0), min(x0 + k, w), max(y0, 0), min(y0 + k, h)
        if xa < xb and ya < yb:
            out[i, ya - y0:yb - y0, xa - x0:xb - x0] = frames[i, ya:yb, xa:xb]
    return out


def leaves(org, r, shape):
    """per window [n]: bits 1 left, 2 right, 4 top, 8 bottom where it leaves the frame of
    ``shape`` = (Hpx, Wpx), 16 where it lies wholly outside"""
    ox, oy, k = org[:, 0].astype(np.int64), org[:, 1].astype(np.int64), 2 * r + 1
    H, W = shape[0] // 48, shape[1] // 48
    out = (ox < 0) * 1 + (ox + k > W) * 2 + (oy < 0) * 4 + (oy + k > H) * 8
    return out + ((ox + k <= 0) | (ox >= W) | (oy + k <= 0) | (oy >= H)) * 16


def oracle_positions(O, n, steps, a0, policy, autoreset, level_dir=None):
    """[n, steps + 1, 2] (playerx, playery) of envs 0..n-1 from the oracle's observations"""
    hp, wp = full_shape(level_dir)
    obs = O.run(0, 0, n, steps, a0, policy, autoreset, level_dir=level_dir)["obs"]
    return np.stack([np.rint(obs[..., 0] * wp), np.rint(obs[..., 1] * hp)], -1).astype(np.int64)


@pytest.fixture(scope="module")
def hostview():
    """Host-only build of the window's per-pixel code (tests/native_view)."""
    d = os.path.join(ROOT, "tests", "native_view")
    subprocess.check_call(["make", "-s", "-C", d])
    L = ctypes.CDLL(os.path.join(d, "libtg_hostcheck_view.so"))
    i = ctypes.c_int
    L.hcv_render_run.restype = i
    L.hcv_render_run.argtypes = [P, P, P, ctypes.c_uint64, P, ctypes.c_int64, i, ctypes.c_uint64,
                                 i, i, P, i, i, i, i, i, i, P, P]
    L.hcv_render_states.restype = i
    L.hcv_render_states.argtypes = [P, P, P, ctypes.c_int64] + [P] * 5 + [i] * 6 + [P, P, i]
    L.hcv_view_group.restype = i
    L.hcv_view_group.argtypes = [i]
    return L


def hcv_run(lib, envs, steps, a0, policy, autoreset, sprites, r, s, gray, fast=1, level_dir=None):
    """(windows, origins) of seeded envs by the host code; TG_ERR_RENDER must be clear"""
    envs = np.ascontiguousarray(envs, np.int64)
    out = np.full((len(envs), side(r, s), side(r, s), 1 if gray else 3), 0xA5, np.uint8)
    org = np.full((len(envs), 2), -9999, np.int32)
    rc = lib.hcv_render_run(*level_texts(level_dir), 0, _p(envs), len(envs), steps, a0, policy,
                            int(autoreset), _p(sprites), sprites.shape[2], sprites.shape[1], r, s,
                            1 if gray else 3, fast, _p(out), _p(org))
    assert rc == 0, "hcv_render_run: %d (-3: an index outside its table)" % rc
    return out, org


def hcv_states(lib, level_dir, st, sprites, r, s, gray, fast=1):
    """(windows, origins, TG_ERR_RENDER bits) of given states by the host code"""
    ins = [np.ascontiguousarray(st["pos"], np.int32), np.ascontiguousarray(st["flags"], np.uint32),
           np.ascontiguousarray(st["objs"], np.int32), np.ascontiguousarray(st["ang"], np.float64)]
    n = len(ins[0])
    out = np.full((n, side(r, s), side(r, s), 1 if gray else 3), 0xA5, np.uint8)
    org = np.full((n, 2), -9999, np.int32)
    rc = lib.hcv_render_states(*level_texts(level_dir), n, *[_p(a) for a in ins], _p(sprites),
                               sprites.shape[2], sprites.shape[1], r, s, 1 if gray else 3, fast,
                               _p(out), _p(org), THREADS)
    assert rc >= 0, "hcv_render_states: %d (-3: an index outside its table)" % rc
    return out, org, rc


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    if len(bad):
        i = int(bad[0])
        px = np.argwhere((got[i] != want[i]).any(-1))
        raise AssertionError("%s: %d of %d windows differ; first: %d, %d pixels, first at (y, x) = %s"
                             ": got %s, want %s" % (what, len(bad), len(want), i, len(px),
                                                    tuple(px[0]), got[i][tuple(px[0])].tolist(),
                                                    want[i][tuple(px[0])].tolist()))


def check_run(lib, full, pos, envs, steps, a0, sprites, cases, level_dir=None):
    """seeded envs: every (r, s) of ``cases``, both channel counts, fast paths on and off"""
    for r, s in cases:
        want_org = origins(pos, r)
        rgb = pool(full, s, False)
        for gray in (False, True):
            want = crop0(pool(full, s, True) if gray else rgb, want_org, r, s)
            for fast in (1, 0):
                got, org = hcv_run(lib, envs, steps, a0, 1, True, sprites, r, s, gray, fast, level_dir)
                assert np.array_equal(org, want_org), (r, s)
                same(got, want, "r %d scale %d gray %s fast %d step %d" % (r, s, gray, fast, steps))


# ---- synthesized states ------------------------------------------------------------------------
def synth_positions(shape=(624, 672)):
    """[(px, py, what)]: positions far outside what a rollout stops on.  Any int16 pair is a
    position tg_write_state accepts."""
    hp, wp = shape
    out = []
    for px in (144, 191):               # px = 0 and 47 (mod 48)
        for py in (119, 120):           # py = 23 and 24 (mod 48): either side of yc's switch
            out.append((px, py, "px %% 48 = %d, py %% 48 = %d" % (px % 48, py % 48)))
    for cx, cy in ((0, 0), (wp // 48 - 1, 0), (0, hp // 48 - 1), (wp // 48 - 1, hp // 48 - 1)):
        out.append((cx * 48 + 24, cy * 48, "corner cell (%d, %d)" % (cx, cy)))
    out += [(-10, 200, "the sprite across the left edge"), (-30, 200, "outside on the left"),
            (-100, 200, "outside on the left, sprite and all"),
            (wp + 10, 200, "the sprite across the right edge"), (wp + 100, 200, "outside on the right"),
            (300, -30, "the sprite across the top edge"), (300, -60, "outside at the top"),
            (300, hp - 20, "the sprite across the bottom edge"), (300, hp + 40, "outside at the bottom"),
            (-60, -80, "outside at the top left"), (wp + 60, hp + 60, "outside at the bottom right"),
            (-2000, 300, "window wholly outside, left"), (300, 3000, "window wholly outside, below"),
            (-32768, -32768, "the least int16 pair"), (32767, 32767, "the greatest int16 pair")]
    return out


def synth_states(mt=False):
    """(states, labels): synth_positions, each facing both ways, on the default level; the other
    columns are those of tests/render_sweep.py's item tier (every combination of door bits,
    handle bits with consistent angles, bolt and bag state) taken in turn.  Needs the oracle
    built (the builder reads its position tables)."""
    sw = rs.sweep(None)
    item = sw.tier_cases("item")
    pos, facing, labels = [], [], []
    for px, py, what in synth_positions():
        for f in (0, 1):
            pos.append((px, py)), facing.append(f), labels.append("%s, facing %d" % (what, f))
    n = len(pos)
    idx = item[(np.arange(n) * 13) % len(item)]
    st = {"pos": np.array(pos, np.int32),
          "flags": np.ascontiguousarray(ss.pack_flags(np.array(facing, np.int32), sw.doors[idx],
                                                      sw.handles[idx], sw.bolt[idx], sw.bag[idx]),
                                        np.uint32),
          "objs": np.ascontiguousarray(sw.objs[idx]), "ang": np.ascontiguousarray(sw.ang[idx]),
          "ep": np.zeros((n, 2), np.int32)}
    if mt:   # any valid words do (all zero would be MT19937's fixed point)
        st["mt"], st["mt_pos"] = np.zeros((n, 624), np.uint32), np.zeros(n, np.uint32)
        st["mt"][:, 0] = 0x80000000
    return st, labels


SYNTH_SPRITES = 77
SYNTH_CASES = [(r, s) for r in RADII for s in (1, 8, 48)]


# ---- tests -------------------------------------------------------------------------------------
def test_crop0_is_the_definition():
    f = np.arange(1, 2 * 96 * 144 * 1 + 1, dtype=np.uint32).reshape(2, 96, 144, 1).astype(np.uint8)
    org = np.array([[0, -1], [2, 1]], np.int32)   # r = 1: 3 x 3 cells of a 3 x 2-cell frame
    got = crop0(f, org, 1, 1)
    assert got.shape == (2, 144, 144, 1)
    assert not got[0, :48].any() and np.array_equal(got[0, 48:], f[0])
    assert np.array_equal(got[1, :48, :48], f[1, 48:, 96:]) and not got[1, 48:].any()
    assert not got[1, :, 48:].any()
    half = crop0(f[:, ::2, ::2], org, 1, 2)      # the same origins at scale 2
    assert np.array_equal(half, got[:, ::2, ::2])
    assert leaves(org, 1, (96, 144)).tolist() == [4, 2 + 8]
    assert leaves(np.array([[3, 0], [-3, 0], [0, 2], [-2, 0]], np.int32), 1, (96, 144)).tolist() == [
        2 + 8 + 16, 1 + 8 + 16, 8 + 16, 1 + 8]
    assert origins([[0, 23], [-1, 24], [47, -25], [48, -24]], 1).tolist() == [
        [-1, -1], [-2, 0], [-1, -2], [0, -1]]


def test_header_compiles_alone(tmp_path):
    assert os.path.exists(os.path.join(CSRC, "tg_render_view.h"))
    unit = tmp_path / "tg_render_view_unit.hip"
    unit.write_text('#include "%s"\n' % os.path.join(CSRC, "tg_render_view.h"))
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-fsyntax-only", "-std=c++17",
                    "-Wno-unused-command-line-argument", str(unit)], check=True)


def test_header_and_exports(tg):
    import re
    src = open(os.path.join(ROOT, "include", "tg_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("tg_frame_shape_view", "tg_render_view"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in tg._lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", tg._lib.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"tg_frame_shape_view", "tg_render_view"} <= exported


def test_group_sizes(hostview):
    """k_render_view's envs per group: a multiple of 4 (a group starts on a dword even with 9-B
    frames), more envs as the frame shrinks"""
    got = {fp: hostview.hcv_view_group(fp) for fp in (9, 324, 900, 1024, 1025, 3600, 20736, 518400)}
    assert all(g % 4 == 0 and g >= 4 for g in got.values()), got
    assert got[324] == 12 and got[9] >= 12 and got[3600] == got[518400] == 4, got


@pytest.mark.parametrize("steps", [0, 7, 60])
def test_default_level(hostview, oracle, steps):
    """24 envs, masked auto-reset policy: r in 1, 2, 3, 7 x scales 1, 8, 48 (and 3, 4 at r = 1,
    2), both channel counts, fast and general paths"""
    sprites = R.synthetic_sprites(seed=steps + 11)
    envs = np.arange(24) * 37
    a0 = 0x52
    full = oracle.run_render(0, envs, steps, a0, 1, True, sprites)
    pos = oracle_positions(oracle, int(envs[-1]) + 1, steps, a0, 1, True)[envs, steps]
    cases = [(r, s) for r in RADII for s in (1, 8, 48)] + [(1, 3), (2, 4)]
    check_run(hostview, full, pos, envs, steps, a0, sprites, cases)


@pytest.mark.parametrize("name,steps,cases", [
    ("render_overlap", 20, ((1, 4), (2, 8), (3, 1))),
    ("corridor", 6, ((3, 8), (3, 1), (1, 48), (7, 8))),   # 44 x 5 cells: r = 3 is taller than it
    ("narrow", 5, ((1, 1), (2, 8), (7, 48))),             # 8 x 3 cells
    ("cascade", 9, ((1, 8), (2, 2), (3, 48)))])
def test_other_levels(hostview, oracle, name, steps, cases):
    level_dir = rs.LEVELS[name]
    sprites = R.synthetic_sprites(seed=len(name))
    envs = np.arange(12)
    full = oracle.run_render(0, envs, steps, 9, 1, True, sprites, level_dir=level_dir)
    pos = oracle_positions(oracle, 12, steps, 9, 1, True, level_dir)[envs, steps]
    if name == "corridor":   # 7 cells of window over 5 of level: none fits
        assert (leaves(origins(pos, 3), 3, full.shape[1:3]) & 12).all()
    check_run(hostview, full, pos, envs, steps, 9, sprites, cases, level_dir)
    # and the level's synthesized hero tier, thinned, through render_states
    sw = rs.sweep(name)
    idx = sw.tier_cases("hero", "door")[::9]
    st = {k: np.ascontiguousarray(v[idx]) for k, v in sw.states(mt=False).items()}
    r, s = cases[0]
    if name == "corridor":   # every other hero lifted to the middle row: out above and below at once
        st["pos"][::2, 1] = 100
        assert (leaves(origins(st["pos"], r), r, full.shape[1:3])[::2] & 12 == 12).all()
    full = oracle.render_states(st, sprites, level_dir=level_dir)
    want = crop0(pool(full, s, False), origins(st["pos"], r), r, s)
    got, org, err = hcv_states(hostview, level_dir, st, sprites, r, s, False)
    assert err == 0 and np.array_equal(org, origins(st["pos"], r))
    same(got, want, "level %s sweep, r %d scale %d" % (name, r, s))


def test_synthesized_states_cover_the_edges(oracle):
    st, labels = synth_states()
    pos = st["pos"].astype(np.int64)
    assert {0, 47} <= set((pos[:, 0] % 48).tolist()) and {23, 24} <= set((pos[:, 1] % 48).tolist())
    a, b = (pos[:, 0] == 144) & (pos[:, 1] == 119), (pos[:, 0] == 144) & (pos[:, 1] == 120)
    assert a.any() and b.any()
    assert (origins(pos[b], 1)[:, 1] - origins(pos[a], 1)[:, 1] == 1).all()   # yc's switch
    cells = set(zip((pos[:, 0] // 48).tolist(), ((pos[:, 1] + 24) // 48).tolist()))
    assert {(0, 0), (13, 0), (0, 12), (13, 12)} <= cells
    assert all(set(st["flags"][(pos == p).all(1)] >> 5 & 1) == {0, 1} for p in pos)   # both facings
    xc, yc = pos[:, 0] // 48, (pos[:, 1] + 24) // 48
    assert (xc < 0).any() and (xc > 13).any() and (yc < 0).any() and (yc > 12).any()
    for r in RADII:
        where = leaves(origins(pos, r), r, (624, 672))
        assert (where & 16).any() and all((where & b).any() for b in (1, 2, 4, 8)), r
    assert len(labels) == len(pos) == 2 * len(synth_positions())


def test_synthesized_states(hostview, oracle):
    """the hero on, across and far off every edge: every (r, s), both channel counts, fast paths
    on and off, against the crop of the pooled oracle frames; no index leaves its table"""
    st, labels = synth_states()
    sprites = R.synthetic_sprites(seed=SYNTH_SPRITES)
    full = oracle.render_states(st, sprites)
    for r, s in SYNTH_CASES:
        want_org = origins(st["pos"], r)
        for gray in (False, True):
            want = crop0(pool(full, s, gray), want_org, r, s)
            for fast in (1, 0):
                if s == 1 and r == 7 and (gray or not fast):
                    continue   # 1.5-MB frames: the general path and gray at r = 1, 2, 3 cover them
                got, org, err = hcv_states(hostview, None, st, sprites, r, s, gray, fast)
                assert err == 0 and np.array_equal(org, want_org), (r, s)
                try:
                    same(got, want, "r %d scale %d gray %s fast %d" % (r, s, gray, fast))
                except AssertionError as e:
                    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
                    raise AssertionError("%s (%s)" % (e, labels[int(bad[0])]))


def test_bad_arguments_are_rejected(hostview):
    sprites = R.synthetic_sprites(seed=1)
    envs = np.zeros(1, np.int64)
    out = np.zeros(1 << 16, np.uint8)
    for r, s, ch in ((0, 8, 3), (8, 8, 3), (-1, 8, 1), (1, 5, 3), (1, 96, 3), (1, 8, 2)):
        assert hostview.hcv_render_run(None, None, None, 0, _p(envs), 1, 0, 0, 1, 1, _p(sprites),
                                       32, 32, r, s, ch, 1, _p(out), None) == -2


def test_no_index_leaves_its_table_under_the_host_sanitizer():
    """tests/native_view's source as a stand-alone program (its own main) under the host
    AddressSanitizer and UBSan: windows of positions on, across and far off every edge of the
    built-in level.  Host code only."""
    d = os.path.join(ROOT, "tests", "native_view")
    out = subprocess.run(["make", "-s", "-C", d, "asan"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "every index inside its table" in out.stdout, out.stdout[-3000:]
