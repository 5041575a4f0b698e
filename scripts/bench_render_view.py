"""Agent-centred windows against the ways to the same pixels without them.

    python scripts/bench_render_view.py [--envs 65536] [--big 1048576] [--launches 20]
                                        [--reps 3] [--legs abcdef] [--out profiles/render_view.json]

Envs after 25 uniform steps.  Legs, alternated in one process, each timed with device events
over --launches launches and the whole set repeated --reps times:
  a  tg_render_scaled, scale 8 gray: the whole pooled frame, the only way to these pixels before
  b  a, then the gather of the radius-1 window per env a user writes today in torch
  c  tg_render_view, radius 1, scale 8, gray   (18 x 18 x 1 = 324 B per env)
  d  tg_render_view, radius 2, scale 4, rgb    (60 x 60 x 3 = 10,800 B)
  e  tg_render_view, radius 1, scale 1, rgb    (144 x 144 x 3 = 62,208 B)
  f  c at --big envs
Per leg: ms per launch, frames/s, algorithmic bytes (output + 32 B of state per env) and the
resulting bytes/s as a share of the measured 6.95 TB/s fill ceiling (leg b gets
no byte rate: its whole-frame intermediate is not in those bytes).  The result is written before
anything is asserted.  Then the bar: leg c's frames equal leg b's, and leg c takes less time per
launch than leg a in every repetition of the same run.  There is no CPU fallback: without a GPU
this fails.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_treasure_game_amd as tg  # noqa: E402

FILL_CEILING = 6.95e12  # B/s, torch.fill_ of the C5 frame buffer
SCALE, RADIUS = 8, 1


def stepped(n, sprites, steps=25):
    vec = tg.TreasureGameVec(n, seed=0, autoreset=True)
    vec.render_init(sprites)
    vec.reset()
    for t in range(steps):
        vec.step(vec.policy_actions(t, 0xC5, "uniform"))
    return vec


def window_origins(vec, r):
    """int64 [n, 2] (ox, oy) in cells from the env positions, as a user computes them"""
    pos = torch.as_tensor(vec.read_state()["pos"], device=vec.device).long()
    return torch.stack([torch.div(pos[:, 0], 48, rounding_mode="floor") - r,
                        torch.div(pos[:, 1] + 24, 48, rounding_mode="floor") - r], 1)


def torch_window(frames, org, r, cs, out):
    """[n, h, w, 1] u8 pooled frames -> [n, k, k, 1] windows at origins org (cells), zero outside:
    pad by r cells, then one gather per env (the hero's cell is inside the level)."""
    k, p = cs * (2 * r + 1), cs * r
    padded = F.pad(frames[..., 0], (p, p, p, p))
    ar = torch.arange(k, device=frames.device)
    ys = (org[:, 1] * cs + p)[:, None] + ar
    xs = (org[:, 0] * cs + p)[:, None] + ar
    n = torch.arange(frames.shape[0], device=frames.device)
    out[..., 0] = padded[n[:, None, None], ys[:, :, None], xs[:, None, :]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="abcdef")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_view.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_view: no GPU")
    sprites = tg.synthetic_sprites(seed=55)
    n = args.envs
    vec = stepped(n, sprites)
    dev = vec.device
    cs = 48 // SCALE

    def buf(count, shape):
        return torch.empty((count,) + shape, dtype=torch.uint8, device=dev)

    legs = {}
    whole = buf(n, vec.frame_shape_scaled(SCALE, True))
    win_shape = vec.frame_shape_view(RADIUS, SCALE, True)
    if "a" in args.legs:
        legs["a"] = (lambda: vec.render(out=whole, scale=SCALE, gray=True), n, whole[0].numel())
    if "b" in args.legs:
        org = window_origins(vec, RADIUS)
        gathered = buf(n, win_shape)
        legs["b"] = (lambda: torch_window(vec.render(out=whole, scale=SCALE, gray=True), org, RADIUS,
                                          cs, gathered), n, gathered[0].numel())
    if "c" in args.legs:
        win = buf(n, win_shape)
        legs["c"] = (lambda: vec.render(out=win, scale=SCALE, gray=True, view=RADIUS), n,
                     win[0].numel())
    if "d" in args.legs:
        wd = buf(n, vec.frame_shape_view(2, 4))
        legs["d"] = (lambda: vec.render(out=wd, scale=4, view=2), n, wd[0].numel())
    if "e" in args.legs:
        we = buf(n, vec.frame_shape_view(1, 1))
        legs["e"] = (lambda: vec.render(out=we, scale=1, view=1), n, we[0].numel())
    if "f" in args.legs:
        bigvec = stepped(args.big, sprites)
        bigbuf = buf(args.big, win_shape)
        legs["f"] = (lambda: bigvec.render(out=bigbuf, scale=SCALE, gray=True, view=RADIUS),
                     args.big, bigbuf[0].numel())
    legs = {k: legs[k] for k in args.legs if k in legs}

    for fn, _, _ in legs.values():  # warm every shape (and build the scales' tables)
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, (fn, _, _) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / args.launches)
    frames_equal = None
    if "b" in legs and "c" in legs:
        frames_equal = bool(torch.equal(win, gathered))

    result = {"envs": n, "big_envs": args.big, "launches": args.launches, "reps": args.reps,
              "fill_ceiling_bytes_per_s": FILL_CEILING, "c_frames_equal_b": frames_equal,
              "errors": int(vec.errors()), "legs": {}}
    for k, (_, count, fb) in legs.items():
        best = min(ms[k])
        nbytes = count * (fb + 32)
        result["legs"][k] = {"envs": count, "frame_bytes": fb,
                             "ms_per_launch": [round(x, 4) for x in ms[k]],
                             "ms_best": round(best, 4), "frames_per_s": count / (best * 1e-3)}
        if k != "b":  # b's whole-frame intermediate is not in these bytes: no rate for it
            result["legs"][k].update({"bytes_per_launch": nbytes,
                                      "bytes_per_s": nbytes / (best * 1e-3),
                                      "share_of_fill_ceiling": nbytes / (best * 1e-3) / FILL_CEILING})
    L = result["legs"]
    for num, den in (("a", "c"), ("b", "c")):
        if num in L and den in L:
            result["ratio_%s_over_%s" % (num, den)] = L[num]["ms_best"] / L[den]["ms_best"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    # the bar: the window kernel's frames are the gathered ones, and it is faster than rendering
    # the whole pooled frame in every repetition of the same run
    assert result["errors"] == 0
    if frames_equal is not None:
        assert frames_equal, "leg c's frames differ from leg b's"
    if "a" in L and "c" in L:
        for rep, (ta, tc) in enumerate(zip(ms["a"], ms["c"])):
            assert tc < ta, "repetition %d: leg c (%s ms) is not faster than leg a (%s ms)" % (
                rep, tc, ta)


if __name__ == "__main__":
    main()
