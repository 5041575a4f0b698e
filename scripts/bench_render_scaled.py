"""Downscaled renderer against the full-size one.

    python scripts/bench_render_scaled.py [--envs 65536] [--big 1048576] [--launches 20]
                                          [--reps 3] [--legs abcde] [--out profiles/render_scaled.json]

Legs, alternated in one process, each timed with device events over --launches launches and
the whole set repeated --reps times:
  a  tg_render, full size
  b  a, then the average pooling a user writes today in torch (chunked to fit memory)
  c  tg_render_scaled, scale 8 rgb
  d  tg_render_scaled, scale 8 gray
  e  c at --big envs
Per leg: ms per launch, frames/s, algorithmic bytes (output + 32 B of state per env) and the
resulting bytes/s as a share of the measured 6.95 TB/s fill ceiling.
(Leg b gets no byte rate: its full-size intermediate is not in those bytes.)  After writing the
result it asserts the speed bar: legs c and d each take less time per launch than leg a in
every repetition of the same run.  There is no CPU fallback: without a GPU this fails.
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
SCALE = 8
POOL_CHUNK = 1024  # envs per torch pooling chunk: 1.3 GB of u8 -> 5.2 GB of float32


def stepped(n, sprites, steps=25):
    vec = tg.TreasureGameVec(n, seed=0, autoreset=True)
    vec.render_init(sprites)
    vec.reset()
    for t in range(steps):
        vec.step(vec.policy_actions(t, 0xC5, "uniform"))
    return vec


def torch_pool(full, out):
    """[n, 624, 672, 3] u8 -> [n, 78, 84, 3] u8, the mean with halves rounded up."""
    for i in range(0, full.shape[0], POOL_CHUNK):
        x = full[i:i + POOL_CHUNK].permute(0, 3, 1, 2).float()
        y = F.avg_pool2d(x, SCALE).add_(0.5).to(torch.uint8)
        out[i:i + POOL_CHUNK].copy_(y.permute(0, 2, 3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="abcde")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_scaled.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_scaled: no GPU")
    sprites = tg.synthetic_sprites(seed=55)
    n = args.envs
    vec = stepped(n, sprites)
    full_shape = vec.frame_shape
    rgb_shape, gray_shape = vec.frame_shape_scaled(SCALE), vec.frame_shape_scaled(SCALE, True)
    dev = vec.device

    def buf(count, shape):
        return torch.empty((count,) + shape, dtype=torch.uint8, device=dev)

    legs = {}
    if "a" in args.legs or "b" in args.legs:
        full = buf(n, full_shape)
        legs["a"] = (lambda: vec.render(out=full), n, full[0].numel())
    if "b" in args.legs:
        pooled = buf(n, rgb_shape)
        legs["b"] = (lambda: torch_pool(vec.render(out=full), pooled), n, pooled[0].numel())
    if "c" in args.legs:
        small = buf(n, rgb_shape)
        legs["c"] = (lambda: vec.render(out=small, scale=SCALE), n, small[0].numel())
    if "d" in args.legs:
        gray = buf(n, gray_shape)
        legs["d"] = (lambda: vec.render(out=gray, scale=SCALE, gray=True), n, gray[0].numel())
    if "e" in args.legs:
        bigvec = stepped(args.big, sprites)
        bigbuf = buf(args.big, rgb_shape)
        legs["e"] = (lambda: bigvec.render(out=bigbuf, scale=SCALE), args.big, bigbuf[0].numel())
    legs = {k: legs[k] for k in args.legs if k in legs}

    for fn, _, _ in legs.values():  # warm every shape (and build the scale's tables)
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
    if "a" in legs and "c" in legs:  # the timed outputs agree: pooled full frames == scaled
        idx = torch.arange(0, n, max(1, n // 256), device=dev)
        want = torch_pool(full.index_select(0, idx), buf(len(idx), rgb_shape))
        assert torch.equal(small.index_select(0, idx), want), "scaled frames differ from pooled"

    result = {"envs": n, "big_envs": args.big, "scale": SCALE, "launches": args.launches,
              "reps": args.reps, "fill_ceiling_bytes_per_s": FILL_CEILING, "legs": {}}
    for k, (_, count, fb) in legs.items():
        best = min(ms[k])
        nbytes = count * (fb + 32)
        result["legs"][k] = {"envs": count, "ms_per_launch": [round(x, 4) for x in ms[k]],
                             "ms_best": round(best, 4), "frames_per_s": count / (best * 1e-3)}
        if k != "b":  # b's full-size intermediate is not in these bytes: no rate for it
            result["legs"][k].update({"bytes_per_launch": nbytes,
                                      "bytes_per_s": nbytes / (best * 1e-3),
                                      "share_of_fill_ceiling": nbytes / (best * 1e-3) / FILL_CEILING})
    L = result["legs"]
    for num, den in (("a", "c"), ("b", "c"), ("a", "d")):
        if num in L and den in L:
            result["ratio_%s_over_%s" % (num, den)] = L[num]["ms_best"] / L[den]["ms_best"]
    assert vec.errors() == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    # the speed bar: each scaled leg takes less time per launch than the full-size render of
    # the same run, in every repetition
    for k in "cd":
        if "a" in L and k in L:
            assert max(ms[k]) < min(ms["a"]), "leg %s (%s ms) is not faster than leg a (%s ms)" % (
                k, ms[k], ms["a"])


if __name__ == "__main__":
    main()
