"""The learned actor on the device against the path users have without it.

    python scripts/bench_policy_mlp.py [--envs 1048576] [--hidden 64] [--steps 16] [--reps 3]
                                       [--out profiles/policy_mlp.json]

1,048,576 envs, H = 64, tanh, masked, auto-reset.  Legs, alternated in one process, each timed
with device events and the whole set repeated --reps times:
  a  rollout(steps, policy="masked")                      ms per step
  b  per step: observe(), the same network in torch f32 with the same weights, masked softmax,
     inverse-CDF sample, .to(int32), step()                ms per step
  c  rollout(steps, policy="mlp")                          ms per step
  d  policy_mlp alone, --steps launches                    ms per launch
The result is written before any assertion.  The bar: c < b per step in every repetition.
d is reported against the FMA floor (2 * (9H + H*H + 10H) FLOP per env at the 157 TFLOP/s f32
vector peak), c - a beside it.  There is no CPU fallback: without a GPU this fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_treasure_game_amd as tg  # noqa: E402

F32_PEAK = 157e12  # FLOP/s, f32 vector peak of an MI355X
SEED = 0x5EED0001


def seeded_params(h, seed=0):
    r = np.random.RandomState(seed)
    f = np.float32
    return {"obs_scale": np.full(9, 1.0 / 700.0, f), "obs_shift": np.full(9, -0.5, f),
            "w1": (r.randn(h, 9) * np.sqrt(2.0 / 9)).astype(f), "b1": (r.randn(h) * 0.1).astype(f),
            "w2": (r.randn(h, h) * np.sqrt(2.0 / h)).astype(f), "b2": (r.randn(h) * 0.1).astype(f),
            "wp": (r.randn(9, h) * np.sqrt(2.0 / h) * 2).astype(f), "bp": (r.randn(9) * 0.1).astype(f),
            "wv": (r.randn(h) * np.sqrt(2.0 / h) * 2).astype(f), "bv": (r.randn(1) * 0.1).astype(f)}


class TorchActor:
    """the same network and sampling in eager torch, as a user would write it"""

    def __init__(self, p, dev):
        self.p = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
        self.bit = (1 << torch.arange(9, device=dev, dtype=torch.int32))

    def __call__(self, obs, avail):
        p = self.p
        x = obs.to(torch.float32) * p["obs_scale"] + p["obs_shift"]
        a1 = torch.tanh(torch.addmm(p["b1"], x, p["w1"].t()))
        a2 = torch.tanh(torch.addmm(p["b2"], a1, p["w2"].t()))
        logits = torch.addmm(p["bp"], a2, p["wp"].t())
        value = a2 @ p["wv"] + p["bv"]
        allowed = (avail.to(torch.int32).unsqueeze(1) & self.bit) != 0
        allowed = allowed | ~allowed.any(1, keepdim=True)
        logits = logits.masked_fill(~allowed, float("-inf"))
        logp_all = torch.log_softmax(logits, 1)
        cdf = logp_all.exp().cumsum(1)
        u = torch.rand(obs.shape[0], 1, device=obs.device)
        last = 8 - allowed.flip(1).to(torch.int32).argmax(1)
        a = torch.minimum((cdf <= u).sum(1), last)
        logp = logp_all.gather(1, a.unsqueeze(1)).squeeze(1)
        return a.to(torch.int32), logp, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_mlp.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_mlp: no GPU")
    n, h, k = args.envs, args.hidden, args.steps
    params = seeded_params(h)
    vec = tg.TreasureGameVec(n, seed=0, autoreset=True)
    vec.reset()
    vec.set_policy_mlp(params, act="tanh", masked=True)
    actor = TorchActor(params, vec.device)
    t = [0]

    def leg_a():
        vec.rollout(k, t0=t[0], action_seed=SEED, policy="masked")

    def leg_b():
        for _ in range(k):
            a, _, _ = actor(vec.observe(), vec.available_mask())
            vec.step(a)

    def leg_c():
        vec.rollout(k, t0=t[0], action_seed=SEED, policy="mlp")

    def leg_d():
        for s in range(k):
            vec.policy_mlp(t[0] + s, SEED)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
    for fn in legs.values():  # warm every leg
        fn()
        t[0] += k
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / k)
            t[0] += k
    errors = vec.errors()
    flop = 2 * (9 * h + h * h + 10 * h) * n
    floor_ms = flop / F32_PEAK * 1e3
    best = {name: min(v) for name, v in ms.items()}
    result = {"envs": n, "hidden": h, "act": "tanh", "masked": True, "steps": k, "reps": args.reps,
              "unit": {"a": "ms per step", "b": "ms per step", "c": "ms per step",
                       "d": "ms per launch"},
              "ms": {name: [round(x, 4) for x in v] for name, v in ms.items()},
              "ms_best": {name: round(x, 4) for name, x in best.items()},
              "flop_per_launch": flop, "fma_floor_ms": round(floor_ms, 4),
              "d_over_floor": best["d"] / floor_ms, "c_minus_a_ms": best["c"] - best["a"],
              "b_over_c": best["b"] / best["c"], "errors": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert errors == 0
    for rep in range(args.reps):  # the bar: the fused path beats today's path in every repetition
        assert ms["c"][rep] < ms["b"][rep], "rep %d: leg c %.4f ms is not below leg b %.4f ms" % (
            rep, ms["c"][rep], ms["b"][rep])


if __name__ == "__main__":
    main()
