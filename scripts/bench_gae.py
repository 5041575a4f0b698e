#!/usr/bin/env python3
"""Advantages on the device against what a user has without them (DESIGN.md §13,
profiles/gae.json).

    PARENT=gym-treasure-game_amd/libtg_amd_parent.so python scripts/bench_gae.py
    MODE=trace rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/bench_gae.py

1,048,576 envs, H = 64 tanh masked, auto-reset, limit 50, episode ages staggered through
write_state (length g % 50, so about 1/50 of the envs truncate in every step), K = 128.  Legs,
alternated in one process, each timed with device events, the whole set repeated REPS times; ms
per rollout of K steps:
  a  rollout(K, "mlp") on the parent commit's build (PARENT: a libtg_amd.so built from it, as
     scripts/ab.py's variants; without it the leg is left out)
  b  rollout(K, "mlp") on this build
  c  rollout(K, "mlp", gae=(0.99, 0.95))
  d  b, then policy_mlp(t) for the bootstrap value and the reverse loop in torch over [N]
     slices that INTEGRATION.md described (it cannot bootstrap the truncated envs at all)
  e  gae() alone on a rollout's rows (k_gae): ms and bytes/s against the copy ceiling
Every leg has a handle of its own, and every handle runs one K-step rollout per repetition from
the same seed and staggered ages, so the legs of a repetition step the same states.  The result
is written before any assertion.  The bars: c - b < d - b in every repetition, and b within
the spread a shows against itself.
MODE=trace: three `c` legs only (for a kernel trace, in a run of its own);
MERGE_TRACE=<rocprofv3's output database>: adds that trace's per-kernel times to the result."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TG_AB_LIB"] = "1"  # (the parent's build lacks the new entry points)
import gym_treasure_game_amd as tg  # noqa: E402
from gym_treasure_game_amd import _lib  # noqa: E402

N = int(os.environ.get("N", 1 << 20))
K = int(os.environ.get("K", 128))
REPS = int(os.environ.get("REPS", 3))
H, LIMIT, SEED, A0 = 64, 50, 0, 0x5EED0001
GAMMA, LAM = 0.99, 0.95
COPY_CEILING = 6.29e12  # B/s, the measured float4 copy of an MI355X
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "gae.json"))


def seeded_params(h, seed=0):
    r = np.random.RandomState(seed)
    f = np.float32
    return {"obs_scale": np.full(9, 1.0 / 700.0, f), "obs_shift": np.full(9, -0.5, f),
            "w1": (r.randn(h, 9) * np.sqrt(2.0 / 9)).astype(f), "b1": (r.randn(h) * 0.1).astype(f),
            "w2": (r.randn(h, h) * np.sqrt(2.0 / h)).astype(f), "b2": (r.randn(h) * 0.1).astype(f),
            "wp": (r.randn(9, h) * np.sqrt(2.0 / h) * 2).astype(f), "bp": (r.randn(9) * 0.1).astype(f),
            "wv": (r.randn(h) * np.sqrt(2.0 / h) * 2).astype(f), "bv": (r.randn(1) * 0.1).astype(f)}


def fresh(path):
    """a handle on the library at `path`: warmed, ages staggered"""
    _lib._lib = None
    _lib.LIB_PATH = path
    v = tg.TreasureGameVec(N, seed=SEED, autoreset=True, max_episode_steps=LIMIT)
    v.reset()
    v.set_policy_mlp(seeded_params(H), act="tanh", masked=True)
    v.rollout(8, t0=0, action_seed=A0, policy="mlp", obs=False)
    st = v.read_state(mt=True)
    st["ep"][:, 1] = np.arange(N) % LIMIT
    v.write_state(st)
    del st
    torch.cuda.synchronize()
    print("ready:", path, flush=True)
    return v


def torch_gae(r, v_boot):
    """the reverse loop a user writes today: both bits end the recursion, only `terminated`
    zeroes the next value (a truncated env's next value is the NEXT episode's: all it has)"""
    gl = GAMMA * LAM
    adv = torch.empty_like(r["value"])
    a = torch.zeros_like(v_boot)
    nv = v_boot
    for s in reversed(range(r["value"].shape[0])):
        term = (r["done"][s] & tg.DONE_TERMINATED) != 0
        cut = r["done"][s] != 0
        delta = r["reward"][s].float() + GAMMA * nv.masked_fill(term, 0.0) - r["value"][s]
        a = delta + gl * a.masked_fill(cut, 0.0)
        adv[s] = a
        nv = r["value"][s]
    return adv, adv + r["value"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def kernel_trace(path):
    """per kernel (and grid) of the traced `c` legs: launches, mean and max us, from rocprofv3's
    output database (its `kernels` view)"""
    import sqlite3
    db = sqlite3.connect(path)
    out = {}
    for name, grid, calls, total, worst in db.execute(
            "select name, grid_x, count(*), sum(duration), max(duration) from kernels "
            "group by name, grid_x"):
        for key in ("k_trunc_list", "k_value_mlp", "k_policy_mlp", "k_timelimit", "k_gae"):
            if key + "<" in name or key + "(" in name or name.endswith(key):
                out.setdefault(key, []).append({"grid_threads": grid, "calls": calls,
                                                "mean_us": round(total / calls / 1e3, 3),
                                                "max_us": round(worst / 1e3, 3)})
    return out


def main():
    if os.environ.get("MERGE_TRACE"):  # add a kernel trace's figures (a run of its own) to OUT
        with open(OUT) as f:
            result = json.load(f)
        tr = kernel_trace(os.environ["MERGE_TRACE"])
        # per step of the traced `c` legs: k_trunc_list and k_policy_mlp run once in each step;
        # k_value_mlp's launches (over the list, and the dense one for vboot) are spread over them
        total = lambda key: sum(r["mean_us"] * r["calls"] for r in tr[key])
        steps = sum(r["calls"] for r in tr["k_trunc_list"])
        per_step = {"k_trunc_list": round(total("k_trunc_list") / steps, 3),
                    "k_value_mlp": round(total("k_value_mlp") / steps, 3),
                    "k_policy_mlp": round(total("k_policy_mlp") / sum(r["calls"] for r in tr["k_policy_mlp"]), 3)}
        tr["us_per_step"] = per_step
        tr["list_and_value_over_policy_mlp"] = round(
            (per_step["k_trunc_list"] + per_step["k_value_mlp"]) / per_step["k_policy_mlp"], 4)
        result["kernel_trace"] = tr
        with open(OUT, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(tr), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_gae: no GPU")
    lib = os.path.join(ROOT, "gym-treasure-game_amd", "libtg_amd.so")
    if os.environ.get("MODE") == "trace":
        new = fresh(lib)
        for r in range(3):
            new.rollout(K, t0=8 + r * K, action_seed=A0, policy="mlp", obs=False, gae=(GAMMA, LAM))
        torch.cuda.synchronize()
        print(json.dumps({"mode": "trace", "errors": new.errors()}), flush=True)
        return
    # A handle per leg, all from the same seed, warm-up and staggered ages: every leg runs one
    # K-step rollout per repetition, so in repetition r all of them step the same states with the
    # same actions (the actor's sampling is keyed by seed, env and step) and differ only in what
    # is launched around the steps.
    parent = os.environ.get("PARENT")
    vec = {name: fresh(lib) for name in ("b", "c", "d")}
    if parent:
        vec = {"a": fresh(os.path.join(ROOT, parent)), **vec}
    t = {name: 8 for name in vec}

    def roll(name, **kw):
        out = vec[name].rollout(K, t0=t[name], action_seed=A0, policy="mlp", obs=False, **kw)
        t[name] += K
        return out

    def leg_d():
        r = roll("d")
        return torch_gae(r, vec["d"].policy_mlp(t["d"], A0)[2])

    legs = {"b": lambda: roll("b"), "c": lambda: roll("c", gae=(GAMMA, LAM)), "d": leg_d}
    if parent:
        legs = {"a": lambda: roll("a"), **legs}
    for fn in legs.values():  # warm every leg (and torch's allocator)
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in list(legs) + ["e"]}
    trunc_share, digests = [], []
    for _ in range(REPS):
        dig = {}
        for name, fn in legs.items():
            dt, out = timed(fn)
            ms[name].append(dt)
            print("leg %s: %.3f ms" % (name, dt), flush=True)
            if name == "c":
                trunc_share.append(float((out["done"] == tg.DONE_TRUNCATED).float().mean()))
                dt, _ = timed(lambda: vec["c"].gae(out["reward"], out["done"], out["value"],
                                                   out["vboot"], GAMMA, LAM, vnext=out["vnext"]))
                ms["e"].append(dt)
            if name != "d":  # the same rows on every handle: the legs ran like states
                dig[name] = int(out["reward"].sum()) * 1000003 + int(out["done"].sum())
            del out
        digests.append(len(set(dig.values())) == 1)
    errors = 0
    for v in vec.values():
        errors |= v.errors()
    # k_gae's traffic: reward 4 + done 1 + value 4 read, adv 4 + ret 4 + vnext 4 written per env
    # and step, vboot once, vnext read where truncated
    gae_bytes = N * K * 21 + N * 4 + int(np.mean(trunc_share) * N * K) * 4
    best_e = min(ms["e"])
    result = {"envs": N, "steps": K, "hidden": H, "act": "tanh", "masked": True, "limit": LIMIT,
              "gamma": GAMMA, "lambda": LAM, "reps": REPS, "unit": "ms per rollout of K steps",
              "handles": "one per leg, the same states in every repetition",
              "same_rows_on_every_handle": digests,
              "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
              "c_minus_b": [round(c - b, 3) for c, b in zip(ms["c"], ms["b"])],
              "d_minus_b": [round(d - b, 3) for d, b in zip(ms["d"], ms["b"])],
              "truncated_share_per_step": round(float(np.mean(trunc_share)), 5),
              "k_gae": {"bytes": gae_bytes, "ms_best": round(best_e, 4),
                        "ms": [round(x, 4) for x in ms["e"]],
                        "bytes_per_s": gae_bytes / (best_e * 1e-3),
                        "of_copy_ceiling": gae_bytes / (best_e * 1e-3) / COPY_CEILING},
              "errors": errors}
    if parent:
        spread = max(ms["a"]) - min(ms["a"])
        result["b_minus_a"] = [round(b - a, 3) for a, b in zip(ms["a"], ms["b"])]
        result["a_spread"] = round(spread, 3)
        result["b_within_a_spread"] = bool(min(ms["a"]) - spread <= min(ms["b"]) and
                                           max(ms["b"]) <= max(ms["a"]) + spread)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)
    assert errors == 0 and all(digests)
    for rep in range(REPS):
        assert ms["c"][rep] - ms["b"][rep] < ms["d"][rep] - ms["b"][rep], (
            "rep %d: the advantages cost %.3f ms on the device, %.3f ms in torch"
            % (rep, ms["c"][rep] - ms["b"][rep], ms["d"][rep] - ms["b"][rep]))
    if parent:
        assert result["b_within_a_spread"], "leg b is outside the parent's own spread"


if __name__ == "__main__":
    main()
