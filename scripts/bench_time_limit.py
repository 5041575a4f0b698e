#!/usr/bin/env python3
"""The step limit's cost (tg_set_time_limit; DESIGN.md §12, profiles/time_limit.json).

    ROUNDS=3 python scripts/bench_time_limit.py
    MODE=trace rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/bench_time_limit.py

1,048,576 envs, uniform policy, auto-reset, episode ages staggered through write_state (length
g % 50, so 1/50 of the envs reach a limit of 50 in every step): ms per step of
  off    rollout(200), no limit
  dev    rollout(200), limit 50 on the device (k_timelimit)
  host   200 x (tg_step + the vector env's length bookkeeping in torch + masked tg_reset), no
         limit: the only way to truncate before tg_set_time_limit
interleaved over ROUNDS rounds, host clock around work that ends in a synchronise.
MODE=trace: one `dev` leg only (for a kernel trace, in a run of its own)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_treasure_game_amd as tg  # noqa: E402

N = int(os.environ.get("N", 1 << 20))
K, LIMIT, SEED, A0 = 200, 50, 0, 0x5EED0001
ROUNDS = int(os.environ.get("ROUNDS", 3))


def fresh(limit):
    v = tg.TreasureGameVec(N, seed=SEED, autoreset=True, max_episode_steps=limit)
    v.reset()
    v.rollout(40, t0=0, action_seed=A0, policy="uniform", obs=False, actions=False)  # warm-up
    st = v.read_state(mt=True)
    st["ep"][:, 1] = np.arange(N) % LIMIT
    v.write_state(st)
    del st
    torch.cuda.synchronize()
    v.stats_reset()
    return v


def run(kind):
    v = fresh(LIMIT if kind == "dev" else None)
    ln = torch.arange(N, dtype=torch.int32, device=v.device) % LIMIT
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "host":
        for t in range(K):
            o, r, va, d, _ = v.step(v.policy_actions(40 + t, A0, "uniform"))
            ln += 1
            ln.masked_fill_(d.bool(), 0)
            tr = ln >= LIMIT
            ln.masked_fill_(tr, 0)
            v.reset(tr.to(torch.uint8))
    else:
        v.rollout(K, t0=40, action_seed=A0, policy="uniform", obs=False, actions=False)
    v.regenerate()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = v.stats()
    res = {"kind": kind, "ms_step": dt / K * 1e3, "episodes": s["episodes"],
           "truncated": s["episodes_truncated"], "draws": s["draws"], "errors": v.errors()}
    v.close()
    return res


def main():
    if os.environ.get("MODE") == "trace":
        print(json.dumps(run("dev")), flush=True)
        return
    best = {}
    for r in range(ROUNDS):
        for kind in ("off", "dev", "host"):
            res = run(kind)
            print("round", r, json.dumps(res), flush=True)
            if kind not in best or res["ms_step"] < best[kind]["ms_step"]:
                best[kind] = res
    print(json.dumps({"best": best, "n": N, "steps": K, "limit": LIMIT}), flush=True)


if __name__ == "__main__":
    main()
