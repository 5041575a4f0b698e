#!/usr/bin/env python3
"""Device-resident snapshots against the only route the parent commit has (DESIGN.md §14,
profiles/snapshot.json).

    python scripts/bench_snapshot.py                        # the per-call times
    PARENT=gym-treasure-game_amd/libtg_amd_parent.so STEP_AB=3 python scripts/bench_snapshot.py

1,048,576 envs, seed 0, auto-reset, 40 masked steps first so that the envs sit in different ring
generations with stale halves among them.  Each call is timed between stream events, after a
warm-up call, three times (best and spread reported), ms per call:
  save       Snapshot.save of every env into its own slot
  load       Snapshot.load of every slot into its own env
  load_seed  the same with seeds
  load_64th  Snapshot.load of N / 64 slots into every 64th env
  host       read_state(mt=True) followed by write_state of the same batch: the parent's route
             to "put the envs into that state" (wall clock: it runs on the host)
Bandwidth: each kernel's algorithmic bytes per second against the 6.29-TB/s copy ceiling.  save
writes a 2,536-B slot per env and reads the 16-B state word, 24 B of angles and episode, and a
generation (an odd one is twisted from the stored one before it: up to ~3 x 2,496 B requested,
counted as the 2,496 B it must read).  load reads the slot and writes 40 B of state, 8 stored
generations and 16 generations of codes: 2,536 + 40 + 19,968 + 4,992 B.
STEP_AB=k with PARENT (a libtg_amd.so built from the parent commit, as scripts/ab.py's
variants): `python bench.py` k times for the parent and k times for this build, interleaved in
this run; both sets of headlines are recorded and this build's must lie within the parent's own
run-to-run spread.  The result is written before any assertion."""
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_treasure_game_amd as tg  # noqa: E402

N = int(os.environ.get("N", 1 << 20))
REPS = int(os.environ.get("REPS", 3))
PRE = int(os.environ.get("PRE", 40))
COPY_CEILING = 6.29e12  # B/s, the measured float4 copy of an MI355X
SAVE_BYTES = 2536 + 16 + 24 + 2496
LOAD_BYTES = 2536 + 40 + 8 * 2496 + 16 * 312
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "snapshot.json"))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def three(fn):
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = [timed(fn) for _ in range(REPS)]
    return {"ms": [round(x, 4) for x in ms], "best": round(min(ms), 4),
            "spread": round(max(ms) - min(ms), 4)}


def bandwidth(leg, entries, per_entry):
    b = entries * per_entry
    leg["bytes"] = b
    leg["bytes_per_s"] = b / (leg["best"] * 1e-3)
    leg["of_copy_ceiling"] = round(leg["bytes_per_s"] / COPY_CEILING, 4)


def headline(path):
    """one `python bench.py` on the library at `path` (None: this build): its JSON line"""
    env = dict(os.environ)
    env.pop("TG_LIB_PATH", None)
    if path:
        env["TG_LIB_PATH"] = os.path.join(ROOT, path)
        env["TG_AB_LIB"] = "1"  # (the parent's build lacks the new entry points)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                          os.environ.get("BENCH_STEPS", "100"), "--warmup", "10"], env=env,
                         check=True, stdout=subprocess.PIPE, text=True).stdout
    line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    return {"value": line["value"], "ms_per_step": line["ms_per_step"], "steps": line["steps"],
            "masked_value": line.get("masked_policy", {}).get("value"),
            "error_flags": line.get("error_flags")}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_snapshot: no GPU")
    result = {"envs": N, "reps": REPS, "pre_steps": PRE, "unit": "ms per call"}
    vec = tg.TreasureGameVec(N, seed=0, autoreset=True)
    vec.reset()
    for t in range(PRE):
        vec.step(vec.policy_actions(t, 0x5EED0001, "masked"))
    snap = vec.snapshot(N)
    every = torch.arange(N, dtype=torch.int64, device=vec.device)
    part = every[::64].contiguous()
    seeds = every + 12345
    legs = {"save": three(lambda: snap.save(every, every)),
            "load": three(lambda: snap.load(every, every)),
            "load_seed": three(lambda: snap.load(every, every, seeds)),
            "load_64th": three(lambda: snap.load(part, part))}
    bandwidth(legs["save"], N, SAVE_BYTES)
    bandwidth(legs["load"], N, LOAD_BYTES)
    bandwidth(legs["load_64th"], part.numel(), LOAD_BYTES)
    legs["load_seed"]["note"] = "k_snap_seed (one env per lane, a 1,247-step chain) + the rebuild"
    result["legs"] = legs
    print(json.dumps(legs), flush=True)
    # the parent's route, on the same handle: host copies of every env, then every ring rebuilt
    host = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = vec.read_state(mt=True)
        t1 = time.perf_counter()
        vec.write_state(st)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append({"read_state_ms": round((t1 - t0) * 1e3, 1), "write_state_ms": round((t2 - t1) * 1e3, 1)})
        del st
    result["host_route"] = host
    best_host = min(h["read_state_ms"] + h["write_state_ms"] for h in host)
    result["host_route_over_save_plus_load"] = round(
        best_host / (legs["save"]["best"] + legs["load"]["best"]), 1)
    result["errors"] = vec.errors()
    snap.close()
    vec.close()
    parent, k = os.environ.get("PARENT"), int(os.environ.get("STEP_AB", 0))
    if parent and k:
        runs = {"parent": [], "this": []}
        for _ in range(k):
            for name, path in (("parent", parent), ("this", None)):
                runs[name].append(headline(path))
                print(name, json.dumps(runs[name][-1]), flush=True)
        key = "value"  # bench.py's headline: env-steps/s
        a = [r[key] for r in runs["parent"]]
        b = [r[key] for r in runs["this"]]
        spread = max(a) - min(a)
        result["step_path"] = {"headline_key": key, "parent": a, "this": b, "parent_spread": spread,
                               "this_within_parent_spread": bool(min(a) - spread <= min(b) and
                                                                 max(b) <= max(a) + spread),
                               "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k_: v for k_, v in result.items() if k_ != "step_path"}), flush=True)
    assert result["errors"] == 0
    if "step_path" in result:
        assert result["step_path"]["this_within_parent_spread"], "the step path moved"


if __name__ == "__main__":
    main()
