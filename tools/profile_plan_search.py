#!/usr/bin/env python3
"""Measurements behind profiles/plan_search.json, J6M6E2 x 1024 instances, K = 32 copies, 32 rounds.

  --mode trace    baselines.local_search from the MOR+SPT plans twice (the first run warms up): 32 launches of k_plan_neighbours
                  per run, N*K = 32 768 plans each; then mtfjsp_footprint_copy WRITING exactly the bytes k_plan_neighbours writes
                  (2*T*N*K*4: both output arrays) and reading nothing — launched the same way (compare kernels
                  launched alike).  Run it under `rocprofv3 --kernel-trace` (program directly after `--`, no counters): --mode
                  reduce reads the trace.
  --mode wall     median of `--reps` wall times of local_search after a warm-up.  Profiler off.
  --mode quality  mean Objective after 0 / 8 / 32 rounds from the MOR+SPT plans and from RANDOM_BEST's (K = 32).  For information only.
  --mode reduce   kernel-trace csv under --trace-dir + the wall and quality json -> --out
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
J, M, E, N = 6, 6, 2, 1024
T = J * M
K, ROUNDS = 32, 32
ARGS = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
OUT_BYTES = 2 * T * N * K * 4                              # what k_plan_neighbours writes: task_out and mach_out


def _setup():
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    mods = {k: import_module("e2e-mappo-for-mt-fjsp_amd." + k) for k in ("baselines", "batch_env", "instances")}
    if not torch.cuda.is_available():
        raise SystemExit("profile_plan_search.py needs the GPU: there is nothing to measure without it")
    data = mods["instances"].generate_instances(N, J, M, E, seed=31)
    return torch, mods, data


def _starts(bl, data, which=("MOR+SPT", "RANDOM_BEST")):
    out = {}
    if "MOR+SPT" in which:
        out["MOR+SPT"] = bl.pdr_baselines(*data, ARGS, rules=[r for r in bl.RULES if r[0] == "MOR+SPT"], seed=0)[bl.PLANS]["MOR+SPT"]
    if "RANDOM_BEST" in which:
        out["RANDOM_BEST"] = bl.random_baselines(*data, ARGS, K=K, seed=0)[bl.PLANS][bl.RANDOM_BEST]
    return out


def mode_trace():
    torch, mods, data = _setup()
    bl = mods["baselines"]
    start = _starts(bl, data, ("MOR+SPT",))["MOR+SPT"]
    for _ in range(2):                                     # run 0 warms up
        bl.local_search(*data, ARGS, start, K=K, rounds=ROUNDS, seed=0)
        torch.cuda.synchronize()
    env = mods["batch_env"].DeviceBatchEnv(J, M, E, 1)
    avg, mn = env.footprint_copy(0, OUT_BYTES, 16, 2048, 50)
    print(json.dumps({"plans_per_launch": N * K, "bytes_written": OUT_BYTES, "footprint_copy_events_us": {"avg": avg, "min": mn}}))
    env.close()


def mode_wall(reps):
    torch, mods, data = _setup()
    bl = mods["baselines"]
    start = _starts(bl, data, ("MOR+SPT",))["MOR+SPT"]
    walls = []
    for i in range(reps + 1):                              # the first call is the warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        bl.local_search(*data, ARGS, start, K=K, rounds=ROUNDS, seed=0)
        if i:
            walls.append(time.perf_counter() - t0)
    return {"shape": "J6M6E2", "N": N, "K": K, "rounds": ROUNDS, "reps": reps, "launches_per_round": T + 4,
            "local_search_wall_s_median": sorted(walls)[len(walls) // 2], "local_search_wall_s_all": walls}


def mode_quality():
    torch, mods, data = _setup()
    bl = mods["baselines"]
    out = {"shape": "J6M6E2", "N": N, "K": K, "seed": 0, "moves": "SWAP | INSERT | REASSIGN",
           "what": "mean Objective over the instances (lower is better) of the incumbents after 0 / 8 / 32 rounds, left shift off"}
    for name, start in _starts(bl, data).items():
        r = bl.local_search(*data, ARGS, start, K=K, rounds=ROUNDS, seed=0)
        out[name] = {"rounds_0": float(r["start_obj"].mean()), "rounds_8": float(r["history"][7].mean()), "rounds_32": float(r["history"][31].mean()),
                     "accepted_SWAP": int((r["accepted"] == bl.MOVE_SWAP).sum()), "accepted_INSERT": int((r["accepted"] == bl.MOVE_INSERT).sum()),
                     "accepted_REASSIGN": int((r["accepted"] == bl.MOVE_REASSIGN).sum()), "rounds_without_a_move": int((r["accepted"] == -1).sum())}
    return out


def mode_reduce(trace_dir, wall_json, quality_json, trace_log, out):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        key = next((k for k in ("k_plan_neighbours", "k_footprint_copy") if k in r["Kernel_Name"]), None)
        if key:
            dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    stat = lambda v: {"launches": len(v), "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}     # noqa: E731
    res = {"shape": "J6M6E2", "N": N, "K": K, "rounds": ROUNDS, "plans_per_launch": N * K, "bytes_written_per_launch": OUT_BYTES,
           "method": "rocprofv3 --kernel-trace, no counters; k_plan_neighbours: the 32 launches of the second (warm) run; "
                     "k_footprint_copy (write only, the same bytes): 60 launches, the first 10 dropped"}
    pn, fp = dur.get("k_plan_neighbours", []), dur.get("k_footprint_copy", [])
    if len(pn) == 2 * ROUNDS:
        res["k_plan_neighbours_us"] = stat(pn[ROUNDS:])
        res["k_plan_neighbours_first_round_us"] = pn[ROUNDS]               # (src_col = NULL, the start plans; the others read `best`)
    if len(fp) == 60:
        res["k_footprint_copy_us"] = stat(fp[10:])
    if "k_plan_neighbours_us" in res and "k_footprint_copy_us" in res:
        res["k_plan_neighbours_over_write_only_copy_of_its_bytes"] = res["k_plan_neighbours_us"]["median"] / res["k_footprint_copy_us"]["median"]
    for line in open(trace_log):
        if line.startswith("{"):
            res["trace_run"] = json.loads(line)
    res["wall"] = json.loads(open(wall_json).read())
    if os.path.exists(quality_json):
        res["quality"] = json.loads(open(quality_json).read())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("wall", "quality")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "quality", "reduce"], required=True)
    ap.add_argument("--reps", type=int, default=5)
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")          # where tools/profile_plan_search.sh writes
    ap.add_argument("--trace-dir", default=os.path.join(out_dir, "plan_search_trace"))
    ap.add_argument("--trace-log", default=os.path.join(out_dir, "plan_search_trace.log"))
    ap.add_argument("--wall-json", default=os.path.join(out_dir, "plan_search_wall.json"))
    ap.add_argument("--quality-json", default=os.path.join(out_dir, "plan_search_quality.json"))
    ap.add_argument("--out", default=os.path.join(out_dir, "plan_search.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace()
    elif a.mode in ("wall", "quality"):
        line = json.dumps(mode_wall(a.reps) if a.mode == "wall" else mode_quality())
        print(line)
        path = a.wall_json if a.mode == "wall" else a.quality_json
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").write(line + "\n")
    else:
        mode_reduce(a.trace_dir, a.wall_json, a.quality_json, a.trace_log, a.out)
