#!/usr/bin/env python3
"""Measurements behind profiles/best_of_k.json, J6M6E2 x 1024 instances.

  --mode trace    evaluate.sample_best_of_k at K = 32 twice (the first run warms up): N*K = 32 768 copies, then
                  mtfjsp_footprint_copy reading exactly the bytes k_final_costs reads (one instance's scalar state) and the bytes
                  k_group_reduce reads (33 B per copy), writing nothing — launched the same way (compare kernels
                  launched alike).  Run it under `rocprofv3 --kernel-trace` (program directly after `--`, no counters): --mode reduce
                  reads the trace.
  --mode wall     median of `--reps` wall times of sample_best_of_k at K = 1, 8, 32 beside validate_cost_batched on the same
                  instances.  Profiler off.  With --only-validate the greedy evaluation alone (for a run against another build of
                  the library, e.g. the parent commit's).
  --mode quality  mean Objective of greedy, best-of-8, best-of-32 and the random rule's best at the same K.  For information only.
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
KS = (1, 8, 32)
K_TRACE = 32
ARGS = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
SCAL_BYTES = 28 * 8                                        # what k_final_costs may touch per instance: its scalar state
GROUP_BYTES = 33                                           # what k_group_reduce reads per copy: cost4 and done


def _setup():
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    mods = {k: import_module("e2e-mappo-for-mt-fjsp_amd." + k) for k in ("baselines", "batch_env", "instances", "evaluate", "encoder")}
    if not torch.cuda.is_available():
        raise SystemExit("profile_best_of_k.py needs the GPU: there is nothing to measure without it")
    data = mods["instances"].generate_instances(N, J, M, E, seed=31)
    return torch, mods, data, mods["encoder"].random_init_weights(seed=0)


def mode_trace():
    torch, mods, data, weights = _setup()
    for _ in range(2):                                     # run 0 warms up
        mods["evaluate"].sample_best_of_k(weights, *data, ARGS, K=K_TRACE, seed=0)
        torch.cuda.synchronize()
    env = mods["batch_env"].DeviceBatchEnv(J, M, E, 1)
    out = {"copies": N * K_TRACE}
    for key, nbytes in (("final_costs", SCAL_BYTES * N * K_TRACE), ("group_reduce", GROUP_BYTES * N * K_TRACE)):
        avg, mn = env.footprint_copy(nbytes, 0, 16, 2048, 50)
        out[key + "_bytes_read"] = nbytes
        out[key + "_footprint_copy_events_us"] = {"avg": avg, "min": mn}
    print(json.dumps(out))
    env.close()


def _median_wall(torch, fn, reps):
    walls = []
    for i in range(reps + 1):                              # the first call is the warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        if i:
            walls.append(time.perf_counter() - t0)
    return sorted(walls)[len(walls) // 2], walls


def mode_wall(reps, only_validate):
    torch, mods, data, weights = _setup()
    out = {"shape": "J6M6E2", "N": N, "reps": reps}
    med, walls = _median_wall(torch, lambda: mods["evaluate"].validate_cost_batched(weights, *data, ARGS), reps)
    out["validate_cost_batched_wall_s_median"], out["validate_cost_batched_wall_s_all"] = med, walls
    if not only_validate:
        for K in KS:
            med, walls = _median_wall(torch, lambda: mods["evaluate"].sample_best_of_k(weights, *data, ARGS, K=K, seed=0), reps)
            out[f"sample_best_of_k_K{K}_wall_s_median"], out[f"sample_best_of_k_K{K}_wall_s_all"] = med, walls
        base = out["sample_best_of_k_K1_wall_s_median"]
        out["wall_over_K1"] = {f"K{K}": out[f"sample_best_of_k_K{K}_wall_s_median"] / base for K in KS}
    return out


def mode_quality():
    torch, mods, data, weights = _setup()
    ev, bl = mods["evaluate"], mods["baselines"]
    out = {"shape": "J6M6E2", "N": N, "weights": "encoder.random_init_weights(seed=0): an untrained policy",
           "what": "mean Objective over the instances (lower is better); policy with left shift on, random rule with left shift off"}
    out["greedy"] = float(ev.validate_cost_batched(weights, *data, ARGS)[2].mean())
    for K in (8, 32):
        r = ev.sample_best_of_k(weights, *data, ARGS, K=K, seed=0)
        out[f"best_of_{K}"] = float(r["best"][2].mean())
        out[f"best_of_{K}_mean_front_size"] = float(r["front"].sum(1).mean())
        rnd = bl.random_baselines(*data, ARGS, K=K, seed=0)
        out[f"RANDOM_BEST_K{K}"] = float(rnd[bl.RANDOM_BEST][2].mean())
        out[f"RANDOM_MEAN_K{K}"] = float(rnd[bl.RANDOM_MEAN][2].mean())
    return out


def mode_reduce(trace_dir, wall_json, parent_json, quality_json, trace_log, out):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        name = r["Kernel_Name"]
        key = next((k for k in ("k_final_costs", "k_group_reduce", "k_footprint_copy") if k in name), None)
        if key:
            dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {"shape": "J6M6E2", "N": N, "K": K_TRACE, "copies": N * K_TRACE,
           "method": "rocprofv3 --kernel-trace, no counters; k_final_costs and k_group_reduce: the launch of the second (warm) run; "
                     "k_footprint_copy: 60 launches per footprint, the first 10 of each dropped"}
    stat = lambda v: {"launches": len(v), "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}     # noqa: E731
    for k in ("k_final_costs", "k_group_reduce"):
        if k in dur:
            res[k + "_us"] = {"launches_seen": len(dur[k]), "warm": dur[k][-1], "all": dur[k]}
    fp = dur.get("k_footprint_copy", [])
    if len(fp) == 120:
        res["k_footprint_copy_final_costs_bytes_us"] = stat(fp[10:60])
        res["k_footprint_copy_group_reduce_bytes_us"] = stat(fp[70:120])
        for k, f in (("k_final_costs", "k_footprint_copy_final_costs_bytes_us"), ("k_group_reduce", "k_footprint_copy_group_reduce_bytes_us")):
            if k + "_us" in res:
                res[k + "_over_read_only_copy_of_its_bytes"] = res[k + "_us"]["warm"] / res[f]["median"]
    for line in open(trace_log):
        if line.startswith("{"):
            res["trace_run"] = json.loads(line)
    res["wall"] = json.loads(open(wall_json).read())
    if os.path.exists(parent_json):
        res["wall_parent_library"] = json.loads(open(parent_json).read())
    if os.path.exists(quality_json):
        res["quality"] = json.loads(open(quality_json).read())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("wall", "quality", "wall_parent_library")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "quality", "reduce"], required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-validate", action="store_true")
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")          # where tools/profile_best_of_k.sh writes
    ap.add_argument("--trace-dir", default=os.path.join(out_dir, "best_of_k_trace"))
    ap.add_argument("--trace-log", default=os.path.join(out_dir, "best_of_k_trace.log"))
    ap.add_argument("--wall-json", default=os.path.join(out_dir, "best_of_k_wall.json"))
    ap.add_argument("--parent-json", default=os.path.join(out_dir, "best_of_k_wall_parent.json"))
    ap.add_argument("--quality-json", default=os.path.join(out_dir, "best_of_k_quality.json"))
    ap.add_argument("--out", default=os.path.join(out_dir, "best_of_k.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace()
    elif a.mode in ("wall", "quality"):
        line = json.dumps(mode_wall(a.reps, a.only_validate) if a.mode == "wall" else mode_quality())
        print(line)
        path = a.wall_json if a.mode == "wall" else a.quality_json
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").write(line + "\n")
    else:
        mode_reduce(a.trace_dir, a.wall_json, a.parent_json, a.quality_json, a.trace_log, a.out)
