#!/usr/bin/env python3
"""Measurements behind profiles/replay_plans.json: what a round of baselines.local_search costs with the copies' replay
as T + 2 launches (replay="steps") and as one (replay="launch", mtfjsp_replay_plans), at the configuration of profiles/plan_search.json —
J6M6E2 x 1024 instances, K = 32 copies, 32 rounds, from the MOR+SPT plans — and at J10M10E2 x 256 x 32; left shift off and on.

  --mode wall     per shape and left-shift setting: a warm-up call of each form, then `--reps` calls of each, ALTERNATING, in one
                  process; medians.  Profiler off.  --replay parent: the tree under --root has no `replay` argument (the parent
                  commit checked out somewhere else): its only form, the step launches, is timed the same way.
  --mode trace    local_search(replay="launch") twice per shape (the first run warms up), then mtfjsp_footprint_copy of the bytes
                  k_replay_plans reads and writes, launched the same way.  Run it under `rocprofv3 --kernel-trace` (program directly
                  after `--`, no counters): --mode reduce reads the trace.
  --mode reduce   kernel-trace csv under --trace-dir + the wall json files -> --out
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"J6M6E2": (6, 6, 2, 1024), "J10M10E2": (10, 10, 2, 256)}
K, ROUNDS = 32, 32


def args_of(J, M, E):
    return {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}


def replay_bytes(J, M, B):
    """what k_replay_plans reads — both plans, a duration and a power per step, the copy's transport times, a {min_dur, min_pt} record
    per task — and writes: four costs and done (no schedule records)"""
    T = J * M
    return B * (2 * T * 4 + 2 * T * 8 + M * M * 8 + T * 16), B * 33


def _setup(root):
    sys.path.insert(0, root)
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    mods = {k: import_module("e2e-mappo-for-mt-fjsp_amd." + k) for k in ("baselines", "batch_env", "instances")}
    if not torch.cuda.is_available():
        raise SystemExit("profile_replay_plans.py needs the GPU: there is nothing to measure without it")
    return torch, mods


def _case(mods, shape):
    J, M, E, N = SHAPES[shape]
    bl = mods["baselines"]
    data = mods["instances"].generate_instances(N, J, M, E, seed=31)
    a = args_of(J, M, E)
    start = bl.pdr_baselines(*data, a, rules=[r for r in bl.RULES if r[0] == "MOR+SPT"], seed=0)[bl.PLANS]["MOR+SPT"]
    return data, a, start


def mode_wall(root, replay, reps):
    torch, mods = _setup(root)
    bl = mods["baselines"]
    forms = {"parent": [("steps_parent", {})], "both": [("steps", {"replay": "steps"}), ("launch", {"replay": "launch"})]}[replay]
    out = {"K": K, "rounds": ROUNDS, "reps": reps, "what": "wall seconds of one local_search call (handle creation, upload and the final "
           "replay included), median of reps after a warm-up call, the forms alternating; per_round_ms = median / rounds", "cases": {}}
    for shape in SHAPES:
        data, a, start = _case(mods, shape)
        for ls in (False, True):
            walls = {name: [] for name, _ in forms}
            obj = {}
            for i in range(reps + 1):                          # the first call of each form is the warm-up
                for name, kw in forms:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    r = bl.local_search(*data, a, start, K=K, rounds=ROUNDS, seed=0, left_shift=ls, **kw)
                    if i:
                        walls[name].append(time.perf_counter() - t0)
                    obj[name] = float(r["history"][-1].mean())
            J, M, E, N = SHAPES[shape]
            case = {"N": N, "T": J * M, "copies": N * K, "left_shift": ls}
            for name, _ in forms:
                med = sorted(walls[name])[len(walls[name]) // 2]
                case[name] = {"wall_s_median": med, "per_round_ms": med / ROUNDS * 1e3, "wall_s_all": walls[name], "mean_objective_after_32": obj[name]}
            if "launch" in case:
                case["steps_over_launch"] = case["steps"]["wall_s_median"] / case["launch"]["wall_s_median"]
            out["cases"][f"{shape}-{'ls' if ls else 'nols'}"] = case
    return out


def mode_trace(root):
    torch, mods = _setup(root)
    bl = mods["baselines"]
    info = {}
    for shape in SHAPES:
        J, M, E, N = SHAPES[shape]
        data, a, start = _case(mods, shape)
        for _ in range(2):                                     # run 0 warms up
            bl.local_search(*data, a, start, K=K, rounds=ROUNDS, seed=0, replay="launch")
            torch.cuda.synchronize()
        env = mods["batch_env"].DeviceBatchEnv(J, M, E, 1)
        rd, wr = replay_bytes(J, M, N * K)
        avg, mn = env.footprint_copy(rd, wr, 16, 2048, 50)
        info[shape] = {"copies_per_launch": N * K, "bytes_read": rd, "bytes_written": wr, "footprint_copy_events_us": {"avg": avg, "min": mn}}
        env.close()
    print(json.dumps(info))


def mode_reduce(trace_dir, wall_jsons, trace_log, out):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    seq = [(next((k for k in ("k_replay_plans", "k_footprint_copy") if k in r["Kernel_Name"]), None),
            (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    seq = [x for x in seq if x[0]]
    stat = lambda v: {"launches": len(v), "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}     # noqa: E731
    res = {"K": K, "rounds": ROUNDS,
           "method": "rocprofv3 --kernel-trace, no counters; k_replay_plans: the 32 launches of the second (warm) local_search(replay='launch') "
                     "per shape, left shift off; k_footprint_copy of the bytes it reads and writes: 60 launches, the first 10 dropped",
           "kernels": {}}
    per = 2 * ROUNDS + 60                                      # the trace holds, per shape in order: 64 replays, then 60 copies
    for i, shape in enumerate(SHAPES):
        part = seq[i * per:(i + 1) * per]
        rp = [d for k, d in part if k == "k_replay_plans"]
        fp = [d for k, d in part if k == "k_footprint_copy"]
        if len(rp) == 2 * ROUNDS and len(fp) == 60:
            e = {"k_replay_plans_us": stat(rp[ROUNDS:]), "k_footprint_copy_us": stat(fp[10:])}
            e["k_replay_plans_over_copy_of_its_bytes"] = e["k_replay_plans_us"]["median"] / e["k_footprint_copy_us"]["median"]
            res["kernels"][shape] = e
    for line in open(trace_log):
        if line.startswith("{"):
            res["trace_run"] = json.loads(line)
    res["wall"] = {os.path.splitext(os.path.basename(p))[0]: json.loads(open(p).read()) for p in wall_jsons if os.path.exists(p)}
    res["not_measured"] = "other K, the largest shapes, chunked runs, the kernel trace with left shift on, walk_search / evolve / evolve_pareto"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernels"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "reduce"], required=True)
    ap.add_argument("--root", default=HERE, help="the tree whose package is measured (default: this one)")
    ap.add_argument("--replay", choices=["both", "parent"], default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="wall")
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")          # where tools/profile_replay_plans.sh writes
    ap.add_argument("--trace-dir", default=os.path.join(out_dir, "replay_plans_trace"))
    ap.add_argument("--trace-log", default=os.path.join(out_dir, "replay_plans_trace.log"))
    ap.add_argument("--wall-json", nargs="*", default=sorted(glob.glob(os.path.join(out_dir, "replay_plans_wall*.json"))))
    ap.add_argument("--out", default=os.path.join(out_dir, "replay_plans.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace(a.root)
    elif a.mode == "wall":
        line = json.dumps(mode_wall(os.path.abspath(a.root), a.replay, a.reps))
        print(line)
        os.makedirs(out_dir, exist_ok=True)
        open(os.path.join(out_dir, f"replay_plans_{a.tag}.json"), "w").write(line + "\n")
    else:
        mode_reduce(a.trace_dir, a.wall_json, a.trace_log, a.out)
