#!/usr/bin/env python3
"""Measurements behind profiles/critical_search.json: local search with the moves a critical path directs,
J6M6E2 x 4096 device-generated instances, K = 16 copies, starts = the MOR+SPT plans.

  --mode trace    baselines.local_search twice with moves = 31 and twice with moves = 7 (8 rounds each; the first run of either
                  warms up).  Run it under `rocprofv3 --kernel-trace --stats` (program directly after `--`, no counters): k_critical_path,
                  k_plan_neighbours<.., true> (the instantiation with a path) and k_plan_neighbours<.., false> (the one the old entry
                  launches) are read from the trace by --mode reduce.
  --mode ab       60 launches of DeviceBatchEnv.plan_neighbours(moves = 7) on the same 65 536 plans, with the package of the checkout
                  --tree (default: this one; another built checkout, e.g. the parent commit, for the A/B).  Under rocprofv3 as above,
                  alternating the two trees on one box; the spread of the parent's own runs is the margin.
  --mode wall     wall time of local_search (32 rounds) with moves = 7 and 31, median of --reps after a warm-up: one round's total.
  --mode quality  mean final Objective and share of instances improved for moves = 7, 24, 31, under w = (1, 0, 0) and the
                  configured (0.4, 0.4, 0.2), left shift off and on, 32 rounds.  For information: no test asserts a ratio.
  --mode reduce   the traces under --out-dir + the wall and quality json -> --out
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J, M, E, N = 6, 6, 2, 4096
T = J * M
K, ROUNDS, TRACE_ROUNDS, AB_LAUNCHES = 16, 32, 8, 60
CONFIG_W = (0.4, 0.4, 0.2)


def _args(w):
    return {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": w[0], "weight_ec": w[1], "weight_tt": w[2]}


def _setup(tree=ROOT):
    sys.path.insert(0, tree)
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    mods = {k: import_module("e2e-mappo-for-mt-fjsp_amd." + k) for k in ("baselines", "batch_env")}
    if not torch.cuda.is_available():
        raise SystemExit("profile_critical_search.py needs the GPU: there is nothing to measure without it")
    env = mods["batch_env"].DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    env.generate_instances(seed=2024)
    bl = mods["baselines"]
    rule = bl.pdr_baselines(None, None, None, None, _args(CONFIG_W), env=env, rules=[r for r in bl.RULES if r[0] == "MOR+SPT"], seed=0)
    data = env.read_instances()
    env.close()
    return torch, mods, data, rule[bl.PLANS]["MOR+SPT"]


def mode_trace():
    torch, mods, data, start = _setup()
    bl = mods["baselines"]
    for _ in range(2):                                     # run 0 warms up
        for moves in (31, 7):
            bl.local_search(*data, _args(CONFIG_W), start, K=K, rounds=TRACE_ROUNDS, seed=0, moves=moves)
            torch.cuda.synchronize()


def mode_ab(tree):
    import numpy as np
    torch, mods, data, start = _setup(tree)
    env = mods["batch_env"].DeviceBatchEnv(J, M, E, N * K, left_shift=False, obs_dtype="f32")
    env.load_instances(*(np.repeat(np.asarray(x), K, axis=0) for x in data[:3]), edge=np.repeat(np.asarray(data[3]), K, axis=0))
    src = tuple(torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.int32).T), device=env.device) for x in start)
    out = tuple(torch.empty(T, N * K, dtype=torch.int32, device=env.device) for _ in range(2))
    kind = torch.empty(N * K, dtype=torch.int8, device=env.device)
    for r in range(AB_LAUNCHES):
        env.plan_neighbours(K, src[0], src[1], None, 0, r, 0, 7, out[0], out[1], kind)
    torch.cuda.synchronize()
    env.close()


def mode_wall(reps):
    torch, mods, data, start = _setup()
    bl = mods["baselines"]
    res = {"shape": "J6M6E2", "N": N, "K": K, "rounds": ROUNDS, "reps": reps,
           "what": "wall time of local_search from the MOR+SPT plans, handles, upload and final replay included; per round = median / rounds"}
    for moves in (7, 31):
        walls = []
        for i in range(reps + 1):                          # the first call is the warm-up
            torch.cuda.synchronize(); t0 = time.perf_counter()
            bl.local_search(*data, _args(CONFIG_W), start, K=K, rounds=ROUNDS, seed=0, moves=moves)
            if i:
                walls.append(time.perf_counter() - t0)
        med = sorted(walls)[len(walls) // 2]
        res[f"moves_{moves}"] = {"launches_per_round": T + (5 if moves & 24 else 4), "wall_s_all": walls, "wall_s_median": med, "round_ms": med / ROUNDS * 1e3}
    return res


def mode_quality():
    torch, mods, data, start = _setup()
    bl = mods["baselines"]
    out = {"shape": "J6M6E2", "N": N, "K": K, "rounds": ROUNDS, "seed": 0, "start": "MOR+SPT (left shift off)",
           "what": "mean Objective of the final incumbents (lower is better) and the share of instances whose Objective fell below the start's"}
    for left_shift in (False, True):
        for w in ((1.0, 0.0, 0.0), CONFIG_W):
            for moves in (7, 24, 31):
                r = bl.local_search(*data, _args(w), start, K=K, rounds=ROUNDS, seed=0, moves=moves, left_shift=left_shift)
                acc = r["accepted"]
                out[f"left_shift_{int(left_shift)}/w_{w[0]}_{w[1]}_{w[2]}/moves_{moves}"] = {
                    "start_objective": float(r["start_obj"].mean()), "final_objective": float(r["LS"][2].mean()),
                    "share_improved": float((r["LS"][2] < r["start_obj"]).mean()),
                    "accepted": {str(k): int((acc == k).sum()) for k in (-1, 1, 2, 4, 8, 16)}}
    return out


KERNELS = {"k_critical_path": ("k_critical_path",), "k_plan_neighbours_with_path": ("k_plan_neighbours<true, true>", "k_plan_neighboursILb1ELb1E"),
           "k_plan_neighbours_old": ("k_plan_neighbours<true, false>", "k_plan_neighboursILb1ELb0E", "k_plan_neighbours<true>", "k_plan_neighboursILb1EE")}


def _durations(trace_dir):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    dur = {}
    if not fs:
        return dur
    for r in sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"])):
        key = next((k for k, names in KERNELS.items() if any(n in r["Kernel_Name"] for n in names)), None)
        if key:
            dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return dur


def _stat(v):
    return {"launches": len(v), "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def mode_reduce(out_dir, out):
    res = {"shape": "J6M6E2", "N": N, "K": K, "plans_per_launch": N * K,
           "method": "rocprofv3 --kernel-trace --stats, no counters, a run of its own; the launches of the second (warm) run of either search"}
    dur = _durations(os.path.join(out_dir, "critical_trace"))
    kt = {}
    for key, v in dur.items():
        n = TRACE_ROUNDS + 1 if key == "k_critical_path" else TRACE_ROUNDS
        kt[key + "_us"] = _stat(v[-n:]) if len(v) >= 2 * n else {"unmeasured": f"{len(v)} launches in the trace"}
    res["kernel_times"] = kt or {"unmeasured": "no kernel trace"}
    ab = {}
    for d in sorted(glob.glob(os.path.join(out_dir, "critical_ab_*"))):
        v = _durations(d).get("k_plan_neighbours_old", [])
        if len(v) == AB_LAUNCHES:
            ab[os.path.basename(d)[len("critical_ab_"):]] = _stat(v[10:])
    if ab:
        par = [v["median"] for k, v in ab.items() if k.startswith("parent")]
        new = [v["median"] for k, v in ab.items() if k.startswith("this")]
        res["old_instantiation_against_parent"] = {
            "what": "k_plan_neighbours<T <= 64>, moves = 7, 65 536 plans, 60 launches a run (the first 10 dropped), the two checkouts alternating on one box",
            "runs": ab, "parent_medians_us": par, "this_medians_us": new,
            "parent_spread_us": (max(par) - min(par)) if par else None,
            "this_minus_parent_us": (sorted(new)[len(new) // 2] - sorted(par)[len(par) // 2]) if par and new else None}
    else:
        res["old_instantiation_against_parent"] = {"unmeasured": "no A/B traces"}
    for name in ("wall", "quality"):
        path = os.path.join(out_dir, f"critical_{name}.json")
        res[name] = json.loads(open(path).read()) if os.path.exists(path) else {"unmeasured": "not run"}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "quality"}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "ab", "wall", "quality", "reduce"], required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out-dir", default=os.environ.get("MTFJSP_TOOL_OUT", "tool_out"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace()
    elif a.mode == "ab":
        mode_ab(os.path.abspath(a.tree))
    elif a.mode in ("wall", "quality"):
        line = json.dumps(mode_wall(a.reps) if a.mode == "wall" else mode_quality())
        print(line)
        os.makedirs(a.out_dir, exist_ok=True)
        open(os.path.join(a.out_dir, f"critical_{a.mode}.json"), "w").write(line + "\n")
    else:
        mode_reduce(a.out_dir, a.out or os.path.join(a.out_dir, "critical_search.json"))
