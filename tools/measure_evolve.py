#!/usr/bin/env python3
"""Measurements behind profiles/evolve.json: baselines.evolve beside baselines.local_search from one build and session,
J6M6E2 x 4096 instances generated on the device, P = K = 16.

  --mode trace --what evolve|ls   the search twice (the first run warms up), 16 generations / rounds.  Run it under `rocprofv3
                  --kernel-trace` (program directly after `--`, no counters): --mode reduce reads the two traces — k_plan_offspring
                  beside k_plan_neighbours, and the T step launches of a generation beside them.
  --mode wall     wall time per generation / round as the difference of two lengths (8 and 24) over 16, median of `--reps` pairs
                  after a warm-up: what the set-up, generation 0 and the final replay cost drops out.  Profiler off.
  --mode quality  mean Objective of evolve seeded with the 12 rule plans (P = 16, 32 generations) and of local_search from every
                  instance's best rule (K = 16, 32 rounds): P * generations = K * rounds replays (evolve replays its generation 0 on
                  top).  For information only.
  --mode reduce   both kernel-trace csv + the wall and quality json -> --out
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
J, M, E, N = 6, 6, 2, 4096
T = J * M
P, TRACE_GENS, QUALITY_GENS, GEN_SEED = 16, 16, 32, 2024
ARGS = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}


def _setup():
    """-> torch, baselines, the instances (generated on the device, read back), the 12 rules' results"""
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    bl, be = (import_module("e2e-mappo-for-mt-fjsp_amd." + k) for k in ("baselines", "batch_env"))
    if not torch.cuda.is_available():
        raise SystemExit("measure_evolve.py needs the GPU: there is nothing to measure without it")
    env = be.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    env.generate_instances(seed=GEN_SEED)
    rules = bl.pdr_baselines(None, None, None, None, ARGS, env=env, seed=0)
    data = env.read_instances()
    env.close()
    return torch, bl, data, rules


def _starts(bl, rules):
    """-> (the 12 rule plans, every instance's best rule's plan, its Objective)"""
    import numpy as np
    names = [r[0] for r in bl.RULES]
    obj = np.stack([rules[k][2] for k in names])                       # [12,N]
    pick, n = obj.argmin(0), np.arange(obj.shape[1])
    task = np.stack([rules[bl.PLANS][k][0] for k in names])[pick, n]
    mach = np.stack([rules[bl.PLANS][k][1] for k in names])[pick, n]
    return [rules[bl.PLANS][k] for k in names], (task, mach), obj.min(0)


def _run(bl, data, what, starts, best_rule, gens):
    if what == "evolve":
        return bl.evolve(*data, ARGS, starts, P=P, generations=gens, seed=0)
    return bl.local_search(*data, ARGS, best_rule, K=P, rounds=gens, seed=0)


def mode_trace(what):
    torch, bl, data, rules = _setup()
    starts, best_rule, _ = _starts(bl, rules)
    for _ in range(2):                                                  # run 0 warms up
        _run(bl, data, what, starts, best_rule, TRACE_GENS)
        torch.cuda.synchronize()
    print(json.dumps({"what": what, "plans_per_launch": N * P, "generations": TRACE_GENS}))


def mode_wall(reps):
    torch, bl, data, rules = _setup()
    starts, best_rule, _ = _starts(bl, rules)
    out = {"shape": "J6M6E2", "N": N, "P": P, "K": P, "reps": reps, "launches_per_generation": T + 4,
           "method": "(wall of 24 generations - wall of 8) / 16, host clock around a call that ends in its own read-back; median of the pairs"}
    for what in ("evolve", "ls"):
        _run(bl, data, what, starts, best_rule, 8)                      # warm-up
        per = []
        for _ in range(reps):
            w = {}
            for gens in (8, 24):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                _run(bl, data, what, starts, best_rule, gens)
                w[gens] = time.perf_counter() - t0
            per.append((w[24] - w[8]) / 16)
        key = "evolve_generation" if what == "evolve" else "local_search_round"
        out[key + "_wall_ms_median"] = sorted(per)[len(per) // 2] * 1e3
        out[key + "_wall_ms_all"] = [x * 1e3 for x in per]
    return out


def mode_quality():
    torch, bl, data, rules = _setup()
    starts, best_rule, best_obj = _starts(bl, rules)
    ga = bl.evolve(*data, ARGS, starts, P=P, generations=QUALITY_GENS, seed=0)
    ls = bl.local_search(*data, ARGS, best_rule, K=P, rounds=QUALITY_GENS, seed=0)
    return {"shape": "J6M6E2", "N": N, "instances": f"generated on the device, seed {GEN_SEED}", "P": P, "K": P, "generations": QUALITY_GENS,
            "rounds": QUALITY_GENS, "seed": 0, "p_cross": 0.8, "p_mut": 0.3, "moves": "SWAP | INSERT | REASSIGN",
            "what": "mean Objective over the instances (lower is better), left shift off; no pass criterion",
            "best_of_12_rules": float(best_obj.mean()), "evolve_start_obj": float(ga["start_obj"].mean()),
            "evolve_from_12_rules": float(ga["GA"][2].mean()), "evolve_after_8_and_16": [float(ga["history"][7].mean()), float(ga["history"][15].mean())],
            "local_search_from_best_rule": float(ls["LS"][2].mean()),
            "local_search_after_8_and_16": [float(ls["history"][7].mean()), float(ls["history"][15].mean())]}


def _generations(trace_dir, marker):
    """the warm run's generations as the trace shows them: a generation = from one launch of `marker` to the next
    -> {"kernels": {name: {launches per generation, median us per launch, median us per generation}}, busy and span per generation}"""
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"].removeprefix("void ").split("(")[0].strip(), int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    at = [i for i, r in enumerate(rows) if marker in r[0]]
    if len(at) != 2 * TRACE_GENS:
        raise SystemExit(f"{trace_dir}: {len(at)} launches of {marker}, expected {2 * TRACE_GENS}")
    at = at[TRACE_GENS:]                                                # the second run
    med = lambda v: sorted(v)[len(v) // 2]                              # noqa: E731
    per, busy, span = {}, [], []
    for lo, hi in zip(at[:-1], at[1:]):
        names = {}
        for name, t0, t1 in rows[lo:hi]:
            names.setdefault(name, []).append((t1 - t0) / 1e3)
        for name, v in names.items():
            per.setdefault(name, []).append(v)
        busy.append(sum(sum(v) for v in names.values()))
        span.append((rows[hi][1] - rows[lo][1]) / 1e3)
    kernels = {name: {"launches_per_generation": med([len(v) for v in g]), "us_per_launch_median": med([x for v in g for x in v]),
                      "us_per_generation_median": med([sum(v) for v in g])} for name, g in sorted(per.items())}
    return {"generations_read": len(busy), "kernels": kernels, "kernel_time_us_per_generation_median": med(busy),
            "marker_to_marker_us_median": med(span)}


def mode_reduce(out_dir, out):
    res = {"shape": "J6M6E2", "N": N, "P": P, "K": P, "plans_per_launch": N * P,
           "method": "rocprofv3 --kernel-trace, no counters, one run per search; the second (warm) run of "
                     f"{TRACE_GENS} generations / rounds, a generation = from one k_plan_offspring / k_plan_neighbours to the next; times in us"}
    res["evolve"] = _generations(os.path.join(out_dir, "evolve_trace_evolve"), "k_plan_offspring")
    res["local_search"] = _generations(os.path.join(out_dir, "evolve_trace_ls"), "k_plan_neighbours")
    off = next(v for k, v in res["evolve"]["kernels"].items() if "k_plan_offspring" in k)
    nb = next(v for k, v in res["local_search"]["kernels"].items() if "k_plan_neighbours" in k)
    res["k_plan_offspring_us"], res["k_plan_neighbours_us"] = off["us_per_launch_median"], nb["us_per_launch_median"]
    res["k_plan_offspring_over_k_plan_neighbours"] = off["us_per_launch_median"] / nb["us_per_launch_median"]
    steps = [v for v in res["evolve"]["kernels"].values() if v["launches_per_generation"] == T]
    if len(steps) == 1:                                                 # the step kernel: the one with T launches a generation
        res["step_launches_of_a_generation_us"] = steps[0]["us_per_generation_median"]
        res["k_plan_offspring_over_the_step_launches_of_a_generation"] = off["us_per_launch_median"] / steps[0]["us_per_generation_median"]
    for key in ("wall", "quality"):
        path = os.path.join(out_dir, f"evolve_{key}.json")
        if os.path.exists(path):
            res[key] = json.loads(open(path).read())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("evolve", "local_search")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "quality", "reduce"], required=True)
    ap.add_argument("--what", choices=["evolve", "ls"], default="evolve")
    ap.add_argument("--reps", type=int, default=5)
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")            # where tools/measure_evolve.sh writes
    ap.add_argument("--out", default=os.path.join(out_dir, "evolve.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace(a.what)
    elif a.mode in ("wall", "quality"):
        line = json.dumps(mode_wall(a.reps) if a.mode == "wall" else mode_quality())
        print(line)
        os.makedirs(out_dir, exist_ok=True)
        open(os.path.join(out_dir, f"evolve_{a.mode}.json"), "w").write(line + "\n")
    else:
        mode_reduce(out_dir, a.out)
