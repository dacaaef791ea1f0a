#!/usr/bin/env python3
"""Measurements behind profiles/pareto.json: baselines.evolve_pareto beside baselines.evolve from one build and session,
J6M6E2 x 4096 instances generated on the device, P = 32, seeded with the 12 rule plans.

  --mode trace --what pareto|evolve   the search twice (the first run warms up), 16 generations.  Run it under `rocprofv3
                  --kernel-trace` (program directly after `--`, no counters): --mode reduce reads the two traces — k_front_rank and
                  k_plan_survivors beside k_plan_offspring and the T step launches of a generation.
  --mode wall     wall time per generation as the difference of two lengths (8 and 24) over 16, median of `--reps` pairs after a
                  warm-up: what the set-up, generation 0 and the final replay cost drops out.  Profiler off.
  --mode chain    k_front_rank on ONE totally ordered group of K = 2048 — every candidate a front of its own, the stated worst case of
                  the peeling — beside one group of 2048 random candidates: HIP events around the launch, median of `--reps`.
  --mode reduce   both kernel-trace csv + the wall and chain json -> --out
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure_evolve as me  # noqa: E402  (the set-up, the starts and the trace reader are shared)

J, M, E, N, T = me.J, me.M, me.E, me.N, me.T
P, TRACE_GENS = 32, me.TRACE_GENS
ARGS = me.ARGS


def _run(bl, data, what, starts, gens):
    if what == "pareto":
        return bl.evolve_pareto(*data, ARGS, starts, P=P, generations=gens, seed=0)
    return bl.evolve(*data, ARGS, starts, P=P, generations=gens, seed=0)


def mode_trace(what):
    torch, bl, data, rules = me._setup()
    starts, _, _ = me._starts(bl, rules)
    for _ in range(2):                                                  # run 0 warms up
        _run(bl, data, what, starts, TRACE_GENS)
        torch.cuda.synchronize()
    print(json.dumps({"what": what, "plans_per_launch": N * P, "generations": TRACE_GENS}))


def mode_wall(reps):
    torch, bl, data, rules = me._setup()
    starts, _, best_obj = me._starts(bl, rules)
    out = {"shape": "J6M6E2", "N": N, "P": P, "reps": reps, "launches_per_generation": {"evolve_pareto": T + 5, "evolve": T + 4},
           "method": "(wall of 24 generations - wall of 8) / 16, host clock around a call that ends in its own read-back; median of the pairs"}
    for what in ("pareto", "evolve"):
        _run(bl, data, what, starts, 8)                                 # warm-up
        per = []
        for _ in range(reps):
            w = {}
            for gens in (8, 24):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                res = _run(bl, data, what, starts, gens)
                w[gens] = time.perf_counter() - t0
            per.append((w[24] - w[8]) / 16)
        key = "evolve_pareto" if what == "pareto" else "evolve"
        out[key + "_generation_wall_ms_median"] = sorted(per)[len(per) // 2] * 1e3
        out[key + "_generation_wall_ms_all"] = [x * 1e3 for x in per]
        out[key + "_mean_objective_after_24"] = float(res["NSGA" if what == "pareto" else "GA"][2].mean())
        if what == "pareto":
            out["evolve_pareto_mean_front_size_after_24"] = float(sum(len(f["obj"]) for f in res["fronts"]) / N)
    out["best_of_12_rules_mean_objective"] = float(best_obj.mean())
    return out


def mode_chain(reps):
    import numpy as np
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    be = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    K = 2048
    env = be.DeviceBatchEnv(3, 4, 2, 1)
    dev = env.device
    rs = np.random.RandomState(0)
    v = rs.permutation(K).astype(np.float64)
    groups = {"chain": np.stack([v, v, v, np.zeros(K)], 1), "random": rs.uniform(0.0, 1000.0, (K, 4))}
    out = {"K": K, "groups": 1, "reps": reps, "method": "HIP events around one mtfjsp_front_rank launch with all five outputs, after a warm-up; median"}
    done = torch.ones(K, dtype=torch.uint8, device=dev)
    for name, c4 in groups.items():
        c4 = torch.as_tensor(c4, device=dev)
        outs = env.front_rank(1, c4, done, None, None, (0.4, 0.4, 0.2))
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            env.front_rank(1, c4, done, None, None, (0.4, 0.4, 0.2), *outs)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name + "_ms_median"] = sorted(ms)[len(ms) // 2]
        out[name + "_fronts"] = int(outs[0].max().item()) + 1
    env.close()
    return out


def mode_reduce(out_dir, out):
    res = {"shape": "J6M6E2", "N": N, "P": P, "plans_per_launch": N * P,
           "method": "rocprofv3 --kernel-trace, no counters, one run per search; the second (warm) run of "
                     f"{TRACE_GENS} generations, a generation = from one k_plan_offspring to the next; times in us"}
    res["evolve_pareto"] = me._generations(os.path.join(out_dir, "pareto_trace_pareto"), "k_plan_offspring")
    res["evolve"] = me._generations(os.path.join(out_dir, "pareto_trace_evolve"), "k_plan_offspring")
    k = res["evolve_pareto"]["kernels"]
    steps = [v for v in k.values() if v["launches_per_generation"] == T]
    for name in ("k_front_rank", "k_plan_survivors", "k_plan_offspring"):
        res[name + "_us"] = next(v["us_per_launch_median"] for key, v in k.items() if name in key)
    if len(steps) == 1:                                                 # the step kernel: the one with T launches a generation
        res["step_launches_of_a_generation_us"] = steps[0]["us_per_generation_median"]
        res["front_rank_and_survivors_over_the_step_launches_of_a_generation"] = (res["k_front_rank_us"] + res["k_plan_survivors_us"]) / steps[0]["us_per_generation_median"]
    for key in ("wall", "chain"):
        path = os.path.join(out_dir, f"pareto_{key}.json")
        if os.path.exists(path):
            res[key] = json.loads(open(path).read())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("evolve_pareto", "evolve")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "chain", "reduce"], required=True)
    ap.add_argument("--what", choices=["pareto", "evolve"], default="pareto")
    ap.add_argument("--reps", type=int, default=5)
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")            # where tools/measure_pareto.sh writes
    ap.add_argument("--out", default=os.path.join(out_dir, "pareto.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace(a.what)
    elif a.mode in ("wall", "chain"):
        line = json.dumps(mode_wall(a.reps) if a.mode == "wall" else mode_chain(a.reps))
        print(line)
        os.makedirs(out_dir, exist_ok=True)
        open(os.path.join(out_dir, f"pareto_{a.mode}.json"), "w").write(line + "\n")
    else:
        mode_reduce(out_dir, a.out)
