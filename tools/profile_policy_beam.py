#!/usr/bin/env python3
"""Measurements behind profiles/policy_beam.json: baselines.PolicyBeamSearch at J6M6E2, N = 256 source instances
at W = 8 (N*W = 2 048 slots, 12 288 rows of the machine forward), the trained J6M6E2 weights kept with the tests.

  --mode trace    two episodes (the first warms up).  Run it under `rocprofv3 --kernel-trace` (program directly after `--`, no
                  counters): --mode reduce reads the trace.
  --mode wall     median over `--reps` episodes of the host clock around T decisions that end in a device synchronise, per
                  decision.  Profiler off.
  --mode reduce   kernel-trace csv under --trace-dir: the last episode's kernel time per decision, split into the actors'
                  forwards, the three launches of csrc/mtfjsp_policy_beam.hip, and the rest (fork, step, signature, the tensor
                  glue: gathers, logarithms); + the wall json, the example's table (--quality-json, what examples/policy_beam.py
                  --json wrote) and the forced-replay maxima the tests print (--replay-log: tests/test_policy_beam_gpu.py -s) -> --out
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
J, M, E, N, W = 6, 6, 2, 256, 8
T = J * M
NEW = ("k_mfea1_jobs", "k_beam_select_policy", "k_beam_merge_slots")
REST = ("k_env_", "k_state_signature", "k_beam_backtrack", "at::", "at_cuda", "elementwise", "index", "Memcpy", "fill")


def _search():
    import numpy as np
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    evaluate = import_module("e2e-mappo-for-mt-fjsp_amd.evaluate")
    instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    if not torch.cuda.is_available():
        raise SystemExit("profile_policy_beam.py needs the GPU: there is nothing to measure without it")
    g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_j6m6e2_top1.npz"))
    weights = tuple({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)} for pre in ("w_ja.", "w_ma."))
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
    env = batch_env.DeviceBatchEnv(J, M, E, N, obs_dtype="f32")
    env.load_instances(t, p, tt, edge=edge)
    evaluate.eval_reset(env, evaluate.config_w3(env, (0.4, 0.4, 0.2)))
    return torch, env, baselines.PolicyBeamSearch(env, weights, W)


def mode_trace():
    torch, env, pb = _search()
    for ep in range(2):                                    # episode 0 warms up
        pb.restart()
        pb.run()
        torch.cuda.synchronize()
    print(json.dumps({"episodes": 2, "decisions_per_episode": T}))
    pb.close(); env.close()


def mode_wall(reps):
    torch, env, pb = _search()
    walls = []
    for i in range(reps + 1):                              # the first episode is the warm-up
        pb.restart()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(T):
            pb.advance()
        torch.cuda.synchronize()
        if i:
            walls.append((time.perf_counter() - t0) / T * 1e3)
    pb.close(); env.close()
    return {"shape": "J6M6E2", "N": N, "W": W, "slots": N * W, "machine_forward_rows": N * W * J, "reps": reps,
            "ms_per_decision_wall_median": sorted(walls)[len(walls) // 2], "ms_per_decision_wall_all": walls}


def mode_reduce(trace_dir, wall_json, quality_json, replay_log, out):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    # the last episode: what follows the forks of its restart (the last forks before its first selection)
    sel = [i for i, r in enumerate(rows) if "k_beam_select_policy" in r["Kernel_Name"]]
    assert len(sel) == 2 * T, f"{len(sel)} selections in the trace, expected {2 * T}"
    first = max(i for i, r in enumerate(rows[:sel[T]]) if "k_env_fork" in r["Kernel_Name"]) + 1      # behind the restart's forks
    group, per_kernel = {"forwards": 0.0, "new_launches": 0.0, "rest": 0.0}, {}
    for r in rows[first:]:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        key = "new_launches" if any(k in name for k in NEW) else "rest" if any(k in name for k in REST) else "forwards"
        group[key] += us
        short = re.sub(r"\(.*", "", name)[:80]
        per_kernel.setdefault(key, {}).setdefault(short, [0, 0.0])
        per_kernel[key][short][0] += 1; per_kernel[key][short][1] += us
    res = {"shape": "J6M6E2", "N": N, "W": W, "slots": N * W, "machine_forward_rows": N * W * J, "decisions": T,
           "method": "rocprofv3 --kernel-trace, no counters; kernel time of the last episode's launches, summed per group and divided by T",
           "kernel_ms_per_decision": {k: v / T / 1e3 for k, v in group.items()},
           "kernel_ms_per_decision_total": sum(group.values()) / T / 1e3,
           "kernels": {k: {n: {"launches": c, "us_total": u} for n, (c, u) in sorted(v.items(), key=lambda x: -x[1][1])} for k, v in per_kernel.items()}}
    res["wall"] = json.loads(open(wall_json).read())
    if quality_json and os.path.exists(quality_json):
        res["quality"] = json.loads(open(quality_json).read())
    if replay_log and os.path.exists(replay_log):
        pat = re.compile(r"policy_beam forced replay (.*): max \|dp\| job (\S+) machine (\S+)")
        cases = {m.group(1): {"job": float(m.group(2)), "machine": float(m.group(3))} for m in map(pat.search, open(replay_log)) if m}
        res["forced_replay_max_abs_probability_difference"] = {
            "what": "PB_TOP's plan teacher-forced through validate_cost_batched: the chosen actions' probabilities against the search's "
                    "(tests/test_policy_beam_gpu.py; bounds 2e-4 job, 1e-4 machine)",
            "job_max": max(c["job"] for c in cases.values()), "machine_max": max(c["machine"] for c in cases.values()), "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("kernels", "quality")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "reduce"], required=True)
    ap.add_argument("--reps", type=int, default=5)
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")          # where tools/profile_policy_beam.sh writes
    ap.add_argument("--trace-dir", default=os.path.join(out_dir, "policy_beam_trace"))
    ap.add_argument("--wall-json", default=os.path.join(out_dir, "policy_beam_wall.json"))
    ap.add_argument("--quality-json", default=os.path.join(out_dir, "policy_beam_quality.json"))
    ap.add_argument("--replay-log", default=os.path.join(out_dir, "policy_beam_replay.log"))
    ap.add_argument("--out", default=os.path.join(out_dir, "policy_beam.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace()
    elif a.mode == "wall":
        line = json.dumps(mode_wall(a.reps))
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.wall_json)), exist_ok=True)
        open(a.wall_json, "w").write(line + "\n")
    else:
        mode_reduce(a.trace_dir, a.wall_json, a.quality_json, a.replay_log, a.out)
