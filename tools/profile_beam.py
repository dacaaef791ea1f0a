#!/usr/bin/env python3
"""Measurements behind profiles/beam_baselines.json, J6M6E2 x 1024 source instances at W = 8 = 294 912 scratch instances.

  --mode trace    two episodes of one beam rule (the first warms up), then mtfjsp_footprint_copy reading exactly the bytes
                  k_state_signature reads (TaskSD + TaskPL, 32 B per task) and writing nothing — launched the same way (DESIGN.md
                  §5: compare kernels launched alike).  Run it under `rocprofv3 --kernel-trace` (program directly after `--`, no
                  counters): --mode reduce reads the trace.
  --mode wall     median of `--reps` wall times of baselines.beam_baselines for one rule, beside baselines.lookahead_baselines for
                  the matching rule on the same instances.  Profiler off.
  --mode quality  mean Objective at W = 1 / 4 / 16 with and without merging, beside the look-ahead rules and the best static rule, on
                  the same generated instances.  For information only.
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
J, M, E, N, W = 6, 6, 2, 1024, 8
T = J * M
RULE, LA_RULE = ("BS_IT", 2), ("LA_IT", 2)
ARGS = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
SIG_BYTES = 2 * T * 16                                     # what k_state_signature touches per instance: TaskSD + TaskPL


def _setup():
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    if not torch.cuda.is_available():
        raise SystemExit("profile_beam.py needs the GPU: there is nothing to measure without it")
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
    return torch, baselines, batch_env, (t, p, tt, edge)


def mode_trace():
    torch, baselines, batch_env, data = _setup()
    env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    env.load_instances(*data[:3], edge=data[3]); env.scaler_init()
    w3 = torch.tensor([[0.4, 0.4, 0.2]], dtype=torch.float64, device=env.device).repeat(N, 1)
    env.reset(w3)
    bs = baselines.BeamSearch(env, W)
    for ep in range(2):                                    # episode 0 warms up
        bs.restart()
        bs.run(RULE[1])
        torch.cuda.synchronize()
    nbytes = SIG_BYTES * N * W * T
    avg, mn = env.footprint_copy(nbytes, 0, 16, 2048, 50)
    print(json.dumps({"footprint_copy_events_us": {"avg": avg, "min": mn}, "signature_bytes_read": nbytes}))
    bs.close(); env.close()


def mode_wall(reps):
    torch, baselines, batch_env, data = _setup()
    out = {"shape": "J6M6E2", "N": N, "W": W, "scratch_instances": N * W * T, "rule": RULE[0], "lookahead_rule": LA_RULE[0], "reps": reps}
    for key, fn in (("beam_baselines", lambda: baselines.beam_baselines(*data, ARGS, rules=[RULE], width=W)),
                    ("lookahead_baselines", lambda: baselines.lookahead_baselines(*data, ARGS, rules=[LA_RULE]))):
        walls = []
        for i in range(reps + 1):                          # the first call is the warm-up
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            if i:
                walls.append(time.perf_counter() - t0)
        out[key + "_wall_s_median"] = sorted(walls)[len(walls) // 2]
        out[key + "_wall_s_all"] = walls
    return out


def mode_quality():
    torch, baselines, batch_env, data = _setup()
    mean = lambda res: {k: float(v[2].mean()) for k, v in res.items() if k != baselines.PLANS}      # noqa: E731
    out = {"shape": "J6M6E2", "N": N, "left_shift": False, "what": "mean Objective over the instances (lower is better)"}
    pdr = mean(baselines.pdr_baselines(*data, ARGS))
    best = min(pdr, key=pdr.get)
    out["best_static_rule"] = {best: pdr[best]}
    out["lookahead"] = mean(baselines.lookahead_baselines(*data, ARGS))
    for width in (1, 4, 16):
        for dedupe in (True, False):
            out[f"beam_W{width}_{'dedupe' if dedupe else 'plain'}"] = mean(baselines.beam_baselines(*data, ARGS, width=width, dedupe=dedupe))
    return out


def mode_reduce(trace_dir, wall_json, quality_json, trace_log, out):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        name = r["Kernel_Name"]
        key = "k_env_fork_expand" if "k_env_fork<true>" in name or "k_env_forkILb1" in name else "k_env_fork_beam" if "k_env_fork" in name else \
            "k_state_signature" if "k_state_signature" in name else "k_beam_select" if "k_beam_select" in name else \
            "k_beam_backtrack" if "k_beam_backtrack" in name else "k_lookahead_actions" if "k_lookahead_actions" in name else \
            "k_footprint_copy" if "k_footprint_copy" in name else "step_scratch" if "k_env_" in name else None
        if key:
            dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {"shape": "J6M6E2", "N": N, "W": W, "scratch_instances": N * W * T, "signature_bytes_per_instance": SIG_BYTES,
           "method": "rocprofv3 --kernel-trace, no counters; the last episode's launches of every kernel"}
    for k, v in dur.items():
        v = v[10:] if k == "k_footprint_copy" else v[-T:] if k != "k_beam_backtrack" else v[-1:]     # (10 warm-up copies; the measured episode is the last)
        s = sorted(v)
        res[k + "_us"] = {"launches": len(s), "median": s[len(s) // 2], "min": s[0], "max": s[-1]}
    parts = ["k_env_fork_expand", "k_lookahead_actions", "step_scratch", "k_state_signature", "k_beam_select", "k_env_fork_beam"]
    if all(k + "_us" in res for k in parts):
        total = sum(res[k + "_us"]["median"] for k in parts)
        res["decision_us_sum_of_medians"] = total
        res["fraction_of_a_decision"] = {k: res[k + "_us"]["median"] / total for k in parts}
    if "k_state_signature_us" in res and "k_footprint_copy_us" in res:
        res["signature_over_read_only_copy_of_its_bytes"] = res["k_state_signature_us"]["median"] / res["k_footprint_copy_us"]["median"]
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
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")          # where tools/profile_beam.sh writes
    ap.add_argument("--trace-dir", default=os.path.join(out_dir, "beam_trace"))
    ap.add_argument("--trace-log", default=os.path.join(out_dir, "beam_trace.log"))
    ap.add_argument("--wall-json", default=os.path.join(out_dir, "beam_wall.json"))
    ap.add_argument("--quality-json", default=os.path.join(out_dir, "beam_quality.json"))
    ap.add_argument("--out", default=os.path.join(out_dir, "beam_baselines.json"))
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
