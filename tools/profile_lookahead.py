#!/usr/bin/env python3
"""Measurements behind profiles/lookahead_baselines.json, J6M6E2 x 1024 source instances = 36 864 scratch instances.

  --mode trace   one episode of one look-ahead rule with every expand (k_env_fork in its STATE form + k_lookahead_actions) and every
                 selection between two event records, then mtfjsp_footprint_copy with the fork's exact read and write byte counts —
                 whose launches are made the same way (compare kernels launched alike).  Run it under
                 `rocprofv3 --kernel-trace` (program directly after `--`, no counters): --mode reduce reads the trace.
  --mode wall    median of `--reps` wall times of baselines.lookahead_baselines for one rule, and the same rule WITHOUT the fork for a
                 few steps: per step, reset of the scratch handle and replay of the prefix with the existing kernels, then the
                 candidate step and the selection.  Profiler off.
  --mode reduce  kernel-trace csv under --trace-dir + the wall json -> --out
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
RULE = ("LA_IT", 2)
ARGS = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
# bytes per destination instance of the STATE fork: TaskSD + TaskPL, JobR, MJRec, f64 machine features, 28 scalars, staged weights
STATE_BYTES = 2 * T * 16 + J * 16 + max(J, M) * 8 + M * 64 + 28 * 8 + 24


def _setup():
    import numpy as np  # noqa: F401
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    if not torch.cuda.is_available():
        raise SystemExit("profile_lookahead.py needs the GPU: there is nothing to measure without it")
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
    return torch, baselines, batch_env, (t, p, tt, edge)


def _env(torch, batch_env, data):
    env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    env.load_instances(*data[:3], edge=data[3]); env.scaler_init()
    w3 = torch.tensor([[0.4, 0.4, 0.2]], dtype=torch.float64, device=env.device).repeat(N, 1)
    return env, w3


def mode_trace():
    torch, baselines, batch_env, data = _setup()
    env, w3 = _env(torch, batch_env, data)
    la = baselines.Lookahead(env)
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    for ep in range(2):                                    # episode 0 warms up
        env.reset(w3)
        for s in range(T):
            a, b, c, d = ev(), ev(), ev(), ev()
            a.record(); la.expand(); b.record()
            la.scratch.step(la.task_c, la.mach_c)
            c.record(); la.select(RULE[1]); d.record()
            env.step(la.task, la.mach)
        torch.cuda.synchronize()
    nbytes = STATE_BYTES * N * T
    avg, mn = env.footprint_copy(nbytes, nbytes, 16, 2048, 50)
    print(json.dumps({"footprint_copy_events_us": {"avg": avg, "min": mn}, "fork_bytes_read": nbytes, "fork_bytes_written": nbytes}))
    la.close(); env.close()


def mode_wall(reps, replay_steps):
    import numpy as np
    torch, baselines, batch_env, data = _setup()
    walls = []
    for i in range(reps + 1):                              # the first call is the warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        baselines.lookahead_baselines(*data, ARGS, rules=[RULE])
        if i:
            walls.append(time.perf_counter() - t0)
    # without the fork: the scratch handle (its constants forked once) is reset and replays the prefix before every candidate step
    env, w3 = _env(torch, batch_env, data)
    la = baselines.Lookahead(env)
    w3s = w3.repeat_interleave(T, 0).contiguous()
    env.reset(w3)
    prefix, per_step = [], []
    for s in range(replay_steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        la.scratch.scaler_init(); la.scratch.reset(w3s)
        for a, m in prefix:
            la.scratch.step(a, m)
        la.expand()                                        # (candidate actions; its copy stands in for nothing here but is not what is timed)
        la.scratch.step(la.task_c, la.mach_c); la.select(RULE[1]); env.step(la.task, la.mach)
        torch.cuda.synchronize(); per_step.append(time.perf_counter() - t0)
        prefix.append((la.task.repeat_interleave(T).contiguous(), la.mach.repeat_interleave(T).contiguous()))
    la.close(); env.close()
    fit = np.polyfit(np.arange(replay_steps), np.array(per_step), 1)           # per-step time = fit[1] + fit[0] * s
    total = float(sum(fit[1] + fit[0] * s for s in range(T)))
    med = sorted(walls)[len(walls) // 2]
    return {"shape": "J6M6E2", "N": N, "scratch_instances": N * T, "rule": RULE[0], "reps": reps, "lookahead_baselines_wall_s_median": med,
            "lookahead_baselines_wall_s_all": walls, "replay_steps_measured": replay_steps, "replay_step_wall_s": per_step,
            "replay_episode_wall_s_extrapolated": total,
            "extrapolation": "least-squares line through the measured per-step times (a step replays s prefix steps), summed over s = 0..T-1; "
                             "the replay path still contains one fork per step (for the candidate actions) and excludes handle creation"}


def mode_reduce(trace_dir, wall_json, trace_log, out):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        name = r["Kernel_Name"]
        key = "k_env_fork" if "k_env_fork" in name else "k_lookahead_select" if "k_lookahead_select" in name else \
            "k_lookahead_actions" if "k_lookahead_actions" in name else "k_footprint_copy" if "k_footprint_copy" in name else \
            "step_scratch_or_source" if "k_env_" in name else None
        if key:
            dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {"shape": "J6M6E2", "N": N, "scratch_instances": N * T, "state_bytes_per_instance": STATE_BYTES, "method": "rocprofv3 --kernel-trace, no counters"}
    for k, v in dur.items():
        if k == "k_env_fork":
            v = v[1 + T:]                                  # drop the INSTANCE fork and the warm-up episode
        elif k == "k_footprint_copy":
            v = v[10:]                                     # its 10 warm-up launches
        elif k in ("k_lookahead_select", "k_lookahead_actions"):
            v = v[T:]
        s = sorted(v)
        res[k + "_us"] = {"launches": len(s), "median": s[len(s) // 2], "min": s[0], "max": s[-1]}
    if "k_env_fork_us" in res and "k_footprint_copy_us" in res:
        res["fork_fraction_of_same_footprint_copy"] = res["k_footprint_copy_us"]["median"] / res["k_env_fork_us"]["median"]
    for line in open(trace_log):
        if line.startswith("{"):
            res["trace_run"] = json.loads(line)
    res["wall"] = json.loads(open(wall_json).read())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "wall"}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "reduce"], required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replay-steps", type=int, default=6)
    out_dir = os.environ.get("MTFJSP_TOOL_OUT", "tool_out")          # where tools/profile_lookahead.sh writes
    ap.add_argument("--trace-dir", default=os.path.join(out_dir, "lookahead_trace"))
    ap.add_argument("--trace-log", default=os.path.join(out_dir, "lookahead_trace.log"))
    ap.add_argument("--wall-json", default=os.path.join(out_dir, "lookahead_wall.json"))
    ap.add_argument("--out", default=os.path.join(out_dir, "lookahead_baselines.json"))
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace()
    elif a.mode == "wall":
        line = json.dumps(mode_wall(a.reps, a.replay_steps))
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.wall_json)), exist_ok=True)
        open(a.wall_json, "w").write(line + "\n")
    else:
        mode_reduce(a.trace_dir, a.wall_json, a.trace_log, a.out)
