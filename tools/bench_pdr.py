#!/usr/bin/env python3
"""Measurements behind profiles/pdr_baselines.json.

  --mode plan   k_pdr_plan at the three full-size shapes (12 rule pairs x N instances in one batch), warmed up, `--reps` launches
                each: run it under `rocprofv3 --kernel-trace --stats` (program directly after `--`) for kernel times — the shapes
                differ in grid size (64 * B threads) — and it prints device-event times per launch as a cross-check.
  --mode wall   wall time of baselines.pdr_baselines for 12 x 4096 J6M6E2 (upload, plan on the device, T steps, read-back), next
                to the same call with the plans computed on the host by tests/pdr_rules_ref.py and uploaded.  Profiler off.
One JSON line on stdout, also written to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mtfjsp_amd  # noqa: F401,E402
from importlib import import_module  # noqa: E402
import pdr_rules_ref as ref  # noqa: E402

baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
SHAPES = [(6, 6, 2, 4096), (10, 10, 2, 1024), (20, 20, 4, 128)]


def rep12(x):
    x = np.asarray(x)
    return np.tile(x, (12,) + (1,) * (x.ndim - 1))


def mode_plan(reps):
    out = {}
    for J, M, E, N in SHAPES:
        t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
        env = batch_env.DeviceBatchEnv(J, M, E, 12 * N, left_shift=False, obs_dtype="f32")
        env.load_instances(rep12(t), rep12(p), rep12(tt), edge=rep12(edge))
        o = torch.as_tensor(np.repeat(np.array([r[1] for r in baselines.RULES], np.int32), N), device=env.device)
        m = torch.as_tensor(np.repeat(np.array([r[2] for r in baselines.RULES], np.int32), N), device=env.device)
        for _ in range(5):
            baselines.pdr_plan(env, o, m, seed=1)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(); baselines.pdr_plan(env, o, m, seed=1); b.record()
        torch.cuda.synchronize()
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        out[f"J{J}M{M}E{E}"] = {"B": 12 * N, "grid_threads": 64 * 12 * N, "reps": reps, "call_us_events_median": us[len(us) // 2], "call_us_events_min": us[0],
                                "note": "device events around the whole call (rule-id read-back + launch + output allocation), not the kernel alone"}
        env.close()
    return out


def rollout_with_host_plans(t, p, tt, edge, J, M, E, N, mor):
    """pdr_baselines' steps with the plans made on the host by the numpy restatement"""
    T, B = J * M, 12 * N
    env = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=False, obs_dtype="f32")
    tb, pb = rep12(t), rep12(p)
    env.load_instances(tb, pb, rep12(tt), edge=rep12(edge))
    env.scaler_init()
    env.reset(torch.tensor([[0.4, 0.4, 0.2]], dtype=torch.float64, device=env.device).repeat(B, 1))
    t0 = time.perf_counter()
    o = np.repeat(np.array([r[1] for r in baselines.RULES], np.int32), N); m = np.repeat(np.array([r[2] for r in baselines.RULES], np.int32), N)
    task, mach = ref.plan_batch(tb, pb, J, M, o, m, rep12(mor))
    t_plan = time.perf_counter() - t0
    ts = torch.as_tensor(np.ascontiguousarray(task.T), device=env.device); ms = torch.as_tensor(np.ascontiguousarray(mach.T), device=env.device)
    cum = torch.zeros(B, 5, dtype=torch.float64, device=env.device)
    for s in range(T):
        env.step(ts[s], ms[s])
        cum += env.raw
    torch.cuda.synchronize()
    prev = env.read_state(batch_env.capi.STATE_PREV_COSTS)
    env.close()
    return cum.cpu().numpy(), prev, t_plan


def mode_wall(reps):
    J, M, E, N = SHAPES[0]
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
    args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
    rng = np.random.RandomState(5)
    mor = np.stack([np.stack([rng.permutation(J) for _ in range(M)]) for _ in range(N)]).astype(np.int32)
    dev, host, host_plan = [], [], []
    for i in range(reps + 1):                                 # alternating; the first pair is the warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        a = baselines.pdr_baselines(t, p, tt, edge, args, mor_order=mor)
        t1 = time.perf_counter()
        cum, prev, t_plan = rollout_with_host_plans(t, p, tt, edge, J, M, E, N, mor)
        t2 = time.perf_counter()
        if i:
            dev.append(t1 - t0); host.append(t2 - t1); host_plan.append(t_plan)
    same = all(np.array_equal(a[name][1][:, 0], prev[r * N:(r + 1) * N, 0]) for r, (name, _, _) in enumerate(baselines.RULES))
    med = lambda x: sorted(x)[len(x) // 2]      # noqa: E731
    return {"shape": "J6M6E2", "N": N, "B": 12 * N, "reps": reps, "pdr_baselines_wall_s_median": med(dev), "pdr_baselines_wall_s_all": dev,
            "host_planned_wall_s_median": med(host), "host_planned_wall_s_all": host, "host_plan_only_s_median": med(host_plan),
            "same_makespans": bool(same)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plan", "wall"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pdr.py needs the GPU: there is nothing to measure without it")
    res = {"mode": a.mode, "result": mode_plan(a.reps) if a.mode == "plan" else mode_wall(a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
