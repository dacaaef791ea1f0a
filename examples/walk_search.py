#!/usr/bin/env python3
"""A walk that leaves local optima beside hill climbing at the same number of replayed plans: baselines.local_search and
baselines.walk_search in three settings — a tabu ring of the last 8 schedules with "always move to the best admissible neighbour",
late acceptance against the incumbent of 8 rounds ago, and a threshold that falls from 5 % of the start's Objective to 0 — all from the
MOR+SPT plans, K neighbours per round, the same rounds and seed: K * rounds replays per instance either way.  One table in the layout
of examples/evolve.py, then how often each walk moved and why.
The instances are generated on the device; everything runs with left shift off, as the dispatch rules do.

    python examples/walk_search.py [--instances 1024] [--size 6 6 2] [--copies 16] [--rounds 64]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtfjsp_amd  # noqa: F401  (alias of the package directory)
from importlib import import_module

baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=1024)
ap.add_argument("--size", type=int, nargs=3, default=[6, 6, 2], metavar=("J", "M", "E"))
ap.add_argument("--copies", type=int, default=16)
ap.add_argument("--rounds", type=int, default=64)
a = ap.parse_args()
(J, M, E), N, K, R = a.size, a.instances, a.copies, a.rounds
args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}

env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
env.generate_instances(seed=2024)
rule = baselines.pdr_baselines(None, None, None, None, args, env=env, rules=[r for r in baselines.RULES if r[0] == "MOR+SPT"], seed=0)
t, p, tt, edge = env.read_instances()
env.close()
start = rule[baselines.PLANS]["MOR+SPT"]
top = 0.05 * float(rule["MOR+SPT"][2].mean())
falling = [top * (R - 1 - r) / max(R - 1, 1) for r in range(R)]

walks = {"WS(tabu 8)": dict(tabu=8, slack=float("inf"), late=0), "WS(late 8)": dict(tabu=0, slack=None, late=8),
         "WS(threshold)": dict(tabu=0, slack=falling, late=0)}
runs = [("LS", lambda: baselines.local_search(t, p, tt, edge, args, start, K=K, rounds=R, seed=0, name="LS"))]
runs += [(name, lambda name=name, kw=kw: baselines.walk_search(t, p, tt, edge, args, start, K=K, rounds=R, seed=0, name=name, **kw)) for name, kw in walks.items()]
searched, walls = {}, {}
for name, run in runs:
    torch.cuda.synchronize(); t0 = time.perf_counter()
    searched[name] = run()
    walls[name] = time.perf_counter() - t0

print(f"{N} instances J{J}M{M}E{E}, {R} rounds of {K} neighbours from MOR+SPT: " + ", ".join(f"{k} in {v * 1e3:.1f} ms" for k, v in walls.items()))
print(f"{'method':<22}{'objective':>12}{'makespan':>12}{'energy':>12}{'transport':>12}{'idle':>12}")
rows = [("MOR+SPT", rule["MOR+SPT"][1], rule["MOR+SPT"][2])] + [(k, s[k][1], s[k][2]) for k, s in searched.items()]
for name, f4, ob in rows:
    print(f"{name:<22}{ob.mean():>12.2f}{f4[:, 0].mean():>12.2f}{f4[:, 1].mean():>12.2f}{f4[:, 2].mean():>12.2f}{f4[:, 3].mean():>12.2f}")
for k, s in searched.items():
    print(f"{k}: mean best Objective {s['start_obj'].mean():.2f} -> " + " -> ".join(f"{s['history'][r - 1].mean():.2f} ({r})" for r in sorted({min(8, R), R // 2, R}) if r))
print(f"{'walk':<22}{'stayed':>10}{'better':>10}{'slack':>10}{'late':>10}{'new best':>10}{'barred':>10}{'last incumbent':>16}")
for k in walks:
    s = searched[k]
    why = s["why"] & 7
    print(f"{k:<22}{int((why < 2).sum()):>10}{int((why == 2).sum()):>10}{int((why == 3).sum()):>10}{int((why == 4).sum()):>10}"
          f"{int(((s['why'] & 8) != 0).sum()):>10}{int(s['barred'].sum()):>10}{s['current'][-1].mean() if R else float('nan'):>16.2f}")
