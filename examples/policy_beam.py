#!/usr/bin/env python3
"""Three ways to decode one trained policy on the SAME generated instances, one table: greedy (evaluate.validate_cost_batched),
best of K sampled schedules (evaluate.sample_best_of_k) and beam decoding by the actors' joint log-probability
(baselines.policy_beam) at W = K = 1, 4, 16 — PB_TOP is the most probable finished schedule the beam holds, PB_BEST the cheapest.
The weights are the trained J6M6E2 actors kept with the tests (tests/golden/encoder_j6m6e2_top1.npz); any (job actor, machine
actor) pair of state dicts works, e.g. (torch.load(job_actor.pth), torch.load(machine_actor.pth)).

    python examples/policy_beam.py [--instances 256] [--json means.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mtfjsp_amd  # noqa: F401,E402  (alias of the package directory)
from importlib import import_module  # noqa: E402

baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
evaluate = import_module("e2e-mappo-for-mt-fjsp_amd.evaluate")
instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=256)
ap.add_argument("--json", default=None, help="also write the table's mean Objectives there")
a = ap.parse_args()
J, M, E, N = 6, 6, 2, a.instances
WIDTHS = (1, 4, 16)
args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_j6m6e2_top1.npz"))
weights = tuple({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)} for pre in ("w_ja.", "w_ma."))
t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=2025)

rows, wall = [], {}


def timed(name, fn):
    t0 = time.perf_counter()
    out = fn()                                                              # (every call ends in a read-back)
    wall[name] = time.perf_counter() - t0
    return out


_, f4, obj = timed("greedy", lambda: evaluate.validate_cost_batched(weights, t, p, tt, edge, args))
rows.append(("greedy", f4, obj))
for K in WIDTHS:
    r = timed(f"best-of-{K}", lambda: evaluate.sample_best_of_k(weights, t, p, tt, edge, args, K=K, seed=0))
    rows.append((f"best-of-{K}", r["best"][1], r["best"][2]))
for W in WIDTHS:
    r = timed(f"policy_beam W={W}", lambda: baselines.policy_beam(weights, t, p, tt, edge, args, width=W))
    rows += [(f"{name} W={W}", r[name][1], r[name][2]) for name in (baselines.PB_TOP, baselines.PB_BEST)]

print(f"{N} generated instances J{J}M{M}E{E}; wall seconds (set-up included): " + ", ".join(f"{k} {v:.2f}" for k, v in wall.items()))
print(f"{'decoding':<18}{'objective':>12}{'makespan':>12}{'energy':>12}{'transport':>12}{'idle':>12}")
for name, f4, ob in rows:
    print(f"{name:<18}{ob.mean():>12.2f}{f4[:, 0].mean():>12.2f}{f4[:, 1].mean():>12.2f}{f4[:, 2].mean():>12.2f}{f4[:, 3].mean():>12.2f}")
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps({"shape": "J6M6E2", "N": N, "weights": "tests/golden/encoder_j6m6e2_top1.npz", "instances_seed": 2025,
                            "what": "mean Objective over the instances (lower is better)",
                            "mean_objective": {name: float(ob.mean()) for name, _, ob in rows}}) + "\n")
