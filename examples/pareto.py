#!/usr/bin/env python3
"""One Pareto front of schedules per instance — in (makespan, energy + idle, transport) — from one search, beside what a user had to do
before: baselines.evolve_pareto seeded with the plans of the 12 dispatch rules (P plans per instance, G generations), and the merged
fronts of V runs of baselines.evolve, each with another weight vector and (G + 1) / V - 1 generations, so that both replay
P * (G + 1) plans per instance.  One table of front size and hypervolume per instance; the reference point of the hypervolume is the
component-wise worst of the 12 rules.  The instances are generated on the device; everything runs with left shift off, as the rules do.

    python examples/pareto.py [--instances 256] [--size 6 6 2] [--population 32] [--generations 31] [--show 8]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtfjsp_amd  # noqa: F401  (alias of the package directory)
from importlib import import_module

baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")

WEIGHTS = [(0.4, 0.4, 0.2), (0.8, 0.1, 0.1), (0.1, 0.8, 0.1), (0.1, 0.1, 0.8)]      # the configured vector and one per objective

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=256)
ap.add_argument("--size", type=int, nargs=3, default=[6, 6, 2], metavar=("J", "M", "E"))
ap.add_argument("--population", type=int, default=32)
ap.add_argument("--generations", type=int, default=31)
ap.add_argument("--show", type=int, default=8)
a = ap.parse_args()
(J, M, E), N, P, G, V = a.size, a.instances, a.population, a.generations, len(WEIGHTS)
if (G + 1) % V:
    raise SystemExit(f"--generations + 1 must be a multiple of {V}, the number of weight vectors")
args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": WEIGHTS[0][0], "weight_ec": WEIGHTS[0][1], "weight_tt": WEIGHTS[0][2]}

env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
env.generate_instances(seed=2024)
rules = baselines.pdr_baselines(None, None, None, None, args, env=env, seed=0)      # 12 rollouts of N on the generated batch
t, p, tt, edge = env.read_instances()
env.close()
names = [r[0] for r in baselines.RULES]
starts = [rules[baselines.PLANS][k] for k in names]
points = lambda f4: np.stack([f4[..., 0], f4[..., 1] + f4[..., 3], f4[..., 2]], -1)  # noqa: E731  Final_4cost -> (mk, ec, tt)
ref = points(np.stack([rules[k][1] for k in names])).max(0)                         # [N,3]: the component-wise worst rule

torch.cuda.synchronize(); t0 = time.perf_counter()
nsga = baselines.evolve_pareto(t, p, tt, edge, args, starts, P=P, generations=G, seed=0)
wall_nsga = time.perf_counter() - t0

torch.cuda.synchronize(); t0 = time.perf_counter()
runs = []
for w in WEIGHTS:
    args_w = dict(args, weight_mk=w[0], weight_ec=w[1], weight_tt=w[2])
    runs.append(points(baselines.evolve(t, p, tt, edge, args_w, starts, P=P, generations=(G + 1) // V - 1, seed=0)["GA"][1]))
wall_ga = time.perf_counter() - t0
merged = np.stack(runs, 1)                                                          # [N,V,3]: one point per weight vector


def front_of(pts):
    """the non-dominated rows of pts [F,3], of duplicates the first"""
    keep = [i for i, x in enumerate(pts) if not any(((y <= x).all() and (y < x).any()) or ((y == x).all() and j < i) for j, y in enumerate(pts))]
    return pts[keep]


size = np.array([[len(nsga["fronts"][n]["obj"]), len(front_of(merged[n]))] for n in range(N)])
hv = np.array([[baselines.hypervolume(nsga["fronts"][n]["cost"], ref[n]), baselines.hypervolume(merged[n], ref[n])] for n in range(N)])
print(f"{N} instances J{J}M{M}E{E}, {P * (G + 1)} replayed plans per instance: evolve_pareto (P = {P}, {G} generations) in {wall_nsga * 1e3:.1f} ms, "
      f"{V} x evolve (P = {P}, {(G + 1) // V - 1} generations each) in {wall_ga * 1e3:.1f} ms")
print(f"{'instance':<10}{'front NSGA':>12}{'front merged':>14}{'hypervolume NSGA':>20}{'hypervolume merged':>20}")
for n in range(min(a.show, N)):
    print(f"{n:<10}{size[n, 0]:>12}{size[n, 1]:>14}{hv[n, 0]:>20.1f}{hv[n, 1]:>20.1f}")
print(f"{'mean':<10}{size[:, 0].mean():>12.2f}{size[:, 1].mean():>14.2f}{hv[:, 0].mean():>20.1f}{hv[:, 1].mean():>20.1f}")
print(f"evolve_pareto has the larger hypervolume on {(hv[:, 0] > hv[:, 1]).sum()} of {N} instances, the smaller on {(hv[:, 0] < hv[:, 1]).sum()}; "
      f"best Objective (weights {WEIGHTS[0]}): mean {nsga['start_obj'].mean():.2f} -> {nsga['NSGA'][2].mean():.2f}")
