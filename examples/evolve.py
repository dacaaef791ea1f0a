#!/usr/bin/env python3
"""Evolutionary search on plans beside local search at the same replay budget: baselines.evolve seeded with the plans of the 12 dispatch
rules and of the best of K random episodes (a population of P plans per instance; per generation child 0 is the best member, every
other child two tournament winners crossed — precedence-preserving order crossover of the job strings, a coin per task for the machine
— and mutated by one move), and baselines.local_search from every instance's best rule, K = P neighbours per round, rounds =
generations: P * generations = K * rounds replays.  One table in the layout of examples/pdr_baselines.py.
The instances are generated on the device; everything runs with left shift off, as the dispatch rules do.

    python examples/evolve.py [--instances 1024] [--size 6 6 2] [--population 32] [--generations 32]
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

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=1024)
ap.add_argument("--size", type=int, nargs=3, default=[6, 6, 2], metavar=("J", "M", "E"))
ap.add_argument("--population", type=int, default=32)
ap.add_argument("--generations", type=int, default=32)
a = ap.parse_args()
(J, M, E), N, P, G = a.size, a.instances, a.population, a.generations
args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}

env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
env.generate_instances(seed=2024)
rules = baselines.pdr_baselines(None, None, None, None, args, env=env, seed=0)      # 12 rollouts of N on the generated batch
t, p, tt, edge = env.read_instances()
env.close()
rnd = baselines.random_baselines(t, p, tt, edge, args, K=P, seed=0)                 # the random rule, best of P episodes

names = [r[0] for r in baselines.RULES]
starts = [rules[baselines.PLANS][k] for k in names] + [rnd[baselines.PLANS][baselines.RANDOM_BEST]]
rule_obj = np.stack([rules[k][2] for k in names])                                   # [12,N]
pick, idx = rule_obj.argmin(0), np.arange(N)
best_rule = tuple(np.stack([rules[baselines.PLANS][k][i] for k in names])[pick, idx] for i in range(2))

searched, walls = {}, {}
for name, run in (("GA(rules+random)", lambda: baselines.evolve(t, p, tt, edge, args, starts, P=P, generations=G, seed=0, name="GA(rules+random)")),
                  ("LS(best rule)", lambda: baselines.local_search(t, p, tt, edge, args, best_rule, K=P, rounds=G, seed=0, name="LS(best rule)"))):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    searched[name] = run()
    walls[name] = time.perf_counter() - t0

print(f"{N} instances J{J}M{M}E{E}, {G} generations of {P} plans = {G} rounds of {P} neighbours: " + ", ".join(f"{k} in {v * 1e3:.1f} ms" for k, v in walls.items()))
print(f"{'method':<22}{'objective':>12}{'makespan':>12}{'energy':>12}{'transport':>12}{'idle':>12}")
rows = [(name, rules[name][1], rules[name][2]) for name in names]
rows += [(f"{baselines.RANDOM_BEST} K={P}", rnd[baselines.RANDOM_BEST][1], rnd[baselines.RANDOM_BEST][2])]
rows += [(k, s[k][1], s[k][2]) for k, s in searched.items()]
for name, f4, ob in rows:
    print(f"{name:<22}{ob.mean():>12.2f}{f4[:, 0].mean():>12.2f}{f4[:, 1].mean():>12.2f}{f4[:, 2].mean():>12.2f}{f4[:, 3].mean():>12.2f}")
print(f"best rule per instance: mean Objective {rule_obj.min(0).mean():.2f}")
for k, s in searched.items():
    print(f"{k}: mean Objective {s['start_obj'].mean():.2f} -> " + " -> ".join(f"{s['history'][r - 1].mean():.2f} ({r})" for r in sorted({min(8, G), G}) if r))
