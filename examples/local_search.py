#!/usr/bin/env python3
"""Local search on plans beside the rules it starts from: the MOR+SPT dispatch rule and the best of K random episodes, each improved by
baselines.local_search (K neighbours of every instance's incumbent per round — one SWAP / INSERT of the job string or one REASSIGN of a
task's machine each —, replayed side by side by the step kernel, the best kept), one table in the layout of examples/pdr_baselines.py.
Every start is searched twice: with the three undirected moves (ALL_MOVES), and with the two moves a critical path of the incumbent's
schedule directs as well (ALL_MOVES | CRIT_MOVES; rows "LS+C").
The instances are generated on the device; everything runs with left shift off, as the dispatch rules do.

    python examples/local_search.py [--instances 1024] [--size 6 6 2] [--copies 32] [--rounds 32]
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
ap.add_argument("--copies", type=int, default=32)
ap.add_argument("--rounds", type=int, default=32)
a = ap.parse_args()
(J, M, E), N, K, R = a.size, a.instances, a.copies, a.rounds
args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}

env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
env.generate_instances(seed=2024)
rules = baselines.pdr_baselines(None, None, None, None, args, env=env, seed=0)      # 12 rollouts of N on the generated batch
t, p, tt, edge = env.read_instances()
env.close()
rnd = baselines.random_baselines(t, p, tt, edge, args, K=K, seed=0)                 # the random rule, best of K episodes

searched, walls = {}, {}
for name, res in (("MOR+SPT", rules), (baselines.RANDOM_BEST, rnd)):
    for tag, moves in (("LS", baselines.ALL_MOVES), ("LS+C", baselines.ALL_MOVES | baselines.CRIT_MOVES)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        searched[f"{tag}({name})"] = baselines.local_search(t, p, tt, edge, args, res[baselines.PLANS][name], K=K, rounds=R, seed=0, moves=moves,
                                                            name=f"{tag}({name})")
        walls[f"{tag}({name})"] = time.perf_counter() - t0

print(f"{N} instances J{J}M{M}E{E}, {R} rounds of {K} neighbours: " + ", ".join(f"{k} in {v * 1e3:.1f} ms" for k, v in walls.items()))
print(f"{'method':<22}{'objective':>12}{'makespan':>12}{'energy':>12}{'transport':>12}{'idle':>12}")
rows = [(name, rules[name][1], rules[name][2]) for name, _, _ in baselines.RULES]
rows += [(f"{baselines.RANDOM_BEST} K={K}", rnd[baselines.RANDOM_BEST][1], rnd[baselines.RANDOM_BEST][2])]
rows += [(k, s[k][1], s[k][2]) for k, s in searched.items()]
for name, f4, ob in rows:
    print(f"{name:<22}{ob.mean():>12.2f}{f4[:, 0].mean():>12.2f}{f4[:, 1].mean():>12.2f}{f4[:, 2].mean():>12.2f}{f4[:, 3].mean():>12.2f}")
for k, s in searched.items():
    acc = s["accepted"]
    print(f"{k}: mean Objective {s['start_obj'].mean():.2f} -> " + " -> ".join(f"{s['history'][r - 1].mean():.2f} (round {r})" for r in sorted({min(8, R), R}) if r) +
          f"; accepted SWAP {int((acc == baselines.MOVE_SWAP).sum())}, INSERT {int((acc == baselines.MOVE_INSERT).sum())}, "
          f"REASSIGN {int((acc == baselines.MOVE_REASSIGN).sum())}, CRIT_SWAP {int((acc == baselines.MOVE_CRIT_SWAP).sum())}, "
          f"CRIT_REASSIGN {int((acc == baselines.MOVE_CRIT_REASSIGN).sum())}, no move in {int((acc == -1).sum())} of {acc.size} instance-rounds")
