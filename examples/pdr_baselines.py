#!/usr/bin/env python3
"""The greedy policy, the 12 priority dispatch rules of the reference's test_all.py, the one-step look-ahead rules and beam search on the SAME
instances, one table (paper Tables V / VI).  The instances are generated on the device; the rules are planned there by k_pdr_plan and replayed by the
step kernel with left shift off; the look-ahead rules (baselines.lookahead_baselines) try every (job, machine) on a forked copy per step; beam search
(baselines.beam_baselines, W = 1, 4, 16) keeps the W best partial schedules per instance instead of one; best-of-8 sampling of the policy
(evaluate.sample_best_of_k) and the random rule as best and mean of 8 episodes (baselines.random_baselines) run K copies of every instance.

    python examples/pdr_baselines.py [--instances 1024] [--size 6 6 2]
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
evaluate = import_module("e2e-mappo-for-mt-fjsp_amd.evaluate")
encoder = import_module("e2e-mappo-for-mt-fjsp_amd.encoder")

ap = argparse.ArgumentParser()
ap.add_argument("--instances", type=int, default=1024)
ap.add_argument("--size", type=int, nargs=3, default=[6, 6, 2], metavar=("J", "M", "E"))
a = ap.parse_args()
(J, M, E), N = a.size, a.instances
args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}

env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
env.generate_instances(seed=2024)
torch.cuda.synchronize(); t0 = time.perf_counter()
rules = baselines.pdr_baselines(None, None, None, None, args, env=env, seed=0)      # 12 rollouts of N on the generated batch
t_rules = time.perf_counter() - t0

t, p, tt, edge = env.read_instances()
t0 = time.perf_counter()
look = baselines.lookahead_baselines(t, p, tt, edge, args)                          # 5 rules, N*T forked copies per decision
t_look = time.perf_counter() - t0
t0 = time.perf_counter()
beams = {w: baselines.beam_baselines(t, p, tt, edge, args, width=w) for w in (1, 4, 16)}     # 5 rules each, N*W*T copies per decision
t_beam = time.perf_counter() - t0
weights = encoder.random_init_weights(seed=0)            # or (torch.load(job_actor.pth), torch.load(machine_actor.pth))
t0 = time.perf_counter()
_, final4, obj = evaluate.validate_cost_batched(weights, t, p, tt, edge, args)
t_policy = time.perf_counter() - t0
t0 = time.perf_counter()
bok = evaluate.sample_best_of_k(weights, t, p, tt, edge, args, K=8, seed=0)         # 8 sampled schedules per instance, the best kept
t_bok = time.perf_counter() - t0
t0 = time.perf_counter()
rnd = baselines.random_baselines(t, p, tt, edge, args, K=8, seed=0)                 # the random rule, best and mean of 8 episodes
t_rnd = time.perf_counter() - t0

print(f"{N} instances J{J}M{M}E{E}: 12 rules in {t_rules * 1e3:.1f} ms, {len(baselines.LOOKAHEAD_RULES)} look-ahead rules in {t_look * 1e3:.1f} ms, "
      f"beam search at W = 1, 4, 16 in {t_beam * 1e3:.1f} ms, greedy policy in {t_policy * 1e3:.1f} ms, "
      f"best of 8 samples in {t_bok * 1e3:.1f} ms, best of 8 random episodes in {t_rnd * 1e3:.1f} ms")
print(f"{'method':<18}{'objective':>12}{'makespan':>12}{'energy':>12}{'transport':>12}{'idle':>12}")
rows = [("policy (greedy)", final4, obj), ("policy best-of-8", bok["best"][1], bok["best"][2])]
rows += [(name + " K=8", rnd[name][1], rnd[name][2]) for name in (baselines.RANDOM_BEST, baselines.RANDOM_MEAN)]
rows += [(name, rules[name][1], rules[name][2]) for name, _, _ in baselines.RULES]
rows += [(name, look[name][1], look[name][2]) for name, _ in baselines.LOOKAHEAD_RULES]
rows += [(f"{name} W={w}", beams[w][name][1], beams[w][name][2]) for w in (1, 4, 16) for name, _ in baselines.BEAM_RULES]
for name, f4, ob in rows:
    print(f"{name:<18}{ob.mean():>12.2f}{f4[:, 0].mean():>12.2f}{f4[:, 1].mean():>12.2f}{f4[:, 2].mean():>12.2f}{f4[:, 3].mean():>12.2f}")
