#!/usr/bin/env python3
"""Measurements behind profiles/walk_search.json: baselines.walk_search beside baselines.local_search, J6M6E2 x 4096
device-generated instances, K = 16 copies, 32 rounds, starts = the MOR+SPT plans (the method of tools/profile_critical_search.py).

  --mode trace    local_search and walk_search (the tabu setting: the ring in use) twice, 8 rounds each; the first run of either warms up.  Run it under
                  `rocprofv3 --kernel-trace --stats` (program directly after `--`, no counters): k_walk_accept, k_group_reduce and
                  k_state_signature are read from the trace by --mode reduce.
  --mode wall     wall time of local_search and walk_search (the tabu setting, 32 rounds), alternating, --reps each after one warm-up of either: one
                  round's total.
  --mode quality  mean final Objective, share of instances improved and the counts of `accepted` / `why` for local_search and three
                  settings of walk_search (SETTINGS below), under w = (1, 0, 0) and the configured (0.4, 0.4, 0.2), left shift off and on;
                  and, left shift off, the same at 128 rounds.
  --mode reduce   the trace under --out-dir + the wall and quality json -> --out
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J, M, E, N = 6, 6, 2, 4096
T = J * M
K, ROUNDS, TRACE_ROUNDS, LONG_ROUNDS = 16, 32, 8, 128
CONFIG_W = (0.4, 0.4, 0.2)
# the three ways out of a local optimum, each alone: a ring of schedules with "always move"; the incumbent of L rounds ago as the bar;
# a threshold that falls linearly from 5 % of the start's mean Objective to 0 (the last round admits sideways steps only)
SETTINGS = {"tabu": dict(tabu=8, slack=float("inf"), late=0), "late": dict(tabu=0, slack=None, late=8), "threshold": dict(tabu=0, slack="falling", late=0)}
THRESHOLD_SHARE = 0.05


def _args(w):
    return {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": w[0], "weight_ec": w[1], "weight_tt": w[2]}


def _setup():
    sys.path.insert(0, ROOT)
    import torch
    import mtfjsp_amd  # noqa: F401
    from importlib import import_module
    mods = {k: import_module("e2e-mappo-for-mt-fjsp_amd." + k) for k in ("baselines", "batch_env")}
    if not torch.cuda.is_available():
        raise SystemExit("profile_walk_search.py needs the GPU: there is nothing to measure without it")
    env = mods["batch_env"].DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    env.generate_instances(seed=2024)
    bl = mods["baselines"]
    rule = bl.pdr_baselines(None, None, None, None, _args(CONFIG_W), env=env, rules=[r for r in bl.RULES if r[0] == "MOR+SPT"], seed=0)
    data = env.read_instances()
    env.close()
    return torch, bl, data, rule[bl.PLANS]["MOR+SPT"]


def _setting(name, start_mean, rounds=ROUNDS):
    kw = dict(SETTINGS[name])
    if kw["slack"] == "falling":
        top = THRESHOLD_SHARE * start_mean
        kw["slack"] = [top * (rounds - 1 - r) / max(rounds - 1, 1) for r in range(rounds)]
    return kw


def mode_trace():
    torch, bl, data, start = _setup()
    for _ in range(2):                                     # run 0 warms up
        bl.local_search(*data, _args(CONFIG_W), start, K=K, rounds=TRACE_ROUNDS, seed=0)
        torch.cuda.synchronize()
        bl.walk_search(*data, _args(CONFIG_W), start, K=K, rounds=TRACE_ROUNDS, seed=0, **SETTINGS["tabu"])
        torch.cuda.synchronize()


def mode_wall(reps):
    torch, bl, data, start = _setup()
    runs = {"local_search": lambda: bl.local_search(*data, _args(CONFIG_W), start, K=K, rounds=ROUNDS, seed=0),
            "walk_search": lambda: bl.walk_search(*data, _args(CONFIG_W), start, K=K, rounds=ROUNDS, seed=0, **SETTINGS["tabu"])}
    walls = {k: [] for k in runs}
    for i in range(reps + 1):                              # the first call of either is the warm-up; then alternating
        for k, run in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            run()
            if i:
                walls[k].append(time.perf_counter() - t0)
    res = {"shape": "J6M6E2", "N": N, "K": K, "rounds": ROUNDS, "reps": reps,
           "what": "wall time from the MOR+SPT plans, handles, upload and final replay included, the two searches alternating; per round = median / rounds"}
    for k, v in walls.items():
        med = sorted(v)[len(v) // 2]
        res[k] = {"launches_per_round": T + (4 if k == "local_search" else 5), "wall_s_all": v, "wall_s_median": med, "round_ms": med / ROUNDS * 1e3}
    res["walk_minus_local_round_us"] = (res["walk_search"]["round_ms"] - res["local_search"]["round_ms"]) * 1e3
    return res


def _counts(x, keys):
    return {str(k): int((x == k).sum()) for k in keys}


def mode_quality():
    torch, bl, data, start = _setup()
    out = {"shape": "J6M6E2", "N": N, "K": K, "rounds": ROUNDS, "long_rounds": LONG_ROUNDS, "seed": 0, "start": "MOR+SPT (left shift off)",
           "settings": {k: {a: (str(b) if isinstance(b, float) else b) for a, b in v.items()} for k, v in SETTINGS.items()},
           "threshold": f"slack falls linearly from {THRESHOLD_SHARE} * mean start Objective to 0 over the rounds",
           "what": "mean Objective of the result (walk_search: the best plan met; lower is better), the share of instances below the start's, the "
                   "mean Objective of the last incumbents, and counts over the rounds x instances of accepted (move kind, -1 stayed) and why (& 7; "
                   "new_best: why & 8) and the sum of barred"}
    for left_shift, rounds in ((False, ROUNDS), (True, ROUNDS), (False, LONG_ROUNDS)):     # (the long runs: for information, where hill climbing has stalled)
        for w in ((1.0, 0.0, 0.0), CONFIG_W):
            key = f"left_shift_{int(left_shift)}/w_{w[0]}_{w[1]}_{w[2]}" + ("" if rounds == ROUNDS else f"/rounds_{rounds}")
            r = bl.local_search(*data, _args(w), start, K=K, rounds=rounds, seed=0, left_shift=left_shift)
            start_mean = float(r["start_obj"].mean())
            out[key + "/local_search"] = {"start_objective": start_mean, "final_objective": float(r["LS"][2].mean()),
                                          "share_improved": float((r["LS"][2] < r["start_obj"]).mean()),
                                          "accepted": _counts(r["accepted"], (-1, 1, 2, 4))}
            for name in SETTINGS:
                r = bl.walk_search(*data, _args(w), start, K=K, rounds=rounds, seed=0, left_shift=left_shift, **_setting(name, start_mean, rounds))
                out[f"{key}/walk_{name}"] = {"start_objective": float(r["start_obj"].mean()), "final_objective": float(r["WS"][2].mean()),
                                             "share_improved": float((r["WS"][2] < r["start_obj"]).mean()),
                                             "last_incumbent_objective": float(r["current"][-1].mean()),
                                             "accepted": _counts(r["accepted"], (-1, 1, 2, 4)), "why": _counts(r["why"] & 7, (0, 1, 2, 3, 4)),
                                             "new_best": int(((r["why"] & 8) != 0).sum()), "barred": int(r["barred"].sum())}
    return out


KERNELS = {"k_walk_accept": ("k_walk_accept",), "k_group_reduce": ("k_group_reduce",), "k_state_signature": ("k_state_signature", "k_signature")}


def _durations(trace_dir):
    fs = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    dur = {}
    if not fs:
        return dur
    for r in sorted(csv.DictReader(open(fs[0])), key=lambda r: int(r["Start_Timestamp"])):
        key = next((k for k, names in KERNELS.items() if any(n in r["Kernel_Name"] for n in names)), None)
        if key:
            dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return dur


def _stat(v):
    return {"launches": len(v), "median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def mode_reduce(out_dir, out):
    res = {"shape": "J6M6E2", "N": N, "K": K, "groups_per_launch": N,
           "method": "rocprofv3 --kernel-trace --stats, no counters, a run of its own; the launches of the second (warm) run of either search"}
    kt = {}
    for key, v in _durations(os.path.join(out_dir, "walk_trace")).items():
        kt[key + "_us"] = _stat(v[-TRACE_ROUNDS:]) if len(v) >= 2 * TRACE_ROUNDS else {"unmeasured": f"{len(v)} launches in the trace"}
    res["kernel_times"] = kt or {"unmeasured": "no kernel trace"}
    for name in ("wall", "quality"):
        path = os.path.join(out_dir, f"walk_{name}.json")
        res[name] = json.loads(open(path).read()) if os.path.exists(path) else {"unmeasured": "not run"}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "quality"}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trace", "wall", "quality", "reduce"], required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-dir", default=os.environ.get("MTFJSP_TOOL_OUT", "tool_out"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "trace":
        mode_trace()
    elif a.mode in ("wall", "quality"):
        line = json.dumps(mode_wall(a.reps) if a.mode == "wall" else mode_quality())
        print(line)
        os.makedirs(a.out_dir, exist_ok=True)
        open(os.path.join(a.out_dir, f"walk_{a.mode}.json"), "w").write(line + "\n")
    else:
        mode_reduce(a.out_dir, a.out or os.path.join(a.out_dir, "walk_search.json"))
