"""GPU: baselines.policy_beam / PolicyBeamSearch — beam decoding of the actors — on the first 4 instances of
tests/golden/trace_j6m6e2_eval16_free.npz with the random and the trained J6M6E2 weights, W = 1, 3, 8, merging on and off, and one
chunked run.  The actors' numbers are the device's own; what is held to a host model (tests/policy_beam_ref.py), exactly, is
everything the search does with them: every decision's selection (seven outputs, the scores to their bits), the merge, the
back-pointers.  The wiring of the forwards is checked bitwise (the machine forward's inputs of row slot*J + j, the embedding a
slot carries), both returned plans give the returned costs through the C oracle to the bit, and PB_TOP's plan, teacher-forced
through `validate_cost_batched`, meets the search's probabilities of the chosen actions within the margins
tests/test_eval_per_instance_bn.py grants two implementations of the per-instance forwards (2e-4 job, 1e-4 machine).  Observed on
the MI355X: 0.0 for both in all 13 cases (the per-instance forwards run one workgroup per instance and do not depend on the batch);
the figures are printed per case and recorded in profiles/policy_beam.json."""
import os
from importlib import import_module

import numpy as np
import pytest

import policy_beam_ref as ref
from env_parity import _same

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
N = 4
JOB_ATOL, MACH_ATOL = 2e-4, 1e-4
CASES = [(tag, W, dedupe, None) for tag in ("rand", "top1") for W in (1, 3, 8) for dedupe in (True, False)] + [("top1", 3, True, 2 * 3 * 6)]
KEEP = ("candidate", "job_mask", "mmask", "logp_job", "logp_mach", "job_prob", "mch_prob", "m_fea2", "m_fea2_rows", "h_o", "h_o_rows",
        "h_mach", "h_m", "h_m_prev", "sig", "score_in", "score_selected", "score_out", "parent", "from_slot", "job", "task", "mach", "child")


def _setup(tag):
    import mtfjsp_amd  # noqa: F401
    from oracle import encoder_oracle as eo
    g = np.load(os.path.join(GOLDEN, "trace_j6m6e2_eval16_free.npz"))
    w = np.load(os.path.join(GOLDEN, f"encoder_j6m6e2_{tag}.npz"))
    J, M, E = 6, 6, 2
    cfg = [float(x) for x in g["cfg_w"][:3]]
    args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": cfg[0], "weight_ec": cfg[1], "weight_tt": cfg[2]}
    return (g["t"][:N], g["p"][:N], g["tt"][:N], g["edge"][:N]), eo.split_weights(w), args, (J, M, E)


def _bits(x):
    a = np.ascontiguousarray(x)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.mark.parametrize("tag,W,dedupe,chunk", CASES, ids=[f"{t}-W{w}-{'dedupe' if d else 'plain'}{'-chunked' if c else ''}" for t, w, d, c in CASES])
def test_policy_beam_equals_the_model_and_its_plans_cost_what_it_says(tag, W, dedupe, chunk):
    from oracle.env_oracle import OracleBatch
    baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
    ev = import_module("e2e-mappo-for-mt-fjsp_amd.evaluate")
    data, weights, args, (J, M, E) = _setup(tag)
    T = J * M
    passes = []                                                             # per pass: the decisions' host copies

    def on_decision(s, tensors):
        if s == 0:
            passes.append([])
        passes[-1].append({k: None if tensors[k] is None else tensors[k].cpu().numpy().copy() for k in KEEP})

    res = baselines.policy_beam(weights, *data, args, width=W, dedupe=dedupe, chunk=chunk, on_decision=on_decision)
    assert sorted(res) == sorted([baselines.PB_TOP, baselines.PB_BEST, baselines.PLANS, "logp"])
    assert len(passes) == (1 if chunk is None else 2) and all(len(x) == T for x in passes)
    top_path = []                                                           # per pass: [n, T] probabilities of PB_TOP's chosen actions
    merged = 0
    for recs in passes:
        NW = recs[0]["score_in"].shape[0]
        n = NW // W
        model = ref.Search(n, W, dedupe)
        for s, r in enumerate(recs):
            tag_s = f"decision {s}"
            # ---- the selection, the merge: exact
            _same(_bits(r["score_in"]), _bits(model.score), f"{tag_s}: scores on entry (bits)")
            with np.errstate(invalid="ignore"):
                want = model.decide(r["logp_job"], r["logp_mach"], r["job_mask"], r["mmask"].reshape(NW * J, M), r["candidate"],
                                    None if r["sig"] is None else r["sig"].view(np.uint64))
            for k in ("parent", "from_slot", "job", "task", "mach", "child"):
                _same(r[k], want[k], f"{tag_s}: {k}")
            _same(_bits(r["score_selected"]), _bits(want["score"]), f"{tag_s}: selected scores (bits)")
            _same(_bits(r["score_out"]), _bits(want["merged"]), f"{tag_s}: merged scores (bits)")
            # ---- the logarithms are torch.log of the binary64 probabilities: -inf exactly where the probability is 0
            assert np.array_equal(np.isneginf(r["logp_job"]), r["job_prob"] == 0) and np.array_equal(np.isneginf(r["logp_mach"]), r["mch_prob"] == 0)
            # ---- wiring, bitwise: row slot*J + j of the machine forward sees slot's machines and slot's job embedding
            slot = np.arange(NW * J) // J
            _same(_bits(r["m_fea2_rows"]), _bits(r["m_fea2"][slot]), f"{tag_s}: m_fea2 of the machine forward's rows")
            _same(_bits(r["h_o_rows"]), _bits(r["h_o"][slot]), f"{tag_s}: h_pooled of the machine forward's rows")
            live = r["parent"] >= 0
            _same(_bits(r["h_m"][live]), _bits(r["h_mach"][r["child"][live]]), f"{tag_s}: the embedding a new slot carries")
            assert np.array_equal(r["child"][live], r["parent"][live] * J + r["job"][live])
            if s == 0:
                assert r["h_m_prev"] is None
            else:
                _same(_bits(r["h_m_prev"]), _bits(recs[s - 1]["h_m"]), f"{tag_s}: the job forward's h_m_prev")
            merged += int((_bits(r["score_out"]) != _bits(r["score_selected"])).sum())
            if dedupe:                                                      # live slots of one instance hold distinct schedules
                sig, alive = r["sig"].reshape(n, W), np.isfinite(r["score_out"]).reshape(n, W)
                for i in range(n):
                    assert len(set(sig[i][alive[i]])) == alive[i].sum(), f"{tag_s} instance {i}: two live slots with one signature"
        # PB_TOP's path through the back-pointers, and the search's probabilities of its actions
        k = np.zeros(n, np.int64)
        pj, pm = np.zeros((n, T)), np.zeros((n, T))
        for s in range(T - 1, -1, -1):
            r, i = recs[s], np.arange(n) * W + k
            pj[:, s], pm[:, s] = r["job_prob"][r["parent"][i], r["job"][i]], r["mch_prob"][r["child"][i], r["mach"][i]]
            k = r["from_slot"][i]
        top_path.append((model, pj, pm))
    # ---- the plans: the model's, and through the C oracle the returned costs, to the bit
    t, p, tt, edge = data
    w_cfg = (args["weight_mk"], args["weight_ec"], args["weight_tt"])
    lo = 0
    for model, _, _ in top_path:
        n = model.N
        want_t, want_m = model.plan(np.zeros(n, np.int64))
        _same(res[baselines.PLANS][baselines.PB_TOP][0][lo:lo + n], want_t, "PB_TOP plan: tasks")
        _same(res[baselines.PLANS][baselines.PB_TOP][1][lo:lo + n], want_m, "PB_TOP plan: machines")
        _same(_bits(res["logp"][lo:lo + n].reshape(-1)), _bits(model.score), "logp (bits)")
        lo += n
    w3 = np.tile(np.array([w_cfg]), (N, 1))
    for name in (baselines.PB_TOP, baselines.PB_BEST):
        task, mach = res[baselines.PLANS][name]
        assert task.shape == (N, T) and (task >= 0).all()
        orc = OracleBatch(t, p, tt, edge, left_shift=True, w_cfg=w_cfg); orc.scaler_init(); orc.reset(w3)
        cum = np.zeros((N, 5))
        for s in range(T):
            cum += orc.step(task[:, s], mach[:, s])[1]
        prev = orc.state()["prev"]
        cost, final4, obj = res[name]
        for k, key in enumerate(ev.COST_KEYS):
            _same(cost[key], cum[:, k], f"{name} {key}")
        want4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
        _same(final4, want4, f"{name} Final_4cost")
        _same(obj, w_cfg[0] * want4[:, 0] + w_cfg[1] * (want4[:, 1] + want4[:, 3]) + w_cfg[2] * want4[:, 2], f"{name} Objective")
    assert (res[baselines.PB_BEST][2] <= res[baselines.PB_TOP][2]).all()
    if W == 1:
        _same(res[baselines.PB_BEST][2], res[baselines.PB_TOP][2], "W = 1: one slot")
    # ---- forced replay of PB_TOP's plan: the sequential evaluation's probabilities of the chosen actions
    task, mach = res[baselines.PLANS][baselines.PB_TOP]
    worst = {"job": 0.0, "mach": 0.0, "steps": 0}
    pj, pm = np.concatenate([x[1] for x in top_path]), np.concatenate([x[2] for x in top_path])

    def on_step(s, job_prob, mch_prob):
        a, b = job_prob.cpu().numpy(), mch_prob.cpu().numpy()
        worst["job"] = max(worst["job"], np.abs(a[np.arange(N), task[:, s] // M] - pj[:, s]).max())
        worst["mach"] = max(worst["mach"], np.abs(b[np.arange(N), mach[:, s]] - pm[:, s]).max())
        worst["steps"] += 1

    _, final4, obj = ev.validate_cost_batched(weights, t, p, tt, edge, args, forced_actions=np.stack([task, mach], 2), on_step=on_step)
    print(f"policy_beam forced replay {tag} W={W} dedupe={dedupe} chunk={chunk}: max |dp| job {worst['job']:.3e} machine {worst['mach']:.3e}")
    _same(obj, res[baselines.PB_TOP][2], "the forced replay's Objective")
    assert worst["steps"] == T and (pj > 0).all() and (pm > 0).all()
    assert worst["job"] < JOB_ATOL and worst["mach"] < MACH_ATOL, worst
    print(f"  slots emptied by the merge: {merged}")
    assert merged == 0 if not dedupe or W == 1 else True
    if dedupe and W == 8:
        assert merged > 0, "at W = 8 several orders of the same decisions meet in one schedule"


def test_width_limits_and_restart():
    import torch
    baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    ev = import_module("e2e-mappo-for-mt-fjsp_amd.evaluate")
    data, weights, args, (J, M, E) = _setup("rand")
    t, p, tt, edge = data
    env = batch_env.DeviceBatchEnv(J, M, E, N, obs_dtype="f32")
    env.load_instances(t, p, tt, edge=edge)
    ev.eval_reset(env, ev.config_w3(env, (0.4, 0.4, 0.2)))
    with pytest.raises(ValueError):
        baselines.PolicyBeamSearch(env, weights, 65)
    with pytest.raises(ValueError):
        baselines.PolicyBeamSearch(env, weights, 0)
    pb = baselines.PolicyBeamSearch(env, weights, 2)
    with pytest.raises(ValueError):
        pb.plans()
    t1, m1, s1 = pb.run(5)
    t1, m1, s1 = t1.cpu().numpy(), m1.cpu().numpy(), s1.cpu().numpy().copy()
    assert t1.shape == (N, 5) and (t1 >= 0).all() and np.isfinite(s1[:, 0]).all() and (np.diff(s1, axis=1) <= 0).all()
    pb.restart()
    t2, m2, s2 = pb.run(5)
    torch.cuda.synchronize()
    _same(t2.cpu().numpy(), t1, "restart: tasks"); _same(m2.cpu().numpy(), m1, "restart: machines")
    _same(_bits(s2.cpu().numpy()), _bits(s1), "restart: scores (bits)")
    pb.close(); env.close()
