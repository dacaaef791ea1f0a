"""The fixed-shape instantiation of the three-in-one heads launch (k_headsx_gat3x_headsx<0, true, H3ShapeFixed<6, 6, 16>>: csrc/mtfjsp_encoder.hip, the
shape read through the HX_FX / GAT_FX macros of the two body headers) against the run-time instantiation of the same kernel text (forced with
MTFJSP_FUSED3_GENERIC=1): it drops work the result does not need and keeps every product, every exchange word, every Philox counter and every
order of additions — so every output BIT is the same.
  * J6M6E2 x 4096 (for M = 6 on 256 compute units the only batch the launch is eligible for), seeded random weights and the shipped `top1`
    checkpoint, sampled and greedy selection, states from the reset (the learned `_input` row) and after 9, 22 and 35 steps (most jobs finished,
    one candidate left): one joint decision without the environment step per kernel, on identical inputs and counters — every array of the
    job part, of the selection's m_fea1 / machine mask and of the machine part, both sets of exchange words, the time-out / range words.
  * (7, 5, 1) at B = 4096 and J6M6 with f64 observations: the run-time kernel is what runs.
  * two whole episodes in fresh processes, one per kernel: every task, machine, reward and critic array.
Reference: model/actor_critic.py:205-293, 359-498."""
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
J, M, E, B = 6, 6, 2, 4096
T = J * M
GENERIC = "k_headsx_gat3x_headsx"
FIXED = "k_headsx_gat3x_headsx<0, true, H3ShapeFixed<6, 6, 16>>"
SWITCH = "MTFJSP_FUSED3_GENERIC"


def _weights(which):
    if which == "top1":
        from oracle import encoder_oracle as eo
        return eo.split_weights(np.load(os.path.join(GOLDEN, "encoder_j6m6e2_top1.npz")))
    return import_module("e2e-mappo-for-mt-fjsp_amd.encoder").random_init_weights(seed=31)


def _rollout(weights, shape=(J, M, E), obs_dtype="f32", greedy=False, seed=7):
    import mtfjsp_amd  # noqa: F401
    rollout = import_module("e2e-mappo-for-mt-fjsp_amd.rollout")
    return rollout.Rollout(*shape, B, policy="actor", obs_dtype=obs_dtype, weights=weights, collect=False, seed=seed, greedy=greedy)


def _one_decision(ro):
    """one joint decision WITHOUT the env step (the inputs stay in place) -> (kernel that ran, every array the launch left)"""
    e, env, act = ro.actor.enc, ro.env, ro.actor
    n0 = e.fused_launches()
    act.act(env, ro.nsteps, ro.task, ro.mach, ro.job)
    torch.cuda.synchronize()
    assert e.fused_launches() - n0 == 1                            # the decision took the three-in-one launch
    words, flags = e.peek_fused3()
    out = {"job_prob": e.job_prob, "job_v": e.job_v, "job_idx": ro.job, "job_logp": act.job_logp, "task": ro.task,
           "m_fea1": env.m_fea1, "mmask": env.mmask,
           "mch_prob": e.mch_prob, "h_pooled_m": e.h_pooled_m, "mach_v": e.mach_v, "mach_idx": ro.mach, "mch_logp": act.mch_logp}
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out["words"], out["flags"] = words, flags
    return e.fused3_kernel_name(), out


def _both(monkeypatch, ro):
    """the same decision by both kernels: the machine embedding of the previous step (input and output of a decision) is put back in between"""
    e, act = ro.actor.enc, ro.actor
    hm0, have = e.h_pooled_m.clone(), act.have_hm
    monkeypatch.delenv(SWITCH, raising=False)
    ka, a = _one_decision(ro)
    e.h_pooled_m.copy_(hm0); act.have_hm = have
    monkeypatch.setenv(SWITCH, "1")
    kb, b = _one_decision(ro)
    monkeypatch.delenv(SWITCH)
    e.h_pooled_m.copy_(hm0); act.have_hm = have
    torch.cuda.synchronize()
    return ka, a, kb, b


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("which", ["random", "top1"])
def test_fixed_and_run_time_instantiation_give_the_same_bits(monkeypatch, which, greedy):
    monkeypatch.delenv(SWITCH, raising=False)
    ro = _rollout(_weights(which), greedy=greedy)
    env, enc = ro.env, ro.actor.enc
    assert enc.check()                                             # the single-launch kernels are in use: the census passed
    ro.env.scaler_reset_returns(); ro.env.reset(ro._episode_w3()); ro.actor.begin_episode()
    stepped = 0
    want = np.full(8, B // 16 // 8, dtype=np.uint64)               # 256 workgroups: 32 arrivals per dispatch group
    for upto in (0, 9, 22, 35):                                    # the reset, then mid-episode states (step 35: one candidate left)
        while stepped < upto:
            ro.step(); stepped += 1
        torch.cuda.synchronize()
        ka, a, kb, b = _both(monkeypatch, ro)
        assert (ka, kb) == (FIXED, GENERIC), (upto, ka, kb)
        assert int(a["flags"][0]) == 0 and int(a["flags"][1]) == 0 and int(b["flags"][0]) == 0 and int(b["flags"][1]) == 0
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (upto, k)
        assert np.isfinite(a["job_prob"]).all() and np.isfinite(a["mch_prob"]).all() and np.isfinite(a["h_pooled_m"]).all()
        # the exchange is complete: a dispatch group's arrivals in the fine and the wide word of a value together are its workgroup count
        cnt = (a["words"] >> np.uint64(58)).sum(axis=0)
        assert np.array_equal(cnt, np.broadcast_to(want[:, None], cnt.shape)), upto
    assert enc.check() and enc.range_fallbacks()[0] == 0 and ro.n_resident_failures == 0


@pytest.mark.parametrize("shape,obs_dtype", [((7, 5, 1), "f32"), ((6, 6, 2), "f64")])
def test_neighbouring_shapes_pick_the_run_time_kernel(monkeypatch, shape, obs_dtype):
    monkeypatch.delenv(SWITCH, raising=False)
    ro = _rollout(_weights("random"), shape=shape, obs_dtype=obs_dtype)
    for _ in range(3):
        ro.step()
    torch.cuda.synchronize()
    assert ro.actor.enc.check()
    k, out = _one_decision(ro)
    assert k == GENERIC
    assert int(out["flags"][0]) == 0 and int(out["flags"][1]) == 0
    for name in ("job_prob", "job_v", "m_fea1", "mch_prob", "h_pooled_m", "mach_v", "job_logp", "mch_logp"):
        assert np.isfinite(out[name]).all(), name


def test_two_whole_episodes_in_fresh_processes_agree_in_every_array(tmp_path):
    outs = {}
    for name, switch in (("fixed", None), ("generic", "1")):
        env = dict(os.environ)
        env.pop(SWITCH, None)
        if switch:
            env[SWITCH] = switch
        out = str(tmp_path / f"{name}.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused3_episode_child.py"), out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = np.load(out)
    a, b = outs["fixed"], outs["generic"]
    assert str(a["kernel"]) == FIXED and str(b["kernel"]) == GENERIC
    assert bool(a["done"][T - 1].all()) and bool(a["done"][2 * T - 1].all())         # both episodes ended on every instance
    assert bool(b["done"][T - 1].all()) and bool(b["done"][2 * T - 1].all())
    for k in ("task", "mach", "reward", "done", "job_v", "mach_v", "info", "tasks_fea"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
