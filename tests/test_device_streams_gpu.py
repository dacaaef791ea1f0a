"""GPU: every random stream of the device equals its host model (tests/device_streams_ref.py, pinned by tests/test_device_streams_cpu.py)
element for element — reward weights (k_draw_w3 and the one-launch episode reset), the instance generator (k_generate), the random
policy (k_random_actions) and the MOR shuffle of the dispatch-rule planner (k_pdr_plan).  No statistical tolerance: the streams are
integer arithmetic plus single IEEE operations, and the library is built without floating-point contraction."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest

import mtfjsp_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_streams_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")

SEEDS = (0, 11, (1 << 32) + 5, (1 << 63) + 1)
EPISODES = (0, 1, (1 << 32) + 3)


def _same(name, got, want):
    """np.array_equal, saying on failure how many elements differ and by how many units in the last place (a difference confined to
    the last bit of t / p would point at a contracted multiply-add in the build, not at the stream)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = got != want
    msg = f"{name}: {int(bad.sum())} of {bad.size} elements differ; first at {tuple(int(x) for x in np.argwhere(bad)[0])}: device {got[bad][0]!r}, model {want[bad][0]!r}"
    if got.dtype == np.float64:
        ulps = np.abs(got[bad] - want[bad]) / np.spacing(np.abs(want[bad]))
        msg += f"; largest difference {float(ulps.max()):.3g} ulps"
    raise AssertionError(msg)


@pytest.mark.parametrize("B", [1, 63, 257, 20000])
def test_reward_weights_equal_the_model(B):
    import torch
    env = batch_env.DeviceBatchEnv(6, 6, 2, B, obs_dtype="f32")
    env.generate_instances(seed=1)
    env.scaler_init()
    seen = set()
    for seed in SEEDS:
        for ep in EPISODES:
            want = ref.draw_w3(B, seed, ep)
            _same(f"draw_reward_weights(seed={seed}, episode={ep})", env.draw_reward_weights(seed, ep).cpu().numpy(), want)
            w = env.reset_episode(seed, ep)
            torch.cuda.synchronize()
            _same(f"reset_episode(seed={seed}, episode={ep})", w.cpu().numpy(), want)
            _same("the weights the reset stored", env.read_state(capi.STATE_W3), want)
            seen.add(want.tobytes())
    assert len(seen) == len(SEEDS) * len(EPISODES), "every word of seed and episode must matter"
    env.close()


def _read(env):
    B, T, M = env.B, env.T, env.M
    t = np.zeros((B, T, M)); p = np.zeros((B, T, M)); tt = np.zeros((B, M, M)); shop = np.zeros((B, M), np.int32)
    capi.check(env.L.mtfjsp_read_instances_host(env.h, t.ctypes.data, p.ctypes.data, tt.ctypes.data, shop.ctypes.data), env.h)
    return t, p, tt, shop


@pytest.mark.parametrize("J,M,E,B", [(6, 6, 2, 4096), (10, 10, 2, 257), (20, 20, 4, 33), (3, 4, 2, 7), (13, 5, 1, 2), (4, 8, 2, 3)])
def test_generated_instances_equal_the_model(J, M, E, B):
    env = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype="f32")
    cases = [(5, 0, None), (5, 5, None), (5, (1 << 32) + 7, None), ((1 << 40) + 9, 5, None),
             (6, 2, dict(t_low=3, t_high=40, p_low=2, p_high=9, weight_low=0.5, weight_high=1.5, transT_in_low=2, transT_in_high=7, transT_out_high=31))]
    for seed, first, scope in cases:
        env.generate_instances(seed=seed, first_instance=first, scope=scope)
        got = _read(env)
        want = ref.generate(B, J, M, E, seed, first_instance=first, scope=scope)
        for name, g, w in zip(("t", "p", "tt", "shop"), got, want):
            _same(f"J{J}M{M}E{E} x {B}, seed {seed}, first_instance {first}, scope {scope}: {name}", g, w)
    env.close()


@pytest.mark.parametrize("J,M,E,B", [(6, 6, 2, 333), (20, 20, 4, 9), (13, 5, 1, 2)])
def test_random_policy_equals_the_model_along_an_episode(J, M, E, B):
    """every step's (task, machine, job) from the environment's own candidate / job_mask / t; the last steps (one unmasked job) included"""
    import torch
    T = J * M
    env = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype="f32")
    env.generate_instances(seed=21)
    t = _read(env)[0]
    env.scaler_init()
    env.reset(env.draw_reward_weights(3, 0))
    seed, c0 = (1 << 32) + 9, (1 << 32) - 5                              # (the counter's high word changes on the way)
    a = torch.zeros(B, dtype=torch.int32, device=env.device); m = torch.zeros_like(a); j = torch.zeros_like(a)
    flags = torch.zeros_like(a)
    single = 0
    for s in range(T):
        cand, jmask = env.candidate.cpu().numpy(), env.job_mask.cpu().numpy()
        env.random_actions(seed, c0 + s, a, m, j)
        wa, wm, wj = ref.random_actions(t, cand, jmask, seed, c0 + s)
        _same(f"step {s}: job", j.cpu().numpy(), wj)
        _same(f"step {s}: task", a.cpu().numpy(), wa)
        _same(f"step {s}: machine", m.cpu().numpy(), wm)
        single += int(((jmask == 0).sum(1) == 1).sum())
        env.step(a, m)
        flags |= env.status
    assert single >= B, "every instance ends with one unmasked job"
    assert bool(env.info[:, 1].all().item()) and int((flags & (capi.ST_INVALID | capi.ST_INFEASIBLE)).ne(0).sum().item()) == 0
    env.close()


@pytest.mark.parametrize("J,M,E,N", [(6, 6, 2, 64), (10, 10, 2, 17)])
@pytest.mark.parametrize("seed", [3, (1 << 32) + 3])
def test_mor_plans_use_the_model_shuffle(J, M, E, N, seed):
    """pdr_baselines with mor_order=None: the task order of the two MOR rules is the model's shuffle of THEIR rows of the 12 N batch"""
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=35)
    args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
    out = baselines.pdr_baselines(t, p, tt, edge, args, mor_order=None, seed=seed)
    want = ref.mor_order(12 * N, J, M, seed)
    n_mor = 0
    for r, (rule, o, _) in enumerate(baselines.RULES):
        if o != 1:
            continue
        n_mor += 1
        task = out[baselines.PLANS][rule][0].reshape(N, M, J)
        _same(f"{rule}: column of every planned task", task % M, np.broadcast_to(np.arange(M)[None, :, None], task.shape))
        _same(f"{rule}: job order per column", task // M, want[r * N:(r + 1) * N])
    assert n_mor == 2
    # ... and the planner alone, one rule for the whole batch (block index = instance)
    env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False)
    env.load_instances(t, p, tt, edge=edge)
    task = baselines.pdr_plan(env, 1, 0, seed=seed)[0].cpu().numpy().reshape(N, M, J)
    _same("pdr_plan: job order per column", task // M, ref.mor_order(N, J, M, seed))
    env.close()
