"""GPU: mtfjsp_observe_mfea1_jobs — the machine actor's first input for EVERY job's candidate task in one launch — equals, bit for
bit, J calls of mtfjsp_observe_mfea1 (task_idx = candidate[:, j], no mask given).  Shapes: the base shape, one whose (job, machine)
rows straddle a 256-thread block unevenly (J3M11), more jobs than a wave (J65M2), the widest machine set (J4M64); both observation
dtypes; states after 0, 1 and T-1 random steps (finished jobs present); batch 5."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"J6M6": (6, 6, 2), "J3M11": (3, 11, 1), "J65M2": (65, 2, 2), "J4M64": (4, 64, 2)}
B = 5


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


def _env(batch_env, J, M, E, obs, seed=11):
    env = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype=obs)
    env.generate_instances(seed); env.scaler_init()
    env.reset(torch.tensor([[0.4, 0.4, 0.2]], dtype=torch.float64, device=env.device).repeat(B, 1))
    return env


def _bits(x):
    a = np.ascontiguousarray(x.cpu().numpy())
    return a.view(np.int32 if a.dtype == np.float32 else np.int64 if a.dtype == np.float64 else a.dtype)


def _check(env, tag):
    J = env.J
    out, mm = env.observe_mfea1_jobs()
    got, got_m = _bits(out), mm.cpu().numpy()
    for j in range(J):
        env.observe_mfea1(env.candidate[:, j].contiguous())
        assert np.array_equal(got[:, j], _bits(env.m_fea1)), f"{tag}: m_fea1 of job {j}"
        assert np.array_equal(got_m[:, j], env.mmask.cpu().numpy()), f"{tag}: machine mask of job {j}"


@pytest.mark.parametrize("obs", ["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_job_row_equals_observe_mfea1(shape, obs):
    batch_env, capi = _mods()
    J, M, E = SHAPES[shape]
    T = J * M
    env = _env(batch_env, J, M, E, obs)
    task = torch.zeros(B, dtype=torch.int32, device=env.device); mach = torch.zeros_like(task); job = torch.zeros_like(task)
    _check(env, f"{shape} {obs} after 0 steps")
    for s in range(T - 1):
        env.random_actions(5, s, task, mach, job)
        env.step(task, mach)
        if s == 0:
            _check(env, f"{shape} {obs} after 1 step")
    assert not (env.status.cpu().numpy() & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any()
    assert env.job_mask.cpu().numpy().sum(1).min() >= J - 1, "finished jobs are present"
    _check(env, f"{shape} {obs} after T-1 steps")
    env.close()


@pytest.mark.parametrize("obs", ["f32", "f64"])
def test_an_index_outside_the_tasks_is_treated_as_observe_mfea1_treats_it(obs):
    batch_env, _ = _mods()
    J, M, E = SHAPES["J6M6"]
    env = _env(batch_env, J, M, E, obs)
    task = torch.zeros(B, dtype=torch.int32, device=env.device); mach = torch.zeros_like(task)
    env.random_actions(5, 0, task, mach)
    env.step(task, mach)
    keep = env.candidate.clone()
    env.candidate[:, 0] = -1
    env.candidate[:, J - 1] = J * M + 3
    env.candidate[2, 1] = J * M
    _check(env, f"{obs} out-of-range candidates")
    env.candidate.copy_(keep)
    env.close()


def test_error_returns_write_nothing():
    batch_env, capi = _mods()
    J, M, E = SHAPES["J6M6"]
    env = _env(batch_env, J, M, E, "f32")
    L, n = env.L, B * J * M
    buf = torch.full((n * 6 * 4 + n,), 0x5A, dtype=torch.uint8, device=env.device)
    mm = torch.full((n,), 0x5A, dtype=torch.uint8, device=env.device)
    assert L.mtfjsp_observe_mfea1_jobs(env.h, C.c_void_p(None), mm.data_ptr()) == capi.ERR_ARG
    assert L.mtfjsp_observe_mfea1_jobs(env.h, buf.data_ptr(), buf.data_ptr() + n * 6 * 4 - 1) == capi.ERR_ARG     # the mask starts inside out
    assert b"overlap" in L.mtfjsp_last_error(env.h)
    assert L.mtfjsp_observe_mfea1_jobs(env.h, buf.data_ptr() + 8, buf.data_ptr()) == capi.ERR_ARG                  # out starts inside the mask
    fresh = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype="f32")
    fresh.generate_instances(11)
    assert L.mtfjsp_observe_mfea1_jobs(fresh.h, buf.data_ptr(), mm.data_ptr()) == capi.ERR_STATE                   # never reset
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all() and (mm.cpu().numpy() == 0x5A).all()
    # the same buffers take a valid call: the mask right behind out, and no mask at all
    assert L.mtfjsp_observe_mfea1_jobs(env.h, buf.data_ptr(), buf.data_ptr() + n * 6 * 4) == capi.OK
    assert L.mtfjsp_observe_mfea1_jobs(env.h, buf.data_ptr(), C.c_void_p(None)) == capi.OK
    torch.cuda.synchronize()
    want, want_m = env.observe_mfea1_jobs()
    assert np.array_equal(buf[:n * 6 * 4].cpu().numpy(), want.cpu().numpy().view(np.uint8).reshape(-1))
    assert np.array_equal(buf[n * 6 * 4:].cpu().numpy(), want_m.cpu().numpy().reshape(-1))
    fresh.close(); env.close()
