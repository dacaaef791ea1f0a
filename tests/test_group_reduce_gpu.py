"""GPU: mtfjsp_group_reduce and mtfjsp_final_costs (csrc/mtfjsp_group.hip) EQUAL their host model (tests/group_reduce_ref.py, pinned by
tests/test_group_reduce_cpu.py) bit for bit: every copy's objective, the best copy, its objective and the front flags; no tolerance.
K covers less than a wavefront (1, 5), the ragged last pass (63, 65), exactly one (64), more than one wavefront (257: also the
second owned copy of thread 0), four owned copies per thread (1024) and the limit (4096: sixteen, 128 KB of LDS)."""
from importlib import import_module

import numpy as np
import pytest
import torch

import group_reduce_ref as ref
from env_parity import _same

pytestmark = pytest.mark.gpu

KS = [1, 5, 63, 64, 65, 257, 1024, 4096]
WEIGHTS = {"integer": (0.4, 0.4, 0.2), "scattered": (0.4, 0.4, 0.2), "none": (0.4, 0.4, 0.2), "random": (0.37, 0.0625, 0.5675)}
SENT_F, SENT_I, SENT_B = 123.5, -77, 9


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


@pytest.fixture(scope="module")
def handle():
    batch_env, _ = _mods()
    env = batch_env.DeviceBatchEnv(3, 4, 2, 1)                          # gives the device and the stream only
    yield env
    env.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _sentinels(N, K, dev):
    return (torch.full((N * K,), SENT_F, dtype=torch.float64, device=dev), torch.full((N,), SENT_I, dtype=torch.int32, device=dev),
            torch.full((N,), SENT_F, dtype=torch.float64, device=dev), torch.full((N * K,), SENT_B, dtype=torch.uint8, device=dev))


def _case(handle, kind, N, K):
    cost4, done = ref.synthetic(kind, N, K, seed=7 * K + N)
    w = WEIGHTS[kind]
    want = ref.group_reduce(cost4, done, w, N, K)
    dev = handle.device
    c4, dn = torch.as_tensor(cost4, device=dev), torch.as_tensor(done, device=dev)
    return c4, dn, w, want


@pytest.mark.parametrize("kind", ["integer", "random", "scattered"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_group_reduce_equals_the_model(handle, kind, N, K):
    c4, dn, w, (obj, best, best_obj, front) = _case(handle, kind, N, K)
    outs = _sentinels(N, K, handle.device)
    got = handle.group_reduce(N, K, c4, dn, w, *outs)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, outs))
    tag = f"{kind} N={N} K={K}"
    _same(_bits(got[0].cpu().numpy()), _bits(obj), tag + " obj (bits)")
    _same(got[1].cpu().numpy(), best, tag + " best")
    _same(_bits(got[2].cpu().numpy()), _bits(best_obj), tag + " best_obj (bits)")
    _same(got[3].cpu().numpy(), front, tag + " front")
    if kind == "scattered" and N > 1:
        assert best[1] == -1 and not front[K:2 * K].any(), "group 1 must have no eligible copy"
    if kind == "integer" and K >= 63:
        assert 0 < front.sum() < N * K


@pytest.mark.parametrize("N,K", [(1, 5), (3, 257)])
def test_a_group_without_any_eligible_copy(handle, N, K):
    c4, dn, w, (obj, best, best_obj, front) = _case(handle, "none", N, K)
    got = handle.group_reduce(N, K, c4, dn, w, *_sentinels(N, K, handle.device))
    torch.cuda.synchronize()
    assert np.isnan(got[0].cpu().numpy()).all() and (got[1].cpu().numpy() == -1).all() and np.isnan(got[2].cpu().numpy()).all()
    assert not got[3].cpu().numpy().any() and (best == -1).all()


@pytest.mark.parametrize("keep", range(4), ids=["obj", "best", "best_obj", "front"])
@pytest.mark.parametrize("K", [5, 257, 1024])
def test_null_outputs_are_skipped(handle, keep, K):
    N = 3
    c4, dn, w, want = _case(handle, "scattered", N, K)
    outs = list(_sentinels(N, K, handle.device))
    flags = [outs[i] if i == keep else None for i in range(4)]
    got = handle.group_reduce(N, K, c4, dn, w, *flags)
    torch.cuda.synchronize()
    assert [g is None for g in got] == [i != keep for i in range(4)]
    g, x = got[keep].cpu().numpy(), want[keep]
    if g.dtype == np.float64:
        g, x = _bits(g), _bits(x)
    _same(g, x, f"only output {keep}, K={K}")


@pytest.mark.parametrize("N,K", [(2, 0), (2, 4097), (0, 4), (2, -1)])
def test_argument_errors_write_nothing(handle, N, K):
    _, capi = _mods()
    dev = handle.device
    c4 = torch.zeros(2 * 4097, 4, dtype=torch.float64, device=dev)
    dn = torch.ones(2 * 4097, dtype=torch.uint8, device=dev)
    outs = [torch.full((2 * 4097,), SENT_F, dtype=torch.float64, device=dev), torch.full((2,), SENT_I, dtype=torch.int32, device=dev),
            torch.full((2,), SENT_F, dtype=torch.float64, device=dev), torch.full((2 * 4097,), SENT_B, dtype=torch.uint8, device=dev)]
    import ctypes as C
    w = (C.c_double * 3)(0.4, 0.4, 0.2)
    rc = handle.L.mtfjsp_group_reduce(handle.h, N, K, c4.data_ptr(), dn.data_ptr(), w, *[o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    assert rc == capi.ERR_ARG and b"mtfjsp_group_reduce" in handle.L.mtfjsp_last_error(handle.h)
    assert (outs[0] == SENT_F).all().item() and (outs[1] == SENT_I).all().item() and (outs[2] == SENT_F).all().item() and (outs[3] == SENT_B).all().item()
    assert handle.L.mtfjsp_group_reduce(handle.h, 2, 4, None, dn.data_ptr(), w, *[o.data_ptr() for o in outs]) == capi.ERR_ARG


# ---------------------------------------------------------------- mtfjsp_final_costs
@pytest.mark.parametrize("J,M,E,B", [(3, 4, 2, 7), (6, 6, 2, 5), (9, 8, 2, 2)], ids=["J3M4", "J6M6", "J9M8"])
def test_final_costs_equal_the_host_formula(J, M, E, B):
    """an episode of random actions in which the last instance is given task -1 throughout (every step rejected: it keeps the costs of its reset) and
    instance 0 from half way on (it stays unfinished with costs): cost4 is Final_4cost of evaluate.validate_cost_batched, done marks
    exactly the finished instances"""
    batch_env, capi = _mods()
    T = J * M
    env = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype="f32")
    env.generate_instances(seed=31)
    with pytest.raises(capi.MtfjspError) as e:
        env.final_costs()
    assert e.value.code == capi.ERR_STATE
    env.scaler_init()
    env.reset(env.draw_reward_weights(5, 0))
    a = torch.zeros(B, dtype=torch.int32, device=env.device); m = torch.zeros_like(a); j = torch.zeros_like(a)
    out = torch.full((B, 4), SENT_F, dtype=torch.float64, device=env.device)
    done = torch.full((B,), SENT_B, dtype=torch.uint8, device=env.device)
    for s in range(T):
        env.random_actions(11, s, a, m, j)
        a[B - 1] = -1
        if s >= T // 2:
            a[0] = -1
        env.step(a, m)
    got, got_done = env.final_costs(out, done)
    torch.cuda.synchronize()
    assert got is out and got_done is done
    prev = env.read_state(capi.STATE_PREV_COSTS)
    finished = env.info.cpu().numpy()[:, 1] == 1.0
    want, _ = ref.final_costs(prev, np.zeros(B), T)
    _same(_bits(out.cpu().numpy()), _bits(want), "cost4 (bits)")
    _same(done.cpu().numpy(), finished.astype(np.uint8), "done")
    assert finished.tolist() == [False] + [True] * (B - 2) + [False]
    assert prev[0, 0] > 0 and (want[:, 1] != prev[:, 1]).all(), "the division must show in every row"
    # cost4 alone: done may be NULL
    out2 = torch.full((B, 4), SENT_F, dtype=torch.float64, device=env.device)
    capi.check(env.L.mtfjsp_final_costs(env.h, out2.data_ptr(), None), env.h)
    torch.cuda.synchronize()
    _same(_bits(out2.cpu().numpy()), _bits(want), "cost4 without done (bits)")
    env.close()
