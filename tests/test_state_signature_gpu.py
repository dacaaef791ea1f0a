"""GPU: mtfjsp_state_signature EQUALS the host model's signature (tests/beam_ref.py) formed from the state the handle reads back
(machine, start time, routes): 0 after reset, then after 1, T/2 and T random valid steps; both observation dtypes, left shift on and
off.  J9M8 has T = 72 (lanes stride over the tasks), J13M10 T = 130.  With left shift off, two decisions on different machines
commute — one signature for both orders — and two decisions on one machine do not."""
from importlib import import_module

import numpy as np
import pytest
import torch

import beam_ref as ref
from env_parity import _same

pytestmark = pytest.mark.gpu

SHAPES = {"J3M3": (3, 3, 3, 5), "J6M6": (6, 6, 2, 7), "J9M8": (9, 8, 2, 3), "J13M10": (13, 10, 2, 2)}


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


def _model(env, capi):
    mach = env.read_state(capi.STATE_MACHINE)
    return ref.signature(mach, mach >= 0, env.read_state(capi.STATE_START), env.read_state(capi.STATE_ROUTES))


@pytest.mark.parametrize("left_shift", [True, False], ids=["left_shift", "no_left_shift"])
@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_signature_equals_the_model_along_a_random_episode(shape, obs_dtype, left_shift):
    batch_env, capi = _mods()
    J, M, E, B = SHAPES[shape]
    T = J * M
    t, p, tt, edge, w3 = ref.cached_data(J, M, E, B)
    env = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=left_shift, obs_dtype=obs_dtype, w_cfg=ref.CONFIG_W)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(w3)
    sig = env.state_signature().cpu().numpy().view(np.uint64)
    _same(sig, np.zeros(B, np.uint64), f"{shape} after reset")
    a = torch.zeros(B, dtype=torch.int32, device=env.device); m = torch.zeros_like(a); j = torch.zeros_like(a)
    seen = []
    for s in range(T):
        env.random_actions(11, s, a, m, j)
        env.step(a, m)
        if s + 1 in (1, T // 2, T):
            sig = env.state_signature().cpu().numpy().view(np.uint64)
            _same(sig, _model(env, capi), f"{shape} after {s + 1} steps")
            assert sig.all()
            seen.append(sig)
    assert len(seen) == 3 and not (seen[0] == seen[1]).any() and not (seen[1] == seen[2]).any()
    assert bool(env.info[:, 1].all().item())
    env.close()


def test_an_unreset_handle_is_a_state_error():
    batch_env, capi = _mods()
    J, M, E, B = SHAPES["J3M3"]
    t, p, tt, edge, w3 = ref.cached_data(J, M, E, B)
    env = batch_env.DeviceBatchEnv(J, M, E, B, w_cfg=ref.CONFIG_W)
    env.load_instances(t, p, tt, edge=edge)
    out = torch.full((B,), 77, dtype=torch.int64, device=env.device)
    assert env.L.mtfjsp_state_signature(env.h, out.data_ptr()) == capi.ERR_STATE
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all()
    env.close()


def test_decisions_on_different_machines_commute_and_on_one_machine_do_not():
    batch_env, capi = _mods()
    J, M, E, B = SHAPES["J3M3"]
    t, p, tt, edge, w3 = ref.cached_data(J, M, E, B)
    found = None
    for b in range(B):                                                  # first operations of jobs 0 and 1: two machines apart, one shared
        ta, tb = 0, M
        for ms in range(M):
            for ma in range(M):
                for mb in range(M):
                    if found is None and ma != mb and min(t[b, ta, ma], t[b, tb, mb], t[b, ta, ms], t[b, tb, ms]) >= 0:
                        found = (b, ta, tb, ma, mb, ms)
    assert found is not None, "the test data have an instance with the machines this case needs"
    b, ta, tb, ma, mb, ms = found
    rep = lambda x: np.ascontiguousarray(np.repeat(np.asarray(x)[b:b + 1], 4, axis=0))      # noqa: E731
    env = batch_env.DeviceBatchEnv(J, M, E, 4, left_shift=False, obs_dtype="f64", w_cfg=ref.CONFIG_W)
    env.load_instances(rep(t), rep(p), rep(tt), edge=rep(edge)); env.scaler_init(); env.reset(rep(w3))
    # instance 0: a then b, 1: b then a (different machines) | 2: a then b, 3: b then a (one machine)
    steps = [([ta, tb, ta, tb], [ma, mb, ms, ms]), ([tb, ta, tb, ta], [mb, ma, ms, ms])]
    for task, mach in steps:
        env.step(torch.as_tensor(np.array(task, np.int32), device=env.device), torch.as_tensor(np.array(mach, np.int32), device=env.device))
        assert not (env.status.cpu().numpy() & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any()
    sig = env.state_signature().cpu().numpy().view(np.uint64)
    _same(sig, _model(env, capi), "the four orders")
    assert sig[0] == sig[1], "different machines, left shift off: one schedule, one signature"
    assert sig[2] != sig[3], "one machine: the order is part of the schedule"
    assert len({int(x) for x in sig}) == 3
    env.close()
