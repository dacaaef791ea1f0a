"""GPU: a live handle names the step kernel the handle-free form names at the device's own LDS capacity, mtfjsp_step_params follows
the same plan, and the launch the plan describes runs.  Tiny handles, one step each."""
from collections import namedtuple
from importlib import import_module

import numpy as np
import pytest
import torch

from env_parity import _SELECTION_VARS

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "J M E B force kernel fused")
CASES = [
    Case(6, 6, 2, 19, None, "k_env_grp16", True),
    Case(10, 10, 2, 19, None, "k_env_grp16x2", False),
    Case(5, 12, 2, 11, None, "k_env_step_grp", False),     # T = 60 but M * M = 144: no register kernel takes it
    Case(6, 6, 2, 3, "lds1", "k_env_step", False),
    Case(6, 6, 2, 19, "reg1", "k_env_reg", False),
]


@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
@pytest.mark.parametrize("c", CASES, ids=lambda c: f"J{c.J}M{c.M}B{c.B}-{c.force or 'default'}")
def test_handle_names_the_planned_kernel_and_steps(monkeypatch, c, obs_dtype):
    import mtfjsp_amd  # noqa: F401
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
    for k in _SELECTION_VARS:
        monkeypatch.delenv(k, raising=False)
    if c.force:
        monkeypatch.setenv("MTFJSP_ENV_KERNEL", c.force)
    lds_max = torch.cuda.get_device_properties(0).shared_memory_per_block
    name, G, nbytes, overridden = batch_env.step_kernel_for(c.J, c.M, c.B, obs_dtype == "f32", lds_max)
    assert name == c.kernel and overridden == bool(c.force), (name, G, nbytes, overridden, lds_max)
    env = batch_env.DeviceBatchEnv(c.J, c.M, c.E, c.B, obs_dtype=obs_dtype)
    try:
        assert env.step_kernel_name() == name
        env.generate_instances(seed=3)
        env.scaler_init()
        env.reset_episode(5, 0)
        a = torch.zeros(c.B, dtype=torch.int32, device=env.device); m = torch.zeros_like(a)
        env.random_actions(7, 0, a, m, None)
        assert (env.step_params(a, m) is not None) == c.fused == (name == "k_env_grp16" and not overridden)
        env.step(a, m)
        env.synchronize()
        status = env.status.cpu()
        assert not (status & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any(), status
        mach = env.read_state(capi.STATE_MACHINE)    # the step ran: every instance has its one operation on the chosen machine
        assert ((mach >= 0).sum(1) == 1).all() and (mach[np.arange(c.B), a.cpu().numpy()] == m.cpu().numpy()).all(), mach
    finally:
        env.close()
