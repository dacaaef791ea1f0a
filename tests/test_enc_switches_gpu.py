"""GPU: a handle keeps the switches it read when it was created (csrc/mtfjsp_enc_switches.h: the create-time class).  One process, two tiny handles
on J10M7 x 5 (T = 70: the streaming launches with the pooling epilogue, a case of tests/test_gin_select_gpu.py): handle A is created under
MTFJSP_FUSE_POOL=0 and the variable deleted before its forward; handle B is created without it and the variable set again before its forward.  Each
handle's plan is what the handle-free entry gives under the environment of ITS creation — a reader shared by all handles that turned the values into
process-wide state would show here — and the two pooling forms agree within the tolerance tests/test_encoder_sizes_gpu.py holds them to."""
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("MTFJSP_FUSE_PAIR", "MTFJSP_FUSE_GIN0", "MTFJSP_FUSE_POOL", "MTFJSP_NO_STREAM_ORDER", "MTFJSP_STREAM_NT", "MTFJSP_POOL_S",
            "MTFJSP_NO_RESIDENT_GIN", "MTFJSP_GIN_RES_GENERIC")


def test_a_handle_keeps_the_switches_of_its_creation(monkeypatch):
    import torch
    import mtfjsp_amd  # noqa: F401
    capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
    enc_mod = import_module("e2e-mappo-for-mt-fjsp_amd.encoder")
    rollout = import_module("e2e-mappo-for-mt-fjsp_amd.rollout")
    J, M, B = 10, 7, 5
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    ja, ma = enc_mod.random_init_weights(seed=J * 100 + M)
    ro = rollout.Rollout(J, M, 1, B, policy="actor", obs_dtype="f32", weights=(ja, ma), collect=False)
    for _ in range(3):
        ro.step()
    env = ro.env
    hm = ro.actor.enc.h_pooled_m.clone()
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count

    def rule():
        return capi.gin_launches_for(B, J, M, num_cu=num_cu, single_ok=False)

    monkeypatch.setenv("MTFJSP_FUSE_POOL", "0")
    a = enc_mod.Encoder(J, M, B, obs_dtype="f32")
    rule_a = rule()
    monkeypatch.delenv("MTFJSP_FUSE_POOL")
    b = enc_mod.Encoder(J, M, B, obs_dtype="f32")
    rule_b = rule()
    monkeypatch.setenv("MTFJSP_FUSE_POOL", "0")
    outs, plans = [], []
    for e in (a, b):
        e.load_weights(ja, ma)
        prob, _, job_v = e.job_actor_forward(env.tasks_fea, env.ell_col, env.ell_val, env.candidate, env.job_mask, hm)
        torch.cuda.synchronize()
        outs.append((prob.cpu().numpy().copy(), job_v.cpu().numpy().copy()))
        plans.append(e.gin_launches())
        e.close()
    print("A:", plans[0], "\nB:", plans[1])
    print("max |prob A - B|", np.abs(outs[0][0] - outs[1][0]).max(), " max |job_v A - B|", np.abs(outs[0][1] - outs[1][1]).max())
    assert plans[0]["pool"] == "pool_gather" and plans[1]["pool"] == "epilogue"
    assert plans[0] == rule_a and plans[1] == rule_b
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=2e-5)            # (test_pooling_epilogue_serves_any_candidate's bounds)
    np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-4)
