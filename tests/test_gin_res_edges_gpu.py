"""`k_gin_res`, the run-time instantiation of the single-launch GIN encoder, at the edges of the shapes it is eligible for
(tests/gin_res_edges.py: T = 16 .. 65, 1 .. 36 instances per workgroup, ragged last workgroups, f64 observations, node output on and
off, the global critic's forward) against the fp32 oracle restatement on the WHOLE batch and a binary64 evaluation of the same
network, on the environment's adjacency after a short rollout and on one whose edges span the instance.

Every test asserts that it ran the kernel it is about (the library's plan for the shape, check(), no range fall-back, no statistics
time-out) and repeats the comparison on the streaming launches — the path these shapes fall back to, and the second opinion that
tells a fault of the kernel from one of the inputs or the oracle.  No tolerance is new: the hard caps and recorded figures of
tests/error_budget.py under the blanket tolerances of tests/test_full_size_gpu.py::test_encoder_headline_partition_vs_oracle, and
that test's yardstick (no further from binary64 than twice the f32 oracle is).  tests/test_gin_res_edges_cpu.py shows that these
bounds catch a ring one tile short, a pool one row late and statistics that miss an instance by more than 10x."""
from importlib import import_module

import numpy as np
import pytest
import torch

import gin_res_edges as ge
from error_budget import HARD_CAP, bound, check as budget

pytestmark = pytest.mark.gpu

IDS = [ge.case_id(c) for c in ge.CASES]


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.rollout"), import_module("e2e-mappo-for-mt-fjsp_amd.encoder"),
            import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi"))


def _rollout(case, candidates, with_critic=False):
    """-> (rollout after T // 2 policy steps on instances drawn on the device, its weight dicts); asserts the preconditions"""
    rollout, enc_mod, batch_env, capi = _mods()
    (J, M, E, B, obs), (T, ipc, grid, last) = case
    assert torch.cuda.get_device_properties(0).multi_processor_count == ge.CUS
    for nodes in (False, True):
        assert capi.gin_res_kernel_for(B, J, M, ge.CUS, candidates=candidates, node_output=nodes) == (ge.GENERIC, ipc, grid)
    ws = enc_mod.random_init_weights(seed=J * 100 + M, with_critic=with_critic)
    ge.perturb(ws, 3)
    gen = batch_env.DeviceBatchEnv(J, M, ge.shops(M, E), B, obs_dtype="f32")
    gen.generate_instances(seed=9)
    ins = gen.read_instances()
    gen.close()
    ro = rollout.Rollout(J, M, ge.shops(M, E), B, policy="actor", obs_dtype=obs, weights=ws, collect=False, instances=ins)
    try:
        assert ro.actor.enc.check()
        for _ in range(T // 2):
            ro.step()
        torch.cuda.synchronize()
        assert ro.actor.enc.check() and ro.n_resident_failures == 0
    except BaseException:
        _free(ro)
        raise
    return ro, ws


def _free(ro):
    ro.actor.enc.close()
    ro.env.close()


def _adjacency(ro, case, adj):
    """-> host (col [B,T,2], val [B,T,2]) and the device tensors the forwards read"""
    (J, M, E, B, obs), (T, ipc, grid, last) = case
    env = ro.env
    col = env.ell_col.cpu().numpy().reshape(B, T, 2)
    val = env.ell_val.cpu().numpy().reshape(B, T, 2)
    if adj == "env":
        return col, val, env.ell_col, env.ell_val
    col, val = ge.far_adjacency(B, T, seed=T, weights=ge.edge_weights(col, val))
    assert ge.tile_distance(col, T, ipc).max() == {16: 0, 32: 0, 64: 1}.get(T, 2 if T >= 63 else 1)
    return col, val, torch.as_tensor(col.reshape(B * T, 2)).cuda(), torch.as_tensor(val.reshape(B * T, 2)).cuda()


def _ran_the_single_launch(e):
    assert e.check(), "the handle left the single-launch kernel"
    assert e.gin_res_kernel_name() == ge.GENERIC
    assert e.range_fallbacks()[0] == 0 and e.resident_failures() == 0


def _compare(name, ipc, o, o64, got, scale):
    """one forward's outputs (h_nodes may be None) against the oracle's under the ledger's bounds; the pooled embedding instance by
    instance, so that a slip at an instance boundary names where it sits"""
    h_nodes, h_o, prob, job_v = got
    per_inst = np.abs(h_o.astype(np.float64) - o["h_pooled"]).max(1) / scale
    b = int(per_inst.argmax())
    over = np.flatnonzero(per_inst > bound(name, "h_pooled_o", 1e-4))
    assert over.size == 0, (f"{name} / h_pooled_o: {over.size} of {per_inst.size} instances beyond {bound(name, 'h_pooled_o', 1e-4):.3e}; worst {per_inst[b]:.3e} at "
                            f"instance {b} = number {b % ipc} of {ipc} in workgroup {b // ipc}; positions in their workgroups: {sorted(set((over % ipc).tolist()))}")
    budget(name, "h_pooled_o", h_o, o["h_pooled"], 1e-4, scale)
    budget(name, "job_prob", prob, o["prob"], 1e-4)
    budget(name, "job_v", job_v, o["job_v"], 1e-3, relative=True)
    if h_nodes is None:
        return
    budget(name, "h_nodes", h_nodes, o["h_nodes"], 1e-4, scale)
    err_hip = budget(name, "h_nodes_vs_binary64", h_nodes, o64["h_nodes"], 1e-4, scale) * scale
    err_f32 = float(np.abs(o["h_nodes"] - o64["h_nodes"]).max())
    print(f"{name}: h_nodes vs binary64: HIP {err_hip:.3g}, f32 oracle {err_f32:.3g}, scale {scale:.3g}; h_pooled_o worst instance {b} ({b % ipc} of {ipc}) {per_inst[b]:.3g}")
    assert err_hip <= max(2 * err_f32, 1e-4 * scale)


@pytest.mark.parametrize("adj", ge.ADJACENCIES)
@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_job_actor_forward_vs_oracle(case, adj):
    from oracle import encoder_oracle as eo
    (J, M, E, B, obs), (T, ipc, grid, last) = case
    ro, (ja, ma) = _rollout(case, candidates=J)
    env, e = ro.env, ro.actor.enc
    try:
        hm = e.h_pooled_m.clone()
        col, val, col_t, val_t = _adjacency(ro, case, adj)
        n = lambda x: x.cpu().numpy().copy()

        gathered = []                                           # the candidates' rows as each single-launch forward left them

        def forward(nodes, resident=True):
            h_nodes = torch.zeros(B * T, 128, dtype=torch.float32, device="cuda") if nodes else None
            prob, h_o, job_v = e.job_actor_forward(env.tasks_fea, col_t, val_t, env.candidate, env.job_mask, hm, h_nodes=h_nodes)
            torch.cuda.synchronize()
            if resident:
                gathered.append(e.peek_gin_res()[0].reshape(B, J, 128))
            return (n(h_nodes) if nodes else None), n(h_o), n(prob), n(job_v)

        with_nodes, without, again = forward(True), forward(False), forward(False)
        _ran_the_single_launch(e)
        # the statistics words carry exact integer sums: the same forward twice gives the same bits
        for a, b, what in zip(without[1:], again[1:], ("h_pooled_o", "job_prob", "job_v")):
            assert np.array_equal(a, b), what
        tf = n(env.tasks_fea)
        cand, mask = n(env.candidate), n(env.job_mask)
        o = eo.job_actor_forward(ja, tf, col, val, cand, mask, n(hm), B, T)
        o64 = eo.job_actor_forward(ja, tf, col, val, cand, mask, n(hm), B, T, dtype=torch.float64)
        scale = max(1.0, float(np.abs(o["h_nodes"]).max()))
        name = ge.case_name(case[0], adj)
        _compare(name, ipc, o, o64, with_nodes, scale)
        _compare(name, ipc, o, o64, without, scale)
        # the candidate table [ipc][J] by itself: the scorer saturates on these weights (job_prob agrees to the last bit whatever
        # it is fed), so the rows the kernel gathered are compared directly — with the node rows the same forward wrote, bit for
        # bit (both are stored from the same registers), and with the oracle's as node embeddings
        assert cand.min() >= 0 and cand.max() < T and all(len(set(r)) == J for r in cand.tolist())
        bi = np.arange(B)[:, None]
        assert np.array_equal(gathered[0], with_nodes[0].reshape(B, T, 128)[bi, cand]), "candidate rows != the node rows of the same forward"
        for g in gathered:
            budget(name, "h_nodes", g, o["h_nodes"].reshape(B, T, 128)[bi, cand], 1e-4, scale)
        e.set_product_mode(16)                                  # the same inputs through the streaming launches
        try:
            assert not e.check()
            streaming = forward(True, resident=False)
            assert not e.check()
        finally:
            e.set_product_mode(0)
        _compare(ge.case_name(case[0], adj, streaming=True), ipc, o, o64, streaming, scale)
        assert e.check()
    finally:
        _free(ro)


@pytest.mark.parametrize("case", ge.CRITIC_CASES, ids=[ge.case_id(c) for c in ge.CRITIC_CASES])
def test_global_critic_forward_vs_oracle(case):
    """no candidates: `A.candidate == nullptr` in k_gin_res; T = 16 and T = 65, full and ragged, `far` adjacency"""
    from oracle import encoder_oracle as eo
    from test_handoff_rollout_gpu import _global_critic64
    (J, M, E, B, obs), (T, ipc, grid, last) = case
    ro, (ja, ma, gc) = _rollout(case, candidates=0, with_critic=True)
    env, e = ro.env, ro.actor.enc
    try:
        col, val, col_t, val_t = _adjacency(ro, case, "far")
        got = e.global_critic_forward(env.tasks_fea, col_t, val_t, env.m_fea1, env.m_fea2).cpu().numpy()
        again = e.global_critic_forward(env.tasks_fea, col_t, val_t, env.m_fea1, env.m_fea2).cpu().numpy()
        _ran_the_single_launch(e)
        assert np.array_equal(got, again)
        n = lambda x: x.cpu().numpy()
        assert float(env.m_fea1.abs().max()) > 0 and float(env.m_fea2.abs().max()) > 0
        args = (n(env.tasks_fea), col, val, n(env.m_fea1), n(env.m_fea2), B, T, M)
        want = eo.global_critic_forward(gc, *args)
        want64 = _global_critic64(gc, *args)
        rel = lambda a, b: float((np.abs(a - b) / (1.0 + np.abs(b))).max())
        name = ge.case_name(case[0], "far")
        print(f"{name}: global_v HIP vs f32 oracle {rel(got, want):.3g}, HIP vs binary64 {rel(got, want64):.3g}, "
              f"f32 oracle vs binary64 {rel(want, want64):.3g} (cap {HARD_CAP['global_v']:.1g})")
        budget(name, "global_v", got, want, 1e-3, relative=True)
    finally:
        _free(ro)
