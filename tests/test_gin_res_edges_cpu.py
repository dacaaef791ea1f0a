"""CPU: the shapes of tests/gin_res_edges.py are what they claim — which kernel and partition the library's rule gives them, how far
apart the `far` adjacency's edges lie — and the bounds that tests/test_gin_res_edges_gpu.py holds `k_gin_res` to tell a right kernel
from three wrong ones: the oracle's GIN encoder with a slip of the kind each structure of the kernel could make (an aggregation ring
one tile too short, a pool that starts one row late, statistics that miss an instance) lands more than 10x outside them.
No handle, no device."""
from importlib import import_module

import numpy as np
import pytest
import torch

import mtfjsp_amd  # noqa: F401
import gin_res_edges as ge
from env_parity import random_valid
from error_budget import bound
from oracle import encoder_oracle as eo

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
enc_mod = import_module("e2e-mappo-for-mt-fjsp_amd.encoder")
inst_mod = import_module("e2e-mappo-for-mt-fjsp_amd.instances")

IDS = [ge.case_id(c) for c in ge.CASES]


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    monkeypatch.delenv("MTFJSP_GIN_RES_GENERIC", raising=False)


# ---------------------------------------------------------------- a. the rule
@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_every_case_runs_the_run_time_kernel_with_the_listed_partition(case):
    (J, M, E, B, obs), (T, ipc, grid, last) = case
    assert T == J * M and B - (grid - 1) * ipc == last and 1 <= last <= ipc
    assert ipc * T <= 576 and ipc * J <= 384
    want = (ge.GENERIC, ipc, grid)
    assert capi.gin_res_kernel_for(B, J, M, ge.CUS) == want
    assert capi.gin_res_kernel_for(B, J, M, ge.CUS, candidates=0) == want               # the global critic's forward
    assert capi.gin_res_kernel_for(B, J, M, ge.CUS, node_output=True) == want


def test_shapes_just_outside_have_no_kernel():
    assert capi.gin_res_kernel_for(4096, 3, 5, ge.CUS)[0] is None                       # T = 15
    assert capi.gin_res_kernel_for(2048, 6, 11, ge.CUS)[0] is None                      # T = 66
    assert capi.gin_res_kernel_for(9217, 4, 4, ge.CUS)[0] is None                       # 37 instances x 16 rows > 576
    assert capi.gin_res_kernel_for(9216, 16, 1, ge.CUS)[0] is None                      # 36 x 16 candidates > 384 table slots
    assert capi.gin_res_kernel_for(6144, 16, 1, ge.CUS) == (ge.GENERIC, 24, 256)        # ... 24 x 16 = 384 fit


# ---------------------------------------------------------------- b. the far adjacency
@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_far_adjacency_is_what_it_claims(case):
    (J, M, E, B, obs), (T, ipc, grid, last) = case
    n = min(B, 2 * ipc + 1)                                   # two workgroups and an instance: both parities at every position
    col, val = ge.far_adjacency(n, T, seed=T, weights=(0.25, 1.0, 3.0))
    assert col.shape == val.shape == (n, T, 2) and col.dtype == np.int32 and val.dtype == np.float32
    assert col.min() == -1 and col.max() == T - 1
    assert (col != np.arange(T)[None, :, None]).all(), "no self loops (the aggregation adds its own)"
    assert ((val != 0) == (col >= 0)).all() and set(np.unique(val[col >= 0])) == {0.25, 1.0, 3.0}
    d = np.where(col >= 0, col - np.arange(T)[None, :, None], 0)
    assert d.max() == T - 1 and d.min() == -(T - 1)
    deg = 1 + (col >= 0).sum(2)
    assert set(np.unique(deg)) == {1, 2, 3}
    assert (col[0, :, 0] >= 0).sum() > (col[0, :, 1] >= 0).sum() and np.array_equal(col[1], col[0][:, ::-1])    # odd instances: the other order
    td = ge.tile_distance(col, T, ipc)
    assert td.max() <= 2, "the aggregation ring holds tiles rt-2 .. rt+2"
    # instances start at multiples of T rows: at T = 16 and 32 an instance lies inside one tile and at T = 64 inside a pair of
    # tiles, whatever the adjacency; everywhere else instances straddle, and from 33 rows on an edge can span two tiles
    assert td.max() == {16: 0, 32: 0, 64: 1}.get(T, 2 if T >= 63 else 1)
    assert T in (16, 32) or (td == 1).any()


# ---------------------------------------------------------------- c. the bounds separate right from wrong
def _bn(x, gamma, beta, rows):
    """training-mode BatchNorm of all rows with the statistics of the first `rows`"""
    mean = x[:rows].mean(0)
    var = x[:rows].var(0, unbiased=False)
    return (x - mean) / torch.sqrt(var + eo.H_EPS) * gamma + beta


def _gin(w, tfea, col, val, B, T, slip=None):
    """oracle/encoder_oracle.gin_encoder in f32 (slip=None: the same operations in the same order, asserted below) with one slip:
    "ring": sources two row tiles from their row contribute nothing, though nnz counts them;
    "pool": the graph pool of instance b averages rows b*T+1 .. (b+1)*T — the first row of the next instance (of nothing, after
            the last) instead of its own first;
    "stats": every BatchNorm's statistics omit the last instance."""
    pre = "encoder.feature_extract."
    w = {k: torch.as_tensor(v) for k, v in w.items()}
    h = torch.as_tensor(np.asarray(tfea), dtype=torch.float64).float()
    col = torch.as_tensor(np.asarray(col).reshape(B * T, 2), dtype=torch.long)
    val = torch.as_tensor(np.asarray(val).reshape(B * T, 2), dtype=torch.float64).float().double()
    row = torch.arange(B * T).unsqueeze(1)
    base = row // T * T
    has = col >= 0
    gidx = torch.where(has, col + base, torch.zeros_like(col))
    deg = 1.0 + has.sum(1).double()
    adds = has & (((gidx >> 5) - (row >> 5)).abs() < 2) if slip == "ring" else has
    rows = (B - 1) * T if slip == "stats" else B * T
    for layer in range(2):
        hd = h.double()
        pooled = hd.clone()
        for s in range(2):
            pooled = pooled + torch.where(adds[:, s:s + 1], val[:, s:s + 1] * hd[gidx[:, s]], torch.zeros_like(hd))
        pooled = (pooled / deg.unsqueeze(1)).float()
        m = pre + f"mlps.{layer}."
        z = torch.relu(_bn(eo._lin(pooled, w, m + "linears.0"), w[m + "batch_norms.0.weight"], w[m + "batch_norms.0.bias"], rows))
        z = torch.relu(_bn(eo._lin(z, w, m + "linears.1"), w[m + "batch_norms.1.weight"], w[m + "batch_norms.1.bias"], rows))
        z = eo._lin(z, w, m + "linears.2")
        h = torch.relu(_bn(z, w[pre + f"batch_norms.{layer}.weight"], w[pre + f"batch_norms.{layer}.bias"], rows))
    if slip == "pool":
        late = torch.cat([h[1:], torch.zeros_like(h[:1])])
        return h.numpy(), late.reshape(B, T, -1).mean(1).numpy()
    return h.numpy(), h.reshape(B, T, -1).mean(1).numpy()


_inputs = {}


def _one_workgroup(case):
    """one workgroup's worth of instances of a case (B = ipc) after T // 2 random valid steps of the C oracle, with the `far`
    adjacency at the environment's own edge weights, and the f32 oracle's embeddings: computed once per case, shared, never changed"""
    key = ge.case_id(case)
    if key not in _inputs:
        from oracle.env_oracle import OracleBatch
        (J, M, E, _, obs), (T, ipc, _, _) = case
        B = ipc
        t, p, tt, edge = inst_mod.generate_instances(B, J, M, ge.shops(M, E), seed=100 * J + M)
        rs = np.random.RandomState(T)
        orc = OracleBatch(t, p, tt, edge)
        orc.scaler_init()
        orc.reset(rs.dirichlet([1, 1, 1], B))
        cand, mask = orc.job_mask_state()
        for _ in range(T // 2):
            job, task, mach = random_valid(rs, cand, mask, t >= 0)
            orc.step(task, mach)
            cand, mask = orc.job_mask_update(job)
        o = orc.observe(dense=False)
        col, val = ge.far_adjacency(B, T, seed=T, weights=ge.edge_weights(o["ell_col"], o["ell_val"]))
        ja, _ = enc_mod.random_init_weights(seed=J * 100 + M)
        ge.perturb((ja,), 3)
        h, hp = eo.gin_encoder({k: torch.as_tensor(v) for k, v in ja.items()}, o["tfea"], col, val, B, T)
        _inputs[key] = dict(w=ja, tfea=o["tfea"], col=col, val=val, B=B, T=T, h=h.numpy(), hp=hp.numpy())
    return _inputs[key]


def _excess(case, tensor, got, want, scale):
    """normalised distance of a slipped tensor from the right one, in units of the bound the GPU test puts on it"""
    return float(np.abs(got - want).max()) / scale / bound(ge.case_name(case[0], "far"), tensor, 1e-4)


@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_the_restated_encoder_is_the_oracles(case):
    x = _one_workgroup(case)
    h, hp = _gin(x["w"], x["tfea"], x["col"], x["val"], x["B"], x["T"])
    assert np.array_equal(h, x["h"]) and np.array_equal(hp, x["hp"])


@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_far_inputs_stay_inside_the_range_of_the_fixed_point_statistics(case):
    """A workgroup's sum of squares of the first Linear's outputs must stay below 2^39 (csrc/mtfjsp_gin_resident.h, gr_fix_encode: beyond
    it the forward repeats on the f32-instruction kernels, and the GPU test would not have run the kernel it is about).  The aggregated
    raw features are the largest numbers of a forward: times in the thousands times edge weights.  A sixteenth of the range here."""
    x = _one_workgroup(case)
    B, T = x["B"], x["T"]
    col = torch.as_tensor(x["col"].reshape(B * T, 2), dtype=torch.long)
    val = torch.as_tensor(x["val"].reshape(B * T, 2), dtype=torch.float64)
    f = torch.as_tensor(x["tfea"], dtype=torch.float64)
    src = torch.where(col >= 0, col + (torch.arange(B * T) // T * T).unsqueeze(1), torch.zeros_like(col))
    agg = (f + val[:, :1] * f[src[:, 0]] + val[:, 1:] * f[src[:, 1]]) / (1.0 + (col >= 0).sum(1, keepdim=True))
    z = agg @ torch.as_tensor(x["w"]["encoder.feature_extract.mlps.0.linears.0.weight"]).double().t()
    used = float((z * z).sum(0).max()) / 2.0 ** 39
    print(f"{ge.case_id(case)}: first Linear, sum of squares of one workgroup = {used:.3g} of the range")
    assert used < 1 / 16


@pytest.mark.parametrize("case", [c for c in ge.CASES if c[1][0] >= 63], ids=[ge.case_id(c) for c in ge.CASES if c[1][0] >= 63])
def test_a_ring_one_tile_too_short_is_far_outside_the_bound(case):
    x = _one_workgroup(case)
    T = x["T"]
    h, hp = _gin(x["w"], x["tfea"], x["col"], x["val"], x["B"], T, slip="ring")
    if T == 64:                                               # no edge spans two tiles at T = 64 (see the adjacency's test): nothing to drop
        assert np.array_equal(h, x["h"]) and np.array_equal(hp, x["hp"])
        return
    scale = max(1.0, float(np.abs(x["h"]).max()))
    q = _excess(case, "h_nodes", h, x["h"], scale), _excess(case, "h_pooled_o", hp, x["hp"], scale)
    print(f"{ge.case_id(case)} ring slip: h_nodes {q[0]:.3g} x bound, h_pooled_o {q[1]:.3g} x bound")
    assert min(q) > 10


@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_a_pool_that_starts_one_row_late_is_far_outside_the_bound(case):
    x = _one_workgroup(case)
    h, hp = _gin(x["w"], x["tfea"], x["col"], x["val"], x["B"], x["T"], slip="pool")
    assert np.array_equal(h, x["h"])
    scale = max(1.0, float(np.abs(x["h"]).max()))
    per_instance = np.abs(hp - x["hp"]).max(1) / scale / bound(ge.case_name(case[0], "far"), "h_pooled_o", 1e-4)
    print(f"{ge.case_id(case)} pool slip: h_pooled_o {per_instance.min():.3g} .. {per_instance.max():.3g} x bound over the instances")
    assert per_instance.max() > 10


@pytest.mark.parametrize("case", ge.CASES, ids=IDS)
def test_statistics_that_miss_an_instance_are_far_outside_the_bound(case):
    x = _one_workgroup(case)
    h, hp = _gin(x["w"], x["tfea"], x["col"], x["val"], x["B"], x["T"], slip="stats")
    scale = max(1.0, float(np.abs(x["h"]).max()))
    q = _excess(case, "h_nodes", h, x["h"], scale), _excess(case, "h_pooled_o", hp, x["hp"], scale)
    print(f"{ge.case_id(case)} statistics slip: h_nodes {q[0]:.3g} x bound, h_pooled_o {q[1]:.3g} x bound")
    assert min(q) > 10
