"""GPU: mtfjsp_front_rank and mtfjsp_plan_survivors (csrc/mtfjsp_nsga.hip) EQUAL their host model (tests/nsga_ref.py, pinned by
tests/test_front_rank_cpu.py): ranks, selection order and front sizes element for element, crowding distances and the best objective by
value with NaN equal to NaN (the data holds no negative zero), rank 0 against the device's own mtfjsp_group_reduce front.
k_front_rank is one wave with one candidate per thread up to K = 64, then four waves with 1, 4 or 8 candidates per thread: K sits on
both sides of every boundary (64 | 65, 256 | 257, 1024 | 1025), below a wavefront (1, 2, 7) and at the limit (2048: 88 KB of LDS)."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import group_reduce_ref as gref
import nsga_ref as ref
from env_parity import _same

pytestmark = pytest.mark.gpu

KS = [1, 2, 7, 64, 65, 256, 257, 1024, 1025, 2048]
N = 3
WEIGHTS = {"integer": (0.4, 0.4, 0.2), "scattered": (0.4, 0.4, 0.2), "none": (0.4, 0.4, 0.2), "random": (0.37, 0.0625, 0.5675),
           "chain": (0.4, 0.4, 0.2), "antichain": (0.4, 0.4, 0.2), "flat": (0.4, 0.4, 0.2), "infinite": (0.0, 0.5, 0.5)}
SENT_F, SENT_I = 123.5, -77


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


@pytest.fixture(scope="module")
def handle():
    batch_env, _ = _mods()
    env = batch_env.DeviceBatchEnv(3, 4, 2, 1)                          # gives the device and the stream only
    yield env
    env.close()


def _data(kind, K, seed):
    """-> cost4 [N*K,4], done [N*K]: group_reduce_ref.synthetic's kinds, or a constructed one — "chain": a total order, every candidate a
    rank of its own (the peeling's slow extreme); "antichain": mk + ec + tt constant, one rank; "flat": tt the same everywhere;
    "infinite": +inf scattered through the costs (NaN distances; with w_mk = 0 NaN objectives)"""
    if kind in ("integer", "random", "scattered", "none"):
        return gref.synthetic(kind, N, K, seed)
    rs = np.random.RandomState(seed)
    c4 = np.zeros((N, K, 4))
    for n in range(N):
        if kind == "chain":
            v = rs.permutation(K).astype(np.float64)
            c4[n, :, 0], c4[n, :, 1], c4[n, :, 2] = v, v, v
        elif kind == "antichain":
            a, b = rs.permutation(K).astype(np.float64), rs.permutation(K).astype(np.float64)
            c4[n, :, 0], c4[n, :, 1], c4[n, :, 2] = a, b, 2.0 * K - a - b
        elif kind == "flat":
            c4[n, :, 0], c4[n, :, 1], c4[n, :, 2] = rs.randint(0, K + 1, K), rs.randint(0, K + 1, K), 5.0
            c4[n, :, 3] = rs.randint(0, 3, K)
        else:
            c4[n] = rs.randint(0, 6, (K, 4))
            c4[n][rs.uniform(size=(K, 4)) < 0.1] = np.inf
    return c4.reshape(N * K, 4), np.ones(N * K, np.uint8)


def _split(x, K, Ka):
    """[N*K, ...] -> the a and b array sets (b None with Ka = K)"""
    x = x.reshape((N, K) + x.shape[1:])
    a = np.ascontiguousarray(x[:, :Ka]).reshape((N * Ka,) + x.shape[2:])
    b = None if Ka == K else np.ascontiguousarray(x[:, Ka:]).reshape((N * (K - Ka),) + x.shape[2:])
    return a, b


def _dev(x, dev):
    return None if x is None else torch.as_tensor(x, device=dev)


def _sentinels(K, dev):
    return (torch.full((N * K,), SENT_I, dtype=torch.int32, device=dev), torch.full((N * K,), SENT_F, dtype=torch.float64, device=dev),
            torch.full((N * K,), SENT_I, dtype=torch.int32, device=dev), torch.full((N,), SENT_I, dtype=torch.int32, device=dev),
            torch.full((N,), SENT_F, dtype=torch.float64, device=dev))


def _values(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    _same(np.isnan(got), np.isnan(want), tag + " (NaNs)")
    _same(np.nan_to_num(got, nan=0.0, posinf=np.inf, neginf=-np.inf), np.nan_to_num(want, nan=0.0, posinf=np.inf, neginf=-np.inf), tag)


@functools.lru_cache(maxsize=None)
def _case(kind, K):
    """the data of a case and the model's answer, computed once and shared by the tests that split it differently"""
    c4, dn = _data(kind, K, seed=11 * K + 3)
    return c4, dn, ref.front_rank(c4, dn, None, None, WEIGHTS[kind], N)


def _check(handle, kind, K, Ka):
    c4, dn, want = _case(kind, K)
    w = WEIGHTS[kind]
    dev = handle.device
    (ca, cb), (da, db) = _split(c4, K, Ka), _split(dn, K, Ka)
    outs = _sentinels(K, dev)
    got = handle.front_rank(N, _dev(ca, dev), _dev(da, dev), _dev(cb, dev), _dev(db, dev), w, *outs)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, outs))
    rank, crowd, order, size, best = [g.cpu().numpy() for g in got]
    tag = f"{kind} K={K} Ka={Ka}"
    _same(rank, want[0], tag + " rank")
    _values(crowd, want[1], tag + " crowd")
    _same(order, want[2], tag + " order")
    _same(size, want[3], tag + " front_size")
    _values(best, want[4], tag + " best_obj")
    return c4, dn, w, rank, want


@pytest.mark.parametrize("kind", ["integer", "random", "scattered", "none"])
@pytest.mark.parametrize("K", KS)
def test_front_rank_equals_the_model(handle, kind, K):
    c4, dn, w, rank, want = _check(handle, kind, K, K)
    dev = handle.device
    front = handle.group_reduce(N, K, _dev(c4, dev), _dev(dn, dev), w, False, False, False, True)[3]
    _same((rank == 0).astype(np.uint8), front.cpu().numpy(), f"{kind} K={K}: rank 0 is the device's own group_reduce front")
    if kind == "scattered":
        assert (rank[K:2 * K] == -1).all() and want[3][1] == 0, "group 1 must have no eligible candidate"
    if kind == "none":
        assert (rank == -1).all() and np.array_equal(want[2], np.tile(np.arange(K), N))
    if kind == "integer" and K >= 64:
        assert rank.max() >= 2, "duplicates fall to later ranks"


@pytest.mark.parametrize("kind", ["integer", "random", "scattered"])
@pytest.mark.parametrize("K", [k for k in KS if k >= 2])
def test_parents_and_children_in_two_array_sets(handle, kind, K):
    """(Ka, Kb) = (K/2, K - K/2); K = 2 is (1, 1)"""
    _check(handle, kind, K, K // 2)


@pytest.mark.parametrize("kind,K", [("chain", 257), ("antichain", 7), ("antichain", 257), ("antichain", 1025), ("flat", 7), ("flat", 257),
                                    ("flat", 1025), ("infinite", 7), ("infinite", 257), ("infinite", 1025)])
def test_constructed_groups(handle, kind, K):
    _, _, _, rank, want = _check(handle, kind, K, K)
    if kind == "chain":
        assert sorted(rank[:K].tolist()) == list(range(K)), "every candidate is a rank of its own"
    if kind == "antichain":
        assert (rank == 0).all() and np.isinf(want[1][:K]).sum() <= 7
    if kind == "infinite" and K >= 257:
        assert np.isnan(want[1]).any(), "the case must hold a NaN distance"


@pytest.mark.parametrize("keep", range(5), ids=["rank", "crowd", "order", "front_size", "best_obj"])
@pytest.mark.parametrize("K", [7, 257, 1025])
def test_null_outputs_are_skipped(handle, keep, K):
    c4, dn = _data("scattered", K, seed=5)
    w = WEIGHTS["scattered"]
    want = ref.front_rank(c4, dn, None, None, w, N)
    dev = handle.device
    outs = _sentinels(K, dev)
    got = handle.front_rank(N, _dev(c4, dev), _dev(dn, dev), None, None, w, *[outs[i] if i == keep else False for i in range(5)])
    torch.cuda.synchronize()
    assert [g is None for g in got] == [i != keep for i in range(5)]
    _values(got[keep].cpu().numpy(), want[keep], f"only output {keep}, K={K}")
    for i in range(5):
        if i != keep:
            assert (outs[i] == (SENT_F if outs[i].dtype == torch.float64 else SENT_I)).all().item()


@pytest.mark.parametrize("what", ["K=2049", "K=1025+1024", "Ka=0", "Kb<0", "N=0", "cost4_a", "done_a", "w", "cost4_b", "done_b"])
def test_front_rank_refusals_write_nothing(handle, what):
    _, capi = _mods()
    dev = handle.device
    c4 = torch.zeros(2 * 2049, 4, dtype=torch.float64, device=dev)
    dn = torch.ones(2 * 2049, dtype=torch.uint8, device=dev)
    outs = [torch.full((2 * 2049,), SENT_I, dtype=torch.int32, device=dev), torch.full((2 * 2049,), SENT_F, dtype=torch.float64, device=dev),
            torch.full((2 * 2049,), SENT_I, dtype=torch.int32, device=dev), torch.full((2,), SENT_I, dtype=torch.int32, device=dev),
            torch.full((2,), SENT_F, dtype=torch.float64, device=dev)]
    w = (C.c_double * 3)(0.4, 0.4, 0.2)
    n, ka, kb = {"K=2049": (2, 2049, 0), "K=1025+1024": (1, 1025, 1024), "Ka=0": (2, 0, 4), "Kb<0": (2, 4, -1), "N=0": (0, 4, 4)}.get(what, (2, 4, 4))
    ptr = {"cost4_a": c4.data_ptr(), "done_a": dn.data_ptr(), "cost4_b": c4.data_ptr(), "done_b": dn.data_ptr(), "w": w}
    if what in ptr:
        ptr[what] = None
    rc = handle.L.mtfjsp_front_rank(handle.h, n, ka, kb, ptr["cost4_a"], ptr["done_a"], ptr["cost4_b"], ptr["done_b"], ptr["w"],
                                    *[o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    assert rc == capi.ERR_ARG and b"mtfjsp_front_rank" in handle.L.mtfjsp_last_error(handle.h)
    for o in outs:
        assert (o == (SENT_F if o.dtype == torch.float64 else SENT_I)).all().item()


# ---------------------------------------------------------------- mtfjsp_plan_survivors
def _surv_case(J, M, P, two):
    """N groups of Ka = P parents and Kb = P children (two) or of K = P alone; every plan word names its array, row and column"""
    T, Ka, Kb = J * M, P, P if two else 0
    K = Ka + Kb
    rs = np.random.RandomState(100 * T + 10 * P + two)
    c4 = rs.randint(0, 4, (N * K, 4)).astype(np.float64)
    dn = (rs.uniform(size=N * K) > 0.2).astype(np.uint8)
    (ca, cb), (da, db) = _split(c4, K, Ka), _split(dn, K, Ka)
    code = lambda base, k: (base + 1000 * np.arange(T)[:, None] + np.arange(N * k)[None, :]).astype(np.int32)    # noqa: E731  [T, N*k]
    ta, ma = code(0, Ka), code(100000, Ka)
    tb, mb = (code(200000, Kb), code(300000, Kb)) if two else (None, None)
    rank, _, order, _, _ = ref.front_rank(ca, da, cb, db, (0.4, 0.4, 0.2), N)
    return T, Ka, Kb, (ta, ma, ca, da), (tb, mb, cb, db) if two else None, order, rank


def _surv_run(env, P, a, b, order, rank):
    dev = env.device
    B, T = env.B, env.T
    outs = (torch.full((T, B), SENT_I, dtype=torch.int32, device=dev), torch.full((T, B), SENT_I, dtype=torch.int32, device=dev),
            torch.full((B, 4), SENT_F, dtype=torch.float64, device=dev), torch.full((B,), 9, dtype=torch.uint8, device=dev),
            torch.full((B,), SENT_I, dtype=torch.int32, device=dev), torch.full((B,), SENT_I, dtype=torch.int32, device=dev),
            torch.full((B,), SENT_F, dtype=torch.float64, device=dev))
    da = tuple(_dev(np.ascontiguousarray(x), dev) for x in a)
    db = None if b is None else tuple(_dev(np.ascontiguousarray(x), dev) for x in b)
    got = env.plan_survivors(P, _dev(order, dev), _dev(rank, dev), da, db, *outs)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, outs))
    rows = lambda s: None if s is None else (s[0].T, s[1].T, s[2], s[3])    # noqa: E731  the model takes plans as rows
    want = ref.survivors(order, rank, P, N, *rows(a), *(rows(b) if b is not None else ()))
    got = [g.cpu().numpy() for g in got]
    tag = f"T={T} P={P} b={b is not None}"
    _same(got[0].T, want[0], tag + " task"); _same(got[1].T, want[1], tag + " mach")
    _values(got[2], want[2], tag + " cost4"); _same(got[3], want[3], tag + " done")
    _same(got[4], want[4], tag + " rank"); _same(got[5], want[5], tag + " src"); _values(got[6], want[6], tag + " fit")
    return got, want


@pytest.mark.parametrize("two", [True, False], ids=["K=2P", "K=P"])
@pytest.mark.parametrize("P", [1, 8, 9])
@pytest.mark.parametrize("J,M", [(2, 2), (3, 4)], ids=["J2M2", "J3M4"])
def test_plan_survivors_equals_the_model(J, M, P, two):
    batch_env, _ = _mods()
    T, Ka, Kb, a, b, order, rank = _surv_case(J, M, P, two)
    env = batch_env.DeviceBatchEnv(J, M, 2, N * P, obs_dtype="f32")
    try:
        got, want = _surv_run(env, P, a, b, order, rank)
        assert (got[0] != SENT_I).all(), "every word of the population is written"
        if P >= 8:
            assert np.isnan(want[6]).any() or (want[4] >= 0).all()
        # an order entry outside [0, K): a column of -1, done 0, and nothing outside the arrays is touched
        bad = order.copy()
        bad[0], bad[(N - 1) * (Ka + Kb) + P - 1] = Ka + Kb, -3
        got, want = _surv_run(env, P, a, b, bad, rank)
        assert (got[0][:, 0] == -1).all() and (got[1][:, N * P - 1] == -1).all() and got[3][0] == 0 and got[5][0] == Ka + Kb and got[5][N * P - 1] == -3
    finally:
        env.close()


@pytest.mark.parametrize("what", ["task_out=task_a", "mach_out=task_b", "fit_out=cost4_a", "rank_out=order", "src_out=rank_out", "task_out=mach_out",
                                  "P=0", "P>K", "batch", "null order", "null task_b", "null task_out", "Ka=0"])
def test_plan_survivors_refusals_write_nothing(what):
    batch_env, capi = _mods()
    J, M, P = 2, 2, 4
    T, Ka, Kb, a, b, order, rank = _surv_case(J, M, P, True)
    env = batch_env.DeviceBatchEnv(J, M, 2, N * P, obs_dtype="f32")
    try:
        dev = env.device
        B = N * P
        x = {k: _dev(np.ascontiguousarray(v), dev) for k, v in zip(("task_a", "mach_a", "cost4_a", "done_a", "task_b", "mach_b", "cost4_b", "done_b"), a + b)}
        x["order"], x["rank"] = _dev(order, dev), _dev(rank, dev)
        x.update(task_out=torch.full((T, B), SENT_I, dtype=torch.int32, device=dev), mach_out=torch.full((T, B), SENT_I, dtype=torch.int32, device=dev),
                 cost4_out=torch.full((B, 4), SENT_F, dtype=torch.float64, device=dev), done_out=torch.full((B,), 9, dtype=torch.uint8, device=dev),
                 rank_out=torch.full((B,), SENT_I, dtype=torch.int32, device=dev), src_out=torch.full((B,), SENT_I, dtype=torch.int32, device=dev),
                 fit_out=torch.full((B,), SENT_F, dtype=torch.float64, device=dev))
        before = {k: v.clone() for k, v in x.items()}
        p = {k: v.data_ptr() for k, v in x.items()}
        n, ka, kb, pp = N, Ka, Kb, P
        if "=" in what and not what.startswith(("P=", "Ka=")):
            dst, src = what.split("=")
            p[dst] = p[src]
        elif what.startswith("null"):
            p[what.split()[1]] = None
        elif what == "P=0":
            pp = 0
        elif what == "P>K":
            pp = Ka + Kb + 1
        elif what == "batch":
            n = N - 1
        elif what == "Ka=0":
            ka, kb = 0, Ka + Kb
        rc = env.L.mtfjsp_plan_survivors(env.h, n, ka, kb, pp, p["order"], p["rank"], p["task_a"], p["mach_a"], p["cost4_a"], p["done_a"], p["task_b"],
                                         p["mach_b"], p["cost4_b"], p["done_b"], p["task_out"], p["mach_out"], p["cost4_out"], p["done_out"],
                                         p["rank_out"], p["src_out"], p["fit_out"])
        torch.cuda.synchronize()
        assert rc == capi.ERR_ARG and b"mtfjsp_plan_survivors" in env.L.mtfjsp_last_error(env.h)
        for k in x:
            assert torch.equal(x[k], before[k]), f"{what}: {k} was written"
    finally:
        env.close()
