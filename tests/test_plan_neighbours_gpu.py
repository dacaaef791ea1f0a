"""GPU: mtfjsp_plan_neighbours (csrc/mtfjsp_plan.hip) EQUALS its host model (tests/plan_moves_ref.py, pinned by
tests/test_plan_moves_cpu.py) element for element, kinds included: T below, at and above one pass of 64 lanes, the T where the tile
of copies shrinks to 32 and to 16, the largest shape with 64 machines that fits a workgroup's LDS (J30M64) and the first that does not, K = 1, 2, 5 (tiles straddle groups), 64, 67, batches that are no multiple of the tile, every
single move mask and all three, every form of the source column, and nothing written outside the outputs or on an error return."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import plan_moves_ref as ref

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 256
SEED, ROUND, FIRST = (1 << 45) + 77, 3, 3
# (J, M, E), K, N: N*K is no multiple of the tile wherever K allows it (64 copies up to T = 236, 32 up to about T = 440, then 16)
CASES = [((3, 2, 1), 1, 70), ((3, 2, 1), 67, 3), ((3, 4, 2), 2, 35), ((6, 6, 2), 5, 27), ((6, 6, 2), 64, 2), ((8, 8, 2), 64, 3),
         ((8, 8, 2), 5, 15), ((5, 13, 1), 67, 3), ((5, 13, 1), 2, 35), ((10, 10, 2), 5, 27), ((10, 10, 2), 1, 70), ((20, 20, 2), 5, 15),
         ((15, 30, 2), 2, 9), ((30, 64, 2), 3, 2), ((4, 64, 2), 5, 7)]
# the launches the cases at a limit are there for: (J, M) -> (tile, bytes of LDS, accepted) of k_plan_neighbours<false, false>.  J30M64 is the
# largest shape with 64 machines the kernel accepts (2 080 bytes below PLAN_LDS_HARD), J31M64 the first it refuses; REASSIGN at M = 64
# ballots its candidates over all 64 lanes
LAUNCH = {(15, 30): (16, 38040, True), (30, 64): (16, 161760, True), (4, 64): (32, 37952, True), (31, 64): (16, 167152, False)}


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi"),
            import_module("e2e-mappo-for-mt-fjsp_amd.instances"))


class Setup:
    """N instances, the handle of their N*K copies and a random valid incumbent per instance"""

    def __init__(self, shape, K, N):
        be, _, inst = _mods()
        J, M, E = shape
        self.J, self.M, self.T, self.K, self.N, self.B = J, M, J * M, K, N, N * K
        t, p, tt, edge = inst.generate_instances(N, J, M, E, seed=7000 + J * 100 + M)
        self.t = np.asarray(t)
        self.env = be.DeviceBatchEnv(J, M, E, self.B, left_shift=False, obs_dtype="f32")
        self.env.load_instances(*(np.repeat(np.asarray(x), K, axis=0) for x in (t, p, tt)), edge=np.repeat(np.asarray(edge), K, axis=0))
        self.task, self.mach = ref.random_plans(self.t, J, M, 31)
        self.dev = self.env.device

    def source(self, cols, stride):
        """[T, stride] device arrays holding incumbent n in column cols[n] (where that is a column), SENT elsewhere"""
        st, sm = np.full((self.T, stride), SENT, np.int32), np.full((self.T, stride), SENT, np.int32)
        for n, c in enumerate(cols):
            if 0 <= c < stride:
                st[:, c], sm[:, c] = self.task[n], self.mach[n]
        return st, sm

    def outputs(self):
        """padded device buffers full of SENT -> (whole task, whole mach, whole kind, the three views the call writes)"""
        T, B = self.T, self.B
        bt = torch.full((T * B + 2 * PAD,), SENT, dtype=torch.int32, device=self.dev)
        bm = torch.full((T * B + 2 * PAD,), SENT, dtype=torch.int32, device=self.dev)
        bk = torch.full((B + 2 * PAD,), SENT, dtype=torch.int8, device=self.dev)
        return bt, bm, bk, bt[PAD:PAD + T * B].view(T, B), bm[PAD:PAD + T * B].view(T, B), bk[PAD:PAD + B]

    def expected(self, moves, bad=(), seed=SEED, rnd=ROUND, first=FIRST):
        et, em, ek = ref.neighbours(self.t, self.task, self.mach, self.K, seed, rnd, first, moves)
        for n in bad:
            et[n * self.K:(n + 1) * self.K] = -1
            em[n * self.K:(n + 1) * self.K] = -1
        return np.ascontiguousarray(et.T), np.ascontiguousarray(em.T), ek

    def run(self, st, sm, col, moves, kinds=True, seed=SEED, rnd=ROUND, first=FIRST):
        """-> (task [T,B], mach [T,B], kind [B] or None) host arrays; the padding around the outputs is checked here"""
        dt, dm = torch.as_tensor(st, device=self.dev), torch.as_tensor(sm, device=self.dev)
        dc = None if col is None else torch.as_tensor(np.asarray(col, np.int32), device=self.dev)
        bt, bm, bk, vt, vm, vk = self.outputs()
        self.env.plan_neighbours(self.K, dt, dm, dc, seed, rnd, first, moves, vt, vm, vk if kinds else None)
        torch.cuda.synchronize(self.dev)
        TB = self.T * self.B
        for whole, n in ((bt, TB), (bm, TB), (bk, self.B)):
            h = whole.cpu().numpy()
            assert (h[:PAD] == SENT).all() and (h[PAD + n:] == SENT).all(), "a store left the output array"
        if not kinds:
            assert (bk.cpu().numpy() == SENT).all(), "kind_out = NULL: no kinds are written"
        assert np.array_equal(dt.cpu().numpy(), st) and np.array_equal(dm.cpu().numpy(), sm), "the sources are only read"
        return vt.cpu().numpy(), vm.cpu().numpy(), vk.cpu().numpy() if kinds else None

    def close(self):
        self.env.close()


@functools.lru_cache(maxsize=2)
def _setup(shape, K, N):
    return Setup(shape, K, N)


def _same(got, exp, tag):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{tag}: {len(bad)} of {exp.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {exp[tuple(bad[0])]}")


@pytest.mark.parametrize("shape,K,N", CASES, ids=[f"J{s[0]}M{s[1]}-K{k}-N{n}" for s, k, n in CASES])
def test_every_mask_equals_the_model(shape, K, N):
    S = _setup(shape, K, N)
    if shape[:2] in LAUNCH:
        tile, nbytes, ok = ref.plan_launch(*shape[:2])
        assert (tile, nbytes, ok) == LAUNCH[shape[:2]] and ok and (N * K) % tile != 0
    stride = N + 5                                                      # wider than the columns used
    st, sm = S.source(range(N), stride)
    for moves in (1, 2, 4, 7):
        tag = f"J{shape[0]}M{shape[1]} K={K} N={N} moves={moves}"
        et, em, ek = S.expected(moves)
        gt, gm, gk = S.run(st, sm, None, moves)
        _same(gk, ek, tag + " kind"); _same(gt, et, tag + " task"); _same(gm, em, tag + " mach")
        if K > 1:
            assert set(np.unique(ek[ek >= 0]).tolist()) <= {b for b in (1, 2, 4) if moves & b}
    # the low words of the instance number and of the round are the counter; no kinds asked for
    et, em, _ = S.expected(7)
    gt, gm, gk = S.run(st, sm, None, 7, kinds=False, first=(1 << 32) + FIRST, rnd=(1 << 32) + ROUND)
    assert gk is None
    _same(gt, et, "first_instance + 2^32, round + 2^32: task"); _same(gm, em, "first_instance + 2^32, round + 2^32: mach")
    if K > 1:
        gt2, _, _ = S.run(st, sm, None, 7, seed=SEED & 0xFFFFFFFF)
        assert not np.array_equal(gt2, et), "the seed's high word is part of the key"
        gt3, gm3, gk3 = S.run(st, sm, None, 7, rnd=0, first=0)
        e3 = S.expected(7, rnd=0, first=0)
        _same(gt3, e3[0], "round 0, first_instance 0: task"); _same(gm3, e3[1], "round 0, first_instance 0: mach"); _same(gk3, e3[2], "round 0: kind")


@pytest.mark.parametrize("shape,K,N", [((6, 6, 2), 5, 27), ((5, 13, 1), 2, 35), ((20, 20, 2), 5, 15)], ids=["J6M6", "J5M13", "J20M20"])
def test_source_columns(shape, K, N):
    S = _setup(shape, K, N)
    T, M = S.T, S.M
    rs = np.random.RandomState(5)
    # a permuted src_col in a wider source
    stride = N + 9
    col = rs.permutation(stride)[:N].astype(np.int32)
    st, sm = S.source(col, stride)
    et, em, ek = S.expected(7)
    gt, gm, gk = S.run(st, sm, col, 7)
    _same(gk, ek, "permuted src_col: kind"); _same(gt, et, "permuted src_col: task"); _same(gm, em, "permuted src_col: mach")
    # one column -1, one equal to the stride: those groups are all -1, the others exact
    col2 = col.copy()
    col2[1], col2[N - 2] = -1, stride
    et, em, ek = S.expected(7, bad=(1, N - 2))
    gt, gm, gk = S.run(st, sm, col2, 7)
    _same(gk, ek, "bad src_col: kind"); _same(gt, et, "bad src_col: task"); _same(gm, em, "bad src_col: mach")
    # without src_col a group beyond the stride has no column
    st_n, sm_n = S.source(range(N - 3), N - 3)
    et, em, ek = S.expected(7, bad=(N - 3, N - 2, N - 1))
    gt, gm, gk = S.run(st_n, sm_n, None, 7)
    _same(gt, et, "src_col NULL, stride < N: task"); _same(gm, em, "src_col NULL, stride < N: mach")
    # an incumbent with one entry out of range: a task T, a task -1, a machine M, a machine -1 (the last position of a second pass included)
    for where, (arr, val) in zip(((0, 0), (T - 1, 2), (T // 2, N - 1), (T - 1, 4)), (("t", T), ("t", -1), ("m", M), ("m", -1))):
        st2, sm2 = st.copy(), sm.copy()
        s, n = where
        (st2 if arr == "t" else sm2)[s, col[n]] = val
        et, em, ek = S.expected(7, bad=(n,))
        gt, gm, gk = S.run(st2, sm2, col, 7)
        tag = f"incumbent {n} with {'task' if arr == 't' else 'machine'} {val} at step {s}"
        _same(gk, ek, tag + ": kind"); _same(gt, et, tag + ": task"); _same(gm, em, tag + ": mach")


def test_copy_zero_is_the_incumbent_word_for_word_and_wrong_counts_stay_in_range():
    """an in-range incumbent that is no plan: with every task once copy 0 still is that column; all entries are in range or -1"""
    S = _setup((6, 6, 2), 5, 27)
    st, sm = S.source(range(S.N), S.N)
    st[3, 2] = st[4, 2]                                                 # group 2: one task twice, another never
    st[:, 5] = st[::-1, 5]                                              # group 5: the operations of every job in reverse order
    gt, gm, gk = S.run(st, sm, None, 7)
    K = S.K
    assert np.array_equal(gt[:, 5 * K], st[:, 5]) and np.array_equal(gm[:, 5 * K], sm[:, 5]), "right counts, wrong order: copy 0 is the column as it is"
    for n in (2, 5):
        blk_t, blk_m = gt[:, n * K:(n + 1) * K], gm[:, n * K:(n + 1) * K]
        assert ((blk_t >= -1) & (blk_t < S.T)).all() and ((blk_m >= -1) & (blk_m < S.M)).all()
    et, em, _ = S.expected(7)
    keep = np.array([g for g in range(S.B) if g // K not in (2, 5)])
    _same(gt[:, keep], et[:, keep], "the other groups: task"); _same(gm[:, keep], em[:, keep], "the other groups: mach")


def test_errors_write_nothing():
    be, capi, _ = _mods()
    S = _setup((6, 6, 2), 5, 27)
    L, h, T, B, K, N = S.env.L, S.env.h, S.T, S.B, S.K, S.N
    st, sm = S.source(range(N), N)
    dt, dm = torch.as_tensor(st, device=S.dev), torch.as_tensor(sm, device=S.dev)
    dc = torch.arange(N, dtype=torch.int32, device=S.dev)
    bt, bm, bk, vt, vm, vk = S.outputs()
    P = lambda x: C.c_void_p(None if x is None else x.data_ptr())      # noqa: E731

    def call(handle=h, K=K, a=dt, b=dm, stride=N, col=dc, moves=7, ot=vt, om=vm, ok=vk):
        return L.mtfjsp_plan_neighbours(handle, K, P(a), P(b), stride, P(col), SEED, ROUND, FIRST, moves, P(ot), P(om), P(ok))

    whole_src = torch.cat([dt.flatten(), dm.flatten()])                 # one allocation: outputs inside it overlap the sources
    src_a, src_b = whole_src[:T * N].view(T, N), whole_src[T * N:].view(T, N)
    cases = {"K = 0": dict(K=0), "K = -1": dict(K=-1), "batch % K != 0": dict(K=4), "moves = 0": dict(moves=0), "moves = 8": dict(moves=8),
             "src_task null": dict(a=None), "src_mach null": dict(b=None), "task_out null": dict(ot=None), "mach_out null": dict(om=None),
             "src_stride = 0": dict(stride=0), "src_stride < 0": dict(stride=-3),
             "task_out is src_task": dict(a=vt, stride=B), "mach_out inside src_mach": dict(b=bm[PAD - 4:].view(-1)[:T * B].view(T, B), stride=B),
             "task_out = mach_out": dict(om=vt), "kind_out inside src_col": dict(col=bk[PAD:PAD + 4 * N].view(torch.int32))}
    for tag, kw in cases.items():
        assert call(**kw) == capi.ERR_ARG, tag
    assert call(a=src_a, b=src_b) == capi.OK                           # (sources in one allocation are fine)
    torch.cuda.synchronize(S.dev)
    good = (vt.cpu().numpy().copy(), vm.cpu().numpy().copy())
    bt.fill_(SENT); bm.fill_(SENT); bk.fill_(SENT)
    fresh = be.DeviceBatchEnv(S.J, S.M, 2, B, left_shift=False, obs_dtype="f32")
    try:
        assert call(handle=fresh.h) == capi.ERR_STATE, "a handle without instances"
        assert b"mtfjsp_plan_neighbours" in L.mtfjsp_last_error(fresh.h)
    finally:
        fresh.close()
    assert call(handle=None) == capi.ERR_ARG
    for tag, kw in cases.items():
        assert call(**kw) == capi.ERR_ARG, tag
    torch.cuda.synchronize(S.dev)
    for whole in (bt, bm, bk):
        assert (whole.cpu().numpy() == SENT).all(), "an error return wrote to an output"
    assert np.array_equal(dt.cpu().numpy(), st) and np.array_equal(dm.cpu().numpy(), sm)
    et, em, _ = S.expected(7)
    _same(good[0], et, "the call between the errors: task"); _same(good[1], em, "the call between the errors: mach")


def test_one_job_more_than_the_largest_shape_with_64_machines_is_refused():
    """J31M64: a tile of 16 plans needs 167 152 bytes of LDS, J30M64 (a case above) 161 760 of the 163 840 a workgroup has.  The refusal
    names the tile, writes nothing, and the handle stays usable"""
    be, capi, _ = _mods()
    assert ref.plan_launch(31, 64) == LAUNCH[31, 64] and ref.plan_launch(30, 64) == LAUNCH[30, 64]
    assert LAUNCH[30, 64][1] <= ref.PLAN_LDS_HARD < LAUNCH[31, 64][1]
    J, M, K, N = 31, 64, 3, 2
    T, B = J * M, K * N
    env = be.DeviceBatchEnv(J, M, 2, B, left_shift=False, obs_dtype="f32")
    try:
        env.generate_instances(1)
        dev, L = env.device, env.L
        src = torch.zeros((T, N), dtype=torch.int32, device=dev)
        outs = [torch.full((T * B,), SENT, dtype=torch.int32, device=dev) for _ in range(2)] + [torch.full((B,), SENT, dtype=torch.int8, device=dev)]
        P = lambda x: C.c_void_p(x.data_ptr())                          # noqa: E731
        for moves in (7, 1, 4):
            assert L.mtfjsp_plan_neighbours(env.h, K, P(src), P(src.clone()), N, None, SEED, ROUND, FIRST, moves, *[P(x) for x in outs]) == capi.ERR_ARG
            msg = L.mtfjsp_last_error(env.h)
            assert b"mtfjsp_plan_neighbours" in msg and b"tile of 16" in msg, msg
        torch.cuda.synchronize(dev)
        assert all((x.cpu().numpy() == SENT).all() for x in outs), "an error return wrote to an output"
        # the handle still works: it reads back its instances and is reset
        t = env.read_instances()[0]
        assert t.shape == (B, T, M)
        env.scaler_init(); env.reset(torch.full((B, 3), 1 / 3, dtype=torch.float64, device=dev))
        assert (env.read_state(capi.STATE_MACHINE) == -1).all()
    finally:
        env.close()
