"""GPU: mtfjsp_plan_offspring (csrc/mtfjsp_evolve.hip) EQUALS its host model (tests/plan_crossover_ref.py, pinned by
tests/test_plan_crossover_cpu.py) element for element — task_out, mach_out, parent_out and kind_out: T = 12 and 36 (one pass), 64 (a
full pass), 65 (two passes) and 260 = J130 x M2 (M = 2 is the smallest the handle accepts: a second and third word block of the "jset"
and "mach" streams, the tile of 32) and 400 = J20 x M20 (the tile of 16, once: P = 5, N = 7); the launches above 48 KiB of LDS — J10M20 (tile 64), J70M8 (tile 16 above
the soft cap), J21M64 (the largest shape with 64 machines that is accepted) — and the refusal of J22M64 right at that edge; P = 1, 3, 64, 100 with N*P no multiple of the tile wherever P allows it (P = 64 never does), so
that groups straddle workgroups and the last tile is partial; objectives with NaNs and ties, a whole group NaN with best = -1, best
outside its group, best NULL; every single move mask and all three; thresholds 0, 2^32 and between; parents that are no plans; nothing
written outside the outputs or on an error return."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import plan_crossover_ref as ref
import plan_moves_ref as mref

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 256
SEED, GEN, FIRST = (1 << 45) + 77, 3, 3
MID_CROSS, MID_MUT = round(0.8 * 2 ** 32), 1 << 31
SHAPES = [(3, 4, 2), (6, 6, 2), (8, 8, 2), (5, 13, 1), (130, 2, 1)]
GROUPS = [(1, 70), (3, 23), (64, 3), (100, 2)]                         # (P, N)
DISTINCT = 12                                                          # random plans per instance; member c holds plan c % DISTINCT


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi"),
            import_module("e2e-mappo-for-mt-fjsp_amd.instances"))


class Setup:
    """N instances, the handle of their N*P copies, a population of random valid plans, objectives with NaNs and ties, best columns"""

    def __init__(self, shape, P, N):
        be, _, inst = _mods()
        J, M, E = shape
        self.J, self.M, self.E, self.T, self.P, self.N, self.B = J, M, E, J * M, P, N, N * P
        t, p, tt, edge = inst.generate_instances(N, J, M, E, seed=7000 + J * 100 + M)
        self.t = np.asarray(t)
        self.env = be.DeviceBatchEnv(J, M, E, self.B, left_shift=False, obs_dtype="f32")
        self.env.load_instances(*(np.repeat(np.asarray(x), P, axis=0) for x in (t, p, tt)), edge=np.repeat(np.asarray(edge), P, axis=0))
        self.dev = self.env.device
        plans = [mref.random_plans(self.t, J, M, 31 + c) for c in range(min(P, DISTINCT))]
        member = np.arange(P) % len(plans)
        self.task = np.stack([x[0] for x in plans], 1)[:, member].reshape(self.B, self.T)          # [N*P,T]
        self.mach = np.stack([x[1] for x in plans], 1)[:, member].reshape(self.B, self.T)
        rs = np.random.RandomState(9)
        self.obj = rs.randint(0, 6, self.B).astype(np.float64)          # few values: many ties
        self.obj[rs.rand(self.B) < 0.2] = np.nan
        self.nan_group = N // 2
        self.obj[self.nan_group * P:(self.nan_group + 1) * P] = np.nan
        self.best = (np.arange(N) * P + rs.randint(0, P, N)).astype(np.int32)
        self.best[self.nan_group] = -1                                  # what the reduction writes for a group without an eligible member
        if N > 2:
            self.best[0] = P                                            # another group's column: outside too

    def outputs(self):
        """padded device buffers full of SENT -> the four whole buffers and the four views the call writes"""
        T, B, d = self.T, self.B, self.dev
        whole = [torch.full((n + 2 * PAD,), SENT, dtype=dt, device=d) for n, dt in ((T * B, torch.int32), (T * B, torch.int32), (2 * B, torch.int32), (B, torch.int8))]
        views = [whole[0][PAD:PAD + T * B].view(T, B), whole[1][PAD:PAD + T * B].view(T, B), whole[2][PAD:PAD + 2 * B].view(B, 2), whole[3][PAD:PAD + B]]
        return whole, views

    def run(self, cross, mut, moves, best=True, task=None, mach=None, obj=None, extras=True, seed=SEED, gen=GEN, first=FIRST):
        """the device and the model on one population -> ((task [T,B], mach [T,B], parent, kind) of the device, the same of the model);
        the padding around the outputs and the sources are checked here"""
        task, mach, obj = (self.task if task is None else task), (self.mach if mach is None else mach), (self.obj if obj is None else obj)
        st, sm = np.ascontiguousarray(task.T), np.ascontiguousarray(mach.T)
        dt, dm, do = torch.as_tensor(st, device=self.dev), torch.as_tensor(sm, device=self.dev), torch.as_tensor(obj, device=self.dev)
        db = torch.as_tensor(self.best, device=self.dev) if best else None
        whole, (vt, vm, vp, vk) = self.outputs()
        self.env.plan_offspring(self.P, dt, dm, do, db, seed, gen, first, cross, mut, moves, vt, vm, vp if extras else None, vk if extras else None)
        torch.cuda.synchronize(self.dev)
        for buf, n in zip(whole, (self.T * self.B, self.T * self.B, 2 * self.B, self.B)):
            h = buf.cpu().numpy()
            assert (h[:PAD] == SENT).all() and (h[PAD + n:] == SENT).all(), "a store left the output array"
            if not extras and buf is not whole[0] and buf is not whole[1]:
                assert (h == SENT).all(), "parent_out = kind_out = NULL: neither is written"
        assert np.array_equal(dt.cpu().numpy(), st) and np.array_equal(dm.cpu().numpy(), sm), "the sources are only read"
        et, em, ep, ek = ref.offspring(self.t, task, mach, obj, self.best if best else None, self.P, seed, gen, first, cross, mut, moves)
        return (vt.cpu().numpy(), vm.cpu().numpy(), vp.cpu().numpy(), vk.cpu().numpy()), (np.ascontiguousarray(et.T), np.ascontiguousarray(em.T), ep, ek)

    def close(self):
        self.env.close()


@functools.lru_cache(maxsize=2)
def _setup(shape, P, N):
    return Setup(shape, P, N)


def _same(got, exp, tag):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{tag}: {len(bad)} of {exp.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {exp[tuple(bad[0])]}")


def _check(S, tag, *a, **kw):
    got, exp = S.run(*a, **kw)
    names = ("parent", "kind", "task", "mach") if kw.get("extras", True) else ("task", "mach")
    for name in names:
        k = ("task", "mach", "parent", "kind").index(name)
        _same(got[k], exp[k], f"{tag}: {name}")
    return got, exp


# every shape with every group, and T = 400: three tiles of 16 children, the last one partial, groups straddling tiles
CASES = [(s, p, n) for s in SHAPES for p, n in GROUPS] + [((20, 20, 2), 5, 7)]
# the launches above 48 KiB of LDS: (J, M) -> (tile, bytes, accepted) of k_plan_offspring.  J10M20: the first at the tile of 64; J70M8: a tile
# of 16 above the soft cap of 64 KiB, three words of the job set; J21M64: the largest shape with 64 machines the kernel accepts, J22M64
# the first it refuses (J30M50, further out, is refused in test_errors_write_nothing)
LAUNCH = {(20, 20): (16, 46944, True), (10, 20): (64, 61888, True), (70, 8): (16, 66416, True), (21, 64): (16, 156928, True),
          (22, 64): (16, 164400, False), (30, 50): (16, 175248, False)}
CASES += [((10, 20, 2), 5, 7), ((70, 8, 2), 5, 7), ((21, 64, 2), 3, 2)]


@pytest.mark.parametrize("shape,P,N", CASES, ids=[f"J{s[0]}M{s[1]}-P{p}-N{n}" for s, p, n in CASES])
def test_offspring_equal_the_model(shape, P, N):
    S = _setup(shape, P, N)
    tag = f"J{shape[0]}M{shape[1]} P={P} N={N}"
    if shape[:2] in LAUNCH:
        tile, nbytes, ok = ref.evo_launch(*shape[:2])
        assert (tile, nbytes, ok) == LAUNCH[shape[:2]] and ok and (N * P) % tile != 0
        assert (nbytes > mref.PLAN_LDS_ASK) == (shape[:2] != (20, 20)) and (nbytes > mref.PLAN_LDS_SOFT) == (shape[:2] in ((70, 8), (21, 64)))
    # thresholds between the ends, all three moves, the elite from `best` (one -1 beside a group of NaNs, one outside its group)
    got, exp = _check(S, tag + " mid", MID_CROSS, MID_MUT, 7)
    assert (got[2][::P] == -1).all() and (got[3][::P] == -1).all(), "child 0 is the elite"
    if P > 1:
        crossed, kinds = got[2][:, 1] >= 0, got[3]
        # (what a batch of 20 or more is bound to draw; the six children of the largest shape need not)
        assert S.B < 20 or crossed.any() and (~crossed[np.arange(S.B) % P != 0]).any() and {0} < set(kinds[kinds >= 0].tolist()) <= {0, 1, 2, 4}
        n = S.nan_group
        i = [(x * P) >> 32 for x in ref.words(SEED, GEN, FIRST + n, 1, ref.TAG_PARE)]
        assert got[2][n * P + 1, 0] == n * P + min(i[0], i[1]), "a whole group NaN selects by index"
    # best NULL: child 0 is an ordinary child; both events always; one move mask each
    got, _ = _check(S, tag + " best NULL, SWAP", ref.ALWAYS, ref.ALWAYS, 1, best=False)
    assert (got[2] >= 0).all() and (got[3] == 1).all()
    _check(S, tag + " no crossover, INSERT", ref.NEVER, ref.ALWAYS, 2)
    got, _ = _check(S, tag + " REASSIGN", ref.ALWAYS, ref.ALWAYS, 4)
    got0, _ = _check(S, tag + " no mutation", ref.ALWAYS, ref.NEVER, 7)
    assert (got0[3][np.arange(S.B) % P != 0] == 0).all()
    got, exp = _check(S, tag + " neither event", ref.NEVER, ref.NEVER, 7, best=False)
    _same(got[0], np.ascontiguousarray(S.task[got[2][:, 0]].T), tag + " neither event: every child is its parent A")
    # the low words of the instance number and of the generation are the counter; no parents and kinds asked for
    _, exp7 = S.run(MID_CROSS, MID_MUT, 7)
    got, _ = S.run(MID_CROSS, MID_MUT, 7, extras=False, first=(1 << 32) + FIRST, gen=(1 << 32) + GEN)
    _same(got[0], exp7[0], tag + " first_instance + 2^32, generation + 2^32: task"); _same(got[1], exp7[1], tag + " + 2^32: mach")
    if P > 1:
        got2, _ = _check(S, tag + " the seed's low word alone", MID_CROSS, MID_MUT, 7, seed=SEED & 0xFFFFFFFF)
        assert not np.array_equal(got2[2], exp7[2]), "the seed's high word is part of the key"
        got3, _ = _check(S, tag + " generation 0, first_instance 0", MID_CROSS, MID_MUT, 7, gen=0, first=0)
        assert not np.array_equal(got3[2], exp7[2])


@pytest.mark.parametrize("shape,P,N", [((6, 6, 2), 3, 23), ((5, 13, 1), 3, 23), ((130, 2, 1), 100, 2)], ids=["J6M6", "J5M13", "J130M2"])
def test_parents_that_are_no_plans(shape, P, N):
    """a parent with a task out of range, one with a job too often (a task twice, another never): every child that draws it is a column
    of -1, parents and kinds are written all the same, the other children do not change; guard regions as in every run"""
    S = _setup(shape, P, N)
    T, M = S.T, S.M
    base, _ = S.run(MID_CROSS, MID_MUT, 7)
    for what, row, pos, val in (("task T", 1, 0, T), ("task -1", S.B - 1, T - 1, -1), ("machine M", P + 1, T // 2, M), ("machine -1", 2, T - 1, -1),
                                ("a task twice", P + 2, T - 1, None)):
        tk, mc = S.task.copy(), S.mach.copy()
        if val is None:
            other = next(s for s in range(T) if tk[row, s] // M != tk[row, pos] // M)       # a job once too often, another once too seldom
            tk[row, pos], mc[row, pos] = tk[row, other], mc[row, other]
        else:
            (tk if what.startswith("task") else mc)[row, pos] = val
        got, exp = _check(S, f"{what} in member {row}", MID_CROSS, MID_MUT, 7, task=tk, mach=mc)
        used = (got[2] == row).any(1)
        assert (got[0][:, used] == -1).all() and (got[1][:, used] == -1).all()
        n = row // P
        rest = ~used
        rest[n * P] = (int(S.best[n]) if n * P <= S.best[n] < (n + 1) * P else n * P) != row      # (the elite is its column, changed or not)
        _same(got[0][:, rest], base[0][:, rest], what + ": the children of other parents")
        _same(got[2], base[2], what + ": parents"); _same(got[3], base[3], what + ": kinds")
    # the elite's column with an entry out of range is a column of -1; one with the operations of a job out of order is itself
    n = 3 % N
    col = int(S.best[n]) if n * P <= S.best[n] < (n + 1) * P else n * P
    tk = S.task.copy()
    tk[col] = tk[col][::-1]
    got, _ = _check(S, "elite in reverse order", MID_CROSS, MID_MUT, 7, task=tk)
    _same(got[0][:, n * P], tk[col], "the elite is its column word for word")
    tk[col, 3] = T
    got, _ = _check(S, "elite with task T", MID_CROSS, MID_MUT, 7, task=tk)
    assert (got[0][:, n * P] == -1).all() and (got[1][:, n * P] == -1).all()


def test_errors_write_nothing():
    be, capi, _ = _mods()
    S = _setup((6, 6, 2), 3, 23)
    L, h, T, B, P, N = S.env.L, S.env.h, S.T, S.B, S.P, S.N
    dt, dm = torch.as_tensor(np.ascontiguousarray(S.task.T), device=S.dev), torch.as_tensor(np.ascontiguousarray(S.mach.T), device=S.dev)
    do, db = torch.as_tensor(S.obj, device=S.dev), torch.as_tensor(S.best, device=S.dev)
    whole, (vt, vm, vp, vk) = S.outputs()
    ptr = lambda x: C.c_void_p(None if x is None else x.data_ptr())    # noqa: E731

    def call(handle=h, P=P, a=dt, b=dm, o=do, best=db, cross=MID_CROSS, mut=MID_MUT, moves=7, ot=vt, om=vm, op=vp, ok=vk):
        return L.mtfjsp_plan_offspring(handle, P, ptr(a), ptr(b), ptr(o), ptr(best), SEED, GEN, FIRST, cross, mut, moves, ptr(ot), ptr(om), ptr(op), ptr(ok))

    cases = {"P = 0": dict(P=0), "P = -1": dict(P=-1), "batch % P != 0": dict(P=4), "moves = 0": dict(moves=0), "moves = 8": dict(moves=8),
             "cross_thr = 2^32 + 1": dict(cross=(1 << 32) + 1), "mut_thr = 2^33": dict(mut=1 << 33),
             "src_task null": dict(a=None), "src_mach null": dict(b=None), "src_obj null": dict(o=None), "task_out null": dict(ot=None),
             "mach_out null": dict(om=None), "task_out is src_task": dict(a=vt), "mach_out inside src_mach": dict(b=whole[1][PAD - 4:].view(-1)[:T * B].view(T, B)),
             "task_out = mach_out": dict(om=vt), "parent_out inside src_obj": dict(o=whole[2][PAD:PAD + 2 * B].view(torch.float64)),
             "kind_out inside src_best": dict(best=whole[3][PAD:PAD + 4 * N].view(torch.int32)), "parent_out = mach_out": dict(op=vm)}
    for tag, kw in cases.items():
        assert call(**kw) == capi.ERR_ARG, tag
        assert b"mtfjsp_plan_offspring" in L.mtfjsp_last_error(h)
    assert call() == capi.OK
    torch.cuda.synchronize(S.dev)
    good = [x.cpu().numpy().copy() for x in (vt, vm, vp, vk)]
    for x in whole:
        x.fill_(SENT)
    fresh = be.DeviceBatchEnv(S.J, S.M, S.E, B, left_shift=False, obs_dtype="f32")
    try:
        assert call(handle=fresh.h) == capi.ERR_STATE, "a handle without instances"
        assert b"mtfjsp_plan_offspring" in L.mtfjsp_last_error(fresh.h)
    finally:
        fresh.close()
    assert call(handle=None) == capi.ERR_ARG
    big = be.DeviceBatchEnv(30, 50, 2, 16, left_shift=False, obs_dtype="f32")       # T = 1500: no tile of 16 plans fits the LDS
    try:
        big.generate_instances(1)
        z = torch.zeros(1500 * 16, dtype=torch.int32, device=S.dev)
        outs = [torch.full((1500 * 16,), SENT, dtype=torch.int32, device=S.dev) for _ in range(2)]
        rc = L.mtfjsp_plan_offspring(big.h, 4, ptr(z), ptr(z), ptr(torch.zeros(16, dtype=torch.float64, device=S.dev)), None, SEED, GEN, FIRST,
                                     MID_CROSS, MID_MUT, 7, ptr(outs[0]), ptr(outs[1]), None, None)
        assert rc == capi.ERR_ARG and b"too large" in L.mtfjsp_last_error(big.h)
        torch.cuda.synchronize(S.dev)
        assert all((x.cpu().numpy() == SENT).all() for x in outs)
    finally:
        big.close()
    # right at the edge: J22M64 needs 164 400 bytes, 560 more than a workgroup has; J21M64 (a case above) is accepted with 156 928
    assert ref.evo_launch(22, 64) == LAUNCH[22, 64] and ref.evo_launch(21, 64) == LAUNCH[21, 64] and ref.evo_launch(30, 50) == LAUNCH[30, 50]
    assert LAUNCH[21, 64][1] <= mref.PLAN_LDS_HARD < LAUNCH[22, 64][1]
    edge = be.DeviceBatchEnv(22, 64, 2, 6, left_shift=False, obs_dtype="f32")
    try:
        edge.generate_instances(1)
        z = torch.zeros(1408 * 6, dtype=torch.int32, device=S.dev)
        outs = [torch.full((1408 * 6,), SENT, dtype=torch.int32, device=S.dev) for _ in range(2)]
        rc = L.mtfjsp_plan_offspring(edge.h, 3, ptr(z), ptr(z), ptr(torch.zeros(6, dtype=torch.float64, device=S.dev)), None, SEED, GEN, FIRST,
                                     MID_CROSS, MID_MUT, 7, ptr(outs[0]), ptr(outs[1]), None, None)
        msg = L.mtfjsp_last_error(edge.h)
        assert rc == capi.ERR_ARG and b"mtfjsp_plan_offspring" in msg and b"tile of 16" in msg, msg
        torch.cuda.synchronize(S.dev)
        assert all((x.cpu().numpy() == SENT).all() for x in outs)
        edge.scaler_init(); edge.reset(torch.full((6, 3), 1 / 3, dtype=torch.float64, device=S.dev))     # the handle stays usable
        assert (edge.read_state(capi.STATE_MACHINE) == -1).all()
    finally:
        edge.close()
    for tag, kw in cases.items():
        assert call(**kw) == capi.ERR_ARG, tag
    torch.cuda.synchronize(S.dev)
    for x in whole:
        assert (x.cpu().numpy() == SENT).all(), "an error return wrote to an output"
    exp = ref.offspring(S.t, S.task, S.mach, S.obj, S.best, P, SEED, GEN, FIRST, MID_CROSS, MID_MUT, 7)
    _same(good[0], np.ascontiguousarray(exp[0].T), "the call between the errors: task"); _same(good[1], np.ascontiguousarray(exp[1].T), "the call between the errors: mach")
    _same(good[2], exp[2], "the call between the errors: parent"); _same(good[3], exp[3], "the call between the errors: kind")
