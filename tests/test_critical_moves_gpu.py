"""GPU: mtfjsp_plan_neighbours_critical and baselines.local_search with the moves a critical path directs EQUAL their host model
(tests/critical_path_ref.py, pinned by tests/test_critical_path_cpu.py) element for element, kinds included.
The moves: path arrays taken from the device (`critical_path` of a handle that replayed the incumbents), T below, at and above one
pass of 64 lanes, N*K no multiple of the tile, complete, half and empty schedules, every mask with a new kind, all five kinds, and
moves = 7 through the new entry against the old entry; path entries out of range; refusals that write nothing.  With paths from the host
model: the tiles of 64, 32 and 16 copies, launches above 48 KiB of LDS, J > 64, the largest shape the directed moves accept (J47M32) and the
first they refuse (J48M32).
The search: the two rows of tests/test_local_search_gpu.py, moves = 31 and 24, left shift on and off, in chunks, with one copy, with no
rounds, twice with one seed — every bit of start_obj, history, accepted, the plans and the three result entries."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import critical_path_ref as ref
import plan_moves_ref as pref

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 64
SEED, ROUND, FIRST = (1 << 45) + 77, 3, 3
KN = 7                                                                  # copies per group in the tests of the moves
ROWS = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}
K, ROUNDS, LS_SEED = 8, 6, 11
MAKESPAN_ONLY = (1.0, 0.0, 0.0)


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi"),
            import_module("e2e-mappo-for-mt-fjsp_amd.baselines"))


def _same(got, exp, tag):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, f"{tag}: {got.shape} {got.dtype} against {exp.shape} {exp.dtype}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{tag}: {len(bad)} of {exp.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {exp[tuple(bad[0])]}")


class Setup:
    """N instances with a random plan each, a handle that replays the plans (the paths come from it) and the handle of the N*KN copies"""

    def __init__(self, shape, KN=KN):
        be, _, _ = _mods()
        (J, M, E, N), variants, (self.task, self.mach) = ref.shape_inputs(shape)
        self.J, self.M, self.E, self.N, self.T, self.B, self.KN = J, M, E, N, J * M, N * KN, KN
        self.data = variants["generated"]
        self.t = self.data[0]
        self.env = be.DeviceBatchEnv(J, M, E, self.B, left_shift=False, obs_dtype="f32")
        self.env.load_instances(*(np.repeat(x, KN, axis=0) for x in self.data[:3]), edge=np.repeat(self.data[3], KN, axis=0))
        self.dev = self.env.device
        self.src = tuple(torch.as_tensor(np.ascontiguousarray(x.T), device=self.dev) for x in (self.task, self.mach))     # [T,N]

    def paths(self, left_shift, steps):
        """the incumbents' first `steps` steps replayed on a handle of their own -> device (path_task, path_arc, path_len)"""
        be, _, _ = _mods()
        top = be.DeviceBatchEnv(self.J, self.M, self.E, self.N, left_shift=left_shift, obs_dtype="f32")
        try:
            top.load_instances(*self.data[:3], edge=self.data[3])
            top.scaler_init()
            top.reset(torch.tensor([ref.CONFIG_W], dtype=torch.float64, device=self.dev).repeat(self.N, 1))
            for s in range(steps):
                top.step(self.src[0][s], self.src[1][s])
            out = top.critical_path()
            torch.cuda.synchronize(self.dev)
            return out
        finally:
            top.close()

    def host_paths(self, left_shift, steps):
        """the same from the host model on the oracle's replay (no kernel but the one under test) -> host arrays"""
        state = ref.replay(self.data, self.task, self.mach, left_shift, ref.CONFIG_W, steps)[4]
        return ref.path_rows(state, np.asarray(self.data[2]), self.J, self.M)

    def run(self, moves, critical, entry="new"):
        """-> host (task [T,B], mach [T,B], kind [B]); the padding around the outputs and the sources are checked here"""
        T, B, KN = self.T, self.B, self.KN
        bt = torch.full((T * B + 2 * PAD,), SENT, dtype=torch.int32, device=self.dev)
        bm = torch.full((T * B + 2 * PAD,), SENT, dtype=torch.int32, device=self.dev)
        bk = torch.full((B + 2 * PAD,), SENT, dtype=torch.int8, device=self.dev)
        before = None if critical is None else [x.cpu().numpy().copy() for x in critical]
        self.env.plan_neighbours(KN, self.src[0], self.src[1], None, SEED, ROUND, FIRST, moves, bt[PAD:PAD + T * B].view(T, B), bm[PAD:PAD + T * B].view(T, B),
                                 bk[PAD:PAD + B], critical=critical if entry == "new" else None)
        torch.cuda.synchronize(self.dev)
        for whole, n in ((bt, T * B), (bm, T * B), (bk, B)):
            h = whole.cpu().numpy()
            assert (h[:PAD] == SENT).all() and (h[PAD + n:] == SENT).all(), "a store left the output array"
        if critical is not None:
            assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(critical, before)), "the path arrays are only read"
        return bt[PAD:PAD + T * B].view(T, B).cpu().numpy(), bm[PAD:PAD + T * B].view(T, B).cpu().numpy(), bk[PAD:PAD + B].cpu().numpy()

    def expected(self, moves, paths, bad=()):
        KN = self.KN
        et, em, ek = ref.neighbours(self.t, self.task, self.mach, KN, SEED, ROUND, FIRST, moves, paths)
        for n in bad:
            et[n * KN:(n + 1) * KN] = -1
            em[n * KN:(n + 1) * KN] = -1
        return np.ascontiguousarray(et.T), np.ascontiguousarray(em.T), ek

    def close(self):
        self.env.close()


@functools.lru_cache(maxsize=1)
def _setup(shape, KN=KN):
    return Setup(shape, KN)


# The launches the larger shapes are there for: shape -> (copies per group, tile, bytes of LDS of k_plan_neighbours<false, true>).  N * K
# is no multiple of the tile; the paths come from the host model on the oracle's replay.  J47M32 is the largest T the directed moves
# accept (656 bytes below PLAN_LDS_HARD): 2 x 3 copies, the masks with a directed kind only
TILES = {"J10M20": (5, 64, 60160),                                      # the first launch above 48 KiB
         "J15M16": (5, 32, 41520), "J20M20": (5, 16, 43520),
         "J70M8": (5, 16, 61600),                                       # a tile of 16 above 48 KiB, J > 64
         "J47M32": (3, 16, 163184)}


@pytest.mark.parametrize("shape", ["J3M4", "J8M8", "J10M10"] + list(TILES))
def test_every_mask_equals_the_model(shape):
    large = shape in TILES
    S = _setup(shape, TILES[shape][0]) if large else _setup(shape)
    T = S.T
    points, masks = ((False, T), (True, T), (False, T // 2), (False, 0)), (8, 16, 24, 31, 7)
    if large:
        K, tile, nbytes = TILES[shape]
        assert pref.plan_launch(S.J, S.M, crit=True) == (tile, nbytes, True) and (S.N * K) % tile != 0 and T > 64
        assert (nbytes > pref.PLAN_LDS_ASK) == (shape in ("J10M20", "J70M8", "J47M32"))
    if shape == "J47M32":
        assert pref.PLAN_LDS_HARD - nbytes == 656 and not pref.plan_launch(48, 32, crit=True)[2]
        points, masks = ((False, T), (True, T // 2)), (24, 31)
    old = S.run(7, None, entry="old")
    kinds = set()
    for left_shift, steps in points:
        if large:
            paths = S.host_paths(left_shift, steps)
            dev_paths = tuple(torch.as_tensor(x, device=S.dev) for x in paths)
        else:
            dev_paths = S.paths(left_shift, steps)
            paths = tuple(x.cpu().numpy() for x in dev_paths)
        assert (paths[2] > 0).all() if steps else (paths[2] == 0).all()
        for moves in masks:
            tag = f"{shape} left_shift={left_shift} steps={steps} moves={moves}"
            et, em, ek = S.expected(moves, paths)
            gt, gm, gk = S.run(moves, dev_paths)
            _same(gk, ek, tag + " kind"); _same(gt, et, tag + " task"); _same(gm, em, tag + " mach")
            kinds |= set(np.unique(gk).tolist())
            if moves == 7:
                for got, exp, what in zip((gt, gm, gk), old, ("task", "mach", "kind")):
                    _same(got, exp, tag + " through the new entry against the old entry: " + what)
    assert {-1, 8, 16} <= kinds <= {-1, 1, 2, 4, 8, 16} if large else kinds == {-1, 1, 2, 4, 8, 16}        # (12 or 4 drawn copies: not every kind)


def test_one_job_more_than_the_directed_moves_accept():
    """J48M32: a tile of 16 with the path arrays needs 166 656 bytes, more than a workgroup has — refused, nothing written; without
    them 129 792 bytes, and the same handle takes the plain call"""
    _, capi, _ = _mods()
    assert pref.plan_launch(48, 32, crit=True) == (16, 166656, False) and pref.plan_launch(48, 32) == (16, 129792, True)
    S = _setup("J48M32", 3)
    L, h, T, B, N, dev, K = S.env.L, S.env.h, S.T, S.B, S.N, S.dev, S.KN
    paths = tuple(torch.as_tensor(x, device=dev) for x in S.host_paths(False, 4))
    bt = torch.full((T * B,), SENT, dtype=torch.int32, device=dev)
    bm = torch.full((T * B,), SENT, dtype=torch.int32, device=dev)
    bk = torch.full((B,), SENT, dtype=torch.int8, device=dev)
    P = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    for moves in (31, 16, 8):                                           # every mask with a directed kind stages the path rows
        rc = L.mtfjsp_plan_neighbours_critical(h, K, P(S.src[0]), P(S.src[1]), N, None, SEED, ROUND, FIRST, moves, P(bt), P(bm), P(bk), *[P(x) for x in paths])
        assert rc == capi.ERR_ARG, moves
        msg = L.mtfjsp_last_error(h)
        assert b"mtfjsp_plan_neighbours_critical" in msg and b"tile of 16" in msg, msg
    torch.cuda.synchronize(dev)
    for whole in (bt, bm, bk):
        assert (whole.cpu().numpy() == SENT).all(), "an error return wrote to an output"
    gt, gm, gk = S.run(7, None, entry="old")
    et, em, ek = pref.neighbours(S.t, S.task, S.mach, K, SEED, ROUND, FIRST, 7)
    _same(gk, ek, "J48M32 plain call after the refusal: kind")
    _same(gt, np.ascontiguousarray(et.T), "J48M32 plain call after the refusal: task"); _same(gm, np.ascontiguousarray(em.T), "J48M32 plain call after the refusal: mach")


@pytest.mark.parametrize("shape", ["J3M4", "J10M10"])
def test_path_entries_out_of_range_give_groups_of_minus_one(shape):
    S = _setup(shape)
    T, N = S.T, S.N
    dev_paths = S.paths(False, T)
    good = tuple(x.cpu().numpy() for x in dev_paths)
    L = good[2]
    cases = {"a task T at the head": (0, lambda p: p[0].__setitem__((0, 0), T)),
             "a task -1 at the path's last element": (1, lambda p: p[0].__setitem__((1, L[1] - 1), -1)),
             "a task 2^20 in the middle": (2, lambda p: p[0].__setitem__((2, L[2] // 2), 1 << 20)),
             "path_len T + 1": (0, lambda p: p[2].__setitem__(0, T + 1)),
             "path_len -1": (N - 1, lambda p: p[2].__setitem__(N - 1, -1))}
    for what, (n_bad, edit) in cases.items():
        p = tuple(x.copy() for x in good)
        edit(p)
        for moves in (8, 31):
            et, em, ek = S.expected(moves, good, bad=(n_bad,))
            gt, gm, gk = S.run(moves, tuple(torch.as_tensor(x, device=S.dev) for x in p))
            _same(gk, ek, f"{what}, moves={moves}: kind"); _same(gt, et, f"{what}, moves={moves}: task"); _same(gm, em, f"{what}, moves={moves}: mach")
    # entries at and after path_len are not read as tasks, arcs other than 1 are no machine arcs
    p = tuple(x.copy() for x in good)
    for n in range(N):
        p[0][n, L[n]:] = 1 << 20
        p[1][n, L[n]:] = 1
        p[1][n, L[n] - 1] = 1                                           # (the last element's arc leads nowhere: k + 1 < L)
    et, em, ek = S.expected(31, good)
    gt, gm, gk = S.run(31, tuple(torch.as_tensor(x, device=S.dev) for x in p))
    _same(gk, ek, "garbage after path_len: kind"); _same(gt, et, "garbage after path_len: task"); _same(gm, em, "garbage after path_len: mach")


def test_errors_write_nothing():
    _, capi, _ = _mods()
    S = _setup("J3M4")
    L, h, T, B, N, dev = S.env.L, S.env.h, S.T, S.B, S.N, S.dev
    pt, pa, pl = S.paths(False, T)
    bt = torch.full((T * B,), SENT, dtype=torch.int32, device=dev)
    bm = torch.full((T * B,), SENT, dtype=torch.int32, device=dev)
    bk = torch.full((B,), SENT, dtype=torch.int8, device=dev)
    P = lambda x: C.c_void_p(None if x is None else x.data_ptr())      # noqa: E731

    def call(moves=31, ot=bt, om=bm, ok=bk, a=pt, b=pa, c=pl, K=KN):
        return L.mtfjsp_plan_neighbours_critical(h, K, P(S.src[0]), P(S.src[1]), N, None, SEED, ROUND, FIRST, moves, P(ot), P(om), P(ok), P(a), P(b), P(c))

    cases = {"moves = 0": dict(moves=0), "moves = 32": dict(moves=32), "K = 0": dict(K=0), "batch % K != 0": dict(K=KN + 1),
             "path_task null, CRIT_SWAP": dict(a=None, moves=8), "path_arc null, CRIT_REASSIGN": dict(b=None, moves=16), "path_len null, all kinds": dict(c=None),
             "task_out null": dict(ot=None),
             "task_out inside path_task": dict(a=bt[T:T + N * T]), "mach_out inside path_len": dict(c=bm[5:5 + N]),
             "kind_out inside path_arc": dict(ok=pa.view(-1)[1:1 + B])}
    assert N * T > B
    for tag, kw in cases.items():
        assert call(**kw) == capi.ERR_ARG, tag
        assert b"mtfjsp_plan_neighbours_critical" in L.mtfjsp_last_error(h)
    torch.cuda.synchronize(dev)
    for whole in (bt, bm, bk):
        assert (whole.cpu().numpy() == SENT).all(), "an error return wrote to an output"
    assert call(moves=7, a=None, b=None, c=None) == capi.OK, "moves <= 7: the path arrays are not needed"
    torch.cuda.synchronize(dev)
    old = S.run(7, None, entry="old")
    _same(bt.view(T, B).cpu().numpy(), old[0], "moves = 7 without path arrays, new entry against the old entry: task")
    _same(bm.view(T, B).cpu().numpy(), old[1], "moves = 7 without path arrays, new entry against the old entry: mach")
    _same(bk.cpu().numpy(), old[2], "moves = 7 without path arrays, new entry against the old entry: kind")
    assert call() == capi.OK
    torch.cuda.synchronize(dev)
    et, em, ek = S.expected(31, tuple(x.cpu().numpy() for x in (pt, pa, pl)))
    _same(bt.view(T, B).cpu().numpy(), et, "the call after the errors: task"); _same(bk.cpu().numpy(), ek, "the call after the errors: kind")
    # the old entry keeps refusing the new kinds
    assert L.mtfjsp_plan_neighbours(h, KN, P(S.src[0]), P(S.src[1]), N, None, SEED, ROUND, FIRST, 8, P(bt), P(bm), P(bk)) == capi.ERR_ARG


# ---- baselines.local_search
def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _row(shape, w=ref.CONFIG_W):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = ROWS[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M, native=False)
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=w[0], weight_ec=w[1], weight_tt=w[2])
    return data, args, pref.first_feasible_plan(data[0]), (J, M, E, N)


@functools.lru_cache(maxsize=None)
def _device(shape, moves, left_shift, chunk=None, k=K, rounds=ROUNDS, w=ref.CONFIG_W):
    data, args, start, _ = _row(shape, w)
    return _mods()[2].local_search(*data, args, start, K=k, rounds=rounds, seed=LS_SEED, moves=moves, left_shift=left_shift, chunk=chunk)


@functools.lru_cache(maxsize=None)
def _model(shape, moves, left_shift, k=K, rounds=ROUNDS, w=ref.CONFIG_W):
    data, _, start, _ = _row(shape, w)
    return ref.search(data, start, k, rounds, LS_SEED, moves, left_shift, w)


def _check(res, exp, tag, name="LS"):
    b = _mods()[2]
    assert sorted(res) == sorted([name, b.PLANS, "start_obj", "history", "accepted"])
    _same(_bits(res["start_obj"]), _bits(exp["start_obj"]), tag + " start_obj (bits)")
    _same(_bits(res["history"]), _bits(exp["history"]), tag + " history (bits)")
    _same(res["accepted"], exp["accepted"], tag + " accepted")
    _same(res[b.PLANS][name][0], exp["plans"][0], tag + " final plans: tasks"); _same(res[b.PLANS][name][1], exp["plans"][1], tag + " final plans: machines")
    cost, final4, obj = res[name]
    assert sorted(cost) == sorted(ref.COST_KEYS)
    for key in ref.COST_KEYS:
        _same(_bits(cost[key]), _bits(exp["cost"][key]), f"{tag} {key} (bits)")
    _same(_bits(final4), _bits(exp["final4"]), tag + " Final_4cost (bits)"); _same(_bits(obj), _bits(exp["obj"]), tag + " Objective (bits)")


def test_constants():
    b = _mods()[2]
    assert (b.MOVE_CRIT_SWAP, b.MOVE_CRIT_REASSIGN, b.CRIT_MOVES, b.ALL_MOVES) == (8, 16, 24, 7)


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("moves", [31, 24])
@pytest.mark.parametrize("shape", list(ROWS))
def test_local_search_equals_the_model(shape, moves, left_shift):
    res, exp = _device(shape, moves, left_shift), _model(shape, moves, left_shift)
    _check(res, exp, f"{shape} moves={moves} left_shift={left_shift}")
    hist = np.vstack([res["start_obj"][None], res["history"]])
    assert (np.diff(hist, axis=0) <= 0).all()
    assert _bits(res["LS"][2]).tolist() == _bits(hist[-1]).tolist(), "the replayed plans have the last round's objectives"
    assert set(np.unique(res["accepted"]).tolist()) & {8, 16}


@pytest.mark.parametrize("shape", list(ROWS))
def test_makespan_only_accepts_both_new_kinds(shape):
    res, exp = _device(shape, 31, False, w=MAKESPAN_ONLY), _model(shape, 31, False, w=MAKESPAN_ONLY)
    _check(res, exp, f"{shape} moves=31 w=(1,0,0)")
    assert {8, 16} <= set(np.unique(res["accepted"]).tolist())


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(ROWS))
def test_chunks_of_two_equal_the_unchunked_run(shape, left_shift):
    """N = 4 in two passes, N = 3 with a padded last pass: draws and paths belong to the instance, not to its place in a pass"""
    b = _mods()[2]
    full, res = _device(shape, 31, left_shift), _device(shape, 31, left_shift, 2)
    _check(res, _model(shape, 31, left_shift), f"{shape} left_shift={left_shift} chunk=2")
    for key in ("start_obj", "history", "accepted"):
        _same(res[key], full[key], f"{shape} chunk=2 against unchunked: {key}")
    _same(res[b.PLANS]["LS"][0], full[b.PLANS]["LS"][0], shape + " chunk=2 against unchunked: plans")


@pytest.mark.parametrize("shape", list(ROWS))
def test_no_rounds_one_copy_and_a_second_run(shape):
    b = _mods()[2]
    data, args, start, (J, M, E, N) = _row(shape)
    res = b.local_search(*data, args, start, K=K, rounds=0, seed=LS_SEED, moves=31, name="START")
    _check(res, _model(shape, 31, False, K, 0), shape + " rounds=0", name="START")
    assert res["history"].shape == (0, N) and res["accepted"].shape == (0, N) and res["accepted"].dtype == np.int8
    _same(res[b.PLANS]["START"][0], start[0], "rounds = 0: the plans are the start plans")
    one = _device(shape, 31, False, None, 1, 3)
    _check(one, _model(shape, 31, False, 1, 3), shape + " K=1")
    assert (_bits(one["history"]) == _bits(one["start_obj"])[None]).all() and (one["accepted"] == -1).all()
    a = _device(shape, 31, False)
    again = b.local_search(*data, args, start, K=K, rounds=ROUNDS, seed=LS_SEED, moves=31)
    for key in ("start_obj", "history", "accepted"):
        _same(again[key], a[key], "second run: " + key)
    _same(again[b.PLANS]["LS"][0], a[b.PLANS]["LS"][0], "second run: tasks"); _same(again[b.PLANS]["LS"][1], a[b.PLANS]["LS"][1], "second run: machines")
    with pytest.raises(ValueError):
        b.local_search(*data, args, start, K=4, rounds=1, moves=32)
