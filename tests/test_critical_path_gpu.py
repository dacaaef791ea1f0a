"""GPU: mtfjsp_critical_path (k_critical_path, csrc/mtfjsp_plan.hip) EQUALS its host model (tests/critical_path_ref.py, pinned by
tests/test_critical_path_cpu.py) element for element — path_task, path_arc and path_len — on the inputs that file proves to cover
both kinds of arc, tasks tight on both sides, equal largest finish times (in different passes of 64 tasks too): T below, at and above
one pass of 64 lanes, T = 128 and 129 (the doubling loop's last round), J > 64, and J28M64 (T = 1792, 50 288 bytes of LDS: the launch
that asks for more than 48 KiB; 64 machines), N = 2..5 rows (the last workgroup's four waves are not all used), left shift on and off, after 0, 2, T / 2 and T steps.  The model
reads `read_state` of the very handle the kernel reads.  Every form of `col`, and nothing written outside the outputs or on an
error return."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import critical_path_ref as ref

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 64


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


def _same(got, exp, tag):
    assert got.shape == exp.shape and got.dtype == exp.dtype, f"{tag}: {got.shape} {got.dtype} against {exp.shape} {exp.dtype}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{tag}: {len(bad)} of {exp.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {exp[tuple(bad[0])]}")


def _open(shape, data, left_shift):
    be, _ = _mods()
    J, M, E, N = ref.SHAPES[shape]
    env = be.DeviceBatchEnv(J, M, E, N, left_shift=left_shift, obs_dtype="f32")
    env.load_instances(*data[:3], edge=data[3])
    env.scaler_init()
    env.reset(torch.tensor([ref.CONFIG_W], dtype=torch.float64, device=env.device).repeat(N, 1))
    return env


def _state(env):
    _, capi = _mods()
    env.synchronize()
    return dict(mach=env.read_state(capi.STATE_MACHINE), st=env.read_state(capi.STATE_START), ft=env.read_state(capi.STATE_FINISH),
                routes=env.read_state(capi.STATE_ROUTES))


def _paths(env, col=None):
    """critical_path into padded buffers full of SENT -> host (path_task, path_arc, path_len); the padding is checked here"""
    n, T, dev = env.B if col is None else len(col), env.T, env.device
    bt = torch.full((n * T + 2 * PAD,), SENT, dtype=torch.int32, device=dev)
    ba = torch.full((n * T + 2 * PAD,), SENT, dtype=torch.int8, device=dev)
    bl = torch.full((n + 2 * PAD,), SENT, dtype=torch.int32, device=dev)
    dc = None if col is None else torch.as_tensor(np.asarray(col, np.int32), device=dev)
    out = env.critical_path(dc, None, bt[PAD:PAD + n * T].view(n, T), ba[PAD:PAD + n * T].view(n, T), bl[PAD:PAD + n])
    torch.cuda.synchronize(dev)
    for whole, m in ((bt, n * T), (ba, n * T), (bl, n)):
        h = whole.cpu().numpy()
        assert (h[:PAD] == SENT).all() and (h[PAD + m:] == SENT).all(), "a store left the output array"
    return tuple(x.cpu().numpy() for x in out)


# every shape on its variants; J28M64 (2 x 1792 replayed steps a case) without the generated one, whose times never tie
INPUTS = [(shape, variant) for shape in ref.SHAPES for variant in ("generated", "grid") + (("coarse",) if shape in ref.COARSE else ())
          if (shape, variant) != ("J28M64", "generated")]
# what the kernel's launch depends on, per shape: bytes of LDS (above 48 KiB the launch asks for them first) and passes of 64 tasks
LAUNCH = {"J3M4": (448, 1), "J6M6": (1120, 1), "J8M8": (1904, 1), "J10M10": (2912, 2), "J16M8": (3696, 2), "J43M3": (3696, 3), "J65M2": (3696, 3),
          "J10M20": (5712, 4), "J28M64": (50288, 28)}


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape,variant", INPUTS, ids=[f"{s}-{v}" for s, v in INPUTS])
def test_paths_equal_the_model(shape, variant, left_shift):
    (J, M, E, N), variants, (task, mach) = ref.shape_inputs(shape)
    data, T = variants[variant], J * M
    assert (ref.crit_lds_bytes(T), (T + 63) // 64) == LAUNCH[shape]
    env = _open(shape, data, left_shift)
    if shape == "J28M64":                                               # M = 64: the copies step two to a workgroup
        assert ref.crit_lds_bytes(T) > 48 * 1024 and (env.step_kernel_name(), env.step_launch_info()[0]) == ("k_env_step_grp", 2)
    try:
        dt, dm = (torch.as_tensor(np.ascontiguousarray(x.T), device=env.device) for x in (task, mach))     # [T,N]: row s = step s
        pt, pa, pl = _paths(env)
        assert (pl == 0).all() and (pt == -1).all() and (pa == -1).all(), "a freshly reset handle: empty paths"
        done = 0
        for stop in ref.stops(T):
            for s in range(done, stop):
                env.step(dt[s], dm[s])
            done = stop
            state = _state(env)
            assert ((state["mach"] >= 0).sum(1) == stop).all(), "every action was accepted"
            tag = f"{shape} {variant} left_shift={left_shift} after {stop} steps"
            exp = ref.path_rows(state, data[2], J, M)
            got = _paths(env)
            _same(got[2], exp[2], tag + ": path_len"); _same(got[0], exp[0], tag + ": path_task"); _same(got[1], exp[1], tag + ": path_arc")
            # the oracle's schedule gives the same path: the device state is the oracle's
            orc = ref.path_rows(ref.replay(data, task, mach, left_shift, ref.CONFIG_W, stop)[4], data[2], J, M)
            _same(got[0], orc[0], tag + ": path_task against the oracle's schedule")
        # col: a permutation, repeats, -1 and `batch`; fewer and more rows than instances
        rs = np.random.RandomState(3)
        for col in (rs.permutation(N), [N - 1] * 3 + [0, 0], [1, -1, 0, N, 2, -5, N + 7], [2]):
            exp = ref.path_rows(state, data[2], J, M, col)
            got = _paths(env, col)
            tag = f"{shape} {variant} col={list(col)}"
            _same(got[2], exp[2], tag + ": path_len"); _same(got[0], exp[0], tag + ": path_task"); _same(got[1], exp[1], tag + ": path_arc")
            for i, c in enumerate(col):
                if not 0 <= c < N:
                    assert got[2][i] == 0 and (got[0][i] == -1).all() and (got[1][i] == -1).all(), "a column outside the batch: an empty row"
    finally:
        env.close()


def test_errors_write_nothing():
    be, capi = _mods()
    (J, M, E, N), variants, (task, mach) = ref.shape_inputs("J6M6")
    env = _open("J6M6", variants["generated"], False)
    fresh = be.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    try:
        L, T, dev = env.L, env.T, env.device
        bt = torch.full((N * T,), SENT, dtype=torch.int32, device=dev)
        ba = torch.full((N * T,), SENT, dtype=torch.int8, device=dev)
        bl = torch.full((N,), SENT, dtype=torch.int32, device=dev)
        col = torch.arange(N, dtype=torch.int32, device=dev)
        P = lambda x: C.c_void_p(None if x is None else x.data_ptr())      # noqa: E731

        def call(handle=None, n=N, c=col, t=bt, a=ba, ln=bl):
            return L.mtfjsp_critical_path(env.h if handle is None else handle, n, P(c), P(t), P(a), P(ln))

        cases = {"path_task null": dict(t=None), "path_arc null": dict(a=None), "path_len null": dict(ln=None), "n = 0": dict(n=0), "n = -1": dict(n=-1),
                 "col null, n < batch": dict(c=None, n=N - 1), "col null, n > batch": dict(c=None, n=N + 1)}
        for tag, kw in cases.items():
            assert call(**kw) == capi.ERR_ARG, tag
            assert b"mtfjsp_critical_path" in L.mtfjsp_last_error(env.h)
        assert L.mtfjsp_critical_path(None, N, P(col), P(bt), P(ba), P(bl)) == capi.ERR_ARG
        fresh.load_instances(*variants["generated"][:3], edge=variants["generated"][3])
        assert call(handle=fresh.h) == capi.ERR_STATE, "a handle that was never reset"
        assert b"mtfjsp_critical_path" in L.mtfjsp_last_error(fresh.h)
        torch.cuda.synchronize(dev)
        for whole in (bt, ba, bl):
            assert (whole.cpu().numpy() == SENT).all(), "an error return wrote to an output"
        assert call() == capi.OK and call(c=None) == capi.OK and call(n=2) == capi.OK
        torch.cuda.synchronize(dev)
        assert (bl.cpu().numpy() == 0).all() and (bt.cpu().numpy() == -1).all() and (ba.cpu().numpy() == -1).all(), "reset, no step: empty paths"
    finally:
        fresh.close()
        env.close()
