"""GPU: DeviceBatchEnv.replay_plans — plans evaluated in one launch (mtfjsp_replay_plans) — EQUALS, bit for bit, what reset, T steps and
final_costs leave on a second handle of the same instances (final costs, done, and with state=True the schedule: machine, start, finish,
routes, state signature, critical path of every copy), and the C oracle's replay.  15 copies = 3 instances x 5 (a ragged last
workgroup), at J3M4, J6M6, J5M13 (one task past a wave), J9M15 (beyond one pairwise leaf block, with a ragged tail) and J65M2 (more
jobs than lanes); left shift on and off; generated times with random plans and the small-integer times of env_parity.integer_data (exact
ties, zero transport between different machines) with the oracle walk's "blocks" plans, whose path words are asserted to reach the
empty route, the front, a gap and the append.  Spoiled plans, zero durations (a finish time of 0.0 with a successor), strided and
offset plan buffers, refused arguments, the state guard and repeatability have a test each.  No tolerance anywhere."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import env_parity
import plan_moves_ref as pref
import replay_ref as ref

pytestmark = pytest.mark.gpu

N, C = ref.N_INST, ref.N_COPY
B = N * C
W = ref.CONFIG_W
SEED = 3
FIELDS = ("machine", "start", "finish", "routes")


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _same(got, exp, tag):
    got, exp = _bits(got), _bits(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, f"{tag}: {got.shape} {got.dtype} against {exp.shape} {exp.dtype}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{tag}: {len(bad)} of {exp.size} differ, first at {bad[0].tolist()}")


def _rep(x):
    return np.repeat(np.asarray(x), C, axis=0)


@functools.lru_cache(maxsize=None)
def _case(shape, data, left_shift):
    """-> dict(J, M, E, inst: (t, p, tt, edge) of the 15 columns, task, mach [15,T] int32, paths or None): copy c of instance n = column n*C + c"""
    J, M, E = ref.SHAPES[shape]
    t, p, tt, edge = env_parity.parity_instances(J, M, E, N, SEED, data)
    inst = (_rep(t), _rep(p), _rep(tt), _rep(edge))
    if data == "integer":                                               # five episodes of the oracle's walk = five plans per instance
        w = env_parity.oracle_walk(J, M, E, N, left_shift=left_shift, episodes=C, seed=SEED, policy="blocks", data="integer")
        act = w["actions"]                                              # [C,T,N,3]
        task = np.ascontiguousarray(act[:, :, :, 1].transpose(2, 0, 1).reshape(B, J * M))
        mach = np.ascontiguousarray(act[:, :, :, 2].transpose(2, 0, 1).reshape(B, J * M))
        paths = w["paths"]
    else:
        task, mach = pref.random_plans(inst[0], J, M, SEED + J)
        paths = None
    return dict(J=J, M=M, E=E, inst=inst, task=task.astype(np.int32), mach=mach.astype(np.int32), paths=paths)


def _handle(case, left_shift, inst=None):
    be, _ = _mods()
    env = be.DeviceBatchEnv(case["J"], case["M"], case["E"], B, left_shift=left_shift, obs_dtype="f32", w_cfg=W)
    t, p, tt, edge = case["inst"] if inst is None else inst
    env.load_instances(t, p, tt, edge=edge)
    return env


def _dev(env, x):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x).T), device=env.device)          # [T,B]: row s = the actions of step s


def _schedule(env):
    """everything the searches read of a handle that holds schedules"""
    _, capi = _mods()
    out = {k: env.read_state(getattr(capi, "STATE_" + k.upper())) for k in FIELDS}
    out["sig"] = env.state_signature().cpu().numpy()
    pt, pa, pl = env.critical_path()
    out["path_task"], out["path_arc"], out["path_len"] = pt.cpu().numpy(), pa.cpu().numpy(), pl.cpu().numpy()
    return out


def _by_steps(case, left_shift, task, mach, inst=None):
    env = _handle(case, left_shift, inst)
    try:
        env.scaler_init()
        env.reset(np.tile(np.array([W], np.float64), (B, 1)))
        tk, mc = _dev(env, task), _dev(env, mach)
        for s in range(tk.shape[0]):
            env.step(tk[s], mc[s])
        cost4, done = env.final_costs()
        out = dict(cost4=cost4.cpu().numpy(), done=done.cpu().numpy())
        out.update(_schedule(env))
        return out
    finally:
        env.close()


def _by_launch(case, left_shift, task, mach, state=True, inst=None):
    env = _handle(case, left_shift, inst)
    try:
        cost4, done = env.replay_plans(_dev(env, task), _dev(env, mach), state=state)
        out = dict(cost4=cost4.cpu().numpy(), done=done.cpu().numpy())
        if state:
            out.update(_schedule(env))
        return out
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def _steps(shape, data, left_shift):
    case = _case(shape, data, left_shift)
    return _by_steps(case, left_shift, case["task"], case["mach"])


@functools.lru_cache(maxsize=None)
def _launch(shape, data, left_shift):
    case = _case(shape, data, left_shift)
    return _by_launch(case, left_shift, case["task"], case["mach"])


def _compare(got, exp, tag, keys=None):
    for k in (exp if keys is None else keys):
        _same(got[k], exp[k], f"{tag}: {k}")


CASES = [(s, d, ls) for s in ref.SHAPES for d in env_parity.DATA for ls in (False, True)]
IDS = [f"{s}-{d}-{'ls' if ls else 'nols'}" for s, d, ls in CASES]


@pytest.mark.parametrize("shape,data,left_shift", CASES, ids=IDS)
def test_one_launch_equals_the_step_launches(shape, data, left_shift):
    """(a): final costs, done, and the schedule every search reads"""
    got, exp = _launch(shape, data, left_shift), _steps(shape, data, left_shift)
    assert exp["done"].all(), "every plan of these cases is valid"
    _compare(got, exp, f"{shape} {data} left_shift={left_shift}")


@pytest.mark.parametrize("shape,data,left_shift", CASES, ids=IDS)
def test_one_launch_equals_the_oracle(shape, data, left_shift):
    """(b): Final_4cost of the C oracle's replay"""
    case = _case(shape, data, left_shift)
    _, final4, done, _ = pref.replay(case["inst"], case["task"], case["mach"], left_shift, W)
    got = _launch(shape, data, left_shift)
    _same(got["done"], done.astype(np.uint8), f"{shape} {data}: done")
    _same(got["cost4"], final4, f"{shape} {data} left_shift={left_shift}: cost4 (bits)")


@pytest.mark.parametrize("shape", ["J3M4", "J6M6", "J5M13", "J9M15"])
def test_the_integer_walks_reach_every_scheduling_path(shape):
    """what the left-shift cases above are worth: the oracle's own path words hold EMPTY, FRONT, BETWEEN and APPEND"""
    paths = _case(shape, "integer", True)["paths"]
    assert {0, 1, 2, 3} <= set(np.unique(paths).tolist()), np.bincount(paths.ravel(), minlength=4)


@pytest.mark.parametrize("shape", ["J6M6", "J5M13"])
def test_spoiled_plans(shape):
    """(c): a task out of range at step 0, a task twice, a job's second operation before its first — rejected, the copy never done — and
    a machine with t < 0, scheduled like any duration; the other 11 copies must be done"""
    case = _case(shape, "generated", True)
    task, mach, cols = ref.spoil(case["task"], case["mach"], case["inst"][0], case["M"])
    exp = _by_steps(case, True, task, mach)
    got = _by_launch(case, True, task, mach)
    plain = _by_launch(case, True, task, mach, state=False)
    _same(got["done"], exp["done"], shape + ": done")
    assert got["done"][[c for c in range(B) if c not in cols]].all(), "the untouched copies must be done"
    assert not got["done"][list(cols[:3])].any() and got["done"][cols[3]] == 1, got["done"]
    nan = np.isnan(got["cost4"])
    assert (nan == (got["done"] == 0)[:, None]).all(), "four NaNs exactly where the copy is not done"
    _same(got["cost4"][got["done"] == 1], exp["cost4"][exp["done"] == 1], shape + ": cost4 of the done copies (bits)")
    _compare(got, exp, shape + " spoiled, partial schedules", [k for k in exp if k not in ("cost4", "done")])
    _same(plain["done"], got["done"], shape + ": done without state")
    _same(plain["cost4"], got["cost4"], shape + ": cost4 without state (bits, NaNs included)")


@pytest.mark.parametrize("left_shift", [False, True], ids=["nols", "ls"])
def test_zero_durations(left_shift):
    """(d): the first operations of two jobs take no time and nothing travels: a scheduled operation finishes at 0.0 and has a successor
    — the step kernel's chain of estimated finishes counts such a finish as none (`ft != 0.0`)"""
    case = dict(_case("J3M4", "generated", left_shift))
    t, p, tt, edge = (x.copy() for x in case["inst"])
    M = case["M"]
    t[:, 0, :] = 0.0; t[:, M, :] = 0.0; tt[:] = 0.0
    inst = (t, p, tt, edge)
    task, mach = pref.random_plans(t, case["J"], M, SEED + 40)
    from oracle.env_oracle import OracleBatch
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=W)
    orc.scaler_init()
    orc.reset(np.tile(np.array([W], np.float64), (B, 1)))
    for s in range(task.shape[1]):
        orc.step(task[:, s], mach[:, s])
    so = orc.state()
    assert ((so["ft"] == 0.0) & (so["sched"] != 0)).any(), "a scheduled task must finish at 0.0"
    _, final4, done, _ = pref.replay(inst, task, mach, left_shift, W)
    exp = _by_steps(case, left_shift, task, mach, inst)
    got = _by_launch(case, left_shift, task, mach, inst=inst)
    assert done.all() and exp["done"].all()
    _compare(got, exp, f"zero durations left_shift={left_shift}")
    _same(got["cost4"], final4, "zero durations: cost4 against the oracle (bits)")


def test_a_wider_stride_and_a_column_offset():
    """(e): the plans as columns 4..18 of [T, 24] buffers — the search's own buffers are views like this"""
    case, exp = _case("J6M6", "generated", True), _launch("J6M6", "generated", True)
    env = _handle(case, True)
    try:
        tk, mc = _dev(env, case["task"]), _dev(env, case["mach"])
        wide_t = torch.full((tk.shape[0], B + 9), -7, dtype=torch.int32, device=env.device)
        wide_m = torch.full_like(wide_t, 99)
        wide_t[:, 4:4 + B] = tk; wide_m[:, 4:4 + B] = mc
        vt, vm = wide_t[:, 4:4 + B], wide_m[:, 4:4 + B]
        assert vt.stride(0) == B + 9 and vt.data_ptr() != wide_t.data_ptr()
        cost4, done = env.replay_plans(vt, vm, state=True)
        _same(cost4.cpu().numpy(), exp["cost4"], "offset view: cost4 (bits)"); _same(done.cpu().numpy(), exp["done"], "offset view: done")
        _compare(_schedule(env), exp, "offset view", [k for k in exp if k not in ("cost4", "done")])
        assert (wide_t[:, :4] == -7).all() and (wide_t[:, 4 + B:] == -7).all() and (wide_m[:, :4] == 99).all()
    finally:
        env.close()


def test_refused_arguments():
    """(f): an output inside the plans, a null argument, a stride below the batch, another flag bit: MTFJSP_ERR_ARG"""
    _, capi = _mods()
    case = _case("J3M4", "generated", True)
    env = _handle(case, True)
    try:
        T = case["task"].shape[1]
        tk, mc = _dev(env, case["task"]), _dev(env, case["mach"])
        both = torch.zeros(T * B, dtype=torch.float64, device=env.device)       # its first half viewed as the int32 task plan
        alias_t = both.view(torch.int32)[:T * B].view(T, B)
        alias_t.copy_(tk)
        alias_c4 = both[:B * 4].view(B, 4)
        with pytest.raises(capi.MtfjspError) as e:
            env.replay_plans(alias_t, mc, cost4=alias_c4)
        assert e.value.code == capi.ERR_ARG and "overlap" in str(e.value)
        c4, dn = torch.empty(B, 4, dtype=torch.float64, device=env.device), torch.empty(B, dtype=torch.uint8, device=env.device)
        L, h = env.L, env.h
        for args in ((None, mc.data_ptr(), B, c4.data_ptr(), dn.data_ptr(), 0), (tk.data_ptr(), None, B, c4.data_ptr(), dn.data_ptr(), 0),
                     (tk.data_ptr(), mc.data_ptr(), B, None, dn.data_ptr(), 0), (tk.data_ptr(), mc.data_ptr(), B, c4.data_ptr(), None, 0),
                     (tk.data_ptr(), mc.data_ptr(), B - 1, c4.data_ptr(), dn.data_ptr(), 0), (tk.data_ptr(), mc.data_ptr(), B, c4.data_ptr(), dn.data_ptr(), 2)):
            assert L.mtfjsp_replay_plans(h, *args) == capi.ERR_ARG, args
        fresh = _mods()[0].DeviceBatchEnv(case["J"], case["M"], case["E"], B)
        try:
            with pytest.raises(capi.MtfjspError) as e:
                fresh.replay_plans(tk, mc)
            assert e.value.code == capi.ERR_STATE
        finally:
            fresh.close()
        env.replay_plans(tk, mc, c4, dn)                                        # the handle is still good
        _same(c4.cpu().numpy(), _launch("J3M4", "generated", True)["cost4"], "after the refusals: cost4 (bits)")
    finally:
        env.close()


def test_the_replayed_state_guards_and_a_reset_clears_it():
    """(g)"""
    be, capi = _mods()
    case = _case("J6M6", "generated", True)
    env, other = _handle(case, True), _handle(case, True)
    try:
        tk, mc = _dev(env, case["task"]), _dev(env, case["mach"])
        idx = torch.arange(B, dtype=torch.int32, device=env.device)

        def refuses(call):
            with pytest.raises(capi.MtfjspError) as e:
                call()
            assert e.value.code == capi.ERR_STATE, e.value
            assert len(str(e.value)) > len("libmtfjsp error -2: "), "a message"

        def others():
            refuses(lambda: env.step(tk[0], mc[0]))
            refuses(lambda: env.step_record(tk[0], mc[0], torch.empty(4, B, dtype=torch.float32, device=env.device),
                                            torch.empty(B, dtype=torch.float32, device=env.device)))
            refuses(env.final_costs)
            refuses(env.valid_action_mask)
            refuses(lambda: env.read_state(capi.STATE_PREV_COSTS))
            refuses(lambda: other.fork_from(env, idx, instance=False, state=True, obs=True))
            obs = capi.Obs(*[x.data_ptr() for x in (other.tasks_fea, other.ell_col, other.ell_val, other.m_fea2, other.info, other.raw,
                                                      other.candidate, other.job_mask, other.status)])
            import ctypes
            assert env.L.mtfjsp_snapshot_obs(env.h, ctypes.byref(obs)) == capi.ERR_STATE

        env.replay_plans(tk, mc)
        others()
        refuses(env.critical_path)
        refuses(env.state_signature)
        refuses(lambda: env.read_state(capi.STATE_MACHINE))
        env.replay_plans(tk, mc, state=True)
        others()
        _compare(_schedule(env), _steps("J6M6", "generated", True), "replayed with state", [k for k in _schedule(env)])
        # a reset clears it: an ordinary episode then equals the oracle
        env.scaler_init()
        env.reset(np.tile(np.array([W], np.float64), (B, 1)))
        for s in range(tk.shape[0]):
            env.step(tk[s], mc[s])
        cost4, done = env.final_costs()
        _, final4, odone, _ = pref.replay(case["inst"], case["task"], case["mach"], True, W)
        _same(cost4.cpu().numpy(), final4, "after the reset: cost4 against the oracle (bits)")
        _same(done.cpu().numpy(), odone.astype(np.uint8), "after the reset: done")
        assert env.read_state(capi.STATE_PREV_COSTS).shape == (B, 4)
    finally:
        env.close(); other.close()


def test_the_same_call_twice_gives_the_same_bits():
    """(h)"""
    case = _case("J9M15", "integer", True)
    env = _handle(case, True)
    try:
        tk, mc = _dev(env, case["task"]), _dev(env, case["mach"])
        a4, ad = env.replay_plans(tk, mc, state=True)
        first = dict(cost4=a4.cpu().numpy(), done=ad.cpu().numpy(), **_schedule(env))
        b4, bd = env.replay_plans(tk, mc, state=True)
        second = dict(cost4=b4.cpu().numpy(), done=bd.cpu().numpy(), **_schedule(env))
        _compare(second, first, "second call")
        _compare(first, _launch("J9M15", "integer", True), "against the shared run")
    finally:
        env.close()
