"""GPU: the device's one-step look-ahead (mtfjsp_lookahead_expand / the ordinary step / mtfjsp_lookahead_select,
baselines.Lookahead and lookahead_baselines) EQUALS the host model of tests/lookahead_ref.py — the same (task, machine) at every step
of the episode and the winning value bit for bit, for all five columns; no tolerance.  J9M8 has more than 64 copies per instance
(the strided pass of the selection).  Where no episode's model reaches — ties across passes, NaN, -inf, both zeros, T a multiple of
64, J > 64, M = 64 — the selection runs on synthetic children against `lookahead_ref.select`; J5M12 also runs over the other bands of
the LDS step kernel (groups of 4 and 2, one instance per workgroup, a ragged last workgroup), and J65M2 at four prefix lengths."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import lookahead_ref as ref
from env_parity import _same

pytestmark = pytest.mark.gpu

SHAPES = {"J3M4": (3, 4, 2, 7), "J6M6": (6, 6, 2, 5), "J5M12": (5, 12, 2, 2), "J9M8": (9, 8, 2, 2)}
RAGGED = {"J5M13": (5, 13, 1, 1)}      # B*T = 65 copies: no multiple of a group of 4
SENT, PAD = -77, 64


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.baselines"),
            import_module("e2e-mappo-for-mt-fjsp_amd.capi"))


@pytest.mark.parametrize("column", range(5))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_decision_of_the_episode_equals_the_model(shape, column):
    _every_decision(shape, column, "generated")


@pytest.mark.parametrize("column", range(5))
def test_every_decision_on_integer_times_equals_the_model(column):
    """J6M6 x 5 with small-integer times (env_parity.integer_data), left shift on: many candidates promise the same value, and the
    selection has to break the tie as the model does — the lowest index.  The forked copies also take the insertion paths on exact
    ties.  Against the host model, as above; there is no reference fixture for this case"""
    _every_decision("J6M6", column, "integer")
    J, M, E, B = SHAPES["J6M6"]
    assert ref.SHARED_MAXIMA[(J, M, E, B, column, True, "integer")] >= B, "the model's maxima must be shared ones"


def _launches(env, kernel, G):
    """the live handle's own answer, with the switches as they are now: the step kernel and its instances per workgroup"""
    assert (env.step_kernel_name(), env.step_launch_info()[0]) == (kernel, G), (env.step_kernel_name(), env.step_launch_info())


def _every_decision(shape, column, data, launch=None, decide=None):
    """launch: (kernel, instances per workgroup) both handles must report.  decide: the steps at which the device decides and is
    compared (None: all); at the others the source just takes the model's action"""
    batch_env, baselines, capi = _mods()
    J, M, E, B = SHAPES[shape] if shape in SHAPES else RAGGED[shape]
    T = J * M
    (t, p, tt, edge, w3), task, mach, best = ref.cached_episode(J, M, E, B, column, True, data)
    env = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=True, obs_dtype="f32", w_cfg=ref.CONFIG_W)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(w3)
    la = baselines.Lookahead(env)
    if launch:
        _launches(env, *launch); _launches(la.scratch, *launch)
    for s in range(T):
        if decide is not None and s not in decide:
            env.step(torch.as_tensor(task[s].copy(), device=env.device), torch.as_tensor(mach[s].copy(), device=env.device))
            continue
        a, m = la.decide(column)
        tag = f"{shape} column {column} step {s}"
        _same(a.cpu().numpy(), task[s], tag + " task"); _same(m.cpu().numpy(), mach[s], tag + " machine")
        _same(la.job.cpu().numpy(), task[s] // M, tag + " job")
        _same(la.best.cpu().numpy().view(np.int64), best[s].view(np.int64), tag + " best value (bits)")
        env.step(a, m)
        assert not (env.status.cpu().numpy() & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any(), tag
        _same(env.raw.cpu().numpy()[:, column], best[s], tag + " the source's step yields the value the copy promised")
    assert bool(env.info[:, 1].all().item())
    la.close(); env.close()


@pytest.mark.parametrize("column", [0, 2])
def test_a_finished_instance_beside_running_ones(column):
    batch_env, baselines, capi = _mods()
    J, M, E, B = SHAPES["J3M4"]
    T = J * M
    (t, p, tt, edge, w3), task, mach, best = ref.cached_episode(J, M, E, B, column, True)
    env = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=True, obs_dtype="f64", w_cfg=ref.CONFIG_W)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(w3)
    # instance 2 alone plays the model's whole episode: the others get task -1, which the step rejects and leaves untouched
    only = np.arange(B) == 2
    for s in range(T):
        a = torch.as_tensor(np.where(only, task[s], -1).astype(np.int32), device=env.device)
        m = torch.as_tensor(np.where(only, mach[s], 0).astype(np.int32), device=env.device)
        env.step(a, m)
    assert env.info.cpu().numpy()[2, 1] == 1.0
    la = baselines.Lookahead(env)
    a, m = la.decide(column)
    a, m, j, b = a.cpu().numpy(), m.cpu().numpy(), la.job.cpu().numpy(), la.best.cpu().numpy()
    assert a[2] == -1 and m[2] == -1 and j[2] == -1 and np.isnan(b[2])
    _same(a[~only], task[0][~only], "running instances: task"); _same(m[~only], mach[0][~only], "running instances: machine")
    _same(b[~only].view(np.int64), best[0][~only].view(np.int64), "running instances: best value (bits)")
    la.close(); env.close()


@pytest.mark.parametrize("left_shift", [True, False], ids=["left_shift", "no_left_shift"])
def test_lookahead_baselines_equal_the_oracle_driven_by_the_models_plans(left_shift):
    from oracle.env_oracle import OracleBatch
    _, baselines, _ = _mods()
    J, M, E, B = SHAPES["J6M6"]
    T = J * M
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=ref.CONFIG_W[0], weight_ec=ref.CONFIG_W[1], weight_tt=ref.CONFIG_W[2])
    data = ref.cached_episode(J, M, E, B, 0, left_shift)[0]
    t, p, tt, edge, w3 = data
    res = baselines.lookahead_baselines(t, p, tt, edge, args, left_shift=left_shift)
    assert sorted(res) == sorted([r[0] for r in baselines.LOOKAHEAD_RULES] + [baselines.PLANS])
    for name, column in baselines.LOOKAHEAD_RULES:
        _, task, mach, _ = ref.cached_episode(J, M, E, B, column, left_shift)
        _same(res[baselines.PLANS][name][0], np.ascontiguousarray(task.T), f"{name} plan: tasks")
        _same(res[baselines.PLANS][name][1], np.ascontiguousarray(mach.T), f"{name} plan: machines")
        orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(w3)
        cum = np.zeros((B, 5))
        for s in range(T):
            cum += orc.step(task[s], mach[s])[1]
        prev = orc.state()["prev"]
        cost, final4, obj = res[name]
        for k, key in enumerate(("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")):
            _same(cost[key], cum[:, k], f"{name} {key}")
        _same(final4, np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1), f"{name} Final_4cost")


def test_the_scratch_handle_inherits_reward_weights_off_the_default():
    """LA_R (raw[0], the weighted total) with the configuration's weights at (0.55, 0.15, 0.30), divisor 1 (the host model takes
    none), on the smallest shape of this file: the B*T copies are stepped by the SCRATCH handle, which must have taken its source's
    weights (baselines.Lookahead) — with the default (0.4, 0.4, 0.2) its totals, and with them the plan, are others"""
    from oracle.env_oracle import OracleBatch
    _, baselines, _ = _mods()
    J, M, E, B = SHAPES["J3M4"]
    T, W_A, left_shift = J * M, (0.55, 0.15, 0.30), True
    assert min(v[0] * v[1] for v in SHAPES.values()) == T
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=W_A[0], weight_ec=W_A[1], weight_tt=W_A[2])
    (t, p, tt, edge, w3), task, mach, best = ref.cached_episode(J, M, E, B, 0, left_shift, w_cfg=W_A)
    _same(w3, np.tile(np.array([W_A]), (B, 1)), "the model's weights")
    default = ref.cached_episode(J, M, E, B, 0, left_shift)
    assert not (np.array_equal(default[1], task) and np.array_equal(default[2], mach)), "the weights must change the model's plan"
    res = baselines.lookahead_baselines(t, p, tt, edge, args, rules=[("LA_R", 0)], left_shift=left_shift)
    _same(res[baselines.PLANS]["LA_R"][0], np.ascontiguousarray(task.T), "LA_R plan: tasks")
    _same(res[baselines.PLANS]["LA_R"][1], np.ascontiguousarray(mach.T), "LA_R plan: machines")
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=W_A); orc.scaler_init(); orc.reset(w3)
    cum = np.zeros((B, 5))
    for s in range(T):
        raw = orc.step(task[s], mach[s])[1]
        _same(raw[:, 0].view(np.int64), best[s].view(np.int64), f"step {s}: the model's promised value (bits)")
        cum += raw
    prev = orc.state()["prev"]
    cost, final4, obj = res["LA_R"]
    for k, key in enumerate(("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")):
        _same(cost[key], cum[:, k], f"LA_R {key}")
    want4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
    _same(final4, want4, "LA_R Final_4cost")
    _same(obj, W_A[0] * want4[:, 0] + W_A[1] * (want4[:, 1] + want4[:, 3]) + W_A[2] * want4[:, 2], "LA_R Objective")


# ---- the other bands of the LDS step kernel (J5M12 takes groups of 8 by default) and J > 64
BANDS = [("MTFJSP_ENV_STEP_G", "4", "k_env_step_grp", 4), ("MTFJSP_ENV_STEP_G", "2", "k_env_step_grp", 2), ("MTFJSP_ENV_KERNEL", "lds1", "k_env_step", 1)]


def _switch(monkeypatch, var, value):
    from env_parity import _SELECTION_VARS
    for k in _SELECTION_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(var, value)


@pytest.mark.parametrize("column", [0, 2])
@pytest.mark.parametrize("var,value,kernel,G", BANDS, ids=["G4", "G2", "lds1"])
def test_every_decision_over_the_other_step_kernel_bands(monkeypatch, var, value, kernel, G, column):
    """the source (B = 2) and the scratch handle (B*T = 120, a multiple of 4 and of 2) both step with the forced band"""
    _switch(monkeypatch, var, value)
    _every_decision("J5M12", column, "generated", launch=(kernel, G))


@pytest.mark.parametrize("column", [0, 2])
def test_decisions_with_a_ragged_last_workgroup(monkeypatch, column):
    """J5M13 x 1 in groups of 4: 65 copies, the last workgroup steps one.  The first 8 and the last 4 decisions of the model's episode"""
    _switch(monkeypatch, "MTFJSP_ENV_STEP_G", "4")
    J, M, E, B = RAGGED["J5M13"]
    assert (B * J * M) % 4 == 1
    _every_decision("J5M13", column, "generated", launch=("k_env_step_grp", 4), decide=set(range(8)) | set(range(J * M - 4, J * M)))


def test_more_jobs_than_lanes_at_four_prefix_lengths():
    """J65M2 x 2 under the default dispatch: job records walk more than one job a lane, T = 130 is a ragged third pass of the selection.
    The prefix is a random plan (tests/plan_moves_ref.py), not the model's own episode; decisions after 0, 1, 65 and 129 steps, all
    five columns, against lookahead_ref.model_step on that prefix"""
    import plan_moves_ref as pref
    batch_env, baselines, capi = _mods()
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, B = 65, 2, 1, 2
    T = J * M
    t, p, tt, edge = inst.generate_instances(B, J, M, E, seed=4200 + J * 100 + M)
    w3 = np.tile(np.array([ref.CONFIG_W]), (B, 1))
    task, mach = pref.random_plans(np.asarray(t), J, M, 23)              # [B,T]
    env = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=True, obs_dtype="f32", w_cfg=ref.CONFIG_W)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(w3)
    la = baselines.Lookahead(env)
    assert env.step_kernel_name() == "k_env_step_grp" and la.scratch.step_kernel_name() == "k_env_step_grp"
    done = 0
    for stop in (0, 1, 65, 129):
        for s in range(done, stop):
            env.step(torch.as_tensor(np.ascontiguousarray(task[:, s]), device=env.device), torch.as_tensor(np.ascontiguousarray(mach[:, s]), device=env.device))
            assert not (env.status.cpu().numpy() & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any(), f"prefix step {s}"
        done = stop
        prefix = [(task[:, s], mach[:, s]) for s in range(stop)]
        for column in range(5):
            ea, em, eb, _, valid = ref.model_step(t, p, tt, edge, w3, prefix, column)
            a, m = la.decide(column)
            tag = f"J65M2 after {stop} steps, column {column}"
            _same(a.cpu().numpy(), ea, tag + " task"); _same(m.cpu().numpy(), em, tag + " machine"); _same(la.job.cpu().numpy(), ea // M, tag + " job")
            _same(la.best.cpu().numpy().view(np.int64), eb.view(np.int64), tag + " best value (bits)")
        assert valid.any(1).all()
    la.close(); env.close()


# ---- the selection alone, on synthetic children
SYNTHETIC = [(9, 8, 2, 6), (16, 8, 2, 6), (65, 2, 1, 6), (16, 16, 2, 6), (4, 64, 2, 6)]        # T = 72, 128, 130, 256, 256 (M = 64)
BAD = 0x300                                                             # MTFJSP_ST_INVALID | MTFJSP_ST_INFEASIBLE


def _synthetic_rows(T, rng):
    """-> (status [6,T] int32, values [6,T,5]): the six constructed instances (a) .. (f) of the test below, every column built anew on
    the instance's status words"""
    P, NEG = (T + 63) // 64, -0.375
    last = rng.randint(64 * (P - 1), T)                                  # an index of the last pass
    small = lambda n: rng.randint(-6, 7, n).astype(np.float64) * 0.375  # noqa: E731
    status, values = np.zeros((6, T), np.int32), np.zeros((6, T, 5))
    for k in range(6):
        st = np.where(rng.rand(T) < 0.3, 0x100, 0) | np.where(rng.rand(T) < 0.2, 0x200, 0) | rng.randint(0, 8, T)
        if k == 1:
            st[T - 1] &= ~BAD
        if k == 2:
            st[[0, 64, last]] &= ~BAD
        if k == 3:
            st[0] |= 0x100; st[rng.randint(1, 64)] &= ~BAD; st[T - 2] &= ~BAD
        if k == 4:
            st |= np.where(rng.rand(T) < 0.5, 0x100, 0x200)
        if k == 5:
            st[[5, 9, 64 + 3, T - 1]] &= ~BAD; st[[0, 2, 66]] |= 0x200
        ok = (st & BAD) == 0
        for col in range(5):
            v = small(T)
            if k == 1:                                                  # (b) the maximum at the last copy alone
                v[T - 1] = 7 * 0.375
            if k == 2:                                                  # (c) the maximum at copy 0, at copy 64 and in the last pass
                v[[0, 64, last]] = 7 * 0.375
            if k == 3:                                                  # (d) every counting copy -inf; copy 0 does not count
                v[ok] = -np.inf
            if k == 5:                                                  # (f) the largest counting value is a zero: one sign first, the other in a later pass
                v = -np.abs(v) + NEG
                lo, hi = (-0.0, 0.0) if col % 2 == 0 else (0.0, -0.0)   # columns 1 and 3: the other way round
                v[5], v[64 + 3], v[T - 1] = lo, hi, hi
                v[9] = hi                                               # and one in the first zero's own pass: the wave maximum of that pass is either zero
                v[[0, 66]] = np.inf                                     # copies that do not count
                v[2] = np.nan
                v[np.flatnonzero(ok & (v < 0))[[0, -1]]] = np.nan       # NaN in counting copies: never selected
            values[k, :, col] = v
        status[k] = st
    return status, values


def _synthetic_case(J, M):
    """-> (status, values, picks [6][5]: lookahead_ref.select's answers); asserts on the host that every instance has its property"""
    T, P = J * M, (J * M + 63) // 64
    assert T > 64
    status, values = _synthetic_rows(T, np.random.RandomState(100 * J + M))
    ok = (status & BAD) == 0
    picks = [[ref.select(values[k, :, col], ok[k]) for col in range(5)] for k in range(6)]
    for col in range(5):
        v = values[:, :, col]
        at_max = lambda k: np.flatnonzero(ok[k] & (v[k] == v[k, picks[k][col]]))       # noqa: E731
        assert ok[0].any() and 0 < (~ok[0]).sum() and len(np.unique(v[0])) <= 13, "(a) few distinct values, some copies do not count"
        assert picks[1][col] == T - 1 and len(at_max(1)) == 1, "(b) the last copy alone holds the maximum"
        assert picks[2][col] == 0 and len(at_max(2)) >= 3 and {0, 64} <= set(at_max(2).tolist()), "(c) copy 0 shares its maximum with copy 64 ..."
        assert len(set((at_max(2) // 64).tolist())) >= min(3, P) and (at_max(2) // 64).max() == P - 1, "(c) ... and with the last pass"
        assert not ok[3, 0] and np.isfinite(v[3, 0]) and ok[3].sum() >= 2 and (v[3][ok[3]] == -np.inf).all(), "(d) only -inf counts, copy 0 does not"
        assert picks[3][col] == np.flatnonzero(ok[3])[0] > 0 and np.flatnonzero(ok[3])[-1] >= 64
        assert not ok[4].any() and picks[4][col] is None, "(e) nothing counts"
        c, z = picks[5][col], at_max(5)
        assert c == 5 and v[5, c] == 0 and len(z) >= 3 and z[1] < 64 <= z[2], "(f) the maximum is a zero, shared within its pass and with a later pass"
        assert np.signbit(v[5, c]) == (col % 2 == 0) and (np.signbit(v[5, z[1:]]) != np.signbit(v[5, c])).all(), "(f) the later zeros have the other sign"
        assert np.isnan(v[5][ok[5]]).sum() >= 2 and np.isinf(v[5][~ok[5]]).sum() >= 2 and not np.isinf(v[5][ok[5]]).any(), "(f) NaN counting, +inf not counting"
    return status, values, picks


@pytest.mark.parametrize("J,M,E,B", SYNTHETIC, ids=[f"J{s[0]}M{s[1]}" for s in SYNTHETIC])
def test_selection_on_synthetic_children(J, M, E, B):
    """k_lookahead_select<false> where no episode's model is affordable or no episode asks: status words and raw values are written
    straight into the scratch handle's bound buffers, and lookahead_ref.select is applied to the same arrays.  Six constructed
    instances per shape (random with ties; the maximum at the last copy; the maximum shared across passes; only -inf counting; nothing
    counting; zeros of both signs with NaN and +inf around them), all five columns; the source is freshly reset, so job j's candidate
    is task j * M"""
    batch_env, baselines, capi = _mods()
    assert (capi.ST_INVALID | capi.ST_INFEASIBLE) == BAD and B == 6
    T = J * M
    status, values, picks = _synthetic_case(J, M)
    bits = lambda x: np.asarray(x, np.float64).view(np.int64)           # noqa: E731
    mk = lambda b: batch_env.DeviceBatchEnv(J, M, E, b, left_shift=False, obs_dtype="f32", w_cfg=ref.CONFIG_W)      # noqa: E731
    src, scratch = mk(B), mk(B * T)
    try:
        for e in (src, scratch):
            e.generate_instances(3); e.scaler_init()
            e.reset(torch.tensor([ref.CONFIG_W], dtype=torch.float64, device=e.device).repeat(e.B, 1))
        dev = src.device
        cand = src.candidate.cpu().numpy()                              # job j's next task: j * M + min(cnt_j, M - 1)
        _same(cand.astype(np.int64), np.tile(np.arange(J) * M, (B, 1)), "fresh after reset: every job's candidate is its first task")
        scratch.raw.copy_(torch.as_tensor(values.reshape(B * T, 5), device=dev))
        scratch.status.copy_(torch.as_tensor(status.reshape(B * T), device=dev))
        for col in range(5):
            ints = [torch.full((B + 2 * PAD,), SENT, dtype=torch.int32, device=dev) for _ in range(3)]
            out = torch.full((B + 2 * PAD,), float(SENT), dtype=torch.float64, device=dev)
            capi.check(src.L.mtfjsp_lookahead_select(scratch.h, src.h, col, *[C.c_void_p(x[PAD:].data_ptr()) for x in ints + [out]]), scratch.h)
            torch.cuda.synchronize(dev)
            for x in ints + [out]:
                h = x.cpu().numpy()
                assert (h[:PAD] == SENT).all() and (h[PAD + B:] == SENT).all(), "a store left the output array"
            task, mach, job = (x[PAD:PAD + B].cpu().numpy() for x in ints)
            best = out[PAD:PAD + B].cpu().numpy()
            for k in range(B):
                tag, c = f"J{J}M{M} instance {'abcdef'[k]} column {col}", picks[k][col]
                if c is None:
                    assert (task[k], mach[k], job[k]) == (-1, -1, -1) and np.isnan(best[k]), f"{tag}: {(task[k], mach[k], job[k], best[k])}"
                    continue
                assert (task[k], mach[k], job[k]) == (cand[k, c // M], c % M, c // M), f"{tag}: {(task[k], mach[k], job[k])}, picked copy {c}"
                assert bits(best[k]) == bits(values[k, c, col]), f"{tag}: best {best[k]!r}, the picked copy {c} holds {values[k, c, col]!r}"
        _same(scratch.raw.cpu().numpy().view(np.int64), values.reshape(B * T, 5).view(np.int64), "the children are only read")
    finally:
        scratch.close(); src.close()
