"""PARITY (GPU): rejected actions in MIXED batches, every step kernel, float32 and float64 observations, against the batch-1 oracles
of tests/rejected_actions_ref.py after EVERY step.  No tolerance anywhere.

include/mtfjsp.h: a step with a bad action (already scheduled, job predecessor unscheduled, an index out of range) leaves the instance
untouched, sets MTFJSP_ST_INVALID and writes info = [0, done, 0, 0, 0, 0], raw = 0 (r4_out = 0, done_out = done).  The one-step
look-ahead, Parallel_env._step_one and finished instances beside running ones rely on it with rejected and valid instances in the same
workgroup: the wave of a rejected instance returns before the work its group-mates go on to do.  A defect would be a rejected
instance whose scaler words, machine record or feature row moved, a valid group-mate disturbed by the wave that left early, or a wrong
done flag on a finished instance — each shows in the full comparison below, which the schedule (step 0: everyone rejected; one step:
exactly the first workgroup; one step: nobody; otherwise a third of the running instances, all eight kinds; finished instances keep
receiving actions) drives through every kernel of the table.

Before every step info, raw and two record buffers are filled with NaN, and the tasks_fea rows the valid instances must rewrite are
poisoned (tests/env_parity.py); rows of rejected instances are NOT poisoned — they must persist.
"""
from importlib import import_module

import numpy as np
import pytest
import torch

import rejected_actions_ref as ref
from env_parity import _SELECTION_VARS, _same, dispatch_kernel

pytestmark = pytest.mark.gpu


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.baselines"),
            import_module("e2e-mappo-for-mt-fjsp_amd.capi"))


def _same_nan(got, want, what):
    """_same for arrays that carry NaN for "unscheduled" (the NaN pattern must agree, then everything else)"""
    got, want = np.asarray(got), np.asarray(want)
    _same(np.isnan(got), np.isnan(want), what + " (NaN pattern)")
    _same(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want), what)


def _state_arrays(env, capi):
    return {"mach": env.read_state(capi.STATE_MACHINE), "st": env.read_state(capi.STATE_START), "ft": env.read_state(capi.STATE_FINISH),
            "routes": env.read_state(capi.STATE_ROUTES), "prev": env.read_state(capi.STATE_PREV_COSTS),
            "scaler": env.read_state(capi.STATE_SCALER), "w3": env.read_state(capi.STATE_W3)}


def _check(env, exp, odt, capi, tag, outputs=True):
    if outputs:
        _same(env.info.cpu().numpy(), exp.info, tag + " info"); _same(env.raw.cpu().numpy(), exp.raw, tag + " raw")
        st = env.status.cpu().numpy()
        _same(st & capi.PATH_MASK, exp.status & capi.PATH_MASK, tag + " scheduling path")
        _same(st, exp.status, tag + " status (ST_INVALID exactly for a rejected instance, the path alone for a valid one)")
    _same(env.tasks_fea.cpu().numpy(), exp.tfea.astype(odt), tag + " tasks_fea")
    _same(env.m_fea2.cpu().numpy(), exp.mfea2.astype(odt), tag + " m_fea2")
    _same(env.dense_adj().cpu().numpy(), exp.adj, tag + " dense_adj")
    _same(env.candidate.cpu().numpy(), exp.cand, tag + " candidate"); _same(env.job_mask.cpu().numpy(), exp.mask, tag + " job_mask")
    _same(env.valid_action_mask().cpu().numpy(), exp.vmask, tag + " valid_action_mask")
    got = _state_arrays(env, capi)
    want = dict(exp.state, w3=exp.w3)
    for k in got:
        (_same_nan if k in ("st", "ft") else _same)(got[k], want[k], f"{tag} state {k}")


def run_case(c, obs_dtype, monkeypatch, mode="device"):
    """-> launches.  mode "device": actions as device tensors through step (never raises); "record": step_record on the even
    launches, plain step on the odd ones; "host": numpy actions through the host entry point, which raises on a mixed batch AFTER the
    launch has stepped the valid instances"""
    batch_env, _, capi = _mods()
    for k in _SELECTION_VARS:
        monkeypatch.delenv(k, raising=False)
    if c.force:
        monkeypatch.setenv("MTFJSP_ENV_KERNEL", c.force)
    assert dispatch_kernel(c.J, c.M, c.B, c.force) == c.kernel
    odt = np.float32 if obs_dtype == "f32" else np.float64
    B, T = c.B, c.J * c.M
    exp, w3, (t, p, tt, edge) = ref.expected_side(c)
    env = batch_env.DeviceBatchEnv(c.J, c.M, c.E, B, left_shift=c.left_shift, obs_dtype=obs_dtype)
    env.load_instances(t, p, tt, edge=edge)
    env.scaler_init()
    dev = env.device
    r4, dn = torch.empty(4, B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    nan = float("nan")
    launches = 0
    for ep in range(c.episodes):
        if ep > 0:
            env.scaler_reset_returns()                # the scaler carries across, also for instances rejected in their last steps
        env.reset(w3[ep])                             # over the dirty terminal state of the episode before
        sch = ref.begin_episode(exp, c, ep, w3)
        _check(env, exp, odt, capi, f"{ref.case_id(c)} {obs_dtype} episode {ep} reset", outputs=False)
        while not sch.over():
            s = sch.s
            tag = f"{ref.case_id(c)} {obs_dtype} {mode} episode {ep} step {s}"
            task, mach, kinds = sch.draw()
            rej = exp.rejected(task, mach)
            assert [k is not None for k in kinds] == rej.tolist(), tag
            env.info.fill_(nan); env.raw.fill_(nan); r4.fill_(nan); dn.fill_(nan)
            rows = exp.rows_rewritten(task, rej)
            if len(rows):
                env.tasks_fea[torch.as_tensor(rows, device=dev)] = nan
            recorded = mode == "record" and s % 2 == 0
            if mode == "host":
                if rej.any():
                    with pytest.raises(capi.MtfjspError) as ei:
                        env.step(task, mach)
                    first = int(np.flatnonzero(rej)[0])
                    assert ei.value.code == capi.ERR_ACTION, tag
                    assert f"invalid action for instance {first}: task {task[first]} machine {mach[first]} " in str(ei.value), (tag, str(ei.value))
                else:
                    env.step(task, mach)
            else:
                ta, ma = torch.as_tensor(task, device=dev), torch.as_tensor(mach, device=dev)
                if recorded:
                    env.step_record(ta, ma, r4, dn)
                else:
                    env.step(ta, ma)
            assert exp.step(task, mach).tolist() == rej.tolist()
            _check(env, exp, odt, capi, tag)
            g4, gd = r4.cpu().numpy(), dn.cpu().numpy()
            if recorded:                              # rejected: 0 and d; valid: the float32 of the scaled components and of the done flag
                _same(g4, np.ascontiguousarray(exp.info[:, 2:6].T).astype(np.float32), tag + " r4_out")
                _same(gd, exp.info[:, 1].astype(np.float32), tag + " done_out")
            else:
                assert np.isnan(g4).all() and np.isnan(gd).all(), tag + ": a step without record pointers wrote a record buffer"
            launches += 1
        assert exp.finished().all() and (exp.status == capi.ST_INVALID).all() and (exp.info[:, 1] == 1.0).all()
    env.close()
    return launches


@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_mixed_batches_of_rejected_and_valid_actions_equal_the_oracles(case, obs_dtype, monkeypatch):
    n = run_case(case, obs_dtype, monkeypatch)
    assert case.episodes * (case.J * case.M + 1 + ref.EXTRA_STEPS) <= n <= case.episodes * (2.5 * case.J * case.M + 10)


def _row(family, kernel, shape):
    (c,) = [c for c in ref.CASES if (c.family, c.kernel, (c.J, c.M, c.E)) == (family, kernel, shape) and c.left_shift and c.episodes == 1]
    return c


# one row per family; between them the four copies of the rejection's record writes: k_env_reg, the batched scalar part (16-instance
# kernels), the sequential scalar part (4-instance kernels and the LDS kernel), k_env_step
RECORD_ROWS = [_row("one_slot", "k_env_reg", ref.J6M6), _row("two_slot", "k_env_grp16x2", ref.J3M11), _row("lds_forced", "k_env_step_grp", ref.J6M6),
               _row("lds_default", "k_env_step_grp", ref.J5M12), _row("lds1", "k_env_step", ref.J6M6)]


@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", RECORD_ROWS, ids=ref.case_id)
def test_step_record_of_a_rejected_instance_is_zero_and_done(case, obs_dtype, monkeypatch):
    assert {c.family for c in RECORD_ROWS} == set(ref.FAMILIES)
    run_case(case, obs_dtype, monkeypatch, mode="record")


@pytest.mark.parametrize("case", [ref.Case("host", None, *ref.J6M6, 19, "k_env_grp16", True, 1, ref.SEED),
                                  ref.Case("host", None, *ref.J5M12, 11, "k_env_step_grp", True, 1, ref.SEED)], ids=ref.case_id)
def test_host_entry_point_raises_after_stepping_the_valid_instances(case, monkeypatch):
    run_case(case, "f32", monkeypatch, mode="host")


@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
def test_lookahead_copies_that_are_rejected_equal_their_source_byte_for_byte(obs_dtype, monkeypatch):
    """J9M8E2 (T = 72: k_env_grp16x2 on the scratch handle of B*T copies): with job 0 finished and the other jobs at different ops,
    expand + step on the scratch rejects the M copies of the finished job of every source instance — in the same workgroups as the
    valid copies — and every rejected copy must equal, byte for byte in every read_state array, the source instance it was forked
    from"""
    batch_env, baselines, capi = _mods()
    for k in _SELECTION_VARS:
        monkeypatch.delenv(k, raising=False)
    J, M, E = ref.J9M8
    B, T = 3, J * M
    assert dispatch_kernel(J, M, B * T) == "k_env_grp16x2"
    t, p, tt, edge = ref.instances(J, M, E, B, seed=4)
    exp = ref.Expected(t, p, tt, edge); exp.scaler_init(); exp.reset(ref.reward_weights(B, 4, 1)[0])
    env = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype=obs_dtype)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(exp.w3)
    rs = np.random.RandomState(4)
    for s in range(M + 2 + B):                     # job 0 to its end everywhere; then instance b takes 2 + b more steps on other jobs
        task, mach = np.full(B, -1, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            if s >= M + 2 + b:
                continue                                # task -1: rejected beside its stepping neighbours
            j = 0 if s < M else (b + s) % (J - 1) + 1
            task[b] = j * M + int(exp.state["sched"][b, j * M:(j + 1) * M].sum())
            mach[b] = rs.choice(np.flatnonzero(t[b, task[b]] >= 0))
        env.step(torch.as_tensor(task, device=env.device), torch.as_tensor(mach, device=env.device))
        assert exp.step(task, mach).tolist() == [s >= M + 2 + b for b in range(B)]
    assert exp.state["sched"][:, :M].all() and not exp.finished().any()
    _check(env, exp, np.float32 if obs_dtype == "f32" else np.float64, capi, f"look-ahead source {obs_dtype}")
    la = baselines.Lookahead(env)
    la.expand()
    la.scratch.step(la.task_c, la.mach_c)
    st = la.scratch.status.cpu().numpy()
    src_of = np.arange(B * T) // T
    invalid = (st & capi.ST_INVALID) != 0
    job_of_copy = (np.arange(B * T) % T) // M                       # copy (b, j, m) = scratch instance (b J + j) M + m
    _same(invalid, job_of_copy == 0, "exactly the copies of the finished job are rejected")
    _same(st[invalid], np.full(int(invalid.sum()), capi.ST_INVALID, np.int32), "a rejected copy carries ST_INVALID alone")
    src, cop = _state_arrays(env, capi), _state_arrays(la.scratch, capi)
    for k in src:
        want, got = src[k][src_of[invalid]], cop[k][invalid]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        bad = [int(i) for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, f"{k}: rejected copies {np.flatnonzero(invalid)[bad][:8].tolist()} differ from their source instances"
    # and the source itself did not move
    _check(env, exp, np.float32 if obs_dtype == "f32" else np.float64, capi, f"look-ahead source after the scratch step {obs_dtype}", outputs=False)
    la.close(); env.close()
