"""No GPU: the expected side and the schedule of tests/rejected_actions_ref.py are sound before the device is held to them.

  * B oracles of batch 1 equal one oracle of batch B when every action is valid — state, observation, info, raw, candidate, masks,
    after every step of a whole episode — so stepping an instance's own oracle is the batched step of that instance;
  * for every row of the table the schedule, run on the oracle alone, meets the conditions the GPU test relies on (they are conditions
    on the seeds, not measurements of the device);
  * the dispatch sends every row to the kernel it names, and the rows cover all seven step kernels.
"""
from importlib import import_module

import numpy as np
import pytest

import rejected_actions_ref as ref
from env_parity import _same, dispatch_kernel, random_valid


def _same_nan(got, want, what):
    _same(np.isnan(got), np.isnan(want), what + " (NaN pattern)")
    _same(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want), what)


@pytest.mark.parametrize("shape", [ref.J6M6, ref.J3M11], ids=["J6M6E2", "J3M11E1"])
@pytest.mark.parametrize("left_shift", [True, False], ids=["left_shift", "no_left_shift"])
def test_batch_one_oracles_equal_the_batched_oracle_on_valid_actions(shape, left_shift):
    from oracle.env_oracle import OracleBatch
    J, M, E = shape
    B, T = 5, J * M
    t, p, tt, edge = ref.instances(J, M, E, B, seed=1)
    w3 = ref.reward_weights(B, 1, 1)[0]
    exp = ref.Expected(t, p, tt, edge, left_shift=left_shift); exp.scaler_init(); exp.reset(w3)
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift); orc.scaler_init()
    o = orc.reset(w3)
    cand, mask = orc.job_mask_state()
    rs = np.random.RandomState(1)

    def check(tag):
        _same(exp.tfea, o["tfea"], tag + " tasks_fea"); _same(exp.mfea2, o["mfea2"], tag + " m_fea2"); _same(exp.adj, o["adj"], tag + " adj")
        _same(exp.cand, cand, tag + " candidate"); _same(exp.mask, mask, tag + " job_mask")
        _same(exp.vmask, orc.valid_action_mask(), tag + " valid_action_mask")
        so = orc.state()
        assert sorted(so) == sorted(exp.state)
        for k in so:
            (_same_nan if k in ("st", "ft") else _same)(exp.state[k], so[k], f"{tag} {k}")

    check("reset")
    for s in range(T):
        job, task, mach = random_valid(rs, cand, mask, t >= 0)
        rej = exp.step(task, mach)
        assert not rej.any(), s
        info, raw, paths = orc.step(task, mach)
        cand, mask = orc.job_mask_update(job)
        o = orc.observe()
        tag = f"step {s}"
        _same(exp.info, info, tag + " info"); _same(exp.raw, raw, tag + " raw"); _same(exp.status, paths, tag + " path")
        check(tag)
    assert exp.finished().all() and exp.info[:, 1].all()


def test_a_rejected_step_moves_nothing_on_the_expected_side():
    """the expected side's own promise, on a hand-made mixed batch: a rejected instance keeps every array and gets the header's
    outputs; its neighbour is stepped"""
    capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
    assert (ref.ST_INVALID, ref.ST_INFEASIBLE) == (capi.ST_INVALID, capi.ST_INFEASIBLE)
    J, M, E = ref.J6M6
    t, p, tt, edge = ref.instances(J, M, E, 3, seed=2)
    exp = ref.Expected(t, p, tt, edge); exp.scaler_init(); exp.reset(ref.reward_weights(3, 2, 1)[0])
    m0 = [int(np.flatnonzero(t[b, 0] >= 0)[0]) for b in range(3)]
    assert not exp.step(np.zeros(3, np.int32), np.array(m0, np.int32)).any()       # task 0 everywhere
    before = {k: v.copy() for k, v in exp.state.items()}
    tfea, adj, cand = exp.tfea.copy(), exp.adj.copy(), exp.cand.copy()
    m1 = int(np.flatnonzero(t[1, 1] >= 0)[0])
    rej = exp.step(np.array([0, 1, 2], np.int32), np.array([m0[0], m1, 0], np.int32))   # scheduled | valid | predecessor unscheduled
    assert rej.tolist() == [True, False, True]
    for b in (0, 2):
        assert exp.info[b].tolist() == [0.0] * 6 and exp.raw[b].tolist() == [0.0] * 5 and exp.status[b] == capi.ST_INVALID
        for k in before:
            assert np.array_equal(before[k][b], exp.state[k][b], equal_nan=True), k
        assert np.array_equal(tfea[b * 36:(b + 1) * 36], exp.tfea[b * 36:(b + 1) * 36]) and np.array_equal(adj[b], exp.adj[b])
        assert np.array_equal(cand[b], exp.cand[b])
    assert exp.state["sched"][1].sum() == 2 and exp.status[1] < 8 and exp.cand[1, 0] == 2


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_the_schedule_meets_its_conditions_on_the_oracle_alone(case):
    c = case
    T, g = c.J * c.M, ref.GROUP[c.kernel]
    exp, w3, _ = ref.expected_side(c)
    for ep in range(c.episodes):
        sch = ref.begin_episode(exp, c, ep, w3)
        cen = ref.Census(c.B, g)
        while not sch.over():
            task, mach, kinds = sch.draw()
            if sch.s - 1 in (0, ref.GROUP_STEP, ref.NOBODY_STEP):
                assert not exp.finished().any()                       # the fixed steps fall on a batch that is running
            rej = exp.step(task, mach)
            cen.note(sch.s - 1, kinds, rej, exp.finished())
        tag = f"{ref.case_id(c)} episode {ep}: {cen.kinds}, {cen.launches} launches, {cen.mixed_steps} mixed steps, finished at {cen.finish_step}"
        assert all(n >= 2 for n in cen.kinds.values()), tag
        assert cen.mixed_steps >= 10, tag
        assert all(cen.fixed.values()), (tag, cen.fixed)
        assert exp.finished().all() and None not in cen.finish_step, tag
        assert len(set(cen.finish_step)) > 1, tag                      # instances finish at different steps
        assert cen.launches <= 2.5 * T + 10, tag
        assert cen.launches == max(cen.finish_step) + 1 + ref.EXTRA_STEPS, tag
        # a finished instance is rejected from then on, with done = 1, beside running neighbours
        assert (exp.info[:, 1] == 1.0).all() and (exp.status == ref.ST_INVALID).all(), tag


def test_the_table_reaches_every_step_kernel_and_every_group_is_ragged():
    for c in ref.CASES:
        assert dispatch_kernel(c.J, c.M, c.B, c.force) == c.kernel, ref.case_id(c)
        assert c.M % c.E == 0 and c.J * c.M <= 130 and c.B <= 19, ref.case_id(c)
        g = ref.GROUP[c.kernel]
        if g > 1:
            assert c.B > g and c.B % g != 0, ref.case_id(c)           # at least one full group and a partly filled last one
    assert {c.kernel for c in ref.CASES} == set(ref.STEP_KERNELS)
    assert {c.family for c in ref.CASES} == set(ref.FAMILIES)
    for fam in ref.FAMILIES:
        rows = [c for c in ref.CASES if c.family == fam]
        assert sum(not c.left_shift for c in rows) == 1 and sum(c.episodes == 2 for c in rows) == 1, fam
    assert any(c.kernel == "k_env_grp16" and c.J * c.M == 64 for c in ref.CASES)                     # every lane a task
    assert any(c.kernel in ("k_env_grp16x2", "k_env_grp4x2") and c.J * c.M <= 64 for c in ref.CASES)  # second slot empty
    assert any(c.kernel == "k_env_step_grp" and c.force is None and c.J * c.M == 130 for c in ref.CASES)
