"""The host model of a recorded trajectory buffer (tests/trajectory_replay_ref.py) pinned without a GPU.

  * the model IS the reference: fed with the instances, reward weights and recorded decisions of the reference's own rollout
    (tests/golden/rollout_gae_j6m6e2_b4.npz) its environment half equals the reference ReplayBuffer's entries (np.array_equal, the
    adjacency densified) and its network half reproduces the reference's probabilities and critic values, the post-terminal pair
    included, within the tolerances tests/test_rollout_handoff.py applies on that fixture;
  * the comparison of tests/test_trajectory_replay_gpu.py catches what it is for: each slip test plants one defect in a copy of the
    model's record and demands a report that names the field and the slot — from compare_slot / compare_record, the GPU test's own
    environment comparator, and from compare_network, which forms the GPU test's figures (exp(log-probability) against the
    probability of the recorded action, values elementwise / (1 + |expected|)) under the hard caps of tests/error_budget.py's
    tensor classes, the loosest bound the GPU test grants a float32-accurate kernel.

The terminal forward's job mask: the two critics read pooled embeddings only, so a post-terminal job forward under the wrong mask
stores the SAME values (test_terminal_values_do_not_depend_on_the_job_mask) — no comparison of stored numbers can see it.  What
the GPU test holds to the model instead is the mask that forward was given (the record's `term_mask`), and that is where the slip
test plants the defect."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_replay_ref as ref  # noqa: E402
from test_rollout_handoff import FIX, _weights  # noqa: E402

# what a float32 evaluation may differ by: the hard caps of tests/error_budget.py's tensor classes
BOUNDS = dict(a_logprob_operation=2e-6, a_logprob=4e-5, job_v=1e-5, machine_v=2e-5, job_v_=1e-5, machine_v_=2e-5)


@pytest.fixture(scope="module")
def case():
    f = np.load(FIX)
    J, M, E, B, eps = [int(x) for x in f["meta"]]
    g, _ = [float(x) for x in f["gamma_lambda"]]
    model = ref.TrajectoryModel((f["t"], f["p"], f["tt"], f["edge"]), seed=0, obs_dtype="f32", gamma=g)
    rec = model.record(f["job"], f["mach"], eps, weights=f["w3"])
    w = _weights(f)
    net = ref.record_network(w["ja"], w["ma"], rec)
    return f, rec, net, w, (J, M, E, B, eps)


def _device_like(rec, net):
    """a record as a correct device would leave it: the model's environment half and the float32 network half"""
    got = copy.deepcopy(rec)
    for k in ref.NET_FIELDS:
        got[k] = net[k].copy()
    return got


def _report(fn, *args):
    with pytest.raises(AssertionError) as ei:
        fn(*args)
    return str(ei.value)


def test_environment_half_equals_the_reference_buffer(case):
    f, rec, _, _, (J, M, E, B, eps) = case
    assert rec["legal"].all()
    tup = ref.reference_tuple(rec)
    env_side = [n for n in ref.TUPLE_NAMES if n not in ("a_logprob_operation", "a_logprob", "job_v", "machine_v", "job_v_", "machine_v_")]
    assert len(env_side) == 21
    for n in env_side:
        want = f["out_" + n]
        if n in ("adj", "adj_"):
            want = want.astype(np.float32)
        assert tup[n].dtype == want.dtype and tup[n].shape == want.shape, (n, tup[n].dtype, want.dtype, tup[n].shape, want.shape)
        assert np.array_equal(tup[n], want), n
    # the task of every decision is candidate[job]; each episode's weights sit on all of its T slots
    S, T = eps * J * M, J * M
    tasks = np.take_along_axis(rec["candidate"], rec["a_operation"][..., None].astype(np.int64), 2)[..., 0]
    assert np.array_equal(tasks, f["task"])
    for e in range(eps):
        assert np.array_equal(rec["random_weight"][e * T:(e + 1) * T], np.broadcast_to(f["w3"][e].astype(np.float32), (T, B, 3)))
    assert not np.array_equal(f["w3"][0], f["w3"][1])


def test_network_half_reproduces_the_reference_rollout(case):
    f, rec, net, _, (J, M, E, B, eps) = case
    T = J * M
    np.testing.assert_allclose(net["job_prob"], f["job_prob"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(net["mch_prob"], f["mch_prob"], rtol=0, atol=1e-4)
    tol = dict(rtol=1e-3, atol=1e-3)
    for k in ("job_v", "machine_v", "job_v_", "machine_v_"):
        np.testing.assert_allclose(net[k], f["out_" + k], err_msg=k, **tol)
    np.testing.assert_allclose(net["term_job_v_"], f["term_job_v_"], **tol)
    np.testing.assert_allclose(net["term_machine_v_"], f["term_machine_v_"], **tol)
    for e in range(eps):                                # the aliasing the device buffer has: v_ of a slot is v of the next, the pair at the end
        o = e * T
        assert np.array_equal(net["job_v_"][o:o + T - 1], net["job_v"][o + 1:o + T]) and np.array_equal(net["job_v_"][o + T - 1], net["term_job_v_"][e])
        assert np.array_equal(net["machine_v_"][o + T - 1], net["term_machine_v_"][e])
    # the reference sampled its actions from these probabilities: its stored log-probabilities are the model's
    np.testing.assert_allclose(np.exp(f["out_a_logprob_operation"]), np.exp(net["a_logprob_operation"]), rtol=0, atol=1e-4)
    np.testing.assert_allclose(np.exp(f["out_a_logprob"]), np.exp(net["a_logprob"]), rtol=0, atol=1e-4)
    # the binary64 evaluation is the same network: as close to the float32 one as round-off allows
    slot = {k: rec[k][1] for k in ref.FIELDS}
    j32, m32 = ref.slot_forward(case[3]["ja"], case[3]["ma"], slot, net["h_m"][0])
    j64, m64 = ref.slot_forward(case[3]["ja"], case[3]["ma"], slot, net["h_m"][0], dtype=torch.float64)
    assert np.array_equal(j32["job_v"], net["job_v"][1]) and j64["prob"].dtype == np.float64
    assert np.abs(j32["prob"] - j64["prob"]).max() < 1e-5 and np.abs(m32["mach_v"] - m64["mach_v"]).max() < 1e-4
    # a given job embedding replaces the evaluation's own
    _, m_other = ref.slot_forward(case[3]["ja"], case[3]["ma"], slot, net["h_m"][0], h_o=net["h_o"][0])
    assert not np.array_equal(m_other["prob"], m32["prob"])


def test_a_correct_record_passes_the_comparator(case):
    _, rec, net, _, _ = case
    got = _device_like(rec, net)
    ref.compare_record(got, rec)
    worst = ref.compare_network(got, net, rec, BOUNDS)
    assert set(worst) == set(ref.NET_FIELDS) and max(worst.values()) < 1e-6


def test_terminal_values_do_not_depend_on_the_job_mask(case):
    """why the wrong terminal mask has to be caught at the mask itself"""
    _, rec, net, w, (J, M, E, B, eps) = case
    T = J * M
    last = {k: rec[k][T - 1] for k in ref.FIELDS}
    assert last["mask_operation_"].all() and not last["mask_operation"].all()          # after the last step every job is masked
    good = ref.terminal_pair(w["ja"], w["ma"], last, net["h_m"][T - 1])
    bad = ref.terminal_pair(w["ja"], w["ma"], last, net["h_m"][T - 1], job_mask=last["mask_operation_"])
    assert np.array_equal(good[0]["job_v"], bad[0]["job_v"]) and np.array_equal(good[1]["mach_v"], bad[1]["mach_v"])
    assert np.array_equal(good[0]["job_v"], net["term_job_v_"][0])
    assert np.isfinite(good[0]["prob"]).all() and not np.isfinite(bad[0]["prob"]).any()     # only the (unused) probabilities show it


# ------------------------------------------------------------------------------------------------------------- planted slips
def test_slip_log_probability_one_slot_late_is_reported(case):
    _, rec, net, _, _ = case
    for field, after in (("a_logprob", 3), ("a_logprob_operation", 6)):
        p = np.exp(net[field].astype(np.float64))
        # the first slot past `after` whose probabilities are not its predecessor's (the reference's machine policy is often certain)
        at = min(s for s in range(after, len(p)) if np.abs(p[s] - p[s - 1]).max() > 1e-3)
        got = _device_like(rec, net)
        got[field][at:] = net[field][at - 1:-1]                       # from slot `at` on every slot holds its predecessor's
        msg = _report(ref.compare_network, got, net, rec, BOUNDS)
        assert msg.startswith(f"slot {at} {field}:"), msg


def test_slip_machine_mask_rows_at_pitch_8_is_reported(case):
    _, rec, net, _, (J, M, E, B, eps) = case
    got = _device_like(rec, net)
    S = rec["mask_machine_"].shape[0]
    flat = np.zeros(S * B * M + 8, bool)
    for s in range(S):                                                # row b of slot s written 8 bytes after row b - 1, not M
        for b in range(B):
            flat[s * B * M + b * 8:s * B * M + b * 8 + M] = rec["mask_machine_"][s, b, 0]
    got["mask_machine_"] = flat[:S * B * M].reshape(S, B, 1, M)
    first = min(s for s in range(S) if not np.array_equal(got["mask_machine_"][s], rec["mask_machine_"][s]))
    msg = _report(ref.compare_record, got, rec)
    assert msg.startswith(f"slot {first} mask_machine_:") and first <= 1, msg
    assert np.array_equal(got["mask_machine_"][:, 0], rec["mask_machine_"][:, 0])       # (row 0 of every slot is where it belongs)


def test_slip_terminal_job_forward_under_the_post_step_mask_is_reported(case):
    _, rec, net, _, (J, M, E, B, eps) = case
    T = J * M
    for e in range(eps):
        got = _device_like(rec, net)
        got["term_mask"][e] = rec["mask_operation_"][e * T + T - 1]
        msg = _report(ref.compare_record, got, rec)
        assert msg.startswith(f"slot {e * T + T - 1} term_mask"), msg


def test_slip_reward_weights_of_the_previous_episode_is_reported(case):
    _, rec, net, _, (J, M, E, B, eps) = case
    T = J * M
    got = _device_like(rec, net)
    got["random_weight"][T:] = rec["random_weight"][:T]               # begin_episode skipped: the storage still holds episode 0's
    msg = _report(ref.compare_record, got, rec)
    assert msg.startswith(f"slot {T} random_weight:"), msg


def test_slip_idle_and_pt_channels_swapped_is_reported(case):
    _, rec, net, _, _ = case
    got = _device_like(rec, net)
    got["r4"] = np.ascontiguousarray(rec["r4"][:, [0, 2, 1, 3]])
    first = min(s for s in range(rec["r4"].shape[0]) if not np.array_equal(rec["r4"][s, 1], rec["r4"][s, 2]))
    msg = _report(ref.compare_record, got, rec)
    assert msg.startswith(f"slot {first} r4:"), msg


def test_an_illegal_recorded_action_is_reported(case):
    f, rec, _, _, (J, M, E, B, eps) = case
    g, _ = [float(x) for x in f["gamma_lambda"]]
    jobs = f["job"].copy()
    masked = np.flatnonzero(rec["mask_operation"][3, 2])
    assert masked.size
    jobs[3, 2] = masked[0]                                            # a masked job at slot 3, instance 2
    model = ref.TrajectoryModel((f["t"], f["p"], f["tt"], f["edge"]), seed=0, obs_dtype="f32", gamma=g)
    out = list(model.slots(jobs, f["mach"], eps, weights=f["w3"]))
    assert len(out) == 4 and not out[3]["legal"][2] and out[3]["legal"].sum() == B - 1
    msg = _report(ref.compare_slot, {k: rec[k][3] for k in ref.FIELDS}, out[3], 3)
    assert msg.startswith("slot 3: the recorded action of instance 2 is not legal"), msg
