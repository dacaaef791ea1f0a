"""CPU: the host models of tests/policy_beam_ref.py on hand-written rows — the rules the device kernels are then held to."""
import numpy as np

import policy_beam_ref as ref

NEG = -np.inf
L = np.log


def _one(score, lj, lm, jm=None, mm=None, W=None):
    score, lj, lm = np.asarray(score, np.float64), np.asarray(lj, np.float64), np.asarray(lm, np.float64)
    jm = np.zeros(lj.shape, np.uint8) if jm is None else np.asarray(jm, np.uint8)
    mm = np.zeros(lm.shape, np.uint8) if mm is None else np.asarray(mm, np.uint8)
    return ref.select(score, lj, lm, jm, mm, len(score) if W is None else W)


def test_ranks_come_out_in_value_order():
    # W = 2, J = 2, M = 2; slot 1 is empty
    picks = _one([0.0, NEG], [[L(0.75), L(0.25)], [0.0, 0.0]], [[[L(0.5), L(0.5)], [L(0.9), L(0.1)]], [[0.0, 0.0], [0.0, 0.0]]])
    assert [p[:3] for p in picks] == [(0, 0, 0), (0, 0, 1)]                 # 0.375 twice (a tie inside the slot: lowest c first), then 0.225
    assert picks[0][3] == (0.0 + L(0.75)) + L(0.5)


def test_ties_across_slots_and_within_a_slot_go_to_the_lowest_candidate():
    lj = np.full((3, 2), L(0.5)); lm = np.full((3, 2, 2), L(0.5))
    picks = _one([-1.0, -1.0, -1.0], lj, lm)
    assert [p[:3] for p in picks] == [(0, 0, 0), (0, 0, 1), (0, 1, 0)]
    picks = _one([-2.0, -1.0, -1.0], lj, lm)
    assert [p[:3] for p in picks] == [(1, 0, 0), (1, 0, 1), (1, 1, 0)]
    # signed zeros tie: the lowest c wins and every rank reports its own candidate's sum
    picks = _one([-0.0, 0.0], [[-0.0], [0.0]], [[[-0.0]], [[0.0]]])
    assert [p[:3] for p in picks] == [(0, 0, 0), (1, 0, 0)] and np.signbit(picks[0][3]) and not np.signbit(picks[1][3])


def test_fewer_eligible_candidates_than_ranks():
    picks = _one([0.0, NEG, NEG], np.zeros((3, 1)), np.array([[[L(0.6), L(0.4)]], [[0.0, 0.0]], [[0.0, 0.0]]]))
    assert [p and p[:3] for p in picks] == [(0, 0, 0), (0, 0, 1), None]


def test_an_empty_slot_offers_nothing_whatever_its_logs_say():
    picks = _one([NEG, -5.0], [[0.0], [L(0.5)]], [[[0.0]], [[L(0.5)]]])
    assert [p and p[:3] for p in picks] == [(1, 0, 0), None]


def test_nan_and_minus_infinity_logs_are_never_selected():
    lj = [[L(0.5), np.nan, NEG]]
    lm = [[[L(0.5), NEG], [0.0, 0.0], [0.0, 0.0]]]
    picks = _one([0.0], lj, lm, W=1)
    assert picks[0][:3] == (0, 0, 0)
    picks = ref.select(np.array([0.0, NEG, NEG, NEG]), np.tile(np.array(lj), (4, 1)), np.tile(np.array(lm), (4, 1, 1)),
                       np.zeros((4, 3), np.uint8), np.zeros((4, 3, 2), np.uint8), 4)
    assert [p and p[:3] for p in picks] == [(0, 0, 0), None, None, None]
    # +inf is a value like any other (only NaN and -inf are not)
    assert _one([0.0], [[np.inf, 0.0]], [[[0.0], [0.0]]], W=1)[0][:3] == (0, 0, 0)


def test_masks_remove_candidates():
    lj = [[L(0.9), L(0.1)]]; lm = [[[L(0.9), L(0.1)], [L(0.5), L(0.5)]]]
    assert _one([0.0], lj, lm, jm=[[1, 0]], W=1)[0][:3] == (0, 1, 0)
    assert _one([0.0], lj, lm, mm=[[[1, 0], [0, 0]]], W=1)[0][:3] == (0, 0, 1)
    assert _one([0.0], lj, lm, jm=[[1, 1]], W=1) == [None]
    assert _one([0.0], lj, lm, mm=[[[1, 1], [1, 1]]], W=1) == [None]


def test_the_two_additions_are_taken_in_order():
    a, b, c = 1.0, 2.0 ** -53, 2.0 ** -53
    assert (a + b) + c != a + (b + c)
    picks = _one([a, a + (b + c)], [[b], [0.0]], [[[c]], [[0.0]]])
    # slot 0's candidate is (a + b) + c = 1.0, slot 1's is the larger a + (b + c): slot 1 ranks first
    assert [p[:3] for p in picks] == [(1, 0, 0), (0, 0, 0)]
    assert picks[1][3] == 1.0 and picks[0][3] == a + (b + c)
    assert ref.values([a], [[b]], [[[c]]])[0, 0, 0] == (a + b) + c


def test_select_batch_forms_the_seven_outputs():
    W, J, M = 2, 2, 2
    score = np.array([0.0, NEG, -1.5, -0.5])
    lm = np.log(np.full((4 * J, M), 0.5))
    cand = np.array([[1, 2], [0, 2], [1, 3], [0, 3]], np.int32)
    with np.errstate(divide="ignore"):
        lj = np.log(np.array([[0.75, 0.25], [0.5, 0.5], [1.0, 0.0], [0.5, 0.5]]))
        out = ref.select_batch(score, lj, lm, np.zeros((4, J), np.uint8), np.zeros((4 * J, M), np.uint8), cand, W)
    assert out["parent"].tolist() == [0, 0, 3, 3] and out["from_slot"].tolist() == [0, 0, 1, 1]
    assert out["job"].tolist() == [0, 0, 0, 0] and out["mach"].tolist() == [0, 1, 0, 1]
    assert out["task"].tolist() == [1, 1, 0, 0] and out["child"].tolist() == [0, 0, 6, 6]
    assert out["score"][2] == (-0.5 + L(0.5)) + L(0.5)


def test_merge_empties_the_later_slots_of_one_signature():
    sig = np.array([7, 7, 7, 9, 5, 5, 5, 5], np.uint64)
    score = np.array([-1.0, -2.0, -3.0, -4.0, NEG, -1.0, -2.0, NEG])
    got = ref.merge(sig, score, 4)
    # source 0: three equal signatures, the first survives; source 1: a -inf holder does not count, the first live one survives
    assert got.tolist() == [-1.0, NEG, NEG, -4.0, NEG, -1.0, NEG, NEG]
    # entry scores decide: slot 2 is emptied by slot 0 even though slot 1 (which also matches) is emptied itself
    assert ref.merge(np.array([1, 2, 1], np.uint64), np.array([-1.0, -1.5, -2.0]), 3).tolist() == [-1.0, -1.5, NEG]
    # groups do not see each other
    assert ref.merge(np.array([3, 3], np.uint64), np.array([-1.0, -2.0]), 1).tolist() == [-1.0, -2.0]


def test_search_keeps_prefixes_through_the_back_pointers():
    N, W, J, M = 1, 2, 2, 1
    s = ref.Search(N, W, dedupe=True)
    lj = np.log(np.array([[0.6, 0.4], [0.5, 0.5]])); lm = np.zeros((W * J, M))
    zeros = lambda *sh: np.zeros(sh, np.uint8)                              # noqa: E731
    r0 = s.decide(lj, lm, zeros(W, J), zeros(W * J, M), np.array([[0, 1], [0, 1]], np.int32), np.array([11, 12], np.uint64))
    assert r0["job"].tolist() == [0, 1] and r0["parent"].tolist() == [0, 0]
    # both slots now finish the other job; the children are one schedule: the second is emptied
    r1 = s.decide(np.zeros((W, J)), lm, np.array([[1, 0], [0, 1]], np.uint8), zeros(W * J, M), np.array([[0, 1], [0, 1]], np.int32),
                  np.array([33, 33], np.uint64))
    assert r1["parent"].tolist() == [0, 1] and r1["job"].tolist() == [1, 0]
    assert r1["merged"][1] == NEG and r1["score"][1] == L(0.4)
    task, mach = s.plan(np.array([1]))
    assert task.tolist() == [[1, 0]] and mach.tolist() == [[0, 0]]
    assert s.plan(np.array([2]))[0].tolist() == [[-1, -1]]
