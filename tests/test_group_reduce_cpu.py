"""CPU: the host model of mtfjsp_group_reduce (tests/group_reduce_ref.py) against a brute-force O(K^2) restatement that shares no
code with it, and against hand-made cases whose answers are written out."""
import itertools

import numpy as np
import pytest

import group_reduce_ref as ref

W = (0.4, 0.4, 0.2)
NAN = float("nan")


def brute(cost4, done, w, N, K):
    """the rule once more, scalar by scalar in Python floats: sorting for the best, the definition for the front"""
    cost4 = [[float(x) for x in row] for row in np.asarray(cost4, np.float64).reshape(N * K, 4)]
    done = [int(x) for x in np.asarray(done).reshape(N * K)]
    obj, best, best_obj, front = [], [], [], []
    for n in range(N):
        pts = []
        for c in range(K):
            r = cost4[n * K + c]
            mk, ec, tt = r[0], r[1] + r[3], r[2]
            ok = done[n * K + c] != 0 and not (mk != mk or ec != ec or tt != tt)
            pts.append((ok, mk, ec, tt, (w[0] * mk + w[1] * ec) + w[2] * tt))
            obj.append(pts[-1][4] if ok else NAN)
        ranked = sorted((p[4], c) for c, p in enumerate(pts) if p[0] and p[4] == p[4])
        best.append(n * K + ranked[0][1] if ranked else -1)
        best_obj.append(ranked[0][0] if ranked else NAN)
        for c, (ok, mk, ec, tt, _) in enumerate(pts):
            beaten = False
            for c2, (ok2, mk2, ec2, tt2, _) in enumerate(pts):
                if not ok2 or c2 == c:
                    continue
                no_worse = mk2 <= mk and ec2 <= ec and tt2 <= tt
                better = mk2 < mk or ec2 < ec or tt2 < tt
                same = (mk2, ec2, tt2) == (mk, ec, tt)
                if no_worse and (better or (same and c2 < c)):
                    beaten = True
            front.append(1 if ok and not beaten else 0)
    return np.array(obj), np.array(best, np.int32), np.array(best_obj), np.array(front, np.uint8)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _check(cost4, done, w, N, K):
    got, want = ref.group_reduce(cost4, done, w, N, K), brute(cost4, done, w, N, K)
    # -0.0 and 0.0 are one value for "smallest": sorting may keep either, the bits of best_obj are compared through the index
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[2]), _bits(want[2]))
    return got


@pytest.mark.parametrize("kind", ["integer", "random", "scattered", "none"])
@pytest.mark.parametrize("N,K", [(1, 1), (3, 1), (1, 5), (3, 5), (2, 37), (3, 65)])
def test_model_equals_the_brute_force_restatement(kind, N, K):
    cost4, done = ref.synthetic(kind, N, K, seed=100 * N + K)
    obj, best, best_obj, front = _check(cost4, done, W, N, K)
    if kind == "none":
        assert (best == -1).all() and np.isnan(best_obj).all() and not front.any() and np.isnan(obj).all()
    if kind == "integer" and K >= 37:
        assert front.sum() < N * K and len(set(map(tuple, cost4))) < N * K, "the integer data must hold ties and duplicates"


def _rows(points):
    """(mk, ec, tt) points -> cost4 rows with the energy split over columns 1 and 3"""
    return np.array([[mk, ec - 1.0, tt, 1.0] for mk, ec, tt in points])


def test_all_equal_group():
    K = 6
    obj, best, best_obj, front = _check(_rows([(3.0, 4.0, 5.0)] * K), np.ones(K, np.uint8), W, 1, K)
    assert best[0] == 0 and front.tolist() == [1, 0, 0, 0, 0, 0] and len(set(_bits(obj))) == 1
    assert best_obj[0] == (0.4 * 3.0 + 0.4 * 4.0) + 0.2 * 5.0


def test_chain_where_each_copy_dominates_the_next():
    K = 5
    obj, best, best_obj, front = _check(_rows([(1.0 + c, 2.0 + c, 3.0 + c) for c in range(K)]), np.ones(K, np.uint8), W, 1, K)
    assert best[0] == 0 and front.tolist() == [1, 0, 0, 0, 0]
    # reversed: the last copy dominates all
    obj, best, best_obj, front = _check(_rows([(9.0 - c, 9.0 - c, 9.0 - c) for c in range(K)]), np.ones(K, np.uint8), W, 1, K)
    assert best[0] == K - 1 and front.tolist() == [0, 0, 0, 0, 1]


def test_group_with_nothing_eligible_beside_a_live_one():
    K = 3
    cost4 = _rows([(1.0, 2.0, 3.0)] * (2 * K))
    done = np.array([0, 0, 0, 1, 1, 1], np.uint8)
    obj, best, best_obj, front = _check(cost4, done, W, 2, K)
    assert best.tolist() == [-1, 3] and np.isnan(best_obj[0]) and front.tolist() == [0, 0, 0, 1, 0, 0]
    assert np.isnan(obj[:K]).all() and not np.isnan(obj[K:]).any()


def test_nan_in_one_objective_removes_the_copy():
    # copy 0 would dominate everything but its transport time is NaN; copy 2's NaN hides in the idle column (ec = c1 + c3)
    cost4 = np.array([[0.0, 0.0, NAN, 0.0], [5.0, 1.0, 5.0, 1.0], [1.0, 1.0, 1.0, NAN], [6.0, 1.0, 4.0, 1.0]])
    obj, best, best_obj, front = _check(cost4, np.ones(4, np.uint8), W, 1, 4)
    assert np.isnan(obj[[0, 2]]).all() and best[0] == 1 and front.tolist() == [0, 1, 0, 1]


def test_duplicate_pair_on_the_front_keeps_its_lowest_index():
    pts = [(5.0, 5.0, 5.0), (1.0, 9.0, 1.0), (9.0, 1.0, 1.0), (1.0, 9.0, 1.0), (9.0, 9.0, 9.0)]
    obj, best, best_obj, front = _check(_rows(pts), np.ones(5, np.uint8), W, 1, 5)
    assert front.tolist() == [1, 1, 1, 0, 0]
    assert best[0] == 1                                                 # obj 4.2 twice (copies 1 and 3) and once more (copy 2): lowest c


def test_objective_tie_between_copies_that_differ_in_their_costs():
    # (2, 4, 6) and (4, 2, 6): equal weights on mk and ec give one objective; neither dominates the other
    pts = [(8.0, 8.0, 8.0), (4.0, 2.0, 6.0), (2.0, 4.0, 6.0)]
    obj, best, best_obj, front = _check(_rows(pts), np.ones(3, np.uint8), W, 1, 3)
    assert _bits(obj[1:2]) == _bits(obj[2:3]) and best[0] == 1 and front.tolist() == [0, 1, 1]


def test_every_small_integer_group_of_three():
    """exhaustive: all 3-copy groups over a 2 x 2 x 2 grid of objectives and all done patterns"""
    pts = list(itertools.product((0.0, 1.0), repeat=3))
    for trio in itertools.product(pts, repeat=3):
        for done in ((1, 1, 1), (1, 0, 1), (0, 1, 1)):
            _check(_rows(trio), np.array(done, np.uint8), W, 1, 3)


def test_signed_zeros_and_infinities():
    cost4 = np.array([[0.0, 0.0, 0.0, 0.0], [-0.0, 0.0, -0.0, 0.0], [np.inf, 0.0, 1.0, 0.0], [1.0, 0.0, -np.inf, 0.0]])
    got = ref.group_reduce(cost4, np.ones(4, np.uint8), W, 1, 4)
    assert got[1][0] == 3 and got[2][0] == -np.inf                      # -inf is the smallest objective
    assert got[3].tolist() == [1, 0, 0, 1]                              # -0.0 == 0.0: copy 1 is a duplicate of copy 0
    got = ref.group_reduce(cost4[:3], np.ones(3, np.uint8), (0.0, 0.4, 0.2), 1, 3)
    assert np.isnan(got[0][2]) and got[1][0] == 0                       # 0 * inf: an objective that is NaN is never the smallest


def test_final_costs_model():
    prev = np.array([[10.0, 72.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]])
    c4, done = ref.final_costs(prev, np.array([36.0, 35.0]), 36)
    assert c4.tolist() == [[10.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]] and done.tolist() == [1, 0]
