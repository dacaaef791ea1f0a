"""CPU: `evaluate.episode_results` — the one place where the summed step rewards and the finished schedule's costs become
(cost_dict_cumsum, Final_4cost, Objective) for `validate_cost_batched` and the three `*_baselines` — against the expressions each of
the four carried itself before they were merged, written out here literally.  Bit for bit: the tables of policy and rules are compared
with each other and with recorded ones."""
from importlib import import_module

import numpy as np
import pytest

import mtfjsp_amd  # noqa: F401

evaluate = import_module("e2e-mappo-for-mt-fjsp_amd.evaluate")

WEIGHTS = [(0.4, 0.4, 0.2), (0.0, 0.7, 0.3), (1.0 / 3.0, 0.1, 0.5666666666666667), (0.5, 0.0, 0.5)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def literal(c, prev, T, w):
    """the former bodies, verbatim"""
    cost = {"opr_Gt": c[:, 0], "opr_mk": c[:, 1], "opr_idleT": c[:, 2], "opr_pt": c[:, 3], "opr_transT": c[:, 4]}
    final4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
    obj = w[0] * final4[:, 0] + w[1] * (final4[:, 1] + final4[:, 3]) + w[2] * final4[:, 2]
    return cost, final4, obj


def draw(rng, N):
    cum = -rng.uniform(0.0, 500.0, (N, 5)) * rng.choice([1.0, 1e-3, 1e3], (N, 5))
    prev = rng.uniform(0.0, 300.0, (N, 4)) * rng.choice([1.0, 1e-3, 1e3], (N, 4))
    return cum, prev


@pytest.mark.parametrize("N", [1, 7, 64])
@pytest.mark.parametrize("T", [4, 36])
def test_bit_equal_to_the_literal_expressions(N, T):
    rng = np.random.default_rng(1000 * N + T)
    for w in WEIGHTS:
        for _ in range(3):
            cum, prev = draw(rng, N)
            cost, final4, obj = evaluate.episode_results(cum, prev, T, w)
            cost_l, final4_l, obj_l = literal(cum, prev, T, w)
            assert tuple(cost) == evaluate.COST_KEYS == ("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")
            assert all(same_bits(cost[k], cost_l[k]) for k in cost_l)
            assert final4.shape == (N, 4) and same_bits(final4, final4_l)
            assert obj.shape == (N,) and same_bits(obj, obj_l)
            # and against scalar arithmetic in the documented association
            for i in range(N):
                f = [float(prev[i, 0]), float(prev[i, 1]) / T, float(prev[i, 2]), float(prev[i, 3])]
                assert final4[i].tolist() == f
                assert float(obj[i]) == w[0] * f[0] + w[1] * (f[1] + f[3]) + w[2] * f[2]


def test_the_costs_are_the_columns_of_cum_in_order():
    cum = np.arange(35, dtype=np.float64).reshape(7, 5)
    cost, _, _ = evaluate.episode_results(cum, np.ones((7, 4)), 4, WEIGHTS[0])
    assert list(cost) == list(evaluate.COST_KEYS)
    for i, key in enumerate(evaluate.COST_KEYS):
        assert same_bits(cost[key], cum[:, i])


@pytest.mark.parametrize("T", [4, 36])
def test_signed_zeros_infinities_and_nans_propagate(T):
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5])
    prev = np.array([[a, b, c, d] for a in special for b in special for c in (0.0, -0.0, np.nan, 2.0) for d in (-0.0, np.inf, 3.0)])
    cum = np.tile(special[:5], (prev.shape[0], 1))
    for w in WEIGHTS:
        with np.errstate(invalid="ignore"):                         # 0 * inf, inf - inf: the NaNs are the point
            cost, final4, obj = evaluate.episode_results(cum, prev, T, w)
            _, final4_l, obj_l = literal(cum, prev, T, w)
        # columns 0, 2, 3 are prev's own words (the sign of a zero, the payload of a NaN); column 1 is ONE division
        for col in (0, 2, 3):
            assert same_bits(final4[:, col], prev[:, col])
        assert same_bits(final4[:, 1], prev[:, 1] / T)
        assert np.array_equal(np.isnan(final4), np.isnan(prev)) and np.array_equal(np.signbit(final4), np.signbit(prev))
        assert same_bits(final4, final4_l) and same_bits(obj, obj_l)
        assert np.array_equal(obj, obj_l, equal_nan=True)
        assert all(same_bits(cost[k], cum[:, i]) for i, k in enumerate(evaluate.COST_KEYS))
