"""The host model of the device's random streams and action selection (tests/device_streams_ref.py) checked on its own, without a GPU:
Philox4x32-10 known answers, the selection against an independent binary64 inverse CDF, the distribution and independence of the
draws, structural facts of the reward weights and of the generator.  tests/test_device_streams_gpu.py and
tests/test_selection_exact_gpu.py then demand the device EQUAL to this model: a correct sampler here is a correct sampler there."""
import os
import sys
from statistics import NormalDist

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_streams_ref as ref  # noqa: E402


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    """the Random123 known-answer vectors of Philox4x32-10"""
    got = ref.philox4x32(*ctr, *key)
    assert tuple(int(x) for x in got) == out
    got = ref.philox4x32(*[np.full(5, c, np.uint64) for c in ctr], *key)          # the vectorised path
    assert all((g == o).all() for g, o in zip(got, out))


def _random_rows(rs, B, n):
    p = rs.uniform(0.0, 1.0, (B, n)).astype(np.float32)
    p[rs.uniform(size=(B, n)) < 0.35] = 0.0                                        # masked entries
    p[np.arange(B), rs.randint(0, n, B)] += np.float32(0.05)                       # at least one positive entry
    p *= rs.choice([0.25, 1.0, 3.0], (B, 1)).astype(np.float32) / np.maximum(p.sum(1, keepdims=True), 1e-6)   # tot = 0.25, 1 or 3 (up to rounding)
    return p.astype(np.float32)


def test_pick_equals_a_binary64_inverse_cdf():
    """pick (binary32, the kernel's order of operations) against a binary64 inverse CDF written independently: equal wherever the
    draw is further than n binary32 ulps of the total from every decision boundary; such near-boundary rows are rare (<= 1e-3)"""
    rs = np.random.RandomState(1)
    rows = excluded = 0
    for n in range(1, 41):
        B = 20000
        p = _random_rows(rs, B, n)
        u = ref.pick_uniform(np.arange(B), 7 + n, n)
        got = ref.pick(p, False, u)
        p64 = p.astype(np.float64)
        cum = np.cumsum(p64, 1)
        thr = u.astype(np.float64) * cum[:, -1]
        pos = p64 > 0
        hit = pos & (thr[:, None] < cum)
        last = n - 1 - np.argmax(pos[:, ::-1], 1)
        want = np.where(hit.any(1), np.argmax(hit, 1), last)
        margin = np.where(pos, np.abs(thr[:, None] - cum), np.inf).min(1)
        sure = margin > n * np.spacing(cum[:, -1].astype(np.float32)).astype(np.float64)
        assert np.array_equal(got[sure], want[sure]), f"n={n}"
        assert pos[np.arange(B), got].all(), "a masked entry was drawn"
        rows += B
        excluded += int((~sure).sum())
    print(f"rows within n ulps of a boundary: {excluded} of {rows} = {excluded / rows:.2e}")
    assert excluded / rows <= 1e-3


def test_pick_greedy_takes_the_first_maximum():
    p = np.array([[0.2, 0.5, 0.5, 0.1], [0.3, 0.3, 0.3, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.1, 0.1]], np.float32)
    assert ref.pick(p, True).tolist() == [1, 0, 0, 2]
    # sampling: an all-zero row gives 0; u just below 1 on a row whose last entries are masked gives the last POSITIVE entry
    assert ref.pick(p, False, np.array([0.5, 0.99999994, 0.5, 0.0], np.float32)).tolist() == [1, 2, 0, 2]


def _chi2_quantile(dof, q=1e-6):
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - q, dof))
    except ImportError:
        if dof == 1:                                                               # the square of a standard normal
            return NormalDist().inv_cdf(1.0 - q / 2) ** 2
        z = NormalDist().inv_cdf(1.0 - q)                                          # Wilson-Hilferty
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3


ROWS = {
    2: [0.3, 0.7],
    6: [0.1, 0.0, 0.35, 0.05, 0.0, 0.5],
    20: [0.02, 0.0, 0.11, 0.07, 0.0, 0.0, 0.2, 0.01, 0.09, 0.0, 0.05, 0.0, 0.15, 0.03, 0.0, 0.12, 0.0, 0.08, 0.04, 0.03],
}


@pytest.mark.parametrize("n", [2, 6, 20])
def test_the_model_samples_the_row(n):
    """2^20 (instance, counter) pairs: chi-square of the drawn indices against the row below the 1 - 1e-6 quantile; masked entries never drawn"""
    row = np.array(ROWS[n], np.float32)
    nb, nc = 4096, 256
    idx = np.concatenate([ref.pick(np.tile(row, (nb, 1)), False, ref.pick_uniform(np.arange(nb), 99, c)) for c in range(nc)])
    N = idx.size
    assert N == 1 << 20
    cnt = np.bincount(idx, minlength=n).astype(np.float64)
    assert (cnt[row == 0] == 0).all(), "a masked entry was drawn"
    pr = row.astype(np.float64)[row > 0] / row.astype(np.float64).sum()
    stat = float((((cnt[row > 0] - N * pr) ** 2) / (N * pr)).sum())
    dof = int((row > 0).sum()) - 1
    bound = _chi2_quantile(dof)
    print(f"n={n}: chi-square {stat:.2f} with {dof} degrees of freedom, bound {bound:.2f}")
    assert stat < bound


def test_draws_are_uncorrelated_across_counters_and_instances():
    nb, nc = 1024, 1024
    u = np.stack([ref.pick_uniform(np.arange(nb + 1), 5, c) for c in range(nc + 1)]).astype(np.float64)       # [counter, b]
    N = nb * nc
    for name, a, b in (("counter", u[:-1, :-1], u[1:, :-1]), ("instance", u[:-1, :-1], u[:-1, 1:])):
        r = float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
        print(f"correlation of u with the next {name}'s: {r:.2e} (bound {5 / N ** 0.5:.2e})")
        assert abs(r) < 5 / N ** 0.5
    assert (u >= 0).all() and (u < 1).all()
    assert abs(u.mean() - 0.5) < 5 / (12 * N) ** 0.5
    # every word of seed and counter matters
    base = ref.pick_uniform(np.arange(64), 3, 9)
    for seed, counter in ((3 + (1 << 32), 9), (3, 9 + (1 << 32)), (4, 9), (3, 10)):
        assert not np.array_equal(base, ref.pick_uniform(np.arange(64), seed, counter))


@pytest.mark.parametrize("seed,episode", [(0, 0), (11, 1), ((1 << 32) + 5, (1 << 32) + 3), ((1 << 63) + 1, 2)])
def test_reward_weights_are_three_positive_numbers_summing_to_one(seed, episode):
    w = ref.draw_w3(5000, seed, episode)
    assert w.shape == (5000, 3) and (w > 0).all() and (w < 1).all()
    assert np.abs((w[:, 0] + w[:, 1]) + w[:, 2] - 1.0).max() <= 2.0 ** -52         # one ulp of 1
    assert len({r.tobytes() for r in w}) == 5000
    assert not np.array_equal(w, ref.draw_w3(5000, seed, episode + 1)) and not np.array_equal(w, ref.draw_w3(5000, seed + 1, episode))
    assert not np.array_equal(w, ref.draw_w3(5000, seed ^ (1 << 40), episode)) and not np.array_equal(w, ref.draw_w3(5000, seed, episode ^ (1 << 40)))
    assert np.abs(w.mean(0) - 1 / 3).max() < 0.01


@pytest.mark.parametrize("J,M,E,B", [(6, 6, 2, 300), (10, 10, 2, 40), (20, 20, 4, 9), (3, 4, 2, 7), (13, 5, 1, 2), (4, 8, 2, 3)])
def test_generator_structure(J, M, E, B):
    t, p, tt, shop = ref.generate(B, J, M, E, 5, first_instance=3)
    T = J * M
    assert t.shape == (B, T, M) and p.shape == t.shape and tt.shape == (B, M, M) and shop.shape == (B, M)
    assert np.array_equal(t < 0, p < 0), "t < 0 exactly where p < 0"
    assert (np.abs(t) >= 0.8).all() and (np.abs(t) <= 99 * 1.2).all() and (np.abs(p) >= 0.8).all() and (np.abs(p) <= 20 * 1.2).all()
    nbad = (t < 0).sum(-1)
    assert nbad.max() <= M - 1, "at least one feasible machine per task"
    assert np.array_equal(tt, np.transpose(tt, (0, 2, 1))) and (np.diagonal(tt, axis1=1, axis2=2) == 0).all()
    same = shop[0][:, None] == shop[0][None, :]
    off = ~np.eye(M, dtype=bool)
    assert (tt[:, same & off] >= 1).all() and (tt[:, same & off] <= 10).all()
    if (~same).any():
        d = np.abs(shop[0][:, None] - shop[0][None, :])[~same]
        assert (tt[:, ~same] >= 10 * d).all() and (tt[:, ~same] <= 20 * d).all()
    assert np.array_equal(shop[0], np.minimum(np.arange(M) // (M // E), E - 1)) and (shop == shop[0]).all()
    # a shard is its rows of the whole set; seed and scope matter
    t2, p2, tt2, _ = ref.generate(B + 3, J, M, E, 5)
    assert np.array_equal(t2[3:], t) and np.array_equal(p2[3:], p) and np.array_equal(tt2[3:], tt)
    assert not np.array_equal(ref.generate(B, J, M, E, 6, first_instance=3)[0], t)
    assert not np.array_equal(ref.generate(B, J, M, E, 5 + (1 << 32), first_instance=3)[0], t)
    t3 = ref.generate(B, J, M, E, 5, first_instance=3, scope=dict(t_low=10, t_high=20))[0]
    assert (np.abs(t3) >= 8).all() and (np.abs(t3) <= 24).all()


def test_generator_infeasible_sets_are_uniform():
    J, M, E, B = 6, 6, 2, 2000
    t = ref.generate(B, J, M, E, 9)[0]
    nbad = (t < 0).sum(-1).ravel()
    hist = np.bincount(nbad, minlength=M) / nbad.size
    assert np.abs(hist - 1.0 / M).max() < 0.01                                     # k uniform on [0, M)
    which = (t < 0).mean((0, 1))
    assert np.abs(which - which.mean()).max() < 0.01                               # every machine equally likely


def test_random_actions_model_picks_valid_actions_uniformly():
    rs = np.random.RandomState(3)
    B, J, M = 4000, 6, 5
    T = J * M
    t = rs.uniform(1, 9, (B, T, M))
    t[rs.uniform(size=t.shape) < 0.4] *= -1
    t[..., 0] = np.abs(t[..., 0])
    cand = (np.arange(J) * M)[None] + rs.randint(0, M, (B, J))
    jmask = (rs.uniform(size=(B, J)) < 0.5).astype(np.uint8)
    jmask[:, 2] = 0
    jmask[:5] = 1; jmask[:5, 4] = 0                                                # one job left: it must be taken
    a, m, j = ref.random_actions(t, cand, jmask, 3, 77)
    assert (jmask[np.arange(B), j] == 0).all() and np.array_equal(a, cand[np.arange(B), j]) and (t[np.arange(B), a, m] >= 0).all()
    assert (j[:5] == 4).all()
    # rank of the drawn job among the unmasked ones is uniform: mean of (rank + 0.5) / n is 1/2
    rank = (np.cumsum(jmask == 0, 1) - 1)[np.arange(B), j]
    n = (jmask == 0).sum(1)
    assert abs(((rank + 0.5) / n).mean() - 0.5) < 0.02


@pytest.mark.parametrize("J,M", [(6, 6), (10, 10), (2, 3), (1, 4)])
def test_mor_order_is_a_permutation_per_column(J, M):
    B = 500
    o = ref.mor_order(B, J, M, 4)
    assert o.shape == (B, M, J) and np.array_equal(np.sort(o, 2), np.broadcast_to(np.arange(J), o.shape))
    if J > 2:
        assert not np.array_equal(o, ref.mor_order(B, J, M, 5)) and not np.array_equal(o, ref.mor_order(B, J, M, 4 + (1 << 32)))
        first = np.bincount(o[:, :, 0].ravel(), minlength=J) / (B * M)
        assert np.abs(first - 1.0 / J).max() < 0.03                               # every job equally likely to come first
