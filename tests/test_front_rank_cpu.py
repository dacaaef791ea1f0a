"""CPU: the host model of mtfjsp_front_rank, mtfjsp_plan_survivors and baselines.evolve_pareto (tests/nsga_ref.py) against hand-made groups
whose ranks and crowding distances are worked out here, a candidate-by-candidate restatement of the header's rule that shares no code
with it, the ranks restated as longest dominance chains, invariants on synthetic data, and what the model search must show at the
shapes and seeds of tests/test_evolve_gpu.py; baselines.hypervolume on hand cases."""
import functools
import math
from importlib import import_module

import numpy as np
import pytest

import group_reduce_ref as gref
import nsga_ref as ref
import plan_moves_ref as mref

INF = float("inf")
W = (0.5, 0.5, 0.0)                      # exact in binary64: obj = (mk + ec) / 2


def _c4(points):
    """(mk, ec, tt) rows -> cost4 rows (makespan, energy, transport, idle) with all of ec in the energy"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    return np.stack([pts[:, 0], pts[:, 1], pts[:, 2], np.zeros(len(pts))], 1)


def _rank1(points, w=W, done=None):
    c4 = _c4(points)
    done = np.ones(len(c4), np.uint8) if done is None else np.asarray(done, np.uint8)
    return ref.front_rank(c4, done, None, None, w, 1)


def _same_values(got, want, tag):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, tag
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{tag}: NaNs at {np.isnan(got).tolist()} against {np.isnan(want).tolist()}"
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), f"{tag}: {got.tolist()} against {want.tolist()}"


# ---------------------------------------------------------------- hand-made groups
def test_textbook_five_points():
    """rank 0 = {0, 1, 2, 3}, candidate 4 = (5, 5) is dominated by 1 = (2, 4).  mk ascending 1, 2, 4, 8: the ends +inf, candidate 1
    (4 - 1) / 7, candidate 2 (8 - 2) / 7; ec ascending 1, 2, 4, 8 is candidates 3, 2, 1, 0: candidate 2 (4 - 1) / 7, candidate 1
    (8 - 2) / 7; tt is flat, so its order is the index: 0 and 3 are the ends, 1 and 2 get 0.0.  obj = 4.5, 3, 3, 4.5, 5: the rank's
    best is candidate 1 (the lower of two equal ones), which becomes +inf.  Candidate 4 is alone in rank 1: +inf."""
    rank, crowd, order, size, best = _rank1([(1, 8, 0), (2, 4, 0), (4, 2, 0), (8, 1, 0), (5, 5, 0)])
    assert rank.tolist() == [0, 0, 0, 0, 1]
    assert crowd.tolist() == [INF, INF, (6 / 7 + 3 / 7) + 0.0, INF, INF]
    assert order.tolist() == [0, 1, 3, 2, 4]
    assert size.tolist() == [4] and best.tolist() == [3.0]
    # without the addition candidate 1 would have had the distance of candidate 2, and the lower index
    assert (3 / 7 + 6 / 7) + 0.0 == (6 / 7 + 3 / 7) + 0.0


def test_chain():
    """a total order: every candidate is a rank of its own, in the order of its costs, and a one-member rank has no neighbours"""
    vals = [3, 0, 4, 1, 2]
    rank, crowd, order, size, best = _rank1([(v, v, v) for v in vals])
    assert rank.tolist() == vals
    assert crowd.tolist() == [INF] * 5
    assert order.tolist() == [1, 3, 4, 0, 2]
    assert size.tolist() == [1] and best.tolist() == [0.0]


def test_antichain_on_a_plane():
    """mk + ec + tt = 6 on a grid: nothing dominates anything, one rank; the distances are the restatement's"""
    pts = [(i, j, 6 - i - j) for i in range(4) for j in range(4)]
    rank, crowd, order, size, best = _rank1(pts)
    assert rank.tolist() == [0] * 16 and size.tolist() == [16]
    b = brute_group(_c4(pts), np.ones(16, np.uint8), W)
    _same_values(crowd, b[1], "crowd")
    assert order.tolist() == b[2]
    assert sorted(order.tolist()) == list(range(16))
    assert np.isinf(crowd).sum() <= 7, "two ends per axis and the best objective"
    # (0, 0, 6): obj 0, the lowest of all
    assert best.tolist() == [0.0] and crowd[0] == INF


def test_exact_duplicates_fall_to_later_ranks():
    rank, crowd, order, size, best = _rank1([(1, 1, 1), (0, 2, 1), (1, 1, 1), (1, 1, 1)])
    assert rank.tolist() == [0, 0, 1, 2]
    assert crowd.tolist() == [INF] * 4                                  # a two-member rank and two one-member ranks
    assert order.tolist() == [0, 1, 2, 3] and size.tolist() == [2]


def test_flat_axes_and_small_ranks():
    """all three axes flat is impossible inside one rank (duplicates fall); two flat axes: mk = tt = 0 would order by ec alone, a chain.
    One flat axis with three members: the middle one by index gets 0.0 there"""
    rank, crowd, order, size, best = _rank1([(1, 3, 7), (2, 2, 7), (3, 1, 7)], w=(1.0, 0.0, 0.0))
    assert rank.tolist() == [0, 0, 0]
    assert crowd.tolist() == [INF, (1.0 + 1.0) + 0.0, INF]
    assert order.tolist() == [0, 2, 1]
    one = _rank1([(4, 4, 4)])
    assert one[0].tolist() == [0] and one[1].tolist() == [INF] and one[2].tolist() == [0] and one[3].tolist() == [1]
    two = _rank1([(1, 2, 0), (2, 1, 0)])
    assert two[0].tolist() == [0, 0] and two[1].tolist() == [INF, INF] and two[2].tolist() == [0, 1]


def test_infinite_cost_gives_nan_crowd_and_nan_obj():
    """mk = 1, 2, inf: the middle candidate's d_mk = (inf - 1) / (inf - 1) = NaN, d_ec = (3 - 1) / (3 - 1) = 1, d_tt = 0: NaN, which
    comes after every number in the order"""
    pts = [(1, 3, 0), (2, 2, 0), (INF, 1, 0)]
    rank, crowd, order, size, best = _rank1(pts)                       # obj = 2, 2, inf: the best is candidate 0, an end anyway
    assert rank.tolist() == [0, 0, 0]
    assert crowd[0] == INF and crowd[2] == INF and math.isnan(crowd[1])
    assert order.tolist() == [0, 2, 1] and best.tolist() == [2.0]
    # w_mk = 0: obj of candidate 2 = 0 * inf = NaN, never the best; the best is candidate 1, whose NaN becomes +inf
    rank, crowd, order, size, best = _rank1(pts, w=(0.0, 1.0, 0.0))
    assert crowd.tolist() == [INF, INF, INF] and order.tolist() == [0, 1, 2] and best.tolist() == [2.0]
    # nothing but NaN objectives: nobody is the best
    rank, crowd, order, size, best = _rank1([(INF, 1, 0), (INF, 2, 0)], w=(0.0, 1.0, 0.0))
    assert rank.tolist() == [0, 1] and math.isnan(best[0])


def test_ineligible_candidates():
    rank, crowd, order, size, best = _rank1([(1, 1, 1), (0, 0, 0), (np.nan, 0, 0), (2, 2, 2)], done=[1, 0, 1, 7])
    assert rank.tolist() == [0, -1, -1, 1]
    assert crowd[0] == INF and crowd[3] == INF and math.isnan(crowd[1]) and math.isnan(crowd[2])
    assert order.tolist() == [0, 3, 1, 2] and size.tolist() == [1] and best.tolist() == [1.0]


def test_two_array_sets_are_one_group():
    """candidates c < Ka from a, the others from b: the same as the concatenated group"""
    c4, dn = gref.synthetic("scattered", 3, 10, 4)
    whole = ref.front_rank(c4, dn, None, None, W, 3)
    a, b = c4.reshape(3, 10, 4)[:, :4].reshape(-1, 4), c4.reshape(3, 10, 4)[:, 4:].reshape(-1, 4)
    da, db = dn.reshape(3, 10)[:, :4].reshape(-1), dn.reshape(3, 10)[:, 4:].reshape(-1)
    split = ref.front_rank(a, da, b, db, W, 3)
    for x, y in zip(whole, split):
        _same_values(x, y, "split")


# ---------------------------------------------------------------- the rule restated candidate by candidate
def brute_group(c4, done, w):
    """include/mtfjsp.h applied literally with Python floats -> (rank, crowd, order) lists of one group"""
    K = len(c4)
    mk, ec, tt, obj = gref.objectives(c4, w)
    pts = [(float(mk[c]), float(ec[c]), float(tt[c])) for c in range(K)]
    elig = [bool(done[c]) and not any(math.isnan(x) for x in pts[c]) for c in range(K)]
    ob = [float(obj[c]) if elig[c] else math.nan for c in range(K)]
    rank = [None if elig[c] else -1 for c in range(K)]
    r = 0
    while any(x is None for x in rank):
        left = [c for c in range(K) if rank[c] is None]
        for c in [c for c in left if not any(gref.dominates(pts[q], pts[c], q, c) for q in left if q != c)]:
            rank[c] = r
        r += 1
    crowd = [math.nan] * K
    for rr in range(r):
        mem = [c for c in range(K) if rank[c] == rr]
        for c in mem:
            d = []
            for a in range(3):
                below = [pts[q][a] for q in mem if (pts[q][a], q) < (pts[c][a], c)]
                above = [pts[q][a] for q in mem if (pts[q][a], q) > (pts[c][a], c)]
                lo, hi = min(pts[q][a] for q in mem), max(pts[q][a] for q in mem)
                if not below or not above:
                    d.append(INF)
                elif hi == lo:
                    d.append(0.0)
                else:
                    with np.errstate(all="ignore"):
                        d.append(float((np.float64(min(above)) - np.float64(max(below))) / (np.float64(hi) - np.float64(lo))))
            with np.errstate(all="ignore"):
                crowd[c] = float((np.float64(d[0]) + np.float64(d[1])) + np.float64(d[2]))
        numbers = [c for c in mem if not math.isnan(ob[c])]
        if numbers:
            crowd[min(numbers, key=lambda c: (ob[c], c))] = INF

    def before(q, c):
        if not elig[c]:
            return elig[q] or q < c
        if not elig[q]:
            return False
        if rank[q] != rank[c]:
            return rank[q] < rank[c]
        for x, y in ((q, c), (c, q)):
            if crowd[x] > crowd[y] or (not math.isnan(crowd[x]) and math.isnan(crowd[y])):
                return x == q
        return q < c

    order = sorted(range(K), key=lambda c: sum(1 for q in range(K) if q != c and before(q, c)))
    return rank, crowd, order


def longest_chain_ranks(c4, done, w):
    """the rank of a candidate = the length of the longest chain of candidates that dominate one another down to it"""
    K = len(c4)
    mk, ec, tt, _ = gref.objectives(c4, w)
    pts = [(float(mk[c]), float(ec[c]), float(tt[c])) for c in range(K)]
    elig = [bool(done[c]) and not any(math.isnan(x) for x in pts[c]) for c in range(K)]

    @functools.lru_cache(maxsize=None)
    def depth(c):
        return max([depth(q) + 1 for q in range(K) if q != c and elig[q] and gref.dominates(pts[q], pts[c], q, c)], default=0)

    return [depth(c) if elig[c] else -1 for c in range(K)]


@pytest.mark.parametrize("K", [1, 2, 7, 33])
@pytest.mark.parametrize("kind", ["integer", "random", "scattered", "none"])
def test_model_equals_the_restatement(kind, K):
    N = 3
    c4, dn = gref.synthetic(kind, N, K, 100 + K)
    rank, crowd, order, size, best = ref.front_rank(c4, dn, None, None, (0.4, 0.4, 0.2), N)
    for n in range(N):
        g = slice(n * K, (n + 1) * K)
        b = brute_group(c4[g], dn[g], (0.4, 0.4, 0.2))
        assert rank[g].tolist() == b[0]
        _same_values(crowd[g], b[1], f"{kind} K={K} group {n}: crowd")
        assert order[g].tolist() == b[2]
        assert rank[g].tolist() == longest_chain_ranks(c4[g], dn[g], (0.4, 0.4, 0.2))


@pytest.mark.parametrize("K", [1, 5, 64, 300])
@pytest.mark.parametrize("kind", ["integer", "random", "scattered", "none"])
def test_invariants(kind, K):
    N, w = 3, (0.4, 0.4, 0.2)
    c4, dn = gref.synthetic(kind, N, K, 7 + K)
    rank, crowd, order, size, best = ref.front_rank(c4, dn, None, None, w, N)
    obj, _, best_obj, front = gref.group_reduce(c4, dn, w, N, K)
    assert np.array_equal(rank == 0, front == 1), "rank 0 is group_reduce's front"
    assert np.array_equal(size, front.reshape(N, K).sum(1))
    _same_values(best, best_obj, "best_obj is group_reduce's")
    assert np.array_equal(rank < 0, np.isnan(obj)) and np.array_equal(rank < 0, np.isnan(crowd) & (rank < 0))
    for n in range(N):
        o, rk = order[n * K:(n + 1) * K], rank[n * K:(n + 1) * K]
        assert sorted(o.tolist()) == list(range(K)), "order is a permutation"
        along = rk[o]
        n_el = int((rk >= 0).sum())
        assert (along[:n_el] >= 0).all() and (along[n_el:] < 0).all(), "ineligible candidates come last"
        assert (np.diff(along[:n_el]) >= 0).all(), "ranks along the order never fall"
        for r in range(rk.max() + 1):
            assert np.isinf(crowd[n * K:(n + 1) * K][rk == r]).sum() <= 7


def test_survivors_model():
    N, Ka, Kb, P, T = 2, 3, 2, 4, 5
    rs = np.random.RandomState(3)
    ta, ma = rs.randint(0, 9, (N * Ka, T)).astype(np.int32), rs.randint(0, 9, (N * Ka, T)).astype(np.int32)
    tb, mb = rs.randint(0, 9, (N * Kb, T)).astype(np.int32), rs.randint(0, 9, (N * Kb, T)).astype(np.int32)
    ca, cb = rs.uniform(size=(N * Ka, 4)), rs.uniform(size=(N * Kb, 4))
    da, db = np.ones(N * Ka, np.uint8), np.array([1, 0, 1, 1], np.uint8)
    rank, _, order, _, _ = ref.front_rank(ca, da, cb, db, W, N)
    order = order.copy()
    order[5 + 1] = 5                                                    # group 1, position 1: an entry outside [0, K)
    t, m, c4, dn, rk, src, fit = ref.survivors(order, rank, P, N, ta, ma, ca, da, tb, mb, cb, db)
    for n in range(N):
        for i in range(P):
            g, c = n * P + i, order[n * 5 + i]
            assert src[g] == c
            if c == 5:
                assert (t[g] == -1).all() and (m[g] == -1).all() and dn[g] == 0 and rk[g] == -1 and math.isnan(fit[g]) and np.isnan(c4[g]).all()
                continue
            want = (ta[n * Ka + c], ma[n * Ka + c], ca[n * Ka + c], da[n * Ka + c]) if c < Ka else (tb[n * Kb + c - Ka], mb[n * Kb + c - Ka], cb[n * Kb + c - Ka], db[n * Kb + c - Ka])
            assert t[g].tolist() == want[0].tolist() and m[g].tolist() == want[1].tolist() and c4[g].tolist() == want[2].tolist() and dn[g] == want[3]
            assert rk[g] == rank[n * 5 + c]
            assert (fit[g] == float(i)) if rk[g] >= 0 else math.isnan(fit[g])
    # group 0 has the ineligible candidate 4 (element 1 of b): the last of its order, outside the first P
    assert order[4] == 4 and rank[4] == -1


# ---------------------------------------------------------------- the model search
SHAPES = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}                  # tests/test_evolve_gpu.py's shapes, seeds and starts
CONFIG_W = (0.4, 0.4, 0.2)
P, GENS, SEED, STARTS = 8, 3, 11, 3


@functools.lru_cache(maxsize=None)
def _setup(shape):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = SHAPES[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M)
    starts = [mref.random_plans(np.asarray(data[0]), J, M, 60 + c) for c in range(STARTS)]
    return data, starts


@functools.lru_cache(maxsize=None)
def _search(shape, left_shift):
    data, starts = _setup(shape)
    return ref.search(data, starts, P, GENS, SEED, left_shift=left_shift, w=CONFIG_W)


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_model_search(shape, left_shift):
    data, starts = _setup(shape)
    res = _search(shape, left_shift)
    N = SHAPES[shape][3]
    start_objs = np.stack([mref.replay(data, s[0], s[1], left_shift, CONFIG_W)[3] for s in starts])
    assert np.array_equal(res["start_obj"], start_objs.min(0)), "start_obj is the best start's Objective"
    hist = np.vstack([res["start_obj"][None], res["history"]])
    assert (np.diff(hist, axis=0) <= 0).all(), "the best Objective never rises"
    assert (res["history"] <= start_objs.min(0)[None]).all()
    assert np.array_equal(res["obj"], hist[-1]), "the replayed best member has the last generation's Objective"
    sizes = []
    for n in range(N):
        f = res["fronts"][n]
        F = len(f["obj"])
        assert 1 <= F <= P and f["cost"].shape == (F, 3) and f["task"].shape == (F, data[0].shape[1])
        for a in range(F):
            for b in range(F):
                assert a == b or not gref.dominates(f["cost"][a], f["cost"][b], a, b), "a front is mutually non-dominated"
        assert res["obj"][n] == f["obj"].min()
        # every front plan replays to its own costs
        _, f4, done, obj = mref.replay(tuple(np.repeat(np.asarray(x)[n:n + 1], F, axis=0) for x in data), f["task"], f["mach"], left_shift, CONFIG_W)
        assert done.all() and np.array_equal(f4, f["final4"]) and np.array_equal(obj, f["obj"])
        sizes.append(F)
    assert max(sizes) >= 2, f"at least one instance ends with two or more front members: {sizes}"
    assert res["front_size"].shape == (GENS + 1, N) and (res["front_size"] >= 1).all()


# ---------------------------------------------------------------- hypervolume
def test_hypervolume_hand_cases():
    import mtfjsp_amd  # noqa: F401
    hv = import_module("e2e-mappo-for-mt-fjsp_amd.baselines").hypervolume
    assert hv(np.zeros((0, 3)), (1, 1, 1)) == 0.0
    assert hv([(1, 1, 1)], (2, 2, 2)) == 1.0
    assert hv([(0, 0, 0)], (2, 3, 4)) == 24.0
    assert hv([(0, 1, 1), (1, 0, 1)], (2, 2, 2)) == 3.0                 # 2 + 2 - 1
    assert hv([(0, 1, 1), (1, 0, 1), (1, 1, 0)], (2, 2, 2)) == 4.0      # 3 x 2 - 3 x 1 + 1
    assert hv([(1, 1, 1), (1, 1, 1), (1.5, 1.5, 1.5)], (2, 2, 2)) == 1.0    # a duplicate and a dominated point
    assert hv([(1, 1, 2), (3, 0, 0)], (2, 2, 2)) == 0.0                 # on or beyond the reference point
    rs = np.random.RandomState(0)
    for F in (1, 2, 5, 12):
        pts = rs.randint(0, 6, (F, 3)).astype(np.float64)
        assert hv(pts, (6, 7, 8)) == ref.hypervolume(pts, (6.0, 7.0, 8.0))
