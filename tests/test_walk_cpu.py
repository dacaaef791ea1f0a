"""CPU: the host model of mtfjsp_walk_accept and baselines.walk_search (tests/walk_ref.py).  `accept` is pinned on hand-written rows, one
assertion per clause of the rule in include/mtfjsp.h; the constructed cases of `synthetic` are shown to produce the events the GPU test
runs them for; and the searches the GPU test compares are shown to step uphill, to be barred by the ring, to accept through the late
ring, to beat hill climbing somewhere — and, with everything switched off, to BE the hill climbing of tests/plan_moves_ref.py."""
import functools
from importlib import import_module

import numpy as np
import pytest

import plan_moves_ref as pref
import walk_ref as ref

INF = np.inf
K, ROUNDS, SEED = 8, 24, 11
SHAPES = {"J2M2": (2, 2, 2, 3), "J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _one(objs, sigs, slack=None, state=None, first=None, round=0, late_len=0, tabu_len=0, T=2):
    """one group: objs (None: not done), sigs per copy -> (out, state'); the plans are task[s][c] = 10 c + s, mach = -task"""
    k = len(objs)
    call = ref._call(1, k, {c: (objs[c], None if sigs is None else sigs[c]) for c in range(k)}, slack)
    task = (10 * np.arange(k)[None, :] + np.arange(T)[:, None]).astype(np.int32)
    st = ref.new_state(1, T, late_len, tabu_len) if state is None else state
    return ref.accept(call["cost4"], call["done"], call["w"], 1, k, None if sigs is None else call["sig"], task, -task, round,
                      (state is None) if first is None else first, slack, st)


# ---------------------------------------------------------------- the rule, clause by clause
def test_objectives_are_the_group_reductions():
    import group_reduce_ref as gref
    cost4, done = gref.synthetic("scattered", 3, 9, 4)
    sig = np.arange(27, dtype=np.uint64)
    plan = np.zeros((2, 27), np.int32)
    out, _ = ref.accept(cost4, done, ref.CONFIG_W, 3, 9, sig, plan, plan, 0, True, None, ref.new_state(3, 2, 0, 0))
    assert _bits(out["obj"]).tolist() == _bits(gref.group_reduce(cost4, done, ref.CONFIG_W, 3, 9)[0]).tolist()


def test_first_call_fills_the_state_and_reads_none_of_it():
    out, st = _one([100.0, 200.0, 300.0], [1, 2, 3], late_len=3, tabu_len=2)
    assert st["late"].tolist() == [[100.0] * 3] and st["tabu_n"].tolist() == [0] and st["best_obj"].tolist() == [100.0]
    assert st["tabu"].tolist() == [[ref.SENT_U] * 2], "no move: the ring's cells stay as they were"
    assert st["best_task"][:, 0].tolist() == [0, 1] and st["best_mach"][:, 0].tolist() == [0, -1], "column n*K, word for word"
    assert out["why"].tolist() == [1] and out["pick"].tolist() == [1] and out["next_col"].tolist() == [0]
    assert out["cur_obj"].tolist() == [100.0] and out["best_obj"].tolist() == [100.0] and out["barred"].tolist() == [0]


def test_why_0_no_candidate():
    for objs in ([100.0], [100.0, None, None]):
        out, _ = _one(objs, list(range(len(objs))), slack=INF)
        assert out["why"].tolist() == [0] and out["pick"].tolist() == [-1] and out["next_col"].tolist() == [0]


def test_why_2_strictly_better_and_plus_8_for_a_new_best():
    out, st = _one([100.0, 90.0, 80.0, 80.0], [1, 2, 3, 4])
    assert out["why"].tolist() == [2 + 8] and out["pick"].tolist() == [2], "the lowest of the equal minima"
    assert out["next_col"].tolist() == [2] and out["cur_obj"].tolist() == [80.0] and out["best_obj"].tolist() == [80.0]
    assert st["best_obj"].tolist() == [80.0] and st["best_task"][:, 0].tolist() == [20, 21] and st["best_mach"][:, 0].tolist() == [-20, -21]


def test_why_1_refused_with_everything_off():
    for slack in (None, -1.0, np.nan):
        out, st = _one([100.0, 100.0, 120.0], [1, 2, 3], slack=slack)
        assert out["why"].tolist() == [1] and out["pick"].tolist() == [1] and out["next_col"].tolist() == [0] and out["cur_obj"].tolist() == [100.0]
        assert st["best_task"][:, 0].tolist() == [0, 1]


def test_why_3_within_the_slack_no_new_best():
    out, st = _one([100.0, 100.0, 120.0], [1, 2, 3], slack=0.0)
    assert out["why"].tolist() == [3] and out["next_col"].tolist() == [1], "a sideways step is no new best"
    out, st = _one([100.0, 130.0, 120.0], [1, 2, 3], slack=20.0)
    assert out["why"].tolist() == [3] and out["pick"].tolist() == [2] and out["cur_obj"].tolist() == [120.0] and out["best_obj"].tolist() == [100.0]
    assert st["best_obj"].tolist() == [100.0] and st["best_task"][:, 0].tolist() == [0, 1], "the best plan stays"
    assert _one([100.0, 130.0, 120.0], [1, 2, 3], slack=19.0)[0]["why"].tolist() == [1]
    assert _one([100.0, 130.0, 1e300], [1, 2, 3], slack=INF)[0]["why"].tolist() == [3]


def test_why_4_through_the_late_ring_and_its_update():
    _, st = _one([100.0, 90.0], [1, 2], late_len=2)                     # round 0: late = [90, 100]
    assert st["late"].tolist() == [[90.0, 100.0]], "filled with cur, then the round's entry takes the new cur"
    out, st2 = _one([90.0, 95.0], [2, 3], state=st, round=1)            # against late[1] = 100
    assert out["why"].tolist() == [4] and out["cur_obj"].tolist() == [95.0] and st2["late"].tolist() == [[90.0, 95.0]]
    out, st3 = _one([95.0, 99.0], [3, 4], state=st2, round=2)           # round 2 wraps to late[0] = 90
    assert out["why"].tolist() == [1] and st3["late"].tolist() == [[95.0, 95.0]], "the entry is written when the walk stays, too"
    out, _ = _one([90.0, 100.0], [2, 3], state=st, round=1)
    assert out["why"].tolist() == [4], "<= : equal to the entry is accepted"
    out, _ = _one([90.0, 95.0], [2, 3], state=st, round=2)
    assert out["why"].tolist() == [1], "round % late_len picks the entry"


def test_plus_8_only_below_the_best():
    _, st = _one([100.0, 90.0], [1, 2])
    out, st = _one([95.0, 92.0], [3, 4], state=st)                      # better than cur, not than the best
    assert out["why"].tolist() == [2] and out["best_obj"].tolist() == [90.0] and st["best_task"][:, 0].tolist() == [10, 11]
    out, st = _one([92.0, 89.0], [4, 5], state=st)
    assert out["why"].tolist() == [10] and st["best_obj"].tolist() == [89.0]


def test_the_same_schedule_filter():
    out, _ = _one([100.0, 50.0, 90.0], [7, 7, 8])
    assert out["pick"].tolist() == [2] and out["barred"].tolist() == [1], "the incumbent's own schedule again is no move"
    out, _ = _one([100.0, 50.0, 90.0], None)
    assert out["pick"].tolist() == [1] and out["barred"].tolist() == [0], "no signatures: no filter"
    out, _ = _one([100.0, None, 90.0], [7, 7, 7], slack=INF)
    assert out["why"].tolist() == [0] and out["barred"].tolist() == [1], "only copies with an objective count as barred"


def test_the_ring_filter_and_the_ring_wrapping():
    _, st = _one([100.0, 90.0], [1, 2], tabu_len=2)
    assert st["tabu"].tolist() == [[1, ref.SENT_U]] and st["tabu_n"].tolist() == [1], "the schedule being left"
    out, st = _one([90.0, 50.0, 95.0], [2, 1, 3], slack=INF, state=st)
    assert out["pick"].tolist() == [2] and out["barred"].tolist() == [1] and st["tabu"].tolist() == [[1, 2]] and st["tabu_n"].tolist() == [2]
    out, st = _one([95.0, 50.0, 60.0, 96.0], [3, 1, 2, 4], slack=INF, state=st)
    assert out["pick"].tolist() == [3] and out["barred"].tolist() == [2]
    assert st["tabu"].tolist() == [[3, 2]] and st["tabu_n"].tolist() == [3], "the third move wraps to entry 0"
    out, st = _one([96.0, 50.0, 60.0], [4, 1, 2], slack=INF, state=st)
    assert out["pick"].tolist() == [1] and out["barred"].tolist() == [1], "1 has left the ring and is admitted again; 2 is still in it"
    _, st = _one([100.0, 90.0], [1, 2], tabu_len=2)
    out, _ = _one([90.0, 50.0], [2, ref.SENT_U], slack=INF, state=st)
    assert out["pick"].tolist() == [1], "only the first min(tabu_n, tabu_len) entries are valid"


def test_a_dead_incumbent():
    out, st = _one([None, 300.0, None], [1, 2, 3])
    assert out["why"].tolist() == [2 + 8] and out["next_col"].tolist() == [1] and st["best_obj"].tolist() == [300.0], "cur NaN: any candidate is better"
    out, st = _one([None, None], [1, 2], slack=INF)
    assert out["why"].tolist() == [0] and out["next_col"].tolist() == [-1] and np.isnan(out["cur_obj"]).all() and np.isnan(st["best_obj"]).all()
    assert st["best_task"][:, 0].tolist() == [0, 1], "the first call copies column n*K whatever it holds"


def test_values_are_the_copys_own_word():
    out, _ = _one([0.0, -0.0], [1, 2], slack=None)
    assert out["why"].tolist() == [1] and _bits(out["cur_obj"]).tolist() == _bits([0.0]).tolist()
    out, _ = _one([0.0, -0.0], [1, 2], slack=0.0)
    assert out["why"].tolist() == [3] and _bits(out["cur_obj"]).tolist() == _bits([-0.0]).tolist() and _bits(out["obj"]).tolist() == _bits([0.0, -0.0]).tolist()


# ---------------------------------------------------------------- the constructed cases show what they are there for
def _run(kind, k=65, late_len=2, tabu_len=3, n=3):
    return ref.run(ref.synthetic(kind, n, k, 5, late_len, tabu_len), n, k, 4, late_len, tabu_len, 5)[1:]


@pytest.mark.parametrize("k", [3, 65, 257])
def test_constructed_cases(k):
    last, n = k - 1, 3
    col = lambda c: [g * k + c for g in range(n)]                      # noqa: E731
    o, _ = _run("shared_min", k)
    assert o[0]["pick"].tolist() == [1] * n and o[0]["why"].tolist() == [10] * n
    o, _ = _run("last_min", k)
    assert o[0]["pick"].tolist() == [last] * n and o[0]["next_col"].tolist() == col(last)
    o, _ = _run("second", k)
    assert o[1]["pick"].tolist() == [last] * n and o[1]["barred"].tolist() == [1] * n and o[1]["why"].tolist() == [10] * n
    o, s = _run("all_barred", k)
    assert [x["why"].tolist() for x in o[1:]] == [[0] * n] * 2 and [x["barred"].tolist() for x in o[1:]] == [[k - 1] * n] * 2
    assert o[2]["next_col"].tolist() == col(0) and s[2]["tabu_n"].tolist() == [1] * n
    o, s = _run("dead0", k)
    assert o[0]["why"].tolist() == [10] * n and o[1]["why"].tolist() == [0] * n and o[1]["next_col"].tolist() == [-1] * n
    assert np.isnan(o[1]["cur_obj"]).all() and o[2]["why"].tolist() == [2] * n
    o, _ = _run("zeros", k, late_len=0)                                # (with a late ring the first call's entry is cur: equal is accepted, why 4)
    assert [x["why"].tolist() for x in o] == [[1] * n, [3] * n, [3] * n] and _run("zeros", k)[0][0]["why"].tolist() == [4] * n
    assert _bits(o[1]["cur_obj"]).tolist() == _bits([-0.0] * n).tolist() and _bits(o[2]["cur_obj"]).tolist() == _bits([0.0] * n).tolist()
    o, _ = _run("nan_obj", k)
    assert o[0]["why"].tolist() == [0] * n and np.isnan(o[0]["obj"][1::k]).all() and o[1]["pick"].tolist() == [last if k > 2 else -1] * n
    o, _ = _run("slack_edge", k)
    assert [x["why"].tolist() for x in o] == [[3] * n, [1] * n, [3] * n]
    o, s = _run("late_only", k)
    assert o[1]["why"].tolist() == [4] * n and o[1]["cur_obj"].tolist() == [95.0 + 1000 * g for g in range(n)] and o[2]["why"].tolist() == [1] * n
    assert _run("late_only", k, late_len=1)[0][1]["why"].tolist() == [1] * n and _run("late_only", k, late_len=5)[0][2]["why"].tolist() == [4] * n
    o, s = _run("no_new_best", k)
    assert o[1]["why"].tolist() == [3] * n and np.array_equal(s[1]["best_task"], s[0]["best_task"]) and np.array_equal(s[1]["best_obj"], s[0]["best_obj"])
    for u in (1, 3, 64):
        o, s = _run("readmit", k, tabu_len=u)
        assert [x["pick"].tolist() for x in o[1:]] == [[last] * n] * u + [[1] * n] and [x["barred"].tolist() for x in o[1:]] == [[1] * n] * u + [[0] * n]
        assert s[-1]["tabu_n"].tolist() == [u + 2] * n, "the ring has wrapped"


@pytest.mark.parametrize("tabu_len,late_len", [(1, 1), (3, 2), (64, 5)])
def test_random_sequences_wrap_both_rings_and_hit_them(tabu_len, late_len):
    calls = max(2 * late_len + 1, tabu_len + 2) + 8
    _, outs, states = ref.run(ref.synthetic("random", 3, 64, 9, late_len, tabu_len, calls), 3, 64, 4, late_len, tabu_len, 9)
    assert (states[-1]["tabu_n"] > tabu_len + 1).all() and sum(int(o["barred"].sum()) for o in outs) > 0
    _, outs, _ = ref.run(ref.synthetic("random", 3, 64, 9, late_len, tabu_len), 3, 64, 4, late_len, tabu_len, 9)
    assert {1, 2, 3} <= {int(x) & 7 for o in outs for x in o["why"]}


# ---------------------------------------------------------------- the searches of the GPU tests
@functools.lru_cache(maxsize=None)
def _setup(shape):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = SHAPES[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M)
    return data, pref.first_feasible_plan(data[0])


@functools.lru_cache(maxsize=None)
def _walk(shape, tabu, slack, late):
    data, start = _setup(shape)
    trace = []
    return ref.search(data, start, K, ROUNDS, SEED, tabu=tabu, slack=slack, late=late, trace=trace), trace


def _steps(res):
    return np.diff(np.vstack([res["start_obj"][None], res["current"]]), axis=0)


@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_tabu_walks_uphill_and_is_barred_by_the_ring(shape):
    res, trace = _walk(shape, 8, INF, 0)
    N = res["history"].shape[1]
    assert (_steps(res) > 0).any(), "current rises somewhere"
    assert (np.diff(np.vstack([res["start_obj"][None], res["history"]]), axis=0) <= 0).all(), "history never does"
    assert (res["history"] <= res["current"]).all() and _bits(res["obj"]).tolist() == _bits(res["history"][-1]).tolist()
    by_ring = sum(1 for rec in trace for n in range(N) for c in range(1, K)
                  if rec["obj"][n * K + c] == rec["obj"][n * K + c] and rec["sig"][n * K + c] != rec["sig"][n * K] and rec["sig"][n * K + c] in rec["ring"][n])
    assert by_ring > 0, "a candidate barred by the ring, not only by the same-schedule test"
    assert res["barred"].sum() > by_ring, "and the incumbent's own schedule does come again"


@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_late_acceptance_accepts_uphill_steps(shape):
    res, _ = _walk(shape, 0, None, 4)
    assert (((res["why"] & 7) == 4) & (_steps(res) > 0)).any()
    assert (np.diff(res["history"], axis=0) <= 0).all()


def test_tabu_ends_below_hill_climbing_somewhere():
    data, start = _setup("J3M4")
    hill = pref.search(data, start, K, ROUNDS, SEED)
    assert (_walk("J3M4", 8, INF, 0)[0]["history"][-1] < hill["history"][-1]).any()


def test_small_instances_run_out_of_schedules():
    """J2M2: 4 operations — the neighbourhood is so small that the ring bars all of it, and schedules come back after eviction"""
    res, trace = _walk("J2M2", 8, INF, 0)
    N = res["history"].shape[1]
    assert (res["why"] == 0).any() and (res["barred"][res["why"] == 0] > 0).all(), "why == 0: everything barred"
    left, again = [[] for _ in range(N)], 0
    for r, rec in enumerate(trace):
        for n in range(N):
            if (res["why"][r, n] & 7) >= 2:
                again += rec["sig"][rec["next_col"][n]] in left[n][:-8]
                left[n].append(rec["sig"][n * K])
    assert again > 0, "an entry that left the ring is picked again"


@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_everything_off_is_the_hill_climbing(shape):
    data, start = _setup(shape)
    res, hill = _walk(shape, 0, None, 0)[0], pref.search(data, start, K, ROUNDS, SEED)
    assert _bits(res["history"]).tolist() == _bits(hill["history"]).tolist() and _bits(res["current"]).tolist() == _bits(hill["history"]).tolist()
    assert np.array_equal(res["accepted"], hill["accepted"]) and _bits(res["start_obj"]).tolist() == _bits(hill["start_obj"]).tolist()
    assert np.array_equal(res["plans"][0], hill["plans"][0]) and np.array_equal(res["plans"][1], hill["plans"][1])
    assert set(np.unique(res["why"] & 7).tolist()) <= {0, 1, 2}
