"""CPU: the host model of mtfjsp_plan_offspring and of baselines.evolve (tests/plan_crossover_ref.py) is itself right — the crossover
on a hand-worked example and at its two ends, every child of valid parents a valid plan, the tournament's rule with NaNs and ties, both
thresholds at 0 and 2^32, the elite word for word, parents that are no plans, the bit addressing past one Philox block — and the
library declares and exports the entry point and refuses a call without a handle."""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest

import plan_crossover_ref as ref
import plan_moves_ref as mref

SHAPES = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}
CONFIG_W = (0.4, 0.4, 0.2)
P, SEED, GEN, FIRST = 6, (1 << 41) + 5, 2, 7
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def population(shape):
    """N instances and P random valid plans of each -> (data, task [N*P,T], mach [N*P,T], (J, M, E, N))"""
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = SHAPES[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M, native=False)
    t = np.asarray(data[0])
    plans = [mref.random_plans(t, J, M, 40 + c) for c in range(P)]
    task = np.stack([x[0] for x in plans], 1).reshape(N * P, J * M)
    mach = np.stack([x[1] for x in plans], 1).reshape(N * P, J * M)
    return data, task, mach, (J, M, E, N)


def assert_valid_plan(t_n, task, mach, J, M, tag):
    T = J * M
    assert sorted(task) == list(range(T)), tag + ": every task once (every job M times)"
    nxt = [0] * J
    for a in task:
        assert a % M == nxt[a // M], tag + ": the operations of a job in order"
        nxt[a // M] += 1
    assert all(0 <= m < M and t_n[a][m] >= 0 for a, m in zip(task, mach)), tag + ": feasible machines"


def test_pox_by_hand():
    # A = 0 1 2 0 1 2, B = 2 2 1 1 0 0, S = {1}: the 1s stay where A has them; the holes 0, 2, 3, 5 take B without its 1s: 2 2 0 0
    assert ref.pox([0, 1, 2, 0, 1, 2], [2, 2, 1, 1, 0, 0], [False, True, False]) == [2, 1, 2, 0, 1, 0]
    # S = {0, 2}: only position 1 and 4 are holes, and B without 0 and 2 is 1 1
    assert ref.pox([0, 1, 2, 0, 1, 2], [2, 2, 1, 1, 0, 0], [True, False, True]) == [0, 1, 2, 0, 1, 2]
    # the order of B among the jobs outside S is kept, and the places of A's jobs inside S
    assert ref.pox([0, 0, 1, 1, 2, 2], [2, 1, 0, 2, 1, 0], [True, False, False]) == [0, 0, 2, 1, 2, 1]
    assert ref.pox([0, 0, 1, 1], [0, 1, 1, 1], [True, False]) is None, "a fill that runs long"
    assert ref.pox([0, 0, 1, 1], [0, 0, 0, 1], [True, False]) is None, "a fill that runs short"


def test_pox_ends_all_jobs_give_a_and_no_job_gives_b():
    qa, qb = [0, 1, 2, 2, 1, 0, 1, 0, 2], [2, 2, 2, 1, 1, 1, 0, 0, 0]
    assert ref.pox(qa, qb, [True] * 3) == qa
    assert ref.pox(qa, qb, [False] * 3) == qb
    # through `child`: the machines follow their own coins, whatever S is
    M, T = 3, 9
    t_n = [[1.0] * M for _ in range(T)]
    A, B = mref.decode(qa, {a: 0 for a in range(T)}, M), mref.decode(qb, {a: 1 for a in range(T)}, M)
    coins = [a % 2 == 0 for a in range(T)]
    task, mach, kind = ref.child(t_n, A, B, [True] * 3, coins, None, 7, M)
    assert task == A[0] and kind == 0 and mach == [0 if a % 2 == 0 else 1 for a in task]
    task, mach, _ = ref.child(t_n, A, B, [False] * 3, coins, None, 7, M)
    assert task == B[0] and mach == [0 if a % 2 == 0 else 1 for a in task]
    task, mach, _ = ref.child(t_n, A, None, None, None, None, 7, M)
    assert (task, mach) == A, "no crossover: the child is A"


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("moves", [1, 2, 4, 7])
def test_children_of_valid_parents_are_valid_plans(shape, moves):
    data, task, mach, (J, M, E, N) = population(shape)
    t, T = np.asarray(data[0]), J * M
    obj = np.random.RandomState(1).rand(N * P)
    thr = 3 << 30
    ot, om, par, kind = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, thr, thr, moves)
    crossed = mutated = changed = 0
    for g in range(N * P):
        n, c = divmod(g, P)
        assert_valid_plan(t[n].tolist(), ot[g].tolist(), om[g].tolist(), J, M, f"{shape} child {g}")
        a, b = par[g]
        assert n * P <= a < (n + 1) * P and (b == -1 or n * P <= b < (n + 1) * P)
        v = ref.words(SEED, GEN, FIRST + n, c, ref.TAG_CROS)
        assert (b >= 0) == (v[0] < thr) and (kind[g] != 0) == (v[1] < thr)
        assert kind[g] == 0 or (kind[g] & moves and kind[g] in (1, 2, 4))
        crossed += b >= 0
        mutated += kind[g] != 0
        if b < 0 and kind[g] == 0:
            assert ot[g].tolist() == task[a].tolist() and om[g].tolist() == mach[a].tolist(), "neither event: the child is A"
        if b >= 0 and kind[g] == 0:
            # every task's machine is one of its parents'; jobs inside S sit where A has them
            mua, mub, muc = dict(zip(task[a], mach[a])), dict(zip(task[b], mach[b])), dict(zip(ot[g], om[g]))
            coins = ref.stream_bits(SEED, GEN, FIRST + n, c, ref.TAG_MACH, T)
            assert all(muc[x] == (mua[x] if coins[x] else mub[x]) for x in range(T))
            in_s = ref.stream_bits(SEED, GEN, FIRST + n, c, ref.TAG_JSET, J)
            qa, qb, qc = task[a] // M, task[b] // M, ot[g] // M
            assert all(qc[s] == qa[s] for s in range(T) if in_s[qa[s]])
            assert [j for j in qc if not in_s[j]] == [j for j in qb if not in_s[j]]
            changed += not np.array_equal(qc, qa)
    assert 0 < crossed < N * P and 0 < mutated < N * P and changed > 0, "both events and their absence are drawn"


def test_tournament_rule():
    obj = [3.0, NAN, 1.0, 1.0, NAN, 2.0]
    assert ref.better(obj, 0, 2) == 2 and ref.better(obj, 2, 0) == 2, "the smaller objective"
    assert ref.better(obj, 1, 0) == 0 and ref.better(obj, 0, 1) == 0 and ref.better(obj, 4, 5) == 5, "a NaN loses to any number"
    assert ref.better(obj, 3, 2) == 2 and ref.better(obj, 2, 3) == 2, "equal values: the lower index"
    assert ref.better(obj, 4, 1) == 1 and ref.better(obj, 1, 4) == 1, "two NaNs: the lower index"
    assert ref.better(obj, 5, 5) == 5
    assert ref.better([0.0, -0.0], 1, 0) == 0, "-0.0 is not below 0.0"
    assert ref.better([float("inf"), NAN], 0, 1) == 0
    # through `offspring`: a whole group NaN selects by index alone, and the parents are min(i0, i1), min(i2, i3)
    data, task, mach, (J, M, E, N) = population("J3M4")
    obj = np.full(N * P, NAN)
    _, _, par, _ = ref.offspring(np.asarray(data[0]), task, mach, obj, None, P, SEED, GEN, FIRST, ref.ALWAYS, 0, 7)
    for g in range(N * P):
        n, c = divmod(g, P)
        i = [(x * P) >> 32 for x in ref.words(SEED, GEN, FIRST + n, c, ref.TAG_PARE)]
        assert par[g].tolist() == [n * P + min(i[0], i[1]), n * P + min(i[2], i[3])]


def test_thresholds_zero_and_two_to_the_32():
    data, task, mach, (J, M, E, N) = population("J6M6")
    t = np.asarray(data[0])
    obj = np.random.RandomState(2).rand(N * P)
    ot, om, par, kind = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, ref.NEVER, ref.NEVER, 7)
    assert (par[:, 1] == -1).all() and (kind == 0).all()
    assert np.array_equal(ot, task[par[:, 0]]) and np.array_equal(om, mach[par[:, 0]]), "neither event: every child is its parent A"
    _, _, par, kind = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, ref.ALWAYS, ref.ALWAYS, 7)
    assert (par[:, 1] >= 0).all() and np.isin(kind, (1, 2, 4)).all() and set(kind.tolist()) == {1, 2, 4}
    _, _, par, kind = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, ref.ALWAYS, ref.NEVER, 4)
    assert (par[:, 1] >= 0).all() and (kind == 0).all()
    _, _, par, kind = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, ref.NEVER, ref.ALWAYS, 4)
    assert (par[:, 1] == -1).all() and (kind == 4).all()
    assert round(0.8 * 2 ** 32) == 3435973837 and round(1.0 * 2 ** 32) == ref.ALWAYS and round(0.0 * 2 ** 32) == ref.NEVER


def test_elite_is_word_for_word():
    data, task, mach, (J, M, E, N) = population("J3M4")
    t, T = np.asarray(data[0]), J * M
    task, mach = task.copy(), mach.copy()
    task[1 * P + 4] = task[1 * P + 4][::-1]                             # every task once, the operations of every job in reverse order
    obj = np.random.RandomState(3).rand(N * P)
    best = np.array([0 * P + 3, 1 * P + 4, -1], np.int32)
    ot, om, par, kind = ref.offspring(t, task, mach, obj, best, P, SEED, GEN, FIRST, ref.ALWAYS, ref.ALWAYS, 7)
    for n, col in enumerate((3, P + 4, 2 * P)):                         # -1 is outside group 2: its member 0
        assert np.array_equal(ot[n * P], task[col]) and np.array_equal(om[n * P], mach[col])
        assert par[n * P].tolist() == [-1, -1] and kind[n * P] == -1
    assert (kind.reshape(N, P)[:, 1:] > 0).all()
    best[0] = 1 * P                                                     # another group's column is outside too
    ot2, om2, _, _ = ref.offspring(t, task, mach, obj, best, P, SEED, GEN, FIRST, ref.ALWAYS, ref.ALWAYS, 7)
    assert np.array_equal(ot2[0], task[0]) and np.array_equal(ot2[1:], ot[1:]) and np.array_equal(om2[1:], om[1:])
    # without `best` child 0 is an ordinary child, and the others do not change
    ot3, om3, par3, kind3 = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, ref.ALWAYS, ref.ALWAYS, 7)
    assert (par3[::P] >= 0).all() and (kind3[::P] > 0).all()
    keep = np.arange(N * P) % P != 0
    assert np.array_equal(ot3[keep], ot[keep]) and np.array_equal(om3[keep], om[keep]) and np.array_equal(par3[keep], par[keep])
    # an elite with an entry out of range is a column of -1
    task[3, 5] = T
    ot4, om4, _, _ = ref.offspring(t, task, mach, obj, np.array([3, P + 4, -1], np.int32), P, SEED, GEN, FIRST, ref.ALWAYS, ref.ALWAYS, 7)
    assert (ot4[0] == -1).all() and (om4[0] == -1).all()


def test_parents_that_are_no_plans_give_columns_of_minus_one():
    data, task, mach, (J, M, E, N) = population("J3M4")
    t, T = np.asarray(data[0]), J * M
    obj = np.random.RandomState(4).rand(N * P)
    base = ref.offspring(t, task, mach, obj, None, P, SEED, GEN, FIRST, 1 << 31, 1 << 31, 7)
    often = np.argsort(np.bincount(base[2][base[2] >= 0], minlength=N * P))[::-1]      # the members the draws use most
    for what, (row, pos, val, arr) in {"task T": (often[0], 0, T, "t"), "task -1": (often[1], T - 1, -1, "t"), "machine M": (often[2], 4, M, "m"),
                                       "a task twice": (often[3], 3, None, "t")}.items():
        tk, mc = task.copy(), mach.copy()
        if val is None:
            tk[row, pos], mc[row, pos] = tk[row, 0], mc[row, 0]
        else:
            (tk if arr == "t" else mc)[row, pos] = val
        ot, om, par, kind = ref.offspring(t, tk, mc, obj, None, P, SEED, GEN, FIRST, 1 << 31, 1 << 31, 7)
        used = (par == row).any(1)
        assert used.any() and not used.all(), what + ": the draws use the bad member somewhere"
        assert (ot[used] == -1).all() and (om[used] == -1).all(), what
        assert np.array_equal(ot[~used], base[0][~used]) and np.array_equal(om[~used], base[1][~used]), what + ": the other children"
        assert np.array_equal(par, base[2]) and np.array_equal(kind, base[3]), what + ": parents and kinds are written all the same"


def test_bits_past_one_philox_block_and_low_words():
    bits = ref.stream_bits(SEED, GEN, FIRST, 3, ref.TAG_JSET, 300)
    for i in (0, 31, 32, 127, 128, 129, 160, 255, 256, 299):
        w = ref.words(SEED, GEN, FIRST, 3, ref.TAG_JSET + i // 128)
        assert bits[i] == bool((w[(i // 32) % 4] >> (i % 32)) & 1)
    assert ref.words(SEED, GEN, FIRST, 3, ref.TAG_JSET + 1) != ref.words(SEED, GEN, FIRST, 3, ref.TAG_JSET)
    assert ref.words(7, 3, 5, 2, ref.TAG_PARE) == ref.words(7, 3 + (1 << 32), 5 + (1 << 32), 2, ref.TAG_PARE)
    assert ref.words(7, 3, 5, 2, ref.TAG_PARE) != ref.words(7 + (1 << 32), 3, 5, 2, ref.TAG_PARE), "the seed's high word is part of the key"
    assert ref.words(SEED, GEN, FIRST, 3, mref.TAG_MOVE) == mref.draw(SEED, GEN, FIRST, 3), "the mutation's words are the move stream's at round = generation"
    assert (ref.TAG_PARE, ref.TAG_CROS, ref.TAG_JSET, ref.TAG_MACH) == tuple(int.from_bytes(s, "big") for s in (b"pare", b"cros", b"jset", b"mach"))


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
def test_search_never_rises_and_starts_at_the_best_start(left_shift):
    data, task, mach, (J, M, E, N) = population("J3M4")
    T = J * M
    starts = [(task.reshape(N, P, T)[:, c], mach.reshape(N, P, T)[:, c]) for c in range(3)]
    res = ref.search(data, starts, 8, 3, 11, left_shift=left_shift, w=CONFIG_W)
    each = np.stack([mref.replay(data, s[0], s[1], left_shift, CONFIG_W)[3] for s in starts])
    assert np.array_equal(res["start_obj"].view(np.int64), each.min(0).view(np.int64)), "start_obj is the best start's Objective"
    hist = np.vstack([res["start_obj"][None], res["history"]])
    assert (np.diff(hist, axis=0) <= 0).all(), "the best Objective never rises"
    assert (hist[-1] < hist[0]).any(), "recombination improves some instance"
    assert np.array_equal(res["obj"].view(np.int64), hist[-1].view(np.int64)), "the replayed plan has the last generation's Objective"
    assert (res["parents"][:, ::8] == -1).all() and (res["kinds"][:, ::8] == -1).all(), "one elite per group"
    r0 = ref.search(data, starts, 8, 0, 11, left_shift=left_shift, w=CONFIG_W)
    assert r0["history"].shape == (0, N) and np.array_equal(r0["obj"].view(np.int64), each.min(0).view(np.int64))
    pick = each.argmin(0)
    assert all(np.array_equal(r0["plans"][0][n], starts[pick[n]][0][n]) for n in range(N)), "generations = 0: the best start, lowest on ties"


def test_library_declares_exports_and_refuses():
    import mtfjsp_amd  # noqa: F401
    capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
    assert "mtfjsp_plan_offspring" in capi.PROTOTYPES
    res, args = capi.PROTOTYPES["mtfjsp_plan_offspring"]
    assert res is C.c_int and len(args) == 16 and args[6:11] == [C.c_uint64] * 5 and args[1] is C.c_int32 and args[11] is C.c_uint32
    L = capi.lib()
    assert hasattr(L, "mtfjsp_plan_offspring")
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)
    # (every other refusal needs a handle, and a handle needs a GPU: tests/test_plan_offspring_gpu.py)
    assert L.mtfjsp_plan_offspring(None, 1, p, p, p, None, 0, 0, 0, 0, 0, 7, p, p, None, None) == capi.ERR_ARG
    assert all(v == 0 for v in buf)
    b = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
    data, task, mach, (J, M, E, N) = population("J3M4")
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=0.4, weight_ec=0.4, weight_tt=0.2)
    start = (task[::P], mach[::P])
    for kw in (dict(P=0), dict(generations=-1), dict(moves=0), dict(moves=8), dict(p_cross=1.5), dict(p_mut=-0.1), dict(P=1, start=[start, start]),
               dict(start=(start[0][:, :-1], start[1][:, :-1])), dict(chunk=0)):
        with pytest.raises(ValueError):
            b.evolve(*data, args, **{"start": start, **kw})
