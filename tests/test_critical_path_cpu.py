"""CPU: the host model of mtfjsp_critical_path, of the two moves a critical path directs and of baselines.local_search with them
(tests/critical_path_ref.py) is itself right, on schedules of the C oracle: random plans on J3M4, J6M6, J8M8 (T = 64), J10M10
(T = 100), J16M8 (T = 128), J43M3 (T = 129), J65M2, J10M20 and J28M64 (T = 1792, 64 machines), left shift on and off, stopped after 2 steps, half way and complete; the generated instances as they are and with their
times on a grid (generated times are real-valued and never tie: the grid gives equal largest finish times and tasks tight on both
sides).  The GPU tests run the same inputs, so what these inputs cover is asserted here.
The search runs on the two rows of tests/test_local_search_gpu.py with their seed 11 where left shift is off; with left shift on
that seed accepts no CRIT_SWAP under moves = 31, w = (1, 0, 0), so those cases take seeds of their own (SEARCH_SEED)."""
import functools
from importlib import import_module

import numpy as np
import pytest

import critical_path_ref as ref
import plan_moves_ref as pref

ROWS = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}
K, ROUNDS = 8, 6
SEARCH_SEED = {("J3M4", False): 11, ("J6M6", False): 11, ("J3M4", True): 17, ("J6M6", True): 14}
MAKESPAN_ONLY = (1.0, 0.0, 0.0)


def assert_valid_plan(t_n, task, mach, J, M, tag):
    assert sorted(task) == list(range(J * M)), tag + ": every task once (every job M times)"
    nxt = [0] * J
    for a in task:
        assert a % M == nxt[a // M], tag + ": the operations of a job in order"
        nxt[a // M] += 1
    assert all(0 <= m < M and t_n[a][m] >= 0 for a, m in zip(task, mach)), tag + ": feasible machines"


@functools.lru_cache(maxsize=None)
def schedules(shape):
    """-> [(tag, data, left_shift, steps, state)] of every input of this shape"""
    (J, M, E, N), variants, (task, mach) = ref.shape_inputs(shape)
    out = []
    for variant, data in variants.items():
        for left_shift in (False, True):
            for steps in ref.stops(J * M):
                state = ref.replay(data, task, mach, left_shift, ref.CONFIG_W, steps)[4]
                out.append((f"{shape} {variant} left_shift={left_shift} steps={steps}", data, left_shift, steps, state))
    return out


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_paths_are_critical_paths(shape):
    J, M, E, N = ref.SHAPES[shape]
    T = J * M
    for tag, data, left_shift, steps, state in schedules(shape):
        tt = np.asarray(data[2])
        pt, pa, pl = ref.path_rows(state, tt, J, M)
        assert pt.shape == (N, T) and pa.shape == (N, T) and pl.shape == (N,)
        for b in range(N):
            mach, st, ft, routes, ttb = (x.tolist() for x in (state["mach"][b], state["st"][b], state["ft"][b], state["routes"][b], tt[b]))
            sched = [a for a in range(T) if mach[a] >= 0]
            assert len(sched) == steps, tag + ": one task a step"
            L = int(pl[b])
            path, arc = pt[b, :L].tolist(), pa[b, :L].tolist()
            assert 1 <= L <= steps and (pt[b, L:] == -1).all() and (pa[b, L:] == -1).all() and len(set(path)) == L, tag
            assert all(mach[a] >= 0 for a in path), tag + ": scheduled tasks only"
            assert ft[path[0]] == max(ft[a] for a in sched) and path[0] == min(a for a in sched if ft[a] == ft[path[0]]), tag + ": element 0 ends last"
            prev = ref.predecessors(mach, routes, M)
            for k in range(L - 1):
                v, u, m = path[k], path[k + 1], mach[path[k]]
                if arc[k] == 1:
                    r = [a for a in routes[m] if a >= 0]
                    assert r[r.index(v) - 1] == u and r.index(v) > 0, tag + ": a machine arc joins route neighbours"
                    assert st[v] == ft[u] + (ttb[m][m] if u // M == v // M else 0.0), tag + ": a machine arc is tight"
                else:
                    assert arc[k] == 0 and u == v - 1 and v % M != 0, tag + ": a job arc joins two operations of a job"
                    assert st[v] == ft[u] + ttb[mach[u]][m], tag + ": a job arc is tight"
                    assert not ref.tight(v, mach, st, ft, prev, ttb, M)[0], tag + ": the machine arc goes first"
            assert arc[L - 1] == -1 and ref.tight(path[-1], mach, st, ft, prev, ttb, M) == (False, False), tag + ": the last element has no tight arc"
            if not left_shift and steps == T:
                assert st[path[-1]] == 0.0, tag + ": without left shift a complete schedule's path starts at 0"


def test_the_large_shapes_are_where_the_kernel_changes_path():
    """what the added shapes are there for, as arithmetic on the kernel's own formulae"""
    T = {k: v[0] * v[1] for k, v in ref.SHAPES.items()}
    assert (T["J16M8"], T["J43M3"], T["J65M2"], T["J28M64"]) == (128, 129, 130, 1792)
    assert ref.crit_lds_bytes(1792) == 50288 > 48 * 1024 >= ref.crit_lds_bytes(27 * 64) and ref.crit_lds_bytes(100) == 4 * 7 * 104
    doublings = lambda t: sum(1 for bit in range(16) if (1 << bit) < t)         # noqa: E731
    assert (doublings(128), doublings(129)) == (7, 8)


@pytest.mark.parametrize("shape", ref.COARSE)
def test_the_coarse_variant_ties_in_the_largest_finish_time_across_passes(shape):
    """the kernel finds element 0 in passes of 64 tasks: some schedule of every large shape must share its largest finish time between
    two passes (the lowest task wins).  The generated and the grid-of-8 variants do not at these sizes"""
    J, M, E, N = ref.SHAPES[shape]
    found = {}
    for tag, data, left_shift, steps, state in schedules(shape):
        ft = np.where(state["mach"] >= 0, state["ft"], -1.0)
        across = sum(len(set((np.flatnonzero(ft[b] == ft[b].max()) // 64).tolist())) > 1 for b in range(N))
        found[tag.split()[1]] = found.get(tag.split()[1], 0) + across
    print(shape, found)
    assert found["coarse"] > 0


def test_the_inputs_cover_every_branch():
    kinds, both, equal_max, swaps = set(), 0, 0, []
    for shape, (J, M, E, N) in ref.SHAPES.items():
        T = J * M
        for tag, data, left_shift, steps, state in schedules(shape):
            tt = np.asarray(data[2])
            pt, pa, pl = ref.path_rows(state, tt, J, M)
            kinds |= set(np.unique(pa).tolist())
            for b in range(N):
                mach, st, ft, routes, ttb = (x.tolist() for x in (state["mach"][b], state["st"][b], state["ft"][b], state["routes"][b], tt[b]))
                prev = ref.predecessors(mach, routes, M)
                sched = [a for a in range(T) if mach[a] >= 0]
                both += sum(1 for a in pt[b, :pl[b]].tolist() if ref.tight(a, mach, st, ft, prev, ttb, M) == (True, True))
                last = max(ft[c] for c in sched)
                equal_max += sum(1 for a in sched if ft[a] == last) > 1
                swaps.append(len(ref.swap_arcs(pt[b, :pl[b]].tolist(), pa[b, :pl[b]].tolist(), M)))
    print("arc kinds", kinds, "path tasks tight on both sides", both, "schedules with equal largest finish times", equal_max, "swap arcs", swaps)
    assert kinds == {-1, 0, 1}, "both kinds of arc occur"
    assert both > 0, "a task of a path is machine- and job-tight: the tie rule is exercised"
    assert equal_max > 0, "equal largest finish times occur"
    assert max(swaps) >= 2 and min(swaps) == 0, "a path with two or more eligible CRIT_SWAP arcs, and one with none"


@functools.lru_cache(maxsize=None)
def table_row(shape):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = ROWS[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M, native=False)
    return data, pref.first_feasible_plan(data[0]), (J, M, E, N)


@pytest.mark.parametrize("shape", ["J3M4", "J6M6", "J8M8"])
@pytest.mark.parametrize("moves", [8, 16, 24, 31])
def test_every_neighbour_is_a_plan_and_each_move_is_what_it_says(shape, moves):
    (J, M, E, N), variants, (task, mach) = ref.shape_inputs(shape)
    data = variants["generated"]
    t, tt, T, Kn = np.asarray(data[0]), np.asarray(data[2]), J * M, 48
    seed, rnd, first = (1 << 40) + 9, 2, 5
    seen = set()
    for left_shift, steps in ((False, T), (True, T), (False, T // 2), (False, 0)):      # (half a schedule: a short path; none: an empty one)
        paths = ref.path_rows(ref.replay(data, task, mach, left_shift, ref.CONFIG_W, steps)[4], tt, J, M)
        out_t, out_m, kind = ref.neighbours(t, task, mach, Kn, seed, rnd, first, moves, paths)
        for n in range(N):
            inc_t, inc_m = task[n].tolist(), mach[n].tolist()
            q, mu = [a // M for a in inc_t], dict(zip(inc_t, inc_m))
            L = int(paths[2][n])
            p_t, p_a = paths[0][n, :L].tolist(), paths[1][n, :L].tolist()
            assert out_t[n * Kn].tolist() == inc_t and out_m[n * Kn].tolist() == inc_m and kind[n * Kn] == -1, "copy 0 is the incumbent"
            for c in range(1, Kn):
                g = n * Kn + c
                tk, mc, kd = out_t[g].tolist(), out_m[g].tolist(), int(kind[g])
                w = pref.draw(seed, rnd, first + n, c)
                assert kd & moves and kd == ref.kind_of(w, moves)
                seen.add(kd)
                assert_valid_plan(t[n].tolist(), tk, mc, J, M, f"{shape} n={n} c={c}")
                q2, mu2 = [a // M for a in tk], dict(zip(tk, mc))
                if kd in (1, 2, 4):
                    assert (tk, mc, kd) == pref.neighbour(t[n].tolist(), inc_t, inc_m, w, kd), "the three undirected kinds are plan_moves_ref's"
                elif kd == ref.CRIT_SWAP:
                    A = ref.swap_arcs(p_t, p_a, M)
                    if not A:
                        assert tk == inc_t and mc == inc_m, "no eligible arc: the identity"
                        continue
                    k = A[(w[1] * len(A)) >> 32]
                    x, y = inc_t.index(p_t[k]), inc_t.index(p_t[k + 1])
                    src = [x if s == y else (s + 1 if x <= s < y else (s - 1 if y < s <= x else s)) for s in range(T)]
                    assert x != y and sorted(src) == list(range(T)) and q2 == [q[i] for i in src] and mu2 == mu, "CRIT_SWAP is INSERT of pos[v] at pos[u]"
                else:
                    assert q2 == q
                    changed = [a for a in mu if mu2[a] != mu[a]]
                    if L == 0:
                        assert not changed, "an empty path: the identity"
                        continue
                    a = p_t[(w[1] * L) >> 32]
                    feas = [m for m in range(M) if t[n, a, m] >= 0]
                    assert changed == ([a] if len(feas) > 1 else []) and mu2[a] in feas, "CRIT_REASSIGN changes only a path task's machine"
    assert seen == {b for b in ref.KINDS if moves & b}, "every allowed kind is drawn"


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(ROWS))
def test_the_search_never_gets_worse_and_accepts_both_new_kinds(shape, left_shift):
    data, start, (J, M, E, N) = table_row(shape)
    seed = SEARCH_SEED[shape, left_shift]
    for moves, w in ((31, MAKESPAN_ONLY), (24, MAKESPAN_ONLY), (31, ref.CONFIG_W), (24, ref.CONFIG_W)):
        res = ref.search(data, start, K, ROUNDS, seed, moves, left_shift, w)
        hist = np.vstack([res["start_obj"][None], res["history"]])
        acc = res["accepted"]
        print(shape, left_shift, moves, w, "mean objective per round", hist.mean(1).round(1), "accepted", sorted(set(acc.ravel().tolist())))
        assert (np.diff(hist, axis=0) <= 0).all(), "the best objective never rises"
        assert np.array_equal(res["obj"].view(np.int64), hist[-1].view(np.int64)), "the replayed plan has the last round's objective"
        assert ((acc == -1) == (np.diff(hist, axis=0) == 0)).all(), "a move is accepted iff it improves strictly"
        assert set(np.unique(acc).tolist()) <= {-1} | {b for b in ref.KINDS if moves & b}
        for n in range(N):
            assert_valid_plan(np.asarray(data[0])[n].tolist(), res["plans"][0][n].tolist(), res["plans"][1][n].tolist(), J, M, f"{shape} final plan {n}")
        if moves == 31 and w == MAKESPAN_ONLY:
            assert {8, 16} <= set(np.unique(acc).tolist()), "both new kinds are accepted"


def test_moves_without_a_new_kind_are_the_old_search():
    data, start, _ = table_row("J3M4")
    a, b = ref.search(data, start, K, 3, 11, 7, False, ref.CONFIG_W), pref.search(data, start, K, 3, 11, 7, False, ref.CONFIG_W)
    assert np.array_equal(a["history"], b["history"]) and np.array_equal(a["plans"][0], b["plans"][0]) and np.array_equal(a["accepted"], b["accepted"])
    r0 = ref.search(data, start, K, 0, 11, 31)
    assert r0["history"].shape == (0, 3) and np.array_equal(r0["plans"][0], start[0]) and np.array_equal(r0["start_obj"], r0["obj"])
    r1 = ref.search(data, start, 1, 3, 11, 31)
    assert (r1["history"] == r1["start_obj"][None]).all() and (r1["accepted"] == -1).all() and np.array_equal(r1["plans"][1], start[1])
