"""Host model of mtfjsp_critical_path, of mtfjsp_plan_neighbours_critical and of baselines.local_search with the moves a critical
path directs (plain module; tests/test_critical_path_cpu.py pins it, tests/test_critical_path_gpu.py and
tests/test_critical_moves_gpu.py hold the device to it element for element).  The rule of include/mtfjsp.h is applied literally with
Python lists, one row and one copy at a time; kinds 1, 2 and 4 are tests/plan_moves_ref.py's, unchanged."""
import numpy as np

import group_reduce_ref as gref
import plan_moves_ref as pref

SWAP, INSERT, REASSIGN, CRIT_SWAP, CRIT_REASSIGN = 1, 2, 4, 8, 16
KINDS = (SWAP, INSERT, REASSIGN, CRIT_SWAP, CRIT_REASSIGN)
ALL_MOVES, CRIT_MOVES, EVERY_MOVE = 7, 24, 31
COST_KEYS = pref.COST_KEYS


def predecessors(mach, routes, M):
    """-> {task: route predecessor or None} of the scheduled tasks, from the routes [M][T] (-1 padded)"""
    prev = {}
    for m in range(M):
        r = [a for a in routes[m] if a >= 0]
        for i, a in enumerate(r):
            prev[a] = r[i - 1] if i else None
    return prev


def tight(a, mach, st, ft, prev, tt, M):
    """-> (machine-tight, job-tight) of the scheduled task a: the two equalities of include/mtfjsp.h"""
    m, mp, jp = mach[a], prev[a], (a - 1 if a % M else None)
    mt = mp is not None and st[a] == ft[mp] + (tt[m][m] if mp // M == a // M else 0.0)
    jt = jp is not None and st[a] == ft[jp] + tt[mach[jp]][m]
    return mt, jt


def critical_path(mach, st, ft, routes, tt, J, M):
    """one instance: mach [T] (-1 unscheduled), st, ft [T], routes [M][T] as `OracleBatch.state()` and `read_state` give them, tt
    [M][M] -> (path_task, path_arc): lists of one length; the last arc is -1; both empty when nothing is scheduled"""
    f = lambda x: x.tolist() if hasattr(x, "tolist") else x          # noqa: E731  (python floats: binary64 sums)
    mach, st, ft, routes, tt = f(mach), f(st), f(ft), f(routes), f(tt)
    T = J * M
    sched = [a for a in range(T) if mach[a] >= 0]
    if not sched:
        return [], []
    prev = predecessors(mach, routes, M)
    a = sched[0]
    for b in sched:
        if ft[b] > ft[a]:
            a = b
    path, arc = [], []
    while True:
        path.append(a)
        mt, jt = tight(a, mach, st, ft, prev, tt, M)
        if mt:
            arc.append(1)
            a = prev[a]
        elif jt:
            arc.append(0)
            a = a - 1
        else:
            arc.append(-1)
            return path, arc
        assert len(path) <= T, "a path visits a task once"


def path_rows(state, tt, J, M, col=None):
    """state: dict(mach, st, ft, routes) of a batch; tt [B,M,M]; col: the instance of every row (None: all, in order; an entry
    outside the batch is an empty row) -> (path_task [n,T] int32, path_arc [n,T] int8, path_len [n] int32), -1 padded"""
    B, T = state["mach"].shape
    col = list(range(B)) if col is None else [int(c) for c in col]
    pt, pa, pl = np.full((len(col), T), -1, np.int32), np.full((len(col), T), -1, np.int8), np.zeros(len(col), np.int32)
    for i, b in enumerate(col):
        if 0 <= b < B:
            p, a = critical_path(state["mach"][b], state["st"][b], state["ft"][b], state["routes"][b], tt[b], J, M)
            pt[i, :len(p)], pa[i, :len(p)], pl[i] = p, a, len(p)
    return pt, pa, pl


def swap_arcs(path_task, path_arc, M):
    """CRIT_SWAP's list A: the positions of the machine arcs between two jobs"""
    return [k for k in range(len(path_task) - 1) if path_arc[k] == 1 and path_task[k] // M != path_task[k + 1] // M]


def kind_of(w, moves):
    bits = [b for b in KINDS if moves & b]
    return bits[(w[0] * len(bits)) >> 32]


def neighbour(t_n, task, mach, w, moves, path_task, path_arc):
    """one copy c >= 1: the incumbent (task, mach) lists of an instance with times t_n [T,M] and the critical path (path_task,
    path_arc: lists of the path's length) after the move the words w name -> (task', mach', kind)"""
    kind = kind_of(w, moves)
    if kind in (SWAP, INSERT, REASSIGN):
        return pref.neighbour(t_n, task, mach, w, kind)                 # (a mask of one bit: that kind, the same x and y)
    M, L = len(t_n[0]), len(path_task)
    q = [a // M for a in task]
    mu = dict(zip(task, mach))
    pos = {a: s for s, a in enumerate(task)}
    if kind == CRIT_SWAP:
        A = swap_arcs(path_task, path_arc, M)
        if A:
            k = A[(w[1] * len(A)) >> 32]
            x, y = pos[path_task[k]], pos[path_task[k + 1]]
            e = q.pop(x)
            q.insert(y, e)
    elif L:
        a = path_task[(w[1] * L) >> 32]
        F = [m for m in range(M) if t_n[a][m] >= 0 and m != mu[a]]
        if F:
            mu[a] = F[(w[2] * len(F)) >> 32]
    task2, mach2 = pref.decode(q, mu, M)
    return task2, mach2, kind


def neighbours(t, task, mach, K, seed, round, first_instance, moves, paths):
    """t [N,T,M]; task, mach [N,T]: the incumbents; paths = (path_task [N,T], path_arc [N,T], path_len [N])
    -> (task [N*K,T], mach [N*K,T], kind [N*K] int8), copy c of group n = row n*K + c"""
    t, task, mach = np.asarray(t), np.asarray(task), np.asarray(mach)
    N, T = task.shape
    out_t, out_m, kind = np.zeros((N * K, T), np.int32), np.zeros((N * K, T), np.int32), np.full(N * K, -1, np.int8)
    for n in range(N):
        tn, inc_t, inc_m = t[n].tolist(), task[n].tolist(), mach[n].tolist()
        L = int(paths[2][n])
        p_t, p_a = paths[0][n][:L].tolist(), paths[1][n][:L].tolist()
        out_t[n * K], out_m[n * K] = inc_t, inc_m
        for c in range(1, K):
            w = pref.draw(seed, round, (int(first_instance) + n) & 0xFFFFFFFFFFFFFFFF, c)
            out_t[n * K + c], out_m[n * K + c], kind[n * K + c] = neighbour(tn, inc_t, inc_m, w, moves, p_t, p_a)
    return out_t, out_m, kind


def replay(data, task, mach, left_shift, w, steps=None):
    """the C oracle on the instances `data` driven by the first `steps` (default: all) steps of the plans task, mach [B,T]
    -> (cum [B,5], final4 [B,4], done [B], obj [B], state: dict(mach, st, ft, routes, ...))"""
    from oracle.env_oracle import OracleBatch
    t, p, tt, edge = data
    B, T = task.shape
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=w)
    orc.scaler_init()
    orc.reset(np.tile(np.array([w], np.float64), (B, 1)))
    cum = np.zeros((B, 5))
    for s in range(T if steps is None else steps):
        cum += orc.step(task[:, s], mach[:, s])[1]
    st = orc.state()
    st["mach"] = np.where(st["sched"] != 0, st["mach"], -1)
    final4, done = gref.final_costs(st["prev"], st["sched"].astype(np.int64).sum(1), T)
    return cum, final4, done, gref.objectives(final4, w)[3], st


def search(data, start, K, rounds, seed, moves=EVERY_MOVE, left_shift=False, w=(0.4, 0.4, 0.2), first_instance=0):
    """baselines.local_search on the host, all five kinds: the paths of `start` before round 0, of every round's best copies after
    it -> dict(start_obj [N], history [rounds,N], accepted [rounds,N] int8, plans (task, mach) [N,T], cost {key: [N]}, final4 [N,4],
    obj [N])"""
    if not moves & CRIT_MOVES:
        return pref.search(data, start, K, rounds, seed, moves, left_shift, w, first_instance)
    t, tt = np.asarray(data[0]), np.asarray(data[2])
    N, T, M = t.shape
    J = T // M
    task, mach = np.array(start[0], np.int32), np.array(start[1], np.int32)
    rep = tuple(np.repeat(np.asarray(x), K, axis=0) for x in data)
    history, accepted, start_obj = [], [], None
    if rounds:
        paths = path_rows(replay(data, task, mach, left_shift, w)[4], tt, J, M)
    for r in range(rounds):
        nt, nm, kind = neighbours(t, task, mach, K, seed, r, first_instance, moves, paths)
        _, final4, done, _, state = replay(rep, nt, nm, left_shift, w)
        obj, best, best_obj, _ = gref.group_reduce(final4, done, w, N, K)
        assert (best >= 0).all()
        if r == 0:
            start_obj = obj[::K].copy()
        history.append(best_obj)
        accepted.append(np.where(best % K == 0, -1, kind[best]).astype(np.int8))
        task, mach = nt[best], nm[best]
        paths = path_rows(state, rep[2], J, M, best)
    cum, final4, done, obj, _ = replay(data, task, mach, left_shift, w)
    assert done.all()
    return dict(start_obj=obj.copy() if start_obj is None else start_obj, history=np.array(history).reshape(rounds, N),
                accepted=np.array(accepted, np.int8).reshape(rounds, N), plans=(task, mach),
                cost={key: cum[:, i] for i, key in enumerate(COST_KEYS)}, final4=final4, obj=obj)


# ---- the inputs the CPU and the GPU tests share
# J, M, E, N.  T = 128 and 129: the kernel's doubling loop ends its two conditions together, and takes one more doubling; J65M2: more
# jobs than lanes; J10M20: the first launch of the directed moves above 48 KiB; J28M64 (T = 1792): the first T at M = 64 whose paths
# need more than 48 KiB of LDS (crit_lds_bytes below), all 64 machines
SHAPES = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4), "J8M8": (8, 8, 2, 5), "J10M10": (10, 10, 2, 3),
          "J16M8": (16, 8, 2, 3), "J43M3": (43, 3, 1, 3), "J65M2": (65, 2, 1, 3), "J10M20": (10, 20, 2, 3), "J28M64": (28, 64, 2, 2)}
# the shapes of the directed moves alone (tests/test_critical_moves_gpu.py): one replay each, no stops
MOVE_SHAPES = {"J15M16": (15, 16, 2, 3), "J20M20": (20, 20, 2, 3), "J70M8": (70, 8, 2, 3), "J47M32": (47, 32, 2, 2),
               "J48M32": (48, 32, 2, 2)}
CONFIG_W = (0.4, 0.4, 0.2)


def on_a_grid(data, dur=8.0, trans=4.0):
    """the instances with every duration a multiple of 8 and every transport time a multiple of 4 (the sign of a duration, which
    marks an infeasible machine, stays): generated times are real-valued and never tie; these tie in the largest finish time and in
    both arcs of a task"""
    t, p, tt, edge = (np.asarray(x) for x in data)
    tg = np.sign(t) * np.maximum(dur, np.round(np.abs(t) / dur) * dur)
    return tg, p, np.round(tt / trans) * trans, edge


# Beyond T = 100 the grid of 8 no longer ties in the LARGEST finish time (measured: no schedule of the five shapes below does, at any
# stop), and never in two passes of 64 tasks.  On a grid of 64 — durations 64 or 128, transport times 0 — every one of these shapes has
# a schedule whose largest finish time is shared by tasks of different passes (tests/test_critical_path_cpu.py asserts it)
COARSE = ("J16M8", "J43M3", "J65M2", "J10M20", "J28M64")


def shape_inputs(shape):
    """-> (J, M, E, N), {variant: data}, (task, mach): N generated instances as they are and on the grid, one random plan each (and on the grid of 64 for the
    shapes of COARSE)"""
    from importlib import import_module
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = SHAPES[shape] if shape in SHAPES else MOVE_SHAPES[shape]
    data = tuple(np.asarray(x) for x in inst.generate_instances(N, J, M, E, seed=8100 + J * 100 + M, native=False))
    variants = {"generated": data, "grid": on_a_grid(data)}
    if shape in COARSE:
        variants["coarse"] = on_a_grid(data, 64.0, 64.0)
    return (J, M, E, N), variants, pref.random_plans(data[0], J, M, 17)


def crit_lds_bytes(T):
    """csrc/mtfjsp_plan.hip's crit_lds_bytes restated: the dynamic LDS of k_critical_path — four waves, seven bytes a task (three u16
    tables and the arc kinds) in rows of T + 1 entries padded to a multiple of 4.  Above 48 KiB the launch first asks for the size"""
    return 4 * 7 * ((T + 4) & ~3)


def stops(T):
    """where the tests stop a replay and look at the path: two tasks, half a schedule, the complete one"""
    return (2, T // 2, T)
