"""Host model of mtfjsp_front_rank, mtfjsp_plan_survivors and baselines.evolve_pareto (plain module; tests/test_front_rank_cpu.py pins it,
tests/test_front_rank_gpu.py and tests/test_evolve_pareto_gpu.py hold the device to it).  The rule of include/mtfjsp.h is applied
literally, group by group (tests/test_front_rank_cpu.py restates it candidate by candidate); objectives and dominance are tests/group_reduce_ref.py's, the offspring and the
replay those of tests/plan_crossover_ref.py and tests/plan_moves_ref.py.
N groups of K = Ka + Kb candidates: candidate c < Ka of group n = element n*Ka + c of the a arrays, c >= Ka = element n*Kb + (c - Ka) of b."""
import numpy as np

import group_reduce_ref as gref
import plan_crossover_ref as xref
import plan_moves_ref as mref

COST_KEYS = mref.COST_KEYS


def gather(a, b, N, width=None):
    """the two array sets side by side: a [N*Ka, ...], b [N*Kb, ...] or None -> [N, K, ...]"""
    a = np.asarray(a)
    a = a.reshape((N, -1) + a.shape[1:]) if width is None else a.reshape(N, -1, width)
    if b is None:
        return a
    b = np.asarray(b)
    b = b.reshape((N, -1) + b.shape[1:]) if width is None else b.reshape(N, -1, width)
    return np.concatenate([a, b], axis=1)


def dominance(mk, ec, tt, elig):
    """D[q, c] = candidate q dominates candidate c (group_reduce_ref.dominates for every pair at once): both eligible, q nowhere worse,
    and somewhere better or equal throughout with q < c"""
    K = len(mk)
    pts = np.stack([mk, ec, tt], 1)
    with np.errstate(invalid="ignore"):
        le = (pts[:, None, :] <= pts[None, :, :]).all(2)
        lt = (pts[:, None, :] < pts[None, :, :]).any(2)
        eq = (pts[:, None, :] == pts[None, :, :]).all(2)
    idx = np.arange(K)
    return elig[:, None] & elig[None, :] & le & (lt | (eq & (idx[:, None] < idx[None, :])))


def rank_group(mk, ec, tt, obj, elig):
    """one group -> (rank [K] int32, crowd [K] f64, order [K] int32, front_size, best_obj)"""
    K = len(mk)
    idx = np.arange(K)
    # ---- the peeling: rank r = the unranked candidates that no unranked candidate dominates
    D = dominance(mk, ec, tt, elig)
    rank = np.where(elig, -2, -1).astype(np.int32)                      # -2: eligible, not ranked yet
    r = 0
    while (rank == -2).any():
        left = rank == -2
        now = left & ~D[left].any(0)
        assert now.any(), "a strict partial order has a minimal element"
        rank[now] = r
        r += 1
    # ---- the crowding distance inside every rank: per axis the neighbours in (value, index) order and the rank's extremes
    crowd = np.full(K, np.nan)
    pts = np.stack([mk, ec, tt], 1)
    for rr in range(r):
        mem = np.flatnonzero(rank == rr)
        d = np.zeros((len(mem), 3))
        for a in range(3):
            x = pts[mem, a]
            by = np.lexsort((mem, x))                                   # ascending value, then ascending index
            xs = x[by]
            lo, hi = xs[0], xs[-1]
            da = np.full(len(mem), np.inf)
            if len(mem) > 2:
                with np.errstate(all="ignore"):
                    da[1:-1] = 0.0 if hi == lo else (xs[2:] - xs[:-2]) / (hi - lo)
            d[by, a] = da
        with np.errstate(all="ignore"):
            crowd[mem] = (d[:, 0] + d[:, 1]) + d[:, 2]
        pick = -1
        for c in mem:                                                   # ascending, strict: ties stay with the lowest c
            if obj[c] == obj[c] and (pick < 0 or obj[c] < obj[pick]):
                pick = c
        if pick >= 0:
            crowd[pick] = np.inf                                        # the one addition: a rank's best objective is never crowded out
    # ---- the selection order: eligible first, ascending rank, descending crowd with NaN last, ascending index
    nan = np.isnan(crowd)
    order = np.lexsort((idx, np.where(nan, 0.0, -crowd), nan, rank, ~elig)).astype(np.int32)
    best = -1
    for c in range(K):
        if elig[c] and obj[c] == obj[c] and (best < 0 or obj[c] < obj[best]):
            best = c
    return rank, crowd, order, int((rank == 0).sum()), (obj[best] if best >= 0 else np.nan)


def front_rank(cost4_a, done_a, cost4_b, done_b, w, N):
    """-> rank [N*K] int32, crowd [N*K] f64, order [N*K] int32, front_size [N] int32, best_obj [N] f64"""
    cost4 = gather(cost4_a, cost4_b, N, 4).astype(np.float64)
    done = gather(done_a, done_b, N)
    K = cost4.shape[1]
    mk, ec, tt, obj = gref.objectives(cost4, w)
    elig = (done != 0) & ~np.isnan(mk) & ~np.isnan(ec) & ~np.isnan(tt)
    obj = np.where(elig, obj, np.nan)
    rank, crowd, order = np.zeros((N, K), np.int32), np.zeros((N, K)), np.zeros((N, K), np.int32)
    front_size, best_obj = np.zeros(N, np.int32), np.zeros(N)
    for n in range(N):
        rank[n], crowd[n], order[n], front_size[n], best_obj[n] = rank_group(mk[n], ec[n], tt[n], obj[n], elig[n])
    return rank.reshape(-1), crowd.reshape(-1), order.reshape(-1), front_size, best_obj


def survivors(order, rank, P, N, task_a, mach_a, cost4_a, done_a, task_b=None, mach_b=None, cost4_b=None, done_b=None):
    """plans as rows: task_a, mach_a [N*Ka,T], task_b, mach_b [N*Kb,T] -> (task [N*P,T], mach [N*P,T], cost4 [N*P,4], done [N*P] uint8,
    rank [N*P] int32, src [N*P] int32, fit [N*P] f64)"""
    task, mach = gather(task_a, task_b, N), gather(mach_a, mach_b, N)
    cost4, done = gather(cost4_a, cost4_b, N, 4).astype(np.float64), gather(done_a, done_b, N)
    K, T = task.shape[1], task.shape[2]
    order, rank = np.asarray(order).reshape(N, K), np.asarray(rank).reshape(N, K)
    o_t, o_m = np.full((N * P, T), -1, np.int32), np.full((N * P, T), -1, np.int32)
    o_c, o_d = np.full((N * P, 4), np.nan), np.zeros(N * P, np.uint8)
    o_r, o_s, o_f = np.full(N * P, -1, np.int32), np.zeros(N * P, np.int32), np.full(N * P, np.nan)
    for n in range(N):
        for i in range(P):
            g, c = n * P + i, int(order[n, i])
            o_s[g] = c
            if not 0 <= c < K:
                continue
            o_t[g], o_m[g], o_c[g], o_d[g], o_r[g] = task[n, c], mach[n, c], cost4[n, c], done[n, c], rank[n, c]
            if rank[n, c] >= 0:
                o_f[g] = float(i)
    return o_t, o_m, o_c, o_d, o_r, o_s, o_f


def search(data, start, P, generations, seed, p_cross=0.8, p_mut=0.3, moves=mref.ALL_MOVES, left_shift=False, w=(0.4, 0.4, 0.2), first_instance=0):
    """baselines.evolve_pareto on the host: plan_crossover_ref.search with the new selection -> dict(start_obj [N], history
    [generations,N], front_size [generations+1,N], fronts: N dicts (cost [F,3], final4 [F,4], obj [F], task [F,T], mach [F,T]),
    plans (task, mach) [N,T], cost {key: [N]}, final4 [N,4], obj [N] of the best-Objective member)"""
    t = np.asarray(data[0])
    N, T = t.shape[0], t.shape[1]
    starts = [start] if len(start) == 2 and np.ndim(start[0]) == 2 else list(start)
    member = np.arange(P) % len(starts)
    task = np.stack([np.asarray(s[0], np.int32) for s in starts], 1)[:, member].reshape(N * P, T)
    mach = np.stack([np.asarray(s[1], np.int32) for s in starts], 1)[:, member].reshape(N * P, T)
    cross_thr, mut_thr = int(round(p_cross * 2 ** 32)), int(round(p_mut * 2 ** 32))
    rep = tuple(np.repeat(np.asarray(x), P, axis=0) for x in data)
    history, sizes = [], []
    _, c4, dn, _ = mref.replay(rep, task, mach, left_shift, w)
    rank, _, order, fs, bo = front_rank(c4, dn, None, None, w, N)
    task, mach, c4, dn, rk, _, fit = survivors(order, rank, P, N, task, mach, c4, dn)
    history.append(bo); sizes.append(fs)
    for g in range(1, generations + 1):
        ct, cm, _, _ = xref.offspring(t, task, mach, fit, None, P, seed, g, first_instance, cross_thr, mut_thr, moves)
        _, cc4, cdn, _ = mref.replay(rep, ct, cm, left_shift, w)
        rank, _, order, fs, bo = front_rank(c4, dn, cc4, cdn, w, N)
        task, mach, c4, dn, rk, _, fit = survivors(order, rank, P, N, task, mach, c4, dn, ct, cm, cc4, cdn)
        history.append(bo); sizes.append(fs)
    obj, best, _, _ = gref.group_reduce(c4, dn, w, N, P)
    fronts = []
    for n in range(N):
        sel = np.flatnonzero(rk[n * P:(n + 1) * P] == 0) + n * P
        f4 = c4[sel]
        fronts.append(dict(cost=np.stack([f4[:, 0], f4[:, 1] + f4[:, 3], f4[:, 2]], 1), final4=f4, obj=obj[sel], task=task[sel], mach=mach[sel]))
    pick = np.where(best < 0, np.arange(N) * P, best)
    bt, bm = task[pick], mach[pick]
    cum, final4, done, bobj = mref.replay(data, bt, bm, left_shift, w)
    assert done.all()
    return dict(start_obj=history[0], history=np.array(history[1:]).reshape(generations, N), front_size=np.array(sizes, np.int32).reshape(generations + 1, N),
                fronts=fronts, plans=(bt, bm), cost={key: cum[:, i] for i, key in enumerate(COST_KEYS)}, final4=final4, obj=bobj)


def hypervolume(points, ref):
    """the volume dominated by `points` [F,3] (three minimised axes) inside the box below `ref`, by inclusion and exclusion over the
    grid the coordinates span: a restatement that shares nothing with baselines.hypervolume's slicing"""
    pts = [tuple(float(x) for x in p) for p in np.asarray(points, np.float64).reshape(-1, 3) if all(p[a] < ref[a] for a in range(3))]
    if not pts:
        return 0.0
    axes = [sorted(set([p[a] for p in pts] + [float(ref[a])])) for a in range(3)]
    vol = 0.0
    for i in range(len(axes[0]) - 1):
        for j in range(len(axes[1]) - 1):
            for k in range(len(axes[2]) - 1):
                lo = (axes[0][i], axes[1][j], axes[2][k])
                if any(p[0] <= lo[0] and p[1] <= lo[1] and p[2] <= lo[2] for p in pts):
                    vol += (axes[0][i + 1] - lo[0]) * (axes[1][j + 1] - lo[1]) * (axes[2][k + 1] - lo[2])
    return vol
