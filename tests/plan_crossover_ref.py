"""Host model of mtfjsp_plan_offspring and of baselines.evolve (plain module; tests/test_plan_crossover_cpu.py pins it,
tests/test_plan_offspring_gpu.py and tests/test_evolve_gpu.py hold the device to it element for element).
The rule of include/mtfjsp.h is applied literally with Python lists, one child at a time; Philox, the move and the decoding are those of
tests/device_streams_ref.py and tests/plan_moves_ref.py; `search` drives the C oracle and the host model of the group reduction."""
import math

import numpy as np

import device_streams_ref as sref
import group_reduce_ref as gref
import plan_moves_ref as mref

TAG_PARE, TAG_CROS, TAG_JSET, TAG_MACH = 0x70617265, 0x63726f73, 0x6a736574, 0x6d616368
ALWAYS, NEVER = 1 << 32, 0
COST_KEYS = mref.COST_KEYS


def words(seed, generation, instance, c, tag):
    """the four Philox words of child c of global instance `instance` in generation `generation` under `tag` (only the low words of
    instance and generation enter)"""
    s0, s1 = sref._lo_hi(seed)
    return [int(x) for x in sref.philox4x32(int(instance) & 0xFFFFFFFF, int(c), int(generation) & 0xFFFFFFFF, int(tag) & 0xFFFFFFFF, s0, s1)]


def stream_bits(seed, generation, instance, c, tag, n):
    """bits 0..n-1 of the stream of `tag`: bit i = bit i % 32 of word (i / 32) % 4 of the block of tag + i / 128"""
    blocks = [words(seed, generation, instance, c, tag + b) for b in range((n + 127) // 128)]
    return [bool((blocks[i // 128][(i // 32) % 4] >> (i % 32)) & 1) for i in range(n)]


def better(obj, i, j):
    """the tournament of members i and j: the smaller objective; a NaN loses to any number; equal values or two NaNs: the lower index"""
    lo, hi = min(i, j), max(i, j)
    ol, oh = float(obj[lo]), float(obj[hi])
    if math.isnan(oh):
        return lo
    if math.isnan(ol):
        return hi
    return hi if oh < ol else lo


def pox(qa, qb, in_s):
    """precedence-preserving order crossover of two job strings: positions whose q_A is in S keep it, the others take q_B's entries
    outside S in order -> q', or None where the fill runs short or long"""
    rest = [j for j in qb if not in_s[j]]
    holes = [s for s, j in enumerate(qa) if not in_s[j]]
    if len(rest) != len(holes):
        return None
    q = list(qa)
    for s, j in zip(holes, rest):
        q[s] = j
    return q


def child(t_n, A, B, in_s, from_a, mut_w, moves, M):
    """A, B = (task, mach) lists of the parents (B None: no crossover), in_s [J] and from_a [T] the crossover's bits, mut_w the four
    "move" words or None -> (task', mach', kind); task' is None for a parent that is no plan (the later Nones are never reached then)"""
    T = len(A[0])
    is_plan = lambda P: sorted(P[0]) == list(range(T)) and all(0 <= m < M for m in P[1])    # noqa: E731  (every task once, in any order)
    ok = is_plan(A) and (B is None or is_plan(B))
    kind = 0
    if mut_w is not None:
        kind = mref.move_of(mut_w, T, moves)[0]
    if not ok:
        return None, None, kind
    qa, mua = [a // M for a in A[0]], dict(zip(A[0], A[1]))
    if B is None:
        q, mu = qa, dict(mua)
    else:
        qb, mub = [a // M for a in B[0]], dict(zip(B[0], B[1]))
        q = pox(qa, qb, in_s)
        if q is None:
            return None, None, kind
        mu = {a: (mua.get(a, -1) if from_a[a] else mub.get(a, -1)) for a in range(T)}
    if mut_w is not None:
        _, x, y = mref.move_of(mut_w, T, moves)
        if kind == mref.SWAP and y is not None:
            q[x], q[y] = q[y], q[x]
        elif kind == mref.INSERT and y is not None:
            e = q.pop(x)
            q.insert(y, e)
        elif kind == mref.REASSIGN:
            rank = sum(1 for s in range(x) if q[s] == q[x])
            if rank >= M:
                return None, None, kind
            a = q[x] * M + rank
            F = [m for m in range(M) if t_n[a][m] >= 0 and m != mu.get(a, -1)]
            if F:
                mu[a] = F[(mut_w[2] * len(F)) >> 32]
    seen, task = {}, []
    for j in q:
        r = seen.get(j, 0)
        if r >= M:
            return None, None, kind
        task.append(j * M + r)
        seen[j] = r + 1
    mach = [mu.get(a, -1) for a in task]
    if any(m < 0 for m in mach):
        return None, None, kind
    return task, mach, kind


def offspring(t, task, mach, obj, best, P, seed, generation, first_instance, cross_thr, mut_thr, moves):
    """t [N,T,M]; task, mach [N*P,T]: the population, member c of group n = row n*P + c; obj [N*P] f64 (NaN: not eligible); best [N]
    or None -> (task [N*P,T], mach [N*P,T], parent [N*P,2] int32, kind [N*P] int8)"""
    t, task, mach = np.asarray(t), np.asarray(task), np.asarray(mach)
    B, T = task.shape
    N, M = B // P, t.shape[2]
    J = T // M
    out_t, out_m = np.full((B, T), -1, np.int32), np.full((B, T), -1, np.int32)
    parent, kind = np.full((B, 2), -1, np.int32), np.full(B, -1, np.int8)
    for n in range(N):
        tn, inst = t[n].tolist(), (int(first_instance) + n) & 0xFFFFFFFFFFFFFFFF
        rows = [(task[n * P + c].tolist(), mach[n * P + c].tolist()) for c in range(P)]
        for c in range(P):
            g = n * P + c
            if best is not None and c == 0:
                col = int(best[n])
                e = rows[col - n * P] if n * P <= col < (n + 1) * P else rows[0]
                if all(0 <= a < T for a in e[0]) and all(0 <= m < M for m in e[1]):
                    out_t[g], out_m[g] = e
                continue
            w = words(seed, generation, inst, c, TAG_PARE)
            i = [(x * P) >> 32 for x in w]
            a, b = better(obj[n * P:(n + 1) * P], i[0], i[1]), better(obj[n * P:(n + 1) * P], i[2], i[3])
            v = words(seed, generation, inst, c, TAG_CROS)
            cross, mut = v[0] < cross_thr, v[1] < mut_thr
            parent[g] = (n * P + a, n * P + b if cross else -1)
            in_s = stream_bits(seed, generation, inst, c, TAG_JSET, J) if cross else None
            from_a = stream_bits(seed, generation, inst, c, TAG_MACH, T) if cross else None
            mw = mref.draw(seed, generation, inst, c) if mut else None
            ct, cm, kd = child(tn, rows[a], rows[b] if cross else None, in_s, from_a, mw, moves, M)
            kind[g] = kd
            if ct is not None:
                out_t[g], out_m[g] = ct, cm
    return out_t, out_m, parent, kind


def search(data, start, P, generations, seed, p_cross=0.8, p_mut=0.3, moves=mref.ALL_MOVES, left_shift=False, w=(0.4, 0.4, 0.2), first_instance=0):
    """baselines.evolve on the host: start = one (task, mach) [N,T] or a list of them -> dict(start_obj [N], history [generations,N],
    plans (task, mach) [N,T], cost {key: [N]}, final4 [N,4], obj [N], parents [generations, N*P, 2], kinds [generations, N*P])"""
    t = np.asarray(data[0])
    N, T = t.shape[0], t.shape[1]
    starts = [start] if len(start) == 2 and np.ndim(start[0]) == 2 else list(start)
    member = np.arange(P) % len(starts)
    task = np.stack([np.asarray(s[0], np.int32) for s in starts], 1)[:, member].reshape(N * P, T)
    mach = np.stack([np.asarray(s[1], np.int32) for s in starts], 1)[:, member].reshape(N * P, T)
    cross_thr, mut_thr = int(round(p_cross * 2 ** 32)), int(round(p_mut * 2 ** 32))
    rep = tuple(np.repeat(np.asarray(x), P, axis=0) for x in data)
    history, parents, kinds = [], [], []
    for g in range(generations + 1):
        if g:
            task, mach, par, kd = offspring(t, task, mach, obj, best, P, seed, g, first_instance, cross_thr, mut_thr, moves)
            parents.append(par); kinds.append(kd)
        _, final4, done, _ = mref.replay(rep, task, mach, left_shift, w)
        obj, best, best_obj, _ = gref.group_reduce(final4, done, w, N, P)
        history.append(best_obj)
    pick = np.where(best < 0, np.arange(N) * P, best)
    task, mach = task[pick], mach[pick]
    cum, final4, done, obj = mref.replay(data, task, mach, left_shift, w)
    assert done.all()
    return dict(start_obj=history[0], history=np.array(history[1:]).reshape(generations, N), plans=(task, mach),
                cost={key: cum[:, i] for i, key in enumerate(COST_KEYS)}, final4=final4, obj=obj,
                parents=np.array(parents, np.int32).reshape(generations, N * P, 2), kinds=np.array(kinds, np.int8).reshape(generations, N * P))


def evo_lds_bytes(T, J, tile):
    """csrc/mtfjsp_evolve.hip's evo_lds_bytes restated: the tile's cells and, per wave, six u16 / i16 arrays of T, the job counts and the
    two bit maps (the job set: J bits, the machine coins: T bits)"""
    return T * (tile + 1) * 4 + 4 * (T * 12 + J * 4 + ((J + 31) // 32 + (T + 31) // 32) * 4)


def evo_launch(J, M):
    """-> (tile, bytes, accepted) of mtfjsp_plan_offspring's launch (tests/plan_moves_ref.py: choose_tile)"""
    return mref.choose_tile(lambda tile: evo_lds_bytes(J * M, J, tile))
