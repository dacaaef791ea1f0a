"""Host model of mtfjsp_plan_neighbours and of baselines.local_search (plain module; tests/test_plan_moves_cpu.py pins it,
tests/test_plan_neighbours_gpu.py and tests/test_local_search_gpu.py hold the device to it element for element).
The rule of include/mtfjsp.h is applied literally with Python lists, one copy at a time; `search` drives the C oracle and the host
model of the group reduction (tests/group_reduce_ref.py)."""
import numpy as np

import device_streams_ref as sref
import group_reduce_ref as gref

TAG_MOVE = 0x6d6f7665
SWAP, INSERT, REASSIGN = 1, 2, 4
ALL_MOVES = 7
COST_KEYS = ("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")


def draw(seed, rnd, instance, c):
    """the four Philox words of copy c >= 1 of global instance `instance` in round `rnd` (only the low words of both enter)"""
    s0, s1 = sref._lo_hi(seed)
    return [int(x) for x in sref.philox4x32(int(instance) & 0xFFFFFFFF, int(c), int(rnd) & 0xFFFFFFFF, TAG_MOVE, s0, s1)]


def move_of(w, T, moves):
    """-> (kind, x, y) the draw names; y is None for REASSIGN"""
    bits = [b for b in (SWAP, INSERT, REASSIGN) if moves & b]
    kind = bits[(w[0] * len(bits)) >> 32]
    x = (w[1] * T) >> 32
    if kind == REASSIGN or T < 2:
        return kind, x, None
    y = (w[2] * (T - 1)) >> 32
    return kind, x, y + (1 if y >= x else 0)


def decode(q, mu, M):
    """job string and machine per task -> (task, mach) per step"""
    seen, task = {}, []
    for j in q:
        task.append(j * M + seen.get(j, 0))
        seen[j] = seen.get(j, 0) + 1
    return task, [mu[a] for a in task]


def neighbour(t_n, task, mach, w, moves):
    """one copy c >= 1: the incumbent (task, mach) lists of an instance with times t_n [T,M] after the move the words w name
    -> (task', mach', kind)"""
    T, M = len(task), len(t_n[0])
    q = [a // M for a in task]
    mu = dict(zip(task, mach))
    kind, x, y = move_of(w, T, moves)
    if kind == SWAP and y is not None:
        q[x], q[y] = q[y], q[x]
    elif kind == INSERT and y is not None:
        e = q.pop(x)
        q.insert(y, e)
    elif kind == REASSIGN:
        a = task[x]
        F = [m for m in range(M) if t_n[a][m] >= 0 and m != mu[a]]
        if F:
            mu[a] = F[(w[2] * len(F)) >> 32]
    task2, mach2 = decode(q, mu, M)
    return task2, mach2, kind


def neighbours(t, task, mach, K, seed, round, first_instance, moves):
    """t [N,T,M]; task, mach [N,T]: the incumbents -> (task [N*K,T], mach [N*K,T], kind [N*K] int8), copy c of group n = row n*K + c"""
    t, task, mach = np.asarray(t), np.asarray(task), np.asarray(mach)
    N, T = task.shape
    out_t, out_m, kind = np.zeros((N * K, T), np.int32), np.zeros((N * K, T), np.int32), np.full(N * K, -1, np.int8)
    for n in range(N):
        tn, inc_t, inc_m = t[n].tolist(), task[n].tolist(), mach[n].tolist()
        out_t[n * K], out_m[n * K] = inc_t, inc_m
        for c in range(1, K):
            w = draw(seed, round, (int(first_instance) + n) & 0xFFFFFFFFFFFFFFFF, c)
            out_t[n * K + c], out_m[n * K + c], kind[n * K + c] = neighbour(tn, inc_t, inc_m, w, moves)
    return out_t, out_m, kind


def first_feasible_plan(t):
    """the start plan of the tests: tasks 0..T-1 in order, each on its first feasible machine -> (task [N,T], mach [N,T]) int32"""
    t = np.asarray(t)
    N, T, _ = t.shape
    return np.tile(np.arange(T, dtype=np.int32), (N, 1)), np.argmax(t >= 0, axis=2).astype(np.int32)


def random_plans(t, J, M, seed):
    """a random valid plan per instance: a shuffled job string, every task on a random feasible machine"""
    rs = np.random.RandomState(seed)
    N, T = t.shape[0], J * M
    task, mach = np.zeros((N, T), np.int32), np.zeros((N, T), np.int32)
    for n in range(N):
        q = rs.permutation(np.repeat(np.arange(J), M))
        tk, _ = decode(q.tolist(), {a: 0 for a in range(T)}, M)
        task[n] = tk
        mach[n] = [rs.choice(np.flatnonzero(t[n, a] >= 0)) for a in tk]
    return task, mach


def replay(data, task, mach, left_shift, w):
    """the C oracle on the instances `data` driven by the plans task, mach [B,T] -> (cum [B,5], final4 [B,4], done [B], obj [B])"""
    from oracle.env_oracle import OracleBatch
    t, p, tt, edge = data
    B, T = task.shape
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=w)
    orc.scaler_init()
    orc.reset(np.tile(np.array([w], np.float64), (B, 1)))
    cum = np.zeros((B, 5))
    for s in range(T):
        cum += orc.step(task[:, s], mach[:, s])[1]
    st = orc.state()
    final4, done = gref.final_costs(st["prev"], st["sched"].astype(np.int64).sum(1), T)
    return cum, final4, done, gref.objectives(final4, w)[3]


def search(data, start, K, rounds, seed, moves=ALL_MOVES, left_shift=False, w=(0.4, 0.4, 0.2), first_instance=0):
    """baselines.local_search on the host: -> dict(start_obj [N], history [rounds,N], accepted [rounds,N] int8, plans (task, mach)
    [N,T], cost {key: [N]}, final4 [N,4], obj [N])"""
    t = np.asarray(data[0])
    N = t.shape[0]
    task, mach = np.array(start[0], np.int32), np.array(start[1], np.int32)
    rep = tuple(np.repeat(np.asarray(x), K, axis=0) for x in data)
    history, accepted, start_obj = [], [], None
    for r in range(rounds):
        nt, nm, kind = neighbours(t, task, mach, K, seed, r, first_instance, moves)
        _, final4, done, _ = replay(rep, nt, nm, left_shift, w)
        obj, best, best_obj, _ = gref.group_reduce(final4, done, w, N, K)
        assert (best >= 0).all()
        if r == 0:
            start_obj = obj[::K].copy()
        history.append(best_obj)
        accepted.append(np.where(best % K == 0, -1, kind[best]).astype(np.int8))
        task, mach = nt[best], nm[best]
    cum, final4, done, obj = replay(data, task, mach, left_shift, w)
    assert done.all()
    return dict(start_obj=obj.copy() if start_obj is None else start_obj, history=np.array(history).reshape(rounds, N),
                accepted=np.array(accepted, np.int8).reshape(rounds, N), plans=(task, mach),
                cost={key: cum[:, i] for i, key in enumerate(COST_KEYS)}, final4=final4, obj=obj)


# ---- the launch of the plan kernels, restated from csrc/mtfjsp_plan_dev.h and csrc/mtfjsp_plan.hip (for the tests that are written to
# reach one tile or one side of a limit: they assert these numbers, so a case that moves to another branch fails instead of passing)
PLAN_LDS_SOFT, PLAN_LDS_HARD, PLAN_LDS_ASK = 64 * 1024, 160 * 1024, 48 * 1024      # two workgroups per CU | all a workgroup can have | above: asked for


def plan_lds_bytes(T, J, tile, crit=False):
    """the tile's cells (odd pitch), four waves' position map and job counts, with a critical path three more arrays per wave"""
    return T * (tile + 1) * 4 + 4 * (T * 4 + J * 4) + (4 * T * 6 if crit else 0)


def choose_tile(nbytes):
    """nbytes(tile) -> (tile, bytes, accepted): the largest of 64, 32, 16 that stays within PLAN_LDS_SOFT, else 16, which may use up to
    PLAN_LDS_HARD"""
    tile = 64
    while tile > 16 and nbytes(tile) > PLAN_LDS_SOFT:
        tile >>= 1
    return tile, nbytes(tile), nbytes(tile) <= PLAN_LDS_HARD


def plan_launch(J, M, crit=False):
    return choose_tile(lambda tile: plan_lds_bytes(J * M, J, tile, crit))
