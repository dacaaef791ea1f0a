"""Host model of mtfjsp_group_reduce and mtfjsp_final_costs (plain module; tests/test_group_reduce_cpu.py pins it against a brute-force
restatement and hand-made cases, tests/test_group_reduce_gpu.py and tests/test_best_of_k_gpu.py hold the device to it bit for bit).
The rule of include/mtfjsp.h is applied literally, copy by copy: N groups of K copies, copy c of group n = element n*K + c."""
import numpy as np


def objectives(cost4, w):
    """cost4 [...,4] (makespan, energy / T, transport, idle), w = (w_mk, w_ec, w_tt) -> (mk, ec, tt, obj), obj in numpy's order of
    `evaluate.validate_cost_batched`: (w_mk*mk + w_ec*ec) + w_tt*tt, every operation a binary64 one"""
    cost4 = np.asarray(cost4, np.float64)
    w = [np.float64(x) for x in w]
    mk, ec, tt = cost4[..., 0], cost4[..., 1] + cost4[..., 3], cost4[..., 2]
    with np.errstate(all="ignore"):
        obj = w[0] * mk + w[1] * ec + w[2] * tt
    return mk, ec, tt, obj


def final_costs(prev, nsched, T):
    """prev [B,4] = the previous-step costs (makespan, e1, transport, idle), nsched [B] scheduled operations -> (cost4, done)"""
    prev = np.asarray(prev, np.float64)
    return np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1), (np.asarray(nsched) == T).astype(np.uint8)


def dominates(a, b, ca, cb):
    """copy ca with objectives a = (mk, ec, tt) dominates copy cb with b"""
    if not (a[0] <= b[0] and a[1] <= b[1] and a[2] <= b[2]):
        return False
    if a[0] < b[0] or a[1] < b[1] or a[2] < b[2]:
        return True
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and ca < cb


def group_reduce(cost4, done, w, N, K):
    """-> obj [N*K] f64 (NaN: not eligible), best [N] int32 (n*K + c, -1: none), best_obj [N] f64 (NaN: none), front [N*K] uint8"""
    cost4 = np.asarray(cost4, np.float64).reshape(N * K, 4)
    done = np.asarray(done).reshape(N * K)
    mk, ec, tt, obj = objectives(cost4, w)
    elig = (done != 0) & ~np.isnan(mk) & ~np.isnan(ec) & ~np.isnan(tt)
    obj = np.where(elig, obj, np.nan)
    best = np.full(N, -1, np.int32)
    best_obj = np.full(N, np.nan)
    front = np.zeros(N * K, np.uint8)
    idx = np.arange(K)
    for n in range(N):
        g = slice(n * K, (n + 1) * K)
        gm, ge, gt, go, gel = mk[g], ec[g], tt[g], obj[g], elig[g]
        pick = -1
        for c in range(K):                                              # ascending, strict: ties stay with the lowest c
            if gel[c] and go[c] == go[c] and (pick < 0 or go[c] < go[pick]):
                pick = c
        if pick >= 0:
            best[n], best_obj[n] = n * K + pick, go[pick]
        for c in range(K):
            if not gel[c]:
                continue
            with np.errstate(invalid="ignore"):
                le = (gm <= gm[c]) & (ge <= ge[c]) & (gt <= gt[c])
                lt = (gm < gm[c]) | (ge < ge[c]) | (gt < gt[c])
                eq = (gm == gm[c]) & (ge == ge[c]) & (gt == gt[c])
            dom = gel & le & (lt | (eq & (idx < c)))
            front[n * K + c] = 0 if dom.any() else 1
    return obj, best, best_obj, front


def synthetic(kind, N, K, seed):
    """test data -> cost4 [N*K,4], done [N*K] uint8.  "integer": costs 0..2, ties and duplicates everywhere; "random": binary64
    draws; "scattered": integer costs with done = 0 and NaN scattered through them and (N > 1) group 1 without any eligible copy;
    "none": nothing eligible at all"""
    rs = np.random.RandomState(seed)
    if kind == "random":
        cost4 = rs.uniform(0.0, 1000.0, (N * K, 4))
    else:
        cost4 = rs.randint(0, 3, (N * K, 4)).astype(np.float64)
    done = np.ones(N * K, np.uint8)
    if kind == "scattered":
        done = (rs.uniform(size=N * K) > 0.3).astype(np.uint8) * rs.randint(1, 256, N * K).astype(np.uint8)
        cost4[rs.uniform(size=(N * K, 4)) < 0.05] = np.nan
        if N > 1:
            done[K:2 * K:2] = 0
            cost4[K + 1:2 * K:2, 2] = np.nan
    elif kind == "none":
        done[:] = 0
    return cost4, done
