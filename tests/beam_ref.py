"""Host model of the beam search on the device fork (plain module; tests/test_beam_cpu.py pins it, tests/test_beam_gpu.py and
tests/test_state_signature_gpu.py hold the device to it).  The oracle has no fork, so the model keeps every slot's full prefix and
makes a decision the long way, as tests/lookahead_ref.py does: per step, an OracleBatch of N*W*T replicas — replica (n, w, j, m)
tries "job j's candidate task on machine m" after slot (n, w)'s prefix — is reset, replays the prefixes and takes the candidate
step.  Replicas that do not count (an empty slot, a finished job, an infeasible machine) take some valid action instead.  The
selection rule of include/mtfjsp.h (mtfjsp_beam_select) is then applied literally, in Python, candidate by candidate.
About N*W*T^3/2 oracle steps per episode.
"""
import functools

import numpy as np

from oracle.env_oracle import OracleBatch

CONFIG_W = (0.4, 0.4, 0.2)
_U = np.uint64


def mix(z):
    """the splitmix64 finaliser on uint64 arrays (the products wrap mod 2^64)"""
    z = np.array(z, dtype=np.uint64)
    z ^= z >> _U(30); z *= _U(0xbf58476d1ce4e5b9)
    z ^= z >> _U(27); z *= _U(0x94d049bb133111eb)
    z ^= z >> _U(31)
    return z


def positions(routes):
    """routes [B,M,T] (task indices in processing order, -1 padded) -> pos [B,T]: rank of every task in its machine's route (0 where unscheduled)"""
    B, M, T = routes.shape
    pos = np.zeros((B, T), np.int64)
    b, m, i = np.nonzero(routes >= 0)
    pos[b, routes[b, m, i]] = i
    return pos


def signature(mach, sched, st, routes):
    """[B] uint64: sum over the scheduled tasks k of mix(mix(bits64(st_k)) + (k << 32 | mach_k << 16 | pos_k)) mod 2^64"""
    mach, st = np.asarray(mach), np.ascontiguousarray(st, np.float64)
    B, T = mach.shape
    sched = np.asarray(sched).astype(bool)
    assert np.array_equal(sched, mach >= 0)
    where = (np.arange(T, dtype=np.uint64)[None, :] << _U(32)) | (np.where(sched, mach, 0).astype(np.uint64) << _U(16)) | positions(routes).astype(np.uint64)
    c = mix(mix(st.view(np.uint64)) + where)
    return np.where(sched, c, _U(0)).sum(axis=1, dtype=np.uint64)


def state_signature(state):
    """signature of orc.state()"""
    return signature(state["mach"], state["sched"], state["st"], state["routes"])


def select(values, eligible, sigs, W):
    """the selection rule for ONE source instance: values [C] f64, eligible [C] bool, sigs [C] uint64 or None -> list of W picks,
    each a candidate index c or None (a rank left without a candidate)"""
    alive = [c for c in range(len(values)) if eligible[c] and values[c] == values[c]]      # a NaN is never selected
    picks = []
    for _ in range(W):
        if not alive:
            picks.append(None)
            continue
        best = alive[0]
        for c in alive[1:]:
            if values[c] > values[best]:                                    # ascending c: the lowest index among equals stays
                best = c
        picks.append(best)
        alive = [c for c in alive if c != best and (sigs is None or sigs[c] != sigs[best])]
    return picks


def model_step(data, prefixes, scores, W, column, dedupe, left_shift, w_cfg=CONFIG_W):
    """prefixes: list [N*W] of lists of (task, mach), None for an empty slot (slot 0 of every instance is never empty); scores [N*W].
    -> dict: parent, from_slot, task, mach [N*W] int32, score [N*W] f64, the next prefixes, and what the pick was made from
    (values, eligible, sigs [N*W*T]; the children's states)"""
    t, p, tt, edge, w3 = data
    N, T, M = t.shape
    J, NW, R = T // M, N * W, N * W * T
    src = np.repeat(np.arange(N), W * T)
    orc = OracleBatch(t[src], p[src], tt[src], edge[src], left_shift=left_shift, w_cfg=w_cfg)
    orc.scaler_init()
    orc.reset(w3[src])
    live = np.array([x is not None for x in prefixes])
    assert live.reshape(N, W)[:, 0].all()
    walk = [prefixes[i] if live[i] else prefixes[i - i % W] for i in range(NW)]               # an empty slot walks slot 0's way
    depth = len(walk[0])
    assert all(len(x) == depth for x in walk)
    for k in range(depth):
        task = np.repeat(np.array([x[k][0] for x in walk], np.int32), T)
        mach = np.repeat(np.array([x[k][1] for x in walk], np.int32), T)
        _, _, path = orc.step(task, mach)
        orc.job_mask_update(task // M)
    cand, mask = orc.job_mask_state()
    cand, mask = cand.reshape(NW, T, J)[:, 0], mask.reshape(NW, T, J)[:, 0]
    jj, mm = np.divmod(np.arange(T), M)                                  # child r = (j, m)
    task_c = cand[:, jj]                                                 # [NW,T]
    can = (mask[:, jj] == 0) & (t[np.arange(N).repeat(W)[:, None], task_c, mm[None, :]] >= 0)
    assert can.any(1).all(), "the model is asked only about running instances"
    first = can.argmax(1)
    act_t = np.where(can, task_c, task_c[np.arange(NW), first][:, None]).astype(np.int32)
    act_m = np.where(can, mm[None, :], mm[first][:, None]).astype(np.int32)
    _, raw, _ = orc.step(act_t.reshape(-1), act_m.reshape(-1))
    eligible = (can & live[:, None] & (scores != -np.inf)[:, None]).reshape(-1)
    values = np.repeat(scores, T) + raw[:, column]                       # one binary64 addition per candidate
    state = orc.state()
    sigs = state_signature(state)
    out = dict(parent=np.full(NW, -1, np.int32), from_slot=np.full(NW, -1, np.int32), task=np.full(NW, -1, np.int32),
               mach=np.full(NW, -1, np.int32), score=np.full(NW, -np.inf), values=values, eligible=eligible, sigs=sigs,
               children={k: state[k] for k in ("mach", "st", "routes")})
    nxt = [None] * NW
    for n in range(N):
        lo = n * W * T
        picks = select(values[lo:lo + W * T], eligible[lo:lo + W * T], sigs[lo:lo + W * T] if dedupe else None, W)
        for k, c in enumerate(picks):
            if c is None:
                continue
            w, r = divmod(c, T)
            i = n * W + k
            out["parent"][i], out["from_slot"][i] = lo + c, w
            out["task"][i], out["mach"][i] = task_c[n * W + w, r], mm[r]
            out["score"][i] = values[lo + c]
            nxt[i] = prefixes[n * W + w] + [(int(task_c[n * W + w, r]), int(mm[r]))]
    out["prefixes"] = nxt
    return out


def start(N, W):
    """the beam before the first decision: one live slot of score 0 per instance"""
    prefixes = [[] if i % W == 0 else None for i in range(N * W)]
    scores = np.where(np.arange(N * W) % W == 0, 0.0, -np.inf)
    return prefixes, scores


def model_episode(data, W, column, dedupe, left_shift, steps=None, w_cfg=CONFIG_W):
    """-> list of the steps' records (model_step's dicts, each with "before": the prefixes and scores it started from)"""
    N, T, _ = data[0].shape
    prefixes, scores = start(N, W)
    recs = []
    for _ in range(T if steps is None else steps):
        rec = model_step(data, prefixes, scores, W, column, dedupe, left_shift, w_cfg)
        rec["before"] = (prefixes, scores)
        recs.append(rec)
        prefixes, scores = rec["prefixes"], rec["score"]
    return recs


def plan_arrays(prefixes, S):
    """final prefixes [N*W] -> (task, mach) [N*W,S] int32, -1 rows for empty slots"""
    task = np.full((len(prefixes), S), -1, np.int32)
    mach = np.full((len(prefixes), S), -1, np.int32)
    for i, x in enumerate(prefixes):
        if x is not None:
            task[i], mach[i] = [a for a, _ in x], [m for _, m in x]
    return task, mach


def tie_rich(data, constant=10.0):
    """the same instances with every feasible processing time overwritten by one constant and no transport times: most candidates
    tie and many orders of decisions meet in one schedule"""
    t, p, tt, edge, w3 = data
    return np.where(t >= 0, constant, t), p, np.zeros_like(tt), edge, w3


@functools.lru_cache(maxsize=None)
def cached_data(J, M, E, N, ties=False, w_cfg=CONFIG_W):
    from importlib import import_module
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    t, p, tt, edge = inst.generate_instances(N, J, M, E, seed=5300 + J * 100 + M)
    data = (t, p, tt, np.asarray(edge), np.tile(np.array([w_cfg], np.float64), (N, 1)))
    if ties:
        data = tie_rich(data)
    data = tuple(np.ascontiguousarray(x) for x in data)
    for x in data:
        x.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def cached_episode(J, M, E, N, W, column, dedupe, left_shift, ties=False, w_cfg=CONFIG_W):
    """the model's episode on the test instances of a shape, computed once per session and shared; w_cfg: the configuration's reward
    weights (w_mk, w_ec, w_tt), which are also every instance's own.  -> (data, records)"""
    data = cached_data(J, M, E, N, ties, w_cfg)
    recs = model_episode(data, W, column, dedupe, left_shift, w_cfg=w_cfg)
    for r in recs:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return data, recs
