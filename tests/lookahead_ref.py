"""Host model of the one-step look-ahead rules (plain module; tests/test_lookahead_cpu.py pins it, tests/test_lookahead_gpu.py holds
the device to it).  The oracle has no fork, so a decision is made the long way, the way the reference's idle-time rule does it
(tester/pdrs.py:465-540): per step, an OracleBatch of T replicas of every source instance — replica (j, m) tries "job j's candidate
task on machine m" — is reset, replays the whole prefix and takes the candidate step; replicas of a job whose mask (job_mask_state: 1 = finished) is set or of an
infeasible machine (t < 0) do not count; the first index of the maximal raw[column] wins (`select`).  About B*T^3/2 oracle steps per episode.
"""
import functools

import numpy as np

from oracle.env_oracle import OracleBatch


def replicas(x, T):
    return np.repeat(np.asarray(x), T, axis=0)


def select(values, counts):
    """the selection rule, on one row: values[c] is copy c's value, counts[c] whether copy c counts.  -> the lowest index among the
    counting copies whose value is not NaN and is not exceeded by any other counting, non-NaN value (a NaN is never selected; -inf
    is a value like any other), or None where there is none.  The winning value is values[index] itself — it is never the result
    of a max, so a -0.0 that ties with a +0.0 stays -0.0.  Plain Python comparisons, one copy at a time"""
    vals, pick = np.asarray(values, np.float64).tolist(), None
    for c, ok in enumerate(np.asarray(counts, bool).tolist()):
        if ok and vals[c] == vals[c] and (pick is None or vals[c] > vals[pick]):
            pick = c
    return pick


def model_step(t, p, tt, edge, w3, prefix, column, left_shift=True, w_cfg=(0.4, 0.4, 0.2)):
    """prefix: list of (task[B], mach[B]) already dispatched.  -> (task[B], mach[B], best[B], values[B,T], valid[B,T]): the model's
    pick for the next step, its value, and every replica's raw[column] with the mask of the replicas that count"""
    t = np.asarray(t, np.float64)
    B, T, M = t.shape
    J = T // M
    orc = OracleBatch(replicas(t, T), replicas(p, T), replicas(tt, T), replicas(edge, T), left_shift=left_shift, w_cfg=w_cfg)
    orc.scaler_init()
    orc.reset(replicas(w3, T))
    for task, mach in prefix:
        orc.step(replicas(task, T), replicas(mach, T))
        orc.job_mask_update(replicas(np.asarray(task) // M, T))
    cand, mask = orc.job_mask_state()
    cand, mask = cand.reshape(B, T, J)[:, 0], mask.reshape(B, T, J)[:, 0]
    jj, mm = np.divmod(np.arange(T), M)                                  # replica c = (j, m)
    task_c = cand[:, jj]                                                 # [B,T]
    valid = (mask[:, jj] == 0) & (t[np.arange(B)[:, None], task_c, mm[None, :]] >= 0)
    assert valid.any(1).all(), "the model is asked only about running instances"
    first = valid.argmax(1)                                              # replicas that do not count take a valid action instead
    act_t = np.where(valid, task_c, task_c[np.arange(B), first][:, None]).astype(np.int32)
    act_m = np.where(valid, mm[None, :], mm[first][:, None]).astype(np.int32)
    _, raw, _ = orc.step(act_t.reshape(-1), act_m.reshape(-1))
    values = raw.reshape(B, T, 5)[:, :, column]
    pick = [select(values[b], valid[b]) for b in range(B)]
    assert None not in pick, "a running instance has a counting copy with a value"
    pick = np.array(pick)
    best = values[np.arange(B), pick]                                    # the picked copy's own value
    return task_c[np.arange(B), pick].astype(np.int32), mm[pick].astype(np.int32), best, values, valid


def model_episode(t, p, tt, edge, w3, column, left_shift=True, w_cfg=(0.4, 0.4, 0.2), shared=None):
    """-> (task[T,B], mach[T,B], best[T,B]): the model's whole episode.  shared: a list that receives, per step, how many
    instances had their maximum at more than one counting replica (the decisions that "first index" made)"""
    T = np.asarray(t).shape[1]
    prefix, best = [], []
    for _ in range(T):
        a, m, b, values, valid = model_step(t, p, tt, edge, w3, prefix, column, left_shift, w_cfg)
        prefix.append((a, m)); best.append(b)
        if shared is not None:
            shared.append(int(((valid & (values == b[:, None])).sum(1) > 1).sum()))
    return np.stack([x[0] for x in prefix]), np.stack([x[1] for x in prefix]), np.stack(best)


CONFIG_W = (0.4, 0.4, 0.2)


SHARED_MAXIMA = {}                    # cached_episode's arguments -> decisions of that episode whose maximum several replicas shared


@functools.lru_cache(maxsize=None)
def cached_episode(J, M, E, B, column, left_shift, data="generated", w_cfg=CONFIG_W):
    """the model's episode on the test instances of a shape, computed once per session and shared; w_cfg: the configuration's reward
    weights (w_mk, w_ec, w_tt), which are also every instance's own (pdrs:675).
    data="integer": the same instances with small-integer times (env_parity.integer_data), where replicas tie"""
    from importlib import import_module
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    t, p, tt, edge = inst.generate_instances(B, J, M, E, seed=4200 + J * 100 + M)
    if data == "integer":
        from env_parity import integer_data
        t, p, tt = integer_data(t, p, tt)
    w3 = np.tile(np.array([w_cfg], np.float64), (B, 1))
    shared = []
    task, mach, best = model_episode(t, p, tt, edge, w3, column, left_shift, w_cfg, shared)
    SHARED_MAXIMA[(J, M, E, B, column, left_shift, data) + (() if w_cfg == CONFIG_W else (w_cfg,))] = sum(shared)
    for x in (t, p, tt, edge, w3, task, mach, best):
        x.setflags(write=False)
    return (t, p, tt, edge, w3), task, mach, best
