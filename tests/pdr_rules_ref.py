"""Plain numpy / Python restatement of the 12 static priority dispatch rules of the reference's tester/pdrs.py (6 operation
rules x 2 machine rules, the pairs test_all.py:484-540 runs), independent of the HIP planner.  tests/test_pdr_rules_cpu.py pins
it to the reference's own lists (tests/golden/pdr_*.npz); the GPU tests then use it as the full-size yardstick.

Every float is binary64 and every sum is taken in the reference's order, because the argmin / argmax decisions below depend on
the last bit: the per-task value is Python's left-to-right `sum` over the positive entries in machine order, the per-job
total is numpy's `np.sum` over a contiguous row (pairwise with 8 accumulators from 8 elements on).
"""
import numpy as np

M_NAMES = ["SPT", "SEC"]                                                          # pdrs.py:729
O_NAMES = ["FIFO", "MOR", "LWKR_T_o", "LWKR_PT_o", "MWKR_T_o", "MWKR_PT_o"]       # pdrs.py:730
RULES = [(f"{O_NAMES[o]}+{M_NAMES[m]}", o, m) for o in range(6) for m in range(2)]   # test_all.py: o_i outer, m_i inner


def machine_rule(t, p, m_rule):
    """[..., T] machine of every task: SPT (0) argmin t, SEC (1) argmin t*|p|; negative entries never win, the first minimum
    does (pdrs.py:46-66).  t, p [..., T, M]."""
    x = np.array(t, np.float64) if m_rule == 0 else np.multiply(t, np.abs(p))
    x[x < 0] = np.inf
    return np.argmin(x, axis=-1).astype(np.int32)


def task_values(t, p, o_rule):
    """[..., T] mean of the positive entries of t (rules 2, 4) or of t*|p| (rules 3, 5), 0 for a task without any
    (pdrs.py:170-178): Python's `sum` adds left to right in machine order, so the loop runs over machines and numpy only
    carries the tasks side by side (0 + e == e: the first add is exact)."""
    x = np.asarray(t, np.float64) if o_rule in (2, 4) else np.multiply(t, np.abs(p))
    s = np.zeros(x.shape[:-1]); n = np.zeros(x.shape[:-1])
    for m in range(x.shape[-1]):
        pos = x[..., m] > 0
        s = np.where(pos, s + x[..., m], s)
        n += pos
    return np.where(n > 0, s / np.maximum(n, 1), 0.0)


def operation_rule(t, p, J, M, o_rule, mor_order=None):
    """[B, T] task of every step for t, p [B,T,M].  mor_order [B,M,J]: the job order of every column (rule 1)."""
    B, T = len(t), J * M
    if o_rule == 0:
        return np.tile(np.arange(T, dtype=np.int32), (B, 1))
    if o_rule == 1:
        mor = np.asarray(mor_order).reshape(B, M, J)
        return (mor * M + np.arange(M)[None, :, None]).reshape(B, T).astype(np.int32)
    most = o_rule >= 4
    v = np.ascontiguousarray(task_values(t, p, o_rule).reshape(B, J, M))
    refer = np.sum(v, axis=2)                       # per job: numpy's add.reduce over a contiguous row of M
    nxt = np.zeros((B, J), np.int64)
    rows = np.arange(B)
    out = np.zeros((B, T), np.int32)
    for s in range(T):
        j = np.argmax(refer, axis=1) if most else np.argmin(refer, axis=1)       # first index on ties
        k = nxt[rows, j]
        if (k > M - 1).any():
            raise IndexError("a finished job was selected again (the reference raises here as well)")
        out[:, s] = j * M + k
        r = refer[rows, j] - v[rows, j, k]
        nxt[rows, j] = k + 1
        refer[rows, j] = np.where((r == 0) | (k + 1 > M - 1), -np.inf if most else np.inf, r)
    return out


def plan(t, p, J, M, o_rule, m_rule, mor_order=None):
    """one instance, t, p [T,M] -> (task[T], mach[T]): the (task, machine) of step s."""
    task, mach = plan_same_rule(np.asarray(t)[None], np.asarray(p)[None], J, M, o_rule, m_rule,
                                None if mor_order is None else np.asarray(mor_order)[None])
    return task[0], mach[0]


def plan_same_rule(t, p, J, M, o_rule, m_rule, mor_order=None):
    """t, p [B,T,M], one rule pair for all -> task, mach [B,T]"""
    task = operation_rule(t, p, J, M, o_rule, mor_order)
    return task, np.take_along_axis(machine_rule(t, p, m_rule), task, axis=1)


def plan_batch(t, p, J, M, o_rule, m_rule, mor_order=None):
    """rules per instance: t, p [B,T,M], o_rule, m_rule [B], mor_order [B,M,J] or None -> task, mach [B,T]"""
    t, p, o_rule, m_rule = np.asarray(t), np.asarray(p), np.asarray(o_rule), np.asarray(m_rule)
    task = np.zeros((len(t), J * M), np.int32); mach = np.zeros_like(task)
    for o in range(6):
        for m in range(2):
            sel = np.nonzero((o_rule == o) & (m_rule == m))[0]
            if len(sel):
                task[sel], mach[sel] = plan_same_rule(t[sel], p[sel], J, M, o, m, None if mor_order is None else np.asarray(mor_order)[sel])
    return task, mach
