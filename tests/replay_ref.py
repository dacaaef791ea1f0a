"""Host model of the launch rule of mtfjsp_replay_plans (plain module; tests/test_replay_select_cpu.py holds
capi.replay_launch_info_for to it) and the cases the GPU tests of the one-launch replay share.
The rule is restated from include/mtfjsp.h and the layout comment of csrc/mtfjsp_replay.hip, not read from the library."""
import numpy as np

GMAX = 4                                # copies (waves) per workgroup at most
LDS_SOFT = 64 * 1024                    # the regions of a workgroup stay within this: two workgroups per CU
LDS_CU = 160 * 1024                     # gfx950: what one workgroup may have
BYTES_PER_TASK = 6 * 8 + 7 * 2          # st, ft, pte, d, pk, tr (f64) | mach, prev, pos, plan task, plan machine, mu, pm (i16)


def region_bytes(J, M):
    """one copy's LDS region: the per-task arrays over T rounded up to 4, the transport matrix, the per-machine and per-job words"""
    T = J * M
    Tp = (T + 3) & ~3
    off = 6 * Tp * 8 + M * M * 8 + (4 * M + 1 + J) * 4
    off = (off + 7) & ~7
    off += 7 * Tp * 2
    return (off + 15) & ~15


def launch(J, M, batch, lds_max=LDS_CU):
    """-> (G, dynamic LDS bytes), or None where one copy does not fit lds_max"""
    nb = region_bytes(J, M)
    if nb > lds_max:
        return None
    soft = min(LDS_SOFT, lds_max)
    g = GMAX
    while g > 1 and (g * nb > soft or g >= 2 * batch):
        g >>= 1
    return g, g * nb


def fits(J, M, lds_max=LDS_CU):
    """derived from the layout's bytes per task alone: a lower bound of the region that already decides the largest shapes"""
    return BYTES_PER_TASK * J * M + 8 * M * M <= lds_max and region_bytes(J, M) <= lds_max


# ---- the GPU cases: N = 3 instances x 5 copies = 15 columns, a ragged last workgroup for any G > 1
N_INST, N_COPY = 3, 5
SHAPES = {"J3M4": (3, 4, 2), "J6M6": (6, 6, 2), "J5M13": (5, 13, 1), "J9M15": (9, 15, 3), "J65M2": (65, 2, 2)}
CONFIG_W = (0.4, 0.4, 0.2)


def spoil(task, mach, t, M):
    """task, mach [B,T] valid plans of the instances t [B,T,M] -> copies of them with four columns spoiled, and the columns:
    1: a task out of range at step 0; 4: a task twice in the middle; 7: a job's second operation before its first; 10: a machine
    with t < 0 (valid, scheduled like any duration: that copy finishes)"""
    task, mach = task.copy(), mach.copy()
    B, T = task.shape
    task[1, 0] = T
    task[4, T // 2] = task[4, T // 2 - 1]
    b = 7
    first = np.flatnonzero(task[b] % M == 0)[0]                 # a first operation; its successor's step comes later: swap the two
    second = np.flatnonzero(task[b] == task[b, first] + 1)[0]
    task[b, [first, second]] = task[b, [second, first]]
    mach[b, [first, second]] = mach[b, [second, first]]
    b = 10
    s = next(s for s in range(T) if (t[b, task[b, s]] < 0).any())
    mach[b, s] = int(np.flatnonzero(t[b, task[b, s]] < 0)[0])
    return task, mach, (1, 4, 7, 10)
