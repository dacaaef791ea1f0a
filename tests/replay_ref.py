"""Host model of the launch rule of mtfjsp_replay_plans (plain module; tests/test_replay_select_cpu.py holds
capi.replay_launch_info_for to it), the cases the GPU tests of the one-launch replay share, numpy's pairwise sum restated, and the table of
launch forms (FORM_ROWS) of tests/test_replay_forms_cpu.py and _gpu.py.  The rule is restated from include/mtfjsp.h and the layout comment
of csrc/mtfjsp_replay.hip, not read from the library."""
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


def spoil_at(task, mach, t, M, cols):
    """task, mach [B,T] valid plans of the instances t [B,T,M] -> copies of them with the columns cols = (range, twice, swap, neg)
    spoiled, None = that kind not at all.  range: a task out of range at step 0; twice: a task twice in the middle; swap: a job's second
    operation before its first; neg: a machine with t < 0 (valid, scheduled like any duration: that copy finishes)"""
    task, mach = task.copy(), mach.copy()
    B, T = task.shape
    c_range, c_twice, c_swap, c_neg = cols
    if c_range is not None:
        task[c_range, 0] = T
    if c_twice is not None:
        task[c_twice, T // 2] = task[c_twice, T // 2 - 1]
    if c_swap is not None:
        b = c_swap
        first = np.flatnonzero(task[b] % M == 0)[0]             # a first operation; its successor's step comes later: swap the two
        second = np.flatnonzero(task[b] == task[b, first] + 1)[0]
        task[b, [first, second]] = task[b, [second, first]]
        mach[b, [first, second]] = mach[b, [second, first]]
    if c_neg is not None:
        b = c_neg
        s = next(s for s in range(T) if (t[b, task[b, s]] < 0).any())
        mach[b, s] = int(np.flatnonzero(t[b, task[b, s]] < 0)[0])
    return task, mach


def spoil(task, mach, t, M):
    """spoil_at with the columns of the 15-copy cases: 1: out of range; 4: twice; 7: swapped; 10: t < 0 -> task, mach, the columns"""
    cols = (1, 4, 7, 10)
    return spoil_at(task, mach, t, M, cols) + (cols,)


# ---- numpy's pairwise sum restated (numpy/core/src/umath/loops_utils.h.src, pairwise_sum): what the energy sum of the kernels must
# reproduce to the bit.  Written from its rule, not read from the library
def pairwise_leaves(T, off=0):
    """-> [(offset, length)] of the blocks numpy sums with 8 accumulators: a block of at most 128 elements is one leaf, a longer one
    is split at n // 2 rounded down to a multiple of 8, left half first"""
    if T <= 128:
        return [(off, T)]
    n2 = T // 2
    n2 -= n2 % 8
    return pairwise_leaves(n2, off) + pairwise_leaves(T - n2, off + n2)


def leaf_sum(x):
    """one leaf: fewer than 8 elements left to right from 0.0; else 8 accumulators over the multiples of 8, combined
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the ragged tail in order"""
    x = np.asarray(x, np.float64)
    n = len(x)
    if n < 8:
        res = np.float64(0.0)
        for v in x:
            res = res + v
        return res
    r = [x[k] for k in range(8)]
    nb = n - n % 8
    for i in range(8, nb, 8):
        for k in range(8):
            r[k] = r[k] + x[i + k]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(nb, n):
        res = res + x[i]
    return res


def pairwise_sum(x, order="recursion"):
    """np.sum(x) of a contiguous float64 vector by the rule above.  order="index": the leaves' sums added left to right instead of in
    the recursion's order (a wrong model: tests use it to show that the cases tell the two apart)"""
    x = np.asarray(x, np.float64)
    if order == "index":
        sums = [leaf_sum(x[o:o + n]) for o, n in pairwise_leaves(len(x))]
        res = sums[0]
        for s in sums[1:]:
            res = res + s
        return res
    n = len(x)
    if n <= 128:
        return leaf_sum(x)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(x[:n2]) + pairwise_sum(x[n2:])


# ---- the forms of the launch, one row each: (J, M, E, B, G, launch_bytes, nleaf, what) where a workgroup may use LDS_CU = 163840 bytes.
# G and launch_bytes follow from `launch`, nleaf from `pairwise_leaves`; tests/test_replay_forms_cpu.py holds the rows to both and to
# the library, tests/test_replay_forms_gpu.py runs every row.  E (edges per instance) as the large-shape rows of the environment.
FORM_ROWS = (
    (3, 2, 1, 5, 4, 2304, 1, "T = 6 < 8: no accumulator block, nothing is shuffled"),
    (1, 8, 1, 5, 4, 4608, 1, "J = 1, T = 8: one accumulator block, no ragged tail"),
    (16, 8, 2, 5, 4, 34624, 1, "T = 128: the full leaf block, the longest accumulator chain"),
    (2, 64, 4, 5, 1, 41744, 1, "M = 64: every lane live in the idle scan; G = 1 by the transport matrix at T = 128"),
    (43, 3, 1, 5, 4, 33920, 2, "T = 129: the first shape past one leaf (64, 65)"),
    (14, 15, 3, 7, 4, 60992, 2, "four copies above 48 KB (104, 106)"),
    (17, 16, 2, 7, 2, 38496, 4, "G = 2 below 48 KB, ragged last workgroup"),
    (20, 20, 4, 5, 2, 56832, 4, "G = 2 above 48 KB (96, 104, 96, 104)"),
    (35, 15, 3, 3, 1, 34928, 5, "G = 1 by LDS, an odd leaf count"),
    (52, 20, 4, 3, 1, 68224, 10, "a second pass over the leaves, partly filled"),
    (24, 64, 4, 2, 1, 129136, 16, "M = 64 at large T"),
    (162, 16, 2, 2, 1, 163664, 32, "the largest shape the launch accepts at M = 16"),
    (6, 6, 2, 1, 1, 2656, 1, "batch rule: B = 1"),
    (6, 6, 2, 2, 2, 5312, 1, "batch rule: B = 2"),
    (6, 6, 2, 4, 4, 10624, 1, "batch rule: one full workgroup"),
    (6, 6, 2, 8, 4, 10624, 1, "batch rule: two full workgroups"),
)
REFUSED = (163, 16, 2, 2)                # (J, M, E, B): 164 656 bytes for one copy, 816 more than a workgroup may have
EMPTY, FRONT, BETWEEN, APPEND = 0, 1, 2, 3      # the oracle's path words
# the path words the integer plans of a row (form_case) must reach under left shift, and do: all four, except where the shape rules
# one out.  J = 1: every operation arrives after its job predecessor, which ends after everything its machine holds: never the
# front, never a gap.  3x2: a gap can exist with six operations on two machines, but the walk's five plans reach only the front.
FORM_PATHS = {(1, 8): (EMPTY, APPEND), (3, 2): (EMPTY, FRONT, APPEND)}
ALL_PATHS = (EMPTY, FRONT, BETWEEN, APPEND)


# spoil_at's columns for the partial schedules at G = 2 and G = 1.  17x16, B = 7, workgroups {0,1} {2,3} {4,5} {6}: a task out of range
# in 1 beside the good 0, a task twice in 6 (alone in the ragged last workgroup), a swapped pair in 4 beside the good 5, t < 0 in 2
# beside the good 3.  35x15, B = 3, a workgroup each: a task twice in 0, a swapped pair in 2, 1 good.
SPOIL_COLS = {(17, 16): (1, 6, 4, 2), (35, 15): (None, 0, 2, None)}


def form_id(row):
    J, M, E, B = row[:4]
    return f"J{J}M{M}E{E}-B{B}"


FORM_SEED = 3
_form_cases = {}


def form_case(row, data):
    """the B instances and plans of a row, one instance per copy -> dict(J, M, E, B, inst: (t, p, tt, edge), task, mach [B,T] int32,
    paths [T,B] or None).  "generated": env_parity's generated times with random plans; "integer": its small-integer times (exact ties)
    with the plans of the oracle's mask-free "blocks" walk, whose path words under left shift come along — the plans do not depend on
    the left shift (the walk draws them from its random words alone), so both settings replay the same ones.  Computed once"""
    import env_parity
    import plan_moves_ref as pref
    J, M, E, B = row[:4]
    key = (J, M, E, B, data)
    if key not in _form_cases:
        inst = env_parity.parity_instances(J, M, E, B, FORM_SEED, data)
        if data == "integer":
            w = env_parity.oracle_walk(J, M, E, B, left_shift=True, episodes=1, seed=FORM_SEED, policy="blocks", data="integer")
            act = w["actions"][0]                                       # [T,B,3]
            task, mach, paths = act[:, :, 1].T, act[:, :, 2].T, w["paths"][0]
        else:
            task, mach = pref.random_plans(inst[0], J, M, FORM_SEED + J)
            paths = None
        task, mach = np.ascontiguousarray(task, np.int32), np.ascontiguousarray(mach, np.int32)
        task.setflags(write=False); mach.setflags(write=False)
        _form_cases[key] = dict(J=J, M=M, E=E, B=B, inst=inst, task=task, mach=mach, paths=paths)
    return _form_cases[key]
