"""No GPU: the table of tests/test_env_insertions_gpu.py cannot pass vacuously.  The dispatch sends every row to the kernel it names,
the rows cover the seven step kernels in both observation types and end in a ragged group, and the oracle alone, run over each
row's exact instances and actions (env_parity.oracle_walk), takes the front and the gap insertion often enough and — on integer data
— meets decisive ties of all three kinds (OracleBatch.ties).  These are conditions on the inputs, not tolerances: a seed that misses
one is replaced, the threshold stays.

Measured over the table (share of all steps): "blocks" front 3.9 to 8.3 %, gap 20.7 to 50.3 %; "jobseq" front 4.6 to 12.9 %, gap
22.2 to 43.8 %; on integer data 2 to 92 decisive ties of each kind per batch, in 6 of 11 to 19 of 19 instances (the batch of three:
1 to 5 of each kind, in 3 of 3 and 2 of 3).  The test prints the figures of every row.
"""
import functools
import hashlib

import numpy as np
import pytest

from env_parity import dispatch_kernel, oracle_walk
from test_env_insertions_gpu import CASES, FAMILIES, JOBSEQ, ROWS, case_id
from trace_utils import load

GROUP = {"k_env_grp16": 16, "k_env_grp16x2": 16, "k_env_grp4": 4, "k_env_grp4x2": 4, "k_env_step_grp": 8}
KERNELS = ("k_env_grp16", "k_env_grp4", "k_env_grp16x2", "k_env_grp4x2", "k_env_reg", "k_env_step_grp", "k_env_step")
PATH_FRONT, PATH_GAP = 1, 2


@functools.lru_cache(maxsize=None)
def _walk(J, M, E, B, seed, policy, data):
    """rows that differ only in the forced kernel or the observation type share instances and actions: walked once"""
    return oracle_walk(J, M, E, B, left_shift=True, seed=seed, policy=policy, data=data)


INPUTS = sorted({(c.row.J, c.row.M, c.row.E, c.row.B, c.row.seed, c.policy, c.data) for c in CASES})


def test_the_table_reaches_every_kernel_in_both_dtypes():
    for r in ROWS:
        assert dispatch_kernel(r.J, r.M, r.B, r.force) == r.kernel, r
        assert r.M % r.E == 0 and r.B <= 19, r
        if r.kernel in GROUP:
            assert r.B > GROUP[r.kernel] and r.B % GROUP[r.kernel] != 0, r            # at least one full group and a ragged last one
    for policy, data, dtypes in (("blocks", "integer", ("f32", "f64")), ("blocks", "generated", ("f32",))):
        reached = {(c.row.kernel, c.obs_dtype) for c in CASES if (c.policy, c.data) == (policy, data)}
        assert {(k, d) for k in KERNELS for d in dtypes} <= reached, (policy, data)
        assert {c.row for c in CASES if (c.policy, c.data) == (policy, data)} == set(ROWS), "every row runs it"
    for k in ("k_env_grp16x2", "k_env_grp4x2"):                                       # second task slot of every lane empty
        assert any(r.kernel == k and r.J * r.M <= 64 for r in ROWS), k
    assert any(r.kernel == "k_env_step_grp" and r.force is None and r.J * r.M > 256 for r in ROWS), "two reduction levels"
    seq = [c for c in CASES if c.policy == "jobseq"]
    assert sorted(c.row.family for c in seq) == sorted(FAMILIES) and set(JOBSEQ) == set(FAMILIES)
    assert all((c.data, c.obs_dtype) == ("integer", "f32") for c in seq)
    assert len({case_id(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("inputs", INPUTS, ids=lambda x: "J%dM%dE%d-B%d-seed%d-%s-%s" % x)
def test_the_oracle_takes_the_insertions_and_meets_the_ties(inputs):
    J, M, E, B, seed, policy, data = inputs
    T = J * M
    assert T >= 36
    w = _walk(*inputs)
    paths, ties = w["paths"][0], w["ties"][0]
    front, gap = (paths == PATH_FRONT).mean(), (paths == PATH_GAP).mean()
    print(f"J{J}M{M} B={B} {policy} {data}: front {100 * front:.1f} %, gap {100 * gap:.1f} % of {paths.size} steps; decisive ties "
          f"{ties.sum(0).tolist()} in {(ties.sum(1) > 0).sum()} of {B} instances")
    assert set(np.unique(paths)) <= {0, 1, 2, 3}
    assert front >= 0.03 and gap >= 0.10
    if data == "integer":
        assert (ties.sum(0) > 0).all(), ties.sum(0)
        assert 4 * (ties.sum(1) > 0).sum() >= B
    else:
        assert not ties.any(), "products of uniform doubles do not tie"


def test_integer_data_is_exact_in_float32_and_keeps_the_shape_of_an_instance():
    from env_parity import parity_instances
    t0, p0, tt0, _ = parity_instances(6, 6, 2, 19, 3, "generated")
    t, p, tt, _ = parity_instances(6, 6, 2, 19, 3, "integer")
    for x in (t, p, tt):
        assert np.array_equal(x, np.round(x)) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    assert np.array_equal(t < 0, t0 < 0) and np.array_equal(p < 0, p0 < 0) and not (t == 0).any() and not (p == 0).any()
    assert np.abs(t).min() == 1 and np.abs(t).max() == 9
    assert np.array_equal(tt, tt.transpose(0, 2, 1)) and (tt[:, np.arange(6), np.arange(6)] == 0).all() and (tt >= 0).all()
    off = ~np.eye(6, dtype=bool)
    assert (tt[:, off] == 0).any() and (tt[:, off] > 0).any(), "zero transport between some different machines, not all"


def test_the_mask_policy_still_draws_the_actions_it_drew_before():
    """policy="mask", data="generated" (the defaults) is the stream every earlier parity case ran on.  The digest is that of the
    (job, task, machine) sequence of J6M6E2 x 19, seed 3, computed with the driver as it was before it learnt other policies"""
    a = oracle_walk(6, 6, 2, 19, seed=3)["actions"]
    assert a.shape == (1, 36, 19, 3) and a.dtype == np.int32
    assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == MASK_DIGEST


MASK_DIGEST = "11038beef333b7fcd673b968f4f2e5c29dc03221305593b43851c2787fb79587"


def test_mask_free_actions_are_valid_and_follow_their_policy():
    """every job's operations in order and exactly once; "jobseq" finishes a job before the next; "blocks" moves in runs of one
    job, longer than a step and shorter than a job's whole route"""
    for policy in ("blocks", "jobseq"):
        J, M, B = 6, 6, 19
        a = oracle_walk(J, M, 2, B, seed=3, policy=policy, data="integer")["actions"][0]          # [T, B, 3]
        for b in range(B):
            job, task = a[:, b, 0], a[:, b, 1]
            for j in range(J):
                assert np.array_equal(task[job == j], j * M + np.arange(M)), (policy, b, j)
            if policy == "jobseq":
                assert (job.reshape(J, M) == job.reshape(J, M)[:, :1]).all()
            else:
                runs = 1 + np.count_nonzero(np.diff(job))
                assert J < runs < J * M, (b, runs)


TIE_TRACES = ("trace_j6m6e2_int_b8_blocks", "trace_j10m10e2_int_b2_blocks")


@pytest.mark.parametrize("name", TIE_TRACES)
def test_the_reference_tie_traces_hold_every_kind_of_decisive_tie(name):
    """the two traces recorded from the reference on integer data (tests/test_oracle_golden.py pins the oracle to them): by the
    oracle's counters each holds at least one decisive tie of each kind, and takes both insertion paths"""
    from oracle.env_oracle import OracleBatch
    g = load(name)
    J, M, E, B, episodes, left_shift, keep_every = [int(x) for x in g["meta"]]
    assert left_shift == 1 and episodes == 1
    for k in ("t", "p", "tt"):
        assert np.array_equal(g[k], np.round(g[k])), k
    w = g["cfg_w"]
    orc = OracleBatch(g["t"], g["p"], g["tt"], g["edge"], left_shift=True, w_cfg=tuple(w[:3]), divisor=float(w[3]), gamma=float(w[4]), n_job=J)
    orc.scaler_init(); orc.reset(g["w3"][0])
    paths = []
    for s in range(J * M):
        paths.append(orc.step(g["actions"][0, s][:, 0], g["actions"][0, s][:, 1])[2])
    ties = orc.ties()
    paths = np.array(paths)
    print(name, "paths (first, front, gap, append):", [int((paths == k).sum()) for k in range(4)], "decisive ties:", ties.sum(0).tolist())
    assert (ties.sum(0) > 0).all(), ties.sum(0)
    assert (paths == PATH_FRONT).any() and (paths == PATH_GAP).any()
