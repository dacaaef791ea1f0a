"""No GPU: what tests/test_env_large_shapes_gpu.py rests on.

* Its table is the library's own plan where a workgroup may use 163840 bytes of LDS, the launched bytes are those of the restated size
  functions, the rows hold every group size and both LDS kernels, and every grouped batch ends in a partly filled group.
* The sparse comparison of env_parity.run_parity is as strong as the dense one: at every step of an oracle walk the oracle's ELL
  (observe(dense=False), what the sparse mode compares the device with) holds, row by row, exactly the off-diagonal non-zeros of its
  dense adjacency as (column, value) pairs, no column twice and no zero value, and the diagonal is 1 — the dense matrix is a function of
  the ELL rows taken as sets.
* The "blocks" variants of the smaller shapes reach the front and the gap insertion (conditions on the inputs, as in
  tests/test_env_insertions_cpu.py: a seed that misses one is replaced, the threshold stays).
"""
from importlib import import_module

import numpy as np
import pytest

import mtfjsp_amd  # noqa: F401
from env_parity import Actions, create_lds_bytes, ell_rows, oracle_walk, parity_instances
from oracle import encoder_oracle as eo
from test_env_large_shapes_gpu import CASES, LDS_GFX950, ROWS, SEED, SPARSE_ABOVE, case_arguments, case_id, expected_plan

batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
PATH_FRONT, PATH_GAP = 1, 2


def test_the_table_is_the_librarys_plan_on_gfx950_and_reaches_what_it_is_about():
    plans = set()
    for r in ROWS:
        assert r.M % r.E == 0 and r.J * r.M <= 32767
        for dt, want in (("f32", r.f32), ("f64", r.f64)):
            assert expected_plan(r, dt, LDS_GFX950) == (want.kernel, want.G, want.launch)      # (asserts the whole row against the rule)
            assert want.launch <= LDS_GFX950
            if want.kernel == "k_env_step_grp":
                assert r.B > want.G and r.B % want.G != 0, (r, "at least one full group and a ragged last one")
                assert 2 * want.G * want.region + 512 > LDS_GFX950 or want.G == 8, (r, "no larger group fits")
            else:
                assert want.launch == create_lds_bytes(r.J, r.M, dt == "f32")[0] and 2 * want.region + 512 > LDS_GFX950
            if dt == "f32" or r.also_f64:
                plans.add((want.kernel, want.G))
        assert r.also_f64 or (r.f32.kernel, r.f32.G) == (r.f64.kernel, r.f64.G), (r, "f64 runs wherever its plan differs")
    assert plans == {("k_env_step_grp", 8), ("k_env_step_grp", 4), ("k_env_step_grp", 2), ("k_env_step", 1)}
    shapes = {(r.J, r.M) for r in ROWS}
    assert any(J > 64 for J, M in shapes) and any(M == 64 for J, M in shapes)
    L = import_module("e2e-mappo-for-mt-fjsp_amd.capi").lib()
    assert L.mtfjsp_step_kernel_name_for(36, 64, 2, 0, LDS_GFX950, None, None, None) == b"k_env_step"
    assert L.mtfjsp_step_kernel_name_for(40, 64, 2, 1, LDS_GFX950, None, None, None) is None
    # the largest shape: one more job of 64 operations no longer fits in f64; the group launch nearest the limit
    assert create_lds_bytes(36, 64, False)[2] == 162308 <= LDS_GFX950 < create_lds_bytes(37, 64, False)[2]
    assert LDS_GFX950 - 512 - 2 * 80304 == 2720                                    # (512 bytes are kept back by the rule)
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        kw, adjacency = case_arguments(c)
        T = c.row.J * c.row.M
        assert (adjacency == "sparse") == (T > SPARSE_ABOVE)
        assert T <= SPARSE_ABOVE or (c.variant == "plain" and kw["policy"] == "mask" and kw["episodes"] == 1)


@pytest.mark.parametrize("shape", [(6, 6, 2, 5), (10, 10, 2, 3)], ids=lambda s: "J%dM%dE%d-B%d" % s)
@pytest.mark.parametrize("policy", ["mask", "blocks"])
def test_the_oracles_ell_is_its_dense_adjacency_row_by_row_as_sets(shape, policy):
    from oracle.env_oracle import OracleBatch
    J, M, E, B = shape
    T = J * M
    t, p, tt, edge = parity_instances(J, M, E, B, SEED)
    rs = np.random.RandomState(SEED)
    orc = OracleBatch(t, p, tt, edge)
    orc.scaler_init()
    o = orc.reset(rs.dirichlet([1, 1, 1], B))
    cand, mask = orc.job_mask_state()
    act = Actions(policy, rs, J, M, B, t >= 0)
    edges = 0
    for s in range(-1, T):
        if s >= 0:
            job, task, mach = act.next(s, cand, mask)
            orc.step(task, mach)
            cand, mask = orc.job_mask_update(job)
            o = orc.observe()
        sparse = orc.observe(dense=False)
        assert "adj" not in sparse and np.array_equal(sparse["ell_col"], o["ell_col"]) and np.array_equal(sparse["ell_val"], o["ell_val"])
        col, val, adj = o["ell_col"], o["ell_val"], o["adj"]
        assert (adj[:, np.arange(T), np.arange(T)] == 1).all(), s
        assert ((col >= 0) == (val != 0)).all() and ((col[..., 0] != col[..., 1]) | (col[..., 0] < 0)).all(), s
        want = eo.ell_from_dense(adj)                                             # asserts: at most two off-diagonal non-zeros per row
        got = ell_rows(col, val)
        ref = ell_rows(*want)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), s
        edges += int((col >= 0).sum())
    assert edges > B * T * T // 2, "rows with one and with two in-edges were compared"
    assert (o["ell_col"] >= 0).all(-1).any(), "rows with two in-edges at the end"


def test_ell_rows_orders_slots_and_keeps_values():
    col = np.array([[3, 1], [-1, 4], [2, -1], [-1, -1], [5, 5]]); val = np.array([[7., 2.], [0., 9.], [1., 0.], [0., 0.], [2., 1.]])
    c, v = ell_rows(col, val)
    assert c.tolist() == [[1, 3], [-1, 4], [-1, 2], [-1, -1], [5, 5]] and v.tolist() == [[2., 7.], [0., 9.], [0., 1.], [0., 0.], [1., 2.]]
    assert col[0].tolist() == [3, 1], "the input is left alone"


BLOCKS = [c for c in CASES if c.variant == "blocks_reset_episode"]


@pytest.mark.parametrize("case", BLOCKS, ids=case_id)
def test_the_blocks_variants_take_the_front_and_the_gap_insertion(case):
    """the first episode of the GPU case: the same instances, the same action stream"""
    r = case.row
    kw, _ = case_arguments(case)
    assert kw["policy"] == "blocks" and kw["left_shift"]
    w = oracle_walk(r.J, r.M, r.E, r.B, left_shift=True, seed=SEED, policy="blocks")
    paths = w["paths"][0]
    front, gap = (paths == PATH_FRONT).mean(), (paths == PATH_GAP).mean()
    print(f"{case_id(case)}: front {100 * front:.1f} %, gap {100 * gap:.1f} % of {paths.size} steps")
    # The gap insertion is as frequent as in tests/test_env_insertions_cpu.py and is held to its threshold.  The front insertion is not a
    # share of the steps here: something fits before a route's first operation only until that is a job's FIRST operation, ready at 0,
    # which with many more jobs than machines happens within a route's first few entries — M * B routes see it, not J * M * B steps.  So it
    # is counted per instance: in at least half of them, for the groups' waves to take it side by side.  At M = 2 (two operations per job,
    # two routes) it exists in the first steps only: reached at all
    in_instances = int((paths == PATH_FRONT).any(0).sum())
    print(f"    front insertions in {in_instances} of {r.B} instances")
    assert gap >= 0.10
    assert in_instances >= ((r.B + 1) // 2 if r.M > 2 else 1)
    assert len(BLOCKS) == sum(r.J * r.M <= SPARSE_ABOVE for r in ROWS) == 3
