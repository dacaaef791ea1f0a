"""GPU: the one-launch plan replay (k_replay_plans, mtfjsp_replay_plans) at every form of its launch, up to the LDS a workgroup may use.
tests/test_replay_plans_gpu.py runs 15 copies at T <= 135: four copies per workgroup, at most 34 KB of dynamic LDS, two pairwise leaves.
The rows of replay_ref.FORM_ROWS reach the rest: two copies and one copy per workgroup — by the LDS of a region and by the batch rule
at B = 1 and 2 — with idle waves leaving after the barrier and regions at other offsets; each copy count above the 48 KB from which
the launch asks for its LDS; the energy sum of 4, 5, 10, 16 and 32 leaves (idle lanes, a partly filled second pass, the longest merge
list) and of one leaf at T = 6, 8, 128 and then 129; 64 machines; one job; and J162M16, 176 bytes under the limit, with J163M16
refused beyond it.  tests/test_replay_forms_cpu.py holds the table to the launch rule and proves on the oracle what the plans reach.

Every row: replay_plans(state=True) EQUALS reset + T steps + final_costs on a second handle, bit for bit — cost4, done, machine, start,
finish, routes, state_signature and critical_path (mtfjsp_critical_path takes every row: 4 x 7 x (T + 4) bytes, 73 KB at T = 2592) —
and cost4 and done equal the C oracle's replay and the launch without state.  Generated times with random plans and small-integer
times (exact ties) with the oracle walk's "blocks" plans; left shift on and off up to T = 600, on only above.  The expectation of a
row's form comes from capi.replay_launch_info_for with the LDS limit the device reports through a handle of another shape, and is the
table's where that limit is 163840 bytes; it is printed per case.  No tolerance anywhere.

What the rows were seen to catch, on library builds broken on purpose and never committed (an MI355X; wrong sums only, every address
in bounds).  The second pass over the leaves dropped: both comparisons fail at J52M20, J24M64 and J162M16 (10, 16, 32 leaves), on
generated and integer data, and the two-handle test fails; nothing else does.  The leaves merged in index order: both comparisons
fail on the generated data of J17M16, J20M20, J35M15, J24M64 and J162M16 and the partial schedules of J35M15 — the rows
test_replay_forms_cpu.test_the_gpu_inputs_tell_the_merge_orders_apart names beforehand; J52M20's energies happen to round alike, and
integer energies sum exactly in any order.  Argued from the code only, not run (they put plan words or a launch where they do not
belong): the plan tile read with the copy shift off by one leaves steps of every copy unfilled or filled from another copy's column at
any G, so every row's done or schedule differs (G = 2: J17M16, J20M20, J6M6 B = 2; G = 1 has shift 0 and only a shift too large can
break it); the launch without its hipFuncSetAttribute call asks for more dynamic LDS than the kernel may have at J14M15, J20M20,
J52M20, J24M64 and J162M16 — one row per copy count — and a refused launch is an MtfjspError."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import plan_moves_ref as pref
import replay_ref as ref
from env_parity import create_lds_bytes
from test_env_large_shapes_gpu import LDS_GFX950, device_lds
from test_replay_plans_gpu import _compare, _mods, _same, _schedule
from test_replay_search_gpu import _baselines, _equal

pytestmark = pytest.mark.gpu

W = ref.CONFIG_W
ROWS = ref.FORM_ROWS
BOTH_ABOVE = 600                                 # T: above, left shift on only
ROW = {ref.form_id(r): r for r in ROWS}
CASES = [(ref.form_id(r), d, ls) for r in ROWS for d in ("generated", "integer") for ls in (False, True) if ls or r[0] * r[1] <= BOTH_ABOVE]
IDS = [f"{r}-{d}-{'ls' if ls else 'nols'}" for r, d, ls in CASES]


def live_form(row):
    """(G, dynamic LDS bytes) the launch must have on this device — from the handle-free rule with the device's own limit — printed"""
    J, M, E, B, G, nbytes = row[:6]
    lds = device_lds()
    exp = _mods()[1].replay_launch_info_for(J, M, B, lds)
    if lds == LDS_GFX950:
        assert exp == (G, nbytes), (row, exp)
    print(f"{ref.form_id(row)}: G = {exp[0]}, {exp[1]} bytes of LDS per launch, {row[6]} leaves ({row[7]})")
    return exp


def _dev(env, x):
    """plans [B,T] -> a fresh int32 device tensor [T,B] with row stride B, also at B = 1 (where a transposed numpy array keeps its
    own strides, which replay_plans' argument check does not take)"""
    x = np.asarray(x)
    out = torch.empty(x.shape[1], x.shape[0], dtype=torch.int32, device=env.device)
    out.copy_(torch.from_numpy(np.array(x.T, np.int32)))
    assert out.stride() == (x.shape[0], 1)
    return out


def _handle(case, left_shift):
    env = _mods()[0].DeviceBatchEnv(case["J"], case["M"], case["E"], case["B"], left_shift=left_shift, obs_dtype="f32", w_cfg=W)
    env.load_instances(*case["inst"][:3], edge=case["inst"][3])
    return env


def _episode(env, task, mach):
    """reset, T steps, final_costs -> dict(cost4, done, the schedule)"""
    env.scaler_init()
    env.reset(np.tile(np.array([W], np.float64), (env.B, 1)))
    tk, mc = _dev(env, task), _dev(env, mach)
    for s in range(tk.shape[0]):
        env.step(tk[s], mc[s])
    cost4, done = env.final_costs()
    return dict(cost4=cost4.cpu().numpy(), done=done.cpu().numpy(), **_schedule(env))


def _by_steps(case, left_shift, task, mach):
    env = _handle(case, left_shift)
    try:
        return _episode(env, task, mach)
    finally:
        env.close()


def _replayed(env, task, mach, state=True):
    cost4, done = env.replay_plans(_dev(env, task), _dev(env, mach), state=state)
    out = dict(cost4=cost4.cpu().numpy(), done=done.cpu().numpy())
    if state:
        out.update(_schedule(env))
    return out


def _by_launch(case, left_shift, task, mach, state=True):
    env = _handle(case, left_shift)
    try:
        return _replayed(env, task, mach, state)
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def _steps(row_id, data, left_shift):
    case = ref.form_case(ROW[row_id], data)
    return _by_steps(case, left_shift, case["task"], case["mach"])


@functools.lru_cache(maxsize=None)
def _launch(row_id, data, left_shift):
    case = ref.form_case(ROW[row_id], data)
    live_form(ROW[row_id])
    return _by_launch(case, left_shift, case["task"], case["mach"])


@pytest.mark.parametrize("row_id,data,left_shift", CASES, ids=IDS)
def test_one_launch_equals_the_step_launches(row_id, data, left_shift):
    """final costs, done, and the schedule every search reads"""
    got, exp = _launch(row_id, data, left_shift), _steps(row_id, data, left_shift)
    assert exp["done"].all(), "every plan of these cases is valid"
    _compare(got, exp, f"{row_id} {data} left_shift={left_shift}")


@pytest.mark.parametrize("row_id,data,left_shift", CASES, ids=IDS)
def test_one_launch_equals_the_oracle(row_id, data, left_shift):
    """Final_4cost of the C oracle's replay"""
    case = ref.form_case(ROW[row_id], data)
    _, final4, done, _ = pref.replay(case["inst"], case["task"], case["mach"], left_shift, W)
    got = _launch(row_id, data, left_shift)
    _same(got["done"], done.astype(np.uint8), f"{row_id} {data}: done")
    _same(got["cost4"], final4, f"{row_id} {data} left_shift={left_shift}: cost4 (bits)")


@pytest.mark.parametrize("row_id,data,left_shift", CASES, ids=IDS)
def test_without_state_the_same_costs(row_id, data, left_shift):
    case = ref.form_case(ROW[row_id], data)
    plain, got = _by_launch(case, left_shift, case["task"], case["mach"], state=False), _launch(row_id, data, left_shift)
    _same(plain["done"], got["done"], f"{row_id} {data}: done without state")
    _same(plain["cost4"], got["cost4"], f"{row_id} {data} left_shift={left_shift}: cost4 without state (bits)")


@pytest.mark.parametrize("row_id", ["J17M16E2-B7", "J35M15E3-B3"])
def test_partial_schedules_at_two_copies_and_one_copy_per_workgroup(row_id):
    """replay_ref.SPOIL_COLS: at 17x16 (G = 2) a task out of range, a swapped pair and a machine with t < 0 each beside a good copy,
    a task twice alone in the ragged last workgroup; at 35x15 (G = 1) a task twice and a swapped pair around a good copy.  The step
    path is the reference of a rejected action"""
    row = ROW[row_id]
    J, M, E, B = row[:4]
    assert live_form(row)[0] == row[4] or device_lds() != LDS_GFX950
    cols = ref.SPOIL_COLS[(J, M)]
    case = ref.form_case(row, "generated")
    task, mach = ref.spoil_at(case["task"], case["mach"], case["inst"][0], M, cols)
    exp = _by_steps(case, True, task, mach)
    got = _by_launch(case, True, task, mach)
    plain = _by_launch(case, True, task, mach, state=False)
    bad = [c for c in cols[:3] if c is not None]
    _same(got["done"], exp["done"], row_id + ": done")
    assert not got["done"][bad].any() and got["done"][[c for c in range(B) if c not in bad]].all(), got["done"]
    nan = np.isnan(got["cost4"])
    assert (nan == (got["done"] == 0)[:, None]).all(), "four NaNs exactly where the copy is not done"
    _same(got["cost4"][got["done"] == 1], exp["cost4"][exp["done"] == 1], row_id + ": cost4 of the done copies (bits)")
    _compare(got, exp, row_id + " spoiled, partial schedules", [k for k in exp if k not in ("cost4", "done")])
    _same(plain["done"], got["done"], row_id + ": done without state")
    _same(plain["cost4"], got["cost4"], row_id + ": cost4 without state (bits, NaNs included)")


def test_one_job_beyond_the_largest_shape_is_refused_and_the_handle_lives():
    """J162M16 (163 664 bytes) is a row above and equals the step path and the oracle.  mtfjsp_create takes J163M16 (its step kernel
    needs 142 640 bytes); replay_plans on that handle raises MtfjspError with ERR_ARG, and the same handle then steps an episode that
    equals the oracle.  On a device whose limit refuses the shape at mtfjsp_create, that refusal is asserted instead"""
    be, capi = _mods()
    J, M, E, B = ref.REFUSED
    lds = device_lds()
    case = ref.form_case(ref.REFUSED, "generated")
    if create_lds_bytes(J, M, True)[2] > lds:
        with pytest.raises(capi.MtfjspError, match="too large") as e:
            be.DeviceBatchEnv(J, M, E, B)
        assert e.value.code == capi.ERR_ARG
        return
    assert ref.region_bytes(J, M) > lds, f"a workgroup has {lds} bytes here: J{J}M{M} fits, the case needs a larger shape"
    with pytest.raises(ValueError):
        capi.replay_launch_info_for(J, M, B, lds)
    env = _handle(case, True)
    try:
        tk, mc = _dev(env, case["task"]), _dev(env, case["mach"])
        for state in (False, True):
            with pytest.raises(capi.MtfjspError, match="too large") as e:
                env.replay_plans(tk, mc, state=state)
            assert e.value.code == capi.ERR_ARG
        got = _episode(env, case["task"], case["mach"])
        _, final4, done, _ = pref.replay(case["inst"], case["task"], case["mach"], True, W)
        assert done.all()
        _same(got["done"], done.astype(np.uint8), "after the refusal: done")
        _same(got["cost4"], final4, "after the refusal: cost4 against the oracle (bits)")
    finally:
        env.close()


def test_a_large_and_a_small_handle_take_turns():
    """hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel, not to a handle: J52M20 launches with 68 224 bytes and asks for
    them, J6M6 with 10 624 and does not.  Large, small, large, small on two live handles: each result equals its first, the first
    ones the step path"""
    big_id, small_id = "J52M20E4-B3", "J6M6E2-B4"
    big, small = ref.form_case(ROW[big_id], "generated"), ref.form_case(ROW[small_id], "generated")
    assert live_form(ROW[big_id])[1] > 48 * 1024 > live_form(ROW[small_id])[1]
    eb, es = _handle(big, True), _handle(small, True)
    try:
        runs = [_replayed(env, c["task"], c["mach"]) for env, c in ((eb, big), (es, small), (eb, big), (es, small))]
        _compare(runs[0], _steps(big_id, "generated", True), "the large handle's first replay")
        _compare(runs[1], _steps(small_id, "generated", True), "the small handle's first replay")
        _compare(runs[2], runs[0], "the large handle again")
        _compare(runs[3], runs[1], "the small handle again")
    finally:
        eb.close(); es.close()


# ---- the searches
K_SEED = 11


@functools.lru_cache(maxsize=None)
def _setup(J, M, E, N):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M)
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=W[0], weight_ec=W[1], weight_tt=W[2])
    return data, args, pref.first_feasible_plan(data[0])


def _search(name, shape, mode, **kw):
    data, args, start = _setup(*shape)
    return getattr(_baselines(), name)(*data, args, start, replay=mode, **kw)


def test_local_search_at_J20M20():
    """N = 2, K = 4: 8 copies of T = 400, two per workgroup with 56 832 bytes; the critical-path moves read the replayed schedules"""
    b = _baselines()
    assert _mods()[1].replay_launch_info_for(20, 20, 8, device_lds())[0] == 2 or device_lds() != LDS_GFX950
    kw = dict(K=4, rounds=2, seed=K_SEED, moves=b.ALL_MOVES | b.CRIT_MOVES, left_shift=True)
    _equal(_search("local_search", (20, 20, 4, 2), "launch", **kw), _search("local_search", (20, 20, 4, 2), "steps", **kw), "local_search J20M20")


def test_evolve_at_J20M20():
    """N = 2, P = 8: 16 copies of T = 400"""
    kw = dict(P=8, generations=2, seed=K_SEED, left_shift=True)
    _equal(_search("evolve", (20, 20, 4, 2), "launch", **kw), _search("evolve", (20, 20, 4, 2), "steps", **kw), "evolve J20M20")


def test_local_search_in_chunks_with_a_short_last_pass():
    """J6M6, N = 3, chunk = 2, K = 2.  evaluate.CopyGroups builds ONE handle of chunk x K = 4 copies for every pass; the last pass,
    which has one instance left, gets no handle of its own: its unused columns hold copies of its last instance (`passes`: the index
    is clamped) and are replayed like any other.  So both passes launch with B = 4, G = 4 — not B = 2, G = 2 — and the results of the
    padded columns are dropped by `host`.  Equal to replay by steps and to the search in one pass"""
    b = _baselines()
    kw = dict(K=2, rounds=4, seed=K_SEED, moves=b.ALL_MOVES | b.CRIT_MOVES, left_shift=True)
    steps = _search("local_search", (6, 6, 2, 3), "steps", chunk=2, **kw)
    _equal(_search("local_search", (6, 6, 2, 3), "launch", chunk=2, **kw), steps, "local_search J6M6 chunk=2")
    _equal(_search("local_search", (6, 6, 2, 3), "launch", chunk=None, **kw), steps, "local_search J6M6 chunk=None against chunk=2")


@pytest.mark.parametrize("N,K,G", [(1, 2, 2), (1, 1, 1)], ids=["B2", "B1"])
def test_local_search_on_a_handle_of_two_copies_and_of_one(N, K, G):
    """what the chunked search above does not reach: a search whose copies' handle really has B = 2 (G = 2) or B = 1 (G = 1)"""
    b = _baselines()
    assert _mods()[1].replay_launch_info_for(6, 6, N * K, device_lds())[0] == G
    kw = dict(K=K, rounds=4, seed=K_SEED, moves=b.ALL_MOVES | b.CRIT_MOVES, left_shift=True)
    _equal(_search("local_search", (6, 6, 2, N), "launch", **kw), _search("local_search", (6, 6, 2, N), "steps", **kw), f"local_search J6M6 N={N} K={K}")
