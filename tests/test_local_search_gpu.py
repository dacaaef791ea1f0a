"""GPU: baselines.local_search EQUALS its host model (tests/plan_moves_ref.py: the model of the moves, the C oracle, the model of the
group reduction) in the start objectives, the history of every round, the accepted moves, the final plans and every bit of the three
result entries — on the two table rows that tests/test_plan_moves_cpu.py proves to improve, to accept all three kinds of moves and
to meet single-machine tasks and identity neighbours; in chunks, with no rounds, with one copy, from a dispatch rule's plans."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch  # noqa: F401  (before anything loads libmtfjsp.so: one HIP runtime per process, torch's)

import plan_moves_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}
CONFIG_W = (0.4, 0.4, 0.2)
K, ROUNDS, SEED = 8, 6, 11


def _baselines():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.baselines")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _same(got, exp, tag):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, f"{tag}: {got.shape} {got.dtype} against {exp.shape} {exp.dtype}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{tag}: {len(bad)} of {exp.size} differ, first at {bad[0].tolist()}")


@functools.lru_cache(maxsize=None)
def _setup(shape):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = SHAPES[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M)
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=CONFIG_W[0], weight_ec=CONFIG_W[1], weight_tt=CONFIG_W[2])
    return data, args, ref.first_feasible_plan(data[0]), (J, M, E, N)


@functools.lru_cache(maxsize=None)
def _device(shape, left_shift, chunk=None, k=K, rounds=ROUNDS, seed=SEED):
    data, args, start, _ = _setup(shape)
    return _baselines().local_search(*data, args, start, K=k, rounds=rounds, seed=seed, left_shift=left_shift, chunk=chunk)


@functools.lru_cache(maxsize=None)
def _model(shape, left_shift, k=K, rounds=ROUNDS, seed=SEED):
    data, _, start, _ = _setup(shape)
    return ref.search(data, start, k, rounds, seed, ref.ALL_MOVES, left_shift, CONFIG_W)


def _check(res, exp, tag, name="LS"):
    b = _baselines()
    assert sorted(res) == sorted([name, b.PLANS, "start_obj", "history", "accepted"])
    _same(_bits(res["start_obj"]), _bits(exp["start_obj"]), tag + " start_obj (bits)")
    _same(_bits(res["history"]), _bits(exp["history"]), tag + " history (bits)")
    _same(res["accepted"], exp["accepted"], tag + " accepted")
    _same(res[b.PLANS][name][0], exp["plans"][0], tag + " final plans: tasks"); _same(res[b.PLANS][name][1], exp["plans"][1], tag + " final plans: machines")
    cost, final4, obj = res[name]
    assert sorted(cost) == sorted(ref.COST_KEYS)
    for key in ref.COST_KEYS:
        _same(_bits(cost[key]), _bits(exp["cost"][key]), f"{tag} {key} (bits)")
    _same(_bits(final4), _bits(exp["final4"]), tag + " Final_4cost (bits)"); _same(_bits(obj), _bits(exp["obj"]), tag + " Objective (bits)")


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_local_search_equals_the_model(shape, left_shift):
    res, exp = _device(shape, left_shift), _model(shape, left_shift)
    _check(res, exp, f"{shape} left_shift={left_shift}")
    hist = np.vstack([res["start_obj"][None], res["history"]])
    assert (np.diff(hist, axis=0) <= 0).all() and (hist[-1] < hist[0]).all()
    assert _bits(res["LS"][2]).tolist() == _bits(hist[-1]).tolist(), "the replayed plans have the last round's objectives"
    assert {1, 2, 4} <= set(np.unique(res["accepted"]).tolist())


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_chunks_of_two_equal_the_unchunked_run(shape, left_shift):
    """N = 4 in two passes, N = 3 with a padded last pass: the draws are keyed by the instance's number in the whole set"""
    b = _baselines()
    full, res = _device(shape, left_shift), _device(shape, left_shift, 2)
    _check(res, _model(shape, left_shift), f"{shape} left_shift={left_shift} chunk=2")
    for key in ("start_obj", "history", "accepted"):
        _same(res[key], full[key], f"{shape} chunk=2 against unchunked: {key}")
    _same(res[b.PLANS]["LS"][0], full[b.PLANS]["LS"][0], shape + " chunk=2 against unchunked: plans")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_rounds_is_a_replay_of_the_start(shape):
    b = _baselines()
    data, args, start, (J, M, E, N) = _setup(shape)
    res = b.local_search(*data, args, start, K=K, rounds=0, seed=SEED, name="START")
    _check(res, _model(shape, False, K, 0), shape + " rounds=0", name="START")
    assert res["history"].shape == (0, N) and res["accepted"].shape == (0, N) and res["accepted"].dtype == np.int8
    _same(res[b.PLANS]["START"][0], start[0], "the plans are the start plans")
    _same(_bits(res["start_obj"]), _bits(res["START"][2]), "start_obj is the replay's Objective")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_copy_never_moves(shape):
    res = _device(shape, False, None, 1, 3)
    _check(res, _model(shape, False, 1, 3), shape + " K=1")
    assert (_bits(res["history"]) == _bits(res["start_obj"])[None]).all() and (res["accepted"] == -1).all()
    _same(_bits(res["start_obj"]), _bits(_model(shape, False, K, 0)["obj"]), "start_obj is the start plan's Objective")


def test_same_seed_twice_and_another_seed():
    b = _baselines()
    data, args, start, _ = _setup("J6M6")
    a = _device("J6M6", False)
    again = b.local_search(*data, args, start, K=K, rounds=ROUNDS, seed=SEED)
    for key in ("start_obj", "history", "accepted"):
        _same(again[key], a[key], "second run: " + key)
    _same(again[b.PLANS]["LS"][0], a[b.PLANS]["LS"][0], "second run: tasks"); _same(again[b.PLANS]["LS"][1], a[b.PLANS]["LS"][1], "second run: machines")
    _same(_bits(again["LS"][2]), _bits(a["LS"][2]), "second run: Objective (bits)")
    other = _device("J6M6", False, None, K, ROUNDS, SEED + 1)
    _check(other, _model("J6M6", False, K, ROUNDS, SEED + 1), "seed + 1")
    assert not np.array_equal(other[b.PLANS]["LS"][0], a[b.PLANS]["LS"][0]), "another seed must give other plans"


def test_from_a_dispatch_rule():
    b = _baselines()
    data, args, _, (J, M, E, N) = _setup("J6M6")
    rule = b.pdr_baselines(*data, args, rules=[r for r in b.RULES if r[0] == "MOR+SPT"], seed=3)
    start = rule[b.PLANS]["MOR+SPT"]
    res = b.local_search(*data, args, start, K=K, rounds=ROUNDS, seed=SEED, left_shift=False, name="LS(MOR+SPT)")
    _same(_bits(res["start_obj"]), _bits(rule["MOR+SPT"][2]), "start_obj = the rule's Objective (bits)")
    assert (res["LS(MOR+SPT)"][2] <= rule["MOR+SPT"][2]).all()
    exp = ref.search(data, start, K, ROUNDS, SEED, ref.ALL_MOVES, False, CONFIG_W)
    _check(res, exp, "from MOR+SPT", name="LS(MOR+SPT)")


@pytest.mark.parametrize("rounds", [0, 2])
@pytest.mark.parametrize("what", ["task out of range", "task twice"])
def test_a_bad_start_plan_raises(what, rounds):
    b = _baselines()
    data, args, start, (J, M, E, N) = _setup("J3M4")
    task, mach = start[0].copy(), start[1].copy()
    task[1, 5] = J * M if what == "task out of range" else task[1, 0]
    with pytest.raises(RuntimeError):
        b.local_search(*data, args, (task, mach), K=4, rounds=rounds, seed=SEED)
    with pytest.raises(ValueError):
        b.local_search(*data, args, (task[:, :-1], mach[:, :-1]), K=4, rounds=1)
    with pytest.raises(ValueError):
        b.local_search(*data, args, start, K=4, rounds=1, moves=0)


def test_argument_errors():
    b = _baselines()
    data, args, start, _ = _setup("J3M4")
    for kw in (dict(moves=0), dict(moves=32), dict(K=0), dict(K=4097), dict(rounds=-1), dict(chunk=0), dict(replay="other")):
        with pytest.raises(ValueError):
            b.local_search(*data, args, start, **{**dict(K=4, rounds=1), **kw})
    with pytest.raises(ValueError):
        b.local_search(*data, args, (start[0][:, :-1], start[1][:, :-1]), K=4, rounds=1)
