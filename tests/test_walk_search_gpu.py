"""GPU: baselines.walk_search EQUALS its host model (tests/walk_ref.py: the models of the moves, the C oracle, the model of the signature,
the model of the acceptance) in every entry of the result, to the bit — on the searches that tests/test_walk_cpu.py proves to step uphill,
to be barred by the ring and to accept through the late ring: tabu, late acceptance, a falling threshold schedule, and tabu with the
moves a critical path directs; in chunks, with no rounds, with one copy, and — everything switched off — against baselines.local_search."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch  # noqa: F401  (before anything loads libmtfjsp.so: one HIP runtime per process, torch's)

import plan_moves_ref as pref
import walk_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = {"J2M2": (2, 2, 2, 3), "J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}
CONFIG_W = (0.4, 0.4, 0.2)
K, ROUNDS, SEED = 8, 24, 11
# tabu, slack, late, moves
SETTINGS = {"tabu": (8, np.inf, 0, 7), "late": (0, None, 4, 7), "threshold": (0, tuple(np.linspace(40.0, 0.0, ROUNDS).tolist()), 0, 7),
            "directed": (8, np.inf, 0, 31), "off": (0, None, 0, 7)}
EXTRA = ("history", "current", "accepted", "why", "barred")


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
    return data, args, pref.first_feasible_plan(data[0]), (J, M, E, N)


@functools.lru_cache(maxsize=None)
def _device(shape, setting, left_shift, chunk=None, k=K, rounds=ROUNDS, seed=SEED):
    data, args, start, _ = _setup(shape)
    tabu, slack, late, moves = SETTINGS[setting]
    slack = slack[:rounds] if isinstance(slack, tuple) else slack
    return _baselines().walk_search(*data, args, start, K=k, rounds=rounds, seed=seed, moves=moves, tabu=tabu, slack=slack, late=late,
                                    left_shift=left_shift, chunk=chunk)


@functools.lru_cache(maxsize=None)
def _model(shape, setting, left_shift, k=K, rounds=ROUNDS, seed=SEED):
    data, _, start, _ = _setup(shape)
    tabu, slack, late, moves = SETTINGS[setting]
    slack = slack[:rounds] if isinstance(slack, tuple) else slack
    return ref.search(data, start, k, rounds, seed, moves, left_shift, CONFIG_W, tabu, slack, late)


def _check(res, exp, tag, name="WS"):
    b = _baselines()
    assert sorted(res) == sorted([name, b.PLANS, "start_obj", *EXTRA])
    _same(_bits(res["start_obj"]), _bits(exp["start_obj"]), tag + " start_obj (bits)")
    _same(_bits(res["history"]), _bits(exp["history"]), tag + " history (bits)")
    _same(_bits(res["current"]), _bits(exp["current"]), tag + " current (bits)")
    for key in ("accepted", "why", "barred"):
        _same(res[key], exp[key], f"{tag} {key}")
    _same(res[b.PLANS][name][0], exp["plans"][0], tag + " best plans: tasks"); _same(res[b.PLANS][name][1], exp["plans"][1], tag + " best plans: machines")
    cost, final4, obj = res[name]
    assert sorted(cost) == sorted(ref.COST_KEYS)
    for key in ref.COST_KEYS:
        _same(_bits(cost[key]), _bits(exp["cost"][key]), f"{tag} {key} (bits)")
    _same(_bits(final4), _bits(exp["final4"]), tag + " Final_4cost (bits)"); _same(_bits(obj), _bits(exp["obj"]), tag + " Objective (bits)")


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("setting", ["tabu", "late", "threshold", "directed"])
@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_walk_search_equals_the_model(shape, setting, left_shift):
    res = _device(shape, setting, left_shift)
    _check(res, _model(shape, setting, left_shift), f"{shape} {setting} left_shift={left_shift}")
    hist = np.vstack([res["start_obj"][None], res["history"]])
    assert (np.diff(hist, axis=0) <= 0).all() and (res["history"] <= res["current"]).all()
    assert _bits(res["WS"][2]).tolist() == _bits(hist[-1]).tolist(), "the replayed best plans have the last round's best objectives"
    assert ((res["accepted"] >= 0) == ((res["why"] & 7) >= 2)).all()
    if not left_shift and setting != "directed":                        # (what tests/test_walk_cpu.py shows of these searches)
        assert (np.diff(np.vstack([res["start_obj"][None], res["current"]]), axis=0) > 0).any(), "the walk steps uphill"


def test_the_smallest_shape_with_a_ring():
    res = _device("J2M2", "tabu", False)
    _check(res, _model("J2M2", "tabu", False), "J2M2 tabu")
    assert (res["why"] == 0).any(), "everything barred somewhere"


@pytest.mark.parametrize("setting", ["tabu", "late"])
@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_chunks_of_two_equal_the_unchunked_run(shape, setting):
    """N = 4 in two passes, N = 3 with a padded last pass: the draws are keyed by the instance's number in the whole set, the state is per pass"""
    b = _baselines()
    full, res = _device(shape, setting, False), _device(shape, setting, False, 2)
    _check(res, _model(shape, setting, False), f"{shape} {setting} chunk=2")
    for key in ("start_obj", *EXTRA):
        _same(res[key], full[key], f"{shape} chunk=2 against unchunked: {key}")
    _same(res[b.PLANS]["WS"][0], full[b.PLANS]["WS"][0], shape + " chunk=2 against unchunked: plans")


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_everything_off_is_local_search(shape, left_shift):
    b = _baselines()
    data, args, start, _ = _setup(shape)
    res = _device(shape, "off", left_shift)
    hill = b.local_search(*data, args, start, K=K, rounds=ROUNDS, seed=SEED, left_shift=left_shift)
    _same(_bits(res["history"]), _bits(hill["history"]), shape + " history (bits)"); _same(_bits(res["current"]), _bits(hill["history"]), shape + " current (bits)")
    _same(res["accepted"], hill["accepted"], shape + " accepted"); _same(_bits(res["start_obj"]), _bits(hill["start_obj"]), shape + " start_obj (bits)")
    _same(res[b.PLANS]["WS"][0], hill[b.PLANS]["LS"][0], shape + " plans: tasks"); _same(res[b.PLANS]["WS"][1], hill[b.PLANS]["LS"][1], shape + " plans: machines")
    _same(_bits(res["WS"][2]), _bits(hill["LS"][2]), shape + " Objective (bits)")


@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_no_rounds_is_a_replay_of_the_start(shape):
    b = _baselines()
    data, args, start, (J, M, E, N) = _setup(shape)
    res = b.walk_search(*data, args, start, K=K, rounds=0, seed=SEED, name="START")
    _check(res, _model(shape, "tabu", False, K, 0), shape + " rounds=0", name="START")
    for key, dt in (("history", np.float64), ("current", np.float64), ("accepted", np.int8), ("why", np.int8), ("barred", np.int32)):
        assert res[key].shape == (0, N) and res[key].dtype == dt
    _same(res[b.PLANS]["START"][0], start[0], "the plans are the start plans")
    _same(_bits(res["start_obj"]), _bits(res["START"][2]), "start_obj is the replay's Objective")


@pytest.mark.parametrize("shape", ["J3M4", "J6M6"])
def test_one_copy_never_moves(shape):
    res = _device(shape, "tabu", False, None, 1, 3)
    _check(res, _model(shape, "tabu", False, 1, 3), shape + " K=1")
    assert (_bits(res["history"]) == _bits(res["start_obj"])[None]).all() and (_bits(res["current"]) == _bits(res["start_obj"])[None]).all()
    assert (res["accepted"] == -1).all() and (res["why"] == 0).all() and (res["barred"] == 0).all()


def test_same_seed_twice_and_another_seed():
    b = _baselines()
    data, args, start, _ = _setup("J6M6")
    a = _device("J6M6", "tabu", False)
    again = b.walk_search(*data, args, start, K=K, rounds=ROUNDS, seed=SEED, tabu=8, slack=np.inf, late=0)
    for key in ("start_obj", *EXTRA):
        _same(again[key], a[key], "second run: " + key)
    _same(again[b.PLANS]["WS"][0], a[b.PLANS]["WS"][0], "second run: tasks"); _same(again[b.PLANS]["WS"][1], a[b.PLANS]["WS"][1], "second run: machines")
    _same(_bits(again["WS"][2]), _bits(a["WS"][2]), "second run: Objective (bits)")
    other = _device("J6M6", "tabu", False, None, K, ROUNDS, SEED + 1)
    _check(other, _model("J6M6", "tabu", False, K, ROUNDS, SEED + 1), "seed + 1")
    assert not np.array_equal(other["current"], a["current"]), "another seed must walk another way"


@pytest.mark.parametrize("rounds", [0, 2])
@pytest.mark.parametrize("what", ["task out of range", "task twice"])
def test_a_bad_start_plan_raises(what, rounds):
    b = _baselines()
    data, args, start, (J, M, E, N) = _setup("J3M4")
    task, mach = start[0].copy(), start[1].copy()
    task[1, 5] = J * M if what == "task out of range" else task[1, 0]
    with pytest.raises(RuntimeError):
        b.walk_search(*data, args, (task, mach), K=4, rounds=rounds, seed=SEED)


def test_argument_errors():
    b = _baselines()
    data, args, start, _ = _setup("J3M4")
    for kw in (dict(moves=0), dict(K=0), dict(K=4097), dict(rounds=-1), dict(tabu=1025), dict(tabu=-1), dict(late=4097), dict(slack=[1.0, 0.0]), dict(chunk=0),
               dict(replay="other")):
        with pytest.raises(ValueError):
            b.walk_search(*data, args, start, **{**dict(K=4, rounds=1), **kw})
    with pytest.raises(ValueError):
        b.walk_search(*data, args, (start[0][:, :-1], start[1][:, :-1]), K=4, rounds=1)


def _layout(x, lead=True):
    """(shape, dtype) of every array of a result, through its dicts, tuples and lists; lead=False: without the leading dimension"""
    if isinstance(x, dict):
        return {k: _layout(v, lead) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x).__name__, [_layout(v, lead) for v in x]
    return (x.shape if lead else x.shape[1:]), x.dtype


# the entries beside (name, PLANS, "start_obj", "history"): (key, dtype, leading dimension with no rounds)
SEARCHES = {"local_search": ("rounds", "K", [("accepted", np.int8, 0)]),
            "walk_search": ("rounds", "K", [("current", np.float64, 0), ("accepted", np.int8, 0), ("why", np.int8, 0), ("barred", np.int32, 0)]),
            "evolve": ("generations", "P", []),
            "evolve_pareto": ("generations", "P", [("front_size", np.int32, 1)])}


@pytest.mark.parametrize("search", list(SEARCHES))
def test_the_result_without_rounds_has_the_layout_of_one_with_rounds(search):
    """rounds (generations) = 0: the exact key set and every entry's shape and dtype; with 2 the same keys and dtypes, and the same
    shapes behind the leading dimension"""
    b = _baselines()
    data, args, start, (J, M, E, N) = _setup("J3M4")
    count, copies, extra = SEARCHES[search]
    T, f64, i32 = J * M, np.dtype(np.float64), np.dtype(np.int32)
    run = lambda r: getattr(b, search)(*data, args, start, **{copies: 8, count: r}, seed=SEED, name="X")      # noqa: E731
    res = run(0)
    exp = {"X": ("tuple", [{key: ((N,), f64) for key in ref.COST_KEYS}, ((N, 4), f64), ((N,), f64)]),
           b.PLANS: {"X": ("tuple", [((N, T), i32), ((N, T), i32)])}, "start_obj": ((N,), f64), "history": ((0, N), f64)}
    exp.update({key: ((lead, N), np.dtype(dt)) for key, dt, lead in extra})
    fronts = res.pop("fronts") if search == "evolve_pareto" else None
    assert _layout(res) == exp
    _same(_bits(res["start_obj"]), _bits(res["X"][2]), "start_obj is the entry's Objective (bits)")
    two = run(2)
    if fronts is not None:
        two_fronts = two.pop("fronts")
        assert isinstance(fronts, list) and len(fronts) == N
        for f in fronts:
            assert _layout(f, False) == {"cost": ((3,), f64), "final4": ((4,), f64), "obj": ((), f64), "task": ((T,), i32), "mach": ((T,), i32)}
        assert _layout(two_fronts, False) == _layout(fronts, False)
    assert _layout(two, False) == _layout(res, False)
    assert two["history"].shape == (2, N) and all(two[key].shape == (lead + 2, N) for key, _, lead in extra)
