"""GPU: baselines.evolve_pareto EQUALS its host model (tests/nsga_ref.py: the models of the offspring, of the front ranks and of the
survivors, the C oracle) in the start objectives, the history and the front sizes of every generation, every front's plans and every
bit of its costs and objectives — J3M4 and J6M6, left shift off and on, P = 8, 3 generations, three random start plans per instance
(tests/test_evolve_gpu.py's); in chunks, twice, with another seed, with no generations, from the dispatch rules' plans, from a start
that is no plan."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch  # noqa: F401  (before anything loads libmtfjsp.so: one HIP runtime per process, torch's)

import group_reduce_ref as gref
import nsga_ref as ref
import plan_moves_ref as mref

pytestmark = pytest.mark.gpu

SHAPES = {"J3M4": (3, 4, 2, 3), "J6M6": (6, 6, 2, 4)}
CONFIG_W = (0.4, 0.4, 0.2)
P, GENS, SEED, STARTS = 8, 3, 11, 3


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
    starts = [mref.random_plans(np.asarray(data[0]), J, M, 60 + c) for c in range(STARTS)]
    return data, args, starts, (J, M, E, N)


@functools.lru_cache(maxsize=None)
def _device(shape, left_shift, chunk=None, gens=GENS, seed=SEED):
    data, args, starts, _ = _setup(shape)
    return _baselines().evolve_pareto(*data, args, starts, P=P, generations=gens, seed=seed, left_shift=left_shift, chunk=chunk)


@functools.lru_cache(maxsize=None)
def _model(shape, left_shift, gens=GENS, seed=SEED):
    data, _, starts, _ = _setup(shape)
    return ref.search(data, starts, P, gens, seed, left_shift=left_shift, w=CONFIG_W)


@functools.lru_cache(maxsize=None)
def _start_objs(shape, left_shift):
    data, _, starts, _ = _setup(shape)
    return np.stack([mref.replay(data, s[0], s[1], left_shift, CONFIG_W)[3] for s in starts])


def _check(res, exp, tag, name="NSGA"):
    b = _baselines()
    assert sorted(res) == sorted([name, b.PLANS, "start_obj", "history", "front_size", "fronts"])
    _same(_bits(res["start_obj"]), _bits(exp["start_obj"]), tag + " start_obj (bits)")
    _same(_bits(res["history"]), _bits(exp["history"]), tag + " history (bits)")
    _same(res["front_size"], exp["front_size"], tag + " front_size")
    assert len(res["fronts"]) == len(exp["fronts"])
    for n, (f, e) in enumerate(zip(res["fronts"], exp["fronts"])):
        assert sorted(f) == ["cost", "final4", "mach", "obj", "task"]
        _same(f["task"], e["task"], f"{tag} front {n}: tasks"); _same(f["mach"], e["mach"], f"{tag} front {n}: machines")
        for key in ("cost", "final4", "obj"):
            _same(_bits(f[key]), _bits(e[key]), f"{tag} front {n}: {key} (bits)")
    _same(res[b.PLANS][name][0], exp["plans"][0], tag + " best plans: tasks"); _same(res[b.PLANS][name][1], exp["plans"][1], tag + " best plans: machines")
    cost, final4, obj = res[name]
    assert sorted(cost) == sorted(ref.COST_KEYS)
    for key in ref.COST_KEYS:
        _same(_bits(cost[key]), _bits(exp["cost"][key]), f"{tag} {key} (bits)")
    _same(_bits(final4), _bits(exp["final4"]), tag + " Final_4cost (bits)"); _same(_bits(obj), _bits(exp["obj"]), tag + " Objective (bits)")


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_evolve_pareto_equals_the_model(shape, left_shift):
    res, exp = _device(shape, left_shift), _model(shape, left_shift)
    _check(res, exp, f"{shape} left_shift={left_shift}")
    data, _, _, (J, M, E, N) = _setup(shape)
    hist = np.vstack([res["start_obj"][None], res["history"]])
    assert (np.diff(hist, axis=0) <= 0).all(), "the best Objective never rises"
    _same(_bits(res["start_obj"]), _bits(_start_objs(shape, left_shift).min(0)), "start_obj is the best start's Objective")
    assert _bits(res["NSGA"][2]).tolist() == _bits(hist[-1]).tolist(), "the replayed best member has the last generation's Objective"
    sizes = []
    for n in range(N):
        f = res["fronts"][n]
        F = len(f["obj"])
        sizes.append(F)
        assert 1 <= F <= P
        for a in range(F):
            for c in range(F):
                assert a == c or not gref.dominates(f["cost"][a], f["cost"][c], a, c), "a front is mutually non-dominated"
        assert res["NSGA"][2][n] == f["obj"].min()
        # the C oracle's replay of every front plan gives that entry's final4, bit for bit
        one = tuple(np.repeat(np.asarray(x)[n:n + 1], F, axis=0) for x in data)
        _, f4, done, obj = mref.replay(one, f["task"], f["mach"], left_shift, CONFIG_W)
        assert done.all()
        _same(_bits(f["final4"]), _bits(f4), f"{shape} front {n}: final4 against the replay (bits)")
        _same(_bits(f["obj"]), _bits(obj), f"{shape} front {n}: obj against the replay (bits)")
    assert max(sizes) >= 2, f"at least one instance ends with two or more front members: {sizes}"


@pytest.mark.parametrize("left_shift", [False, True], ids=["no_left_shift", "left_shift"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_chunks_of_two_equal_the_unchunked_run(shape, left_shift):
    """N = 4 in two passes, N = 3 with a padded last pass: the draws are keyed by the instance's number in the whole set"""
    _check(_device(shape, left_shift, 2), _model(shape, left_shift), f"{shape} left_shift={left_shift} chunk=2")
    full, res = _device(shape, left_shift), _device(shape, left_shift, 2)
    for key in ("start_obj", "history", "front_size"):
        _same(res[key], full[key], f"{shape} chunk=2 against unchunked: {key}")


def test_same_seed_twice_and_another_seed():
    b = _baselines()
    data, args, starts, _ = _setup("J6M6")
    a = _device("J6M6", False)
    again = b.evolve_pareto(*data, args, starts, P=P, generations=GENS, seed=SEED)
    _check(again, _model("J6M6", False), "second run")
    for key in ("start_obj", "history", "front_size"):
        _same(again[key], a[key], "second run: " + key)
    other = _device("J6M6", False, None, GENS, SEED + 1)
    _check(other, _model("J6M6", False, GENS, SEED + 1), "seed + 1")
    assert any(len(x["obj"]) != len(y["obj"]) or not np.array_equal(x["task"], y["task"]) for x, y in zip(a["fronts"], other["fronts"])), \
        "another seed must give other fronts"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_generations_is_the_front_of_the_starts(shape):
    b = _baselines()
    data, args, starts, (J, M, E, N) = _setup(shape)
    res = b.evolve_pareto(*data, args, starts, P=P, generations=0, seed=SEED, name="START")
    _check(res, _model(shape, False, 0), shape + " generations=0", name="START")
    assert res["history"].shape == (0, N) and res["front_size"].shape == (1, N)
    objs = _start_objs(shape, False)
    _same(_bits(res["START"][2]), _bits(objs.min(0)), "the Objective is the best start's")
    for n in range(N):
        # the front of the three starts (member c = start c % 3: of the duplicates only the first is on the front)
        f4 = np.stack([mref.replay(tuple(np.asarray(x)[n:n + 1] for x in data), s[0][n:n + 1], s[1][n:n + 1], False, CONFIG_W)[1][0] for s in starts])
        front = gref.group_reduce(f4, np.ones(STARTS, np.uint8), CONFIG_W, 1, STARTS)[3]
        assert len(res["fronts"][n]["obj"]) == front.sum() == res["front_size"][0, n]
        assert sorted(map(tuple, _bits(res["fronts"][n]["final4"]).tolist())) == sorted(map(tuple, _bits(f4[front == 1]).tolist()))


def test_from_the_dispatch_rules():
    b = _baselines()
    data, args, _, (J, M, E, N) = _setup("J6M6")
    rules = b.pdr_baselines(*data, args, seed=3)
    starts = [rules[b.PLANS][r[0]] for r in b.RULES]
    res = b.evolve_pareto(*data, args, starts, P=16, generations=GENS, seed=SEED, left_shift=False, name="NSGA(rules)")
    best_rule = np.min([rules[r[0]][2] for r in b.RULES], axis=0)
    _same(_bits(res["start_obj"]), _bits(best_rule), "start_obj = the best rule's Objective (bits)")
    assert (res["history"] <= res["start_obj"][None]).all()
    assert (res["NSGA(rules)"][2] <= best_rule).all()
    _check(res, ref.search(data, starts, 16, GENS, SEED, left_shift=False, w=CONFIG_W), "from the 12 rules", name="NSGA(rules)")


def test_argument_errors():
    b = _baselines()
    data, args, starts, _ = _setup("J3M4")
    for bad in (4, 7, 1025):
        with pytest.raises(ValueError):
            b.evolve_pareto(*data, args, starts, P=bad, generations=1, seed=SEED)
    with pytest.raises(ValueError):
        b.evolve_pareto(*data, args, starts, P=8, generations=-1)
    with pytest.raises(ValueError):
        b.evolve_pareto(*data, args, starts, P=8, moves=8)
    with pytest.raises(ValueError):
        b.evolve_pareto(*data, args, starts, P=8, generations=1, replay="other")


@pytest.mark.parametrize("gens", [0, 2])
@pytest.mark.parametrize("what", ["task out of range", "task twice"])
def test_a_bad_start_plan_is_handled_as_evolve_handles_it(what, gens):
    b = _baselines()
    data, args, starts, (J, M, E, N) = _setup("J3M4")
    task, mach = starts[0][0].copy(), starts[0][1].copy()
    task[1, 5] = J * M if what == "task out of range" else task[1, 0]
    with pytest.raises(RuntimeError):
        b.evolve_pareto(*data, args, (task, mach), P=8, generations=gens, seed=SEED)
    # beside valid starts it only never wins
    res = b.evolve_pareto(*data, args, [(task, mach), starts[1]], P=8, generations=gens, seed=SEED)
    assert (res["NSGA"][2] <= _start_objs("J3M4", False)[1]).all()
    assert (res["history"] <= res["start_obj"][None]).all() and all(len(f["obj"]) >= 1 for f in res["fronts"])
