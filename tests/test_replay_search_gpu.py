"""GPU: the searches on plans with replay="launch" — every round's or generation's replay in one launch (mtfjsp_replay_plans) — return
what replay="steps" returns for the same call, entry for entry and bit for bit: local_search (plain and with the moves a critical path
directs, which read the replayed schedules; left shift on and off; in chunks of two), walk_search (a tabu ring over the replayed
schedules' signatures; the default late acceptance), evolve and evolve_pareto.  The shapes and constants are
tests/test_local_search_gpu.py's."""
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


@functools.lru_cache(maxsize=None)
def _setup(shape):
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    J, M, E, N = SHAPES[shape]
    data = inst.generate_instances(N, J, M, E, seed=5100 + J * 100 + M)
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=CONFIG_W[0], weight_ec=CONFIG_W[1], weight_tt=CONFIG_W[2])
    return data, args, ref.first_feasible_plan(data[0])


def _equal(a, b, tag):
    """two results of one search: the same keys, and under every key the same bits (dicts, tuples and lists walked through)"""
    assert type(a) is type(b), f"{tag}: {type(a)} against {type(b)}"
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), f"{tag}: keys {sorted(a)} against {sorted(b)}"
        for k in a:
            _equal(a[k], b[k], f"{tag}[{k!r}]")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), f"{tag}: {len(a)} entries against {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{tag}[{i}]")
    else:
        x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype, f"{tag}: {x.shape} {x.dtype} against {y.shape} {y.dtype}"
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), f"{tag}: {int((x != y).sum())} of {x.size} differ"


def _both(search, shape, **kw):
    data, args, start = _setup(shape)
    fn = getattr(_baselines(), search)
    steps = fn(*data, args, start, replay="steps", **kw)
    _equal(fn(*data, args, start, replay="launch", **kw), steps, f"{search} {shape} {kw}")
    return steps


@pytest.mark.parametrize("left_shift", [False, True], ids=["nols", "ls"])
@pytest.mark.parametrize("moves", ["plain", "crit"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_local_search(shape, moves, left_shift):
    b = _baselines()
    mv = b.ALL_MOVES | (b.CRIT_MOVES if moves == "crit" else 0)
    res = _both("local_search", shape, K=K, rounds=ROUNDS, seed=SEED, moves=mv, left_shift=left_shift)
    if moves == "plain":                                                # (tests/test_local_search_gpu.py's runs: they improve every instance)
        assert (res["history"][-1] < res["start_obj"]).all(), "the search must have moved"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_local_search_in_chunks_of_two(shape):
    b = _baselines()
    _both("local_search", shape, K=K, rounds=ROUNDS, seed=SEED, moves=b.ALL_MOVES | b.CRIT_MOVES, left_shift=True, chunk=2)


@pytest.mark.parametrize("how", ["tabu", "late"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_walk_search(shape, how):
    kw = dict(tabu=4) if how == "tabu" else {}
    res = _both("walk_search", shape, K=K, rounds=ROUNDS, seed=SEED, left_shift=True, **kw)
    assert ((res["why"] & 7) >= 2).any(), "the walk must have moved"


@pytest.mark.parametrize("search", ["evolve", "evolve_pareto"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_evolutionary_searches(shape, search):
    _both(search, shape, P=8, generations=3, seed=SEED, left_shift=True)


def test_any_other_mode_is_refused():
    b = _baselines()
    data, args, start = _setup("J3M4")
    for fn, kw in ((b.local_search, dict(K=4, rounds=1)), (b.walk_search, dict(K=4, rounds=1)), (b.evolve, dict(P=8, generations=1)),
                   (b.evolve_pareto, dict(P=8, generations=1))):
        with pytest.raises(ValueError):
            fn(*data, args, start, replay="graph", **kw)
