"""CPU: what the weight-reload tests on the GPU (tests/test_weight_reload_gpu.py) can see.  In binary64, on the inputs and weight sets those
tests use (tests/weight_reload_ref.py), every tensor of a checkpoint that is not on the list of mathematically unobservable ones moves at least
one compared output by 1e-3 of its scale — alone from the first set, along the cumulative single-key walk, and between the two whole sets on
every compared output.  A derived image the library failed to refresh therefore shows at 500 times the 2e-6 the GPU tests allow."""
import numpy as np
import pytest

import weight_reload_ref as R


@pytest.fixture(scope="module")
def sets():
    return R.weight_sets()


@pytest.fixture(scope="module", params=["j6m6_fixture", "j10m10_synthetic"])
def case(request, sets):
    inp = R.fixture_inputs() if request.param == "j6m6_fixture" else R.synthetic_inputs()
    return request.param, inp, R.oracle_outputs(sets[0], inp), R.oracle_outputs(sets[1], inp)


def test_unobservable_list_is_exactly_the_known_one():
    gin_biases = [f"encoder.feature_extract.mlps.{l}.linears.{i}.bias" for l in (0, 1) for i in (0, 1, 2)]
    want = (["job_actor." + k for k in gin_biases] + ["global_critic." + k for k in gin_biases] +
            ["job_actor.o_policy.linears.2.bias", "machine_actor.m_policy.linears.2.bias"] +
            ["machine_actor.fcl_pooling.weight", "global_critic.fcl_pooling.weight"] +
            [p + "encoder.feature_extract.bn." + s for p in ("job_actor.", "global_critic.") for s in ("weight", "bias")] +
            ["job_actor._input[later]"])
    assert sorted(R.UNOBSERVABLE) == sorted(want) and len(set(want)) == 21


def test_weight_sets_hold_every_tensor_of_a_reference_checkpoint(sets):
    """the keys of the reference modules' own state dicts (the fixture stores them), the unused modules' included"""
    import os
    from oracle import encoder_oracle as eo
    g = np.load(os.path.join(R.GOLDEN, "encoder_j6m6e2_rand.npz"))
    ref = eo.split_weights(g) + (eo.critic_weights(g),)
    for w in sets:
        for d, r in zip(w, ref):
            assert sorted(d) == sorted(r)
            assert all(np.asarray(d[k]).size == np.asarray(r[k]).size for k in d)
    assert all(k in R.all_keys(sets[0]) or k.endswith("[later]") for k in R.UNOBSERVABLE)


def test_second_set_moves_the_image_scales(sets):
    """max |W| of every 128-wide Linear and of gat_layer.W lies in another binade under W2 than under W1: the power-of-two scale of its f16 operand
    image and the inverse kept on the host both change with the reload"""
    moved = total = 0
    for d1, d2 in zip(*sets):
        for k in d1:
            if (k.endswith(".weight") and "linears" in k and d1[k].size % (R.H * R.H) == 0) or k == "gat_layer.W":
                total += 1
                moved += int(np.frexp(np.abs(d1[k]).max())[1] != np.frexp(np.abs(d2[k]).max())[1])
    assert total >= 20 and moved == total, (moved, total)


def test_the_two_sets_differ_on_every_compared_output(case):
    name, inp, o1, o2 = case
    d = R.distances(o2, o1)
    print(name, {k: f"{v:.2e}" for k, v in d.items()})
    assert len(d) == 10 and min(d.values()) >= R.OBSERVABLE_AT, d


def test_every_other_tensor_is_observable_alone(case, sets):
    name, inp, o1, _ = case
    worst = {}                                                      # a job-actor tensor must show in BOTH forms of its forward
    for key in R.all_keys(sets[0]):
        fs = R.forwards_reading(key) if key != "job_actor._input" else ("first", "later")
        d = R.distances(R.oracle_outputs(R.replaced(sets[0], key, R.perturb(key, R.get(sets[0], key))), inp, fs), o1)
        for f in fs:
            entry = key + "[later]" if key == "job_actor._input" and f == "later" else key
            worst[entry] = min(worst.get(entry, np.inf), max(v for (ff, _), v in d.items() if ff == f))
    assert all(k in worst for k in R.UNOBSERVABLE)
    print(name, "least observable:", [(f"{v:.2e}", k) for v, k in sorted((v, k) for k, v in worst.items() if k not in R.UNOBSERVABLE)[:6]])
    for k, v in worst.items():
        if k in R.UNOBSERVABLE:
            assert v < 1e-12, (k, v)                                # (measured: 0 or 1e-15, the round-off of the binary64 BatchNorm)
        else:
            assert v >= R.OBSERVABLE_AT, (k, v)


def test_every_step_of_the_cumulative_walk_is_observable(case, sets):
    name, inp, o1, _ = case
    prev, n = o1, 0
    for key, w in R.walk(sets[0]):
        fs = R.forwards_reading(key)
        cur = R.oracle_outputs(w, inp, fs)
        d = R.distances(cur, prev)
        for f in fs:
            assert max(v for (ff, _), v in d.items() if ff == f) >= R.OBSERVABLE_AT, (key, f, d)
        prev = dict(prev, **cur)
        n += 1
    assert n == len(R.all_keys(sets[0])) - (len(R.UNOBSERVABLE) - 1)
