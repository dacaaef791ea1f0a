"""GPU: loading weights again on a USED encoder handle — what a training loop does between two rollouts — on every forward path.

The reference for a reloaded handle is a fresh handle that has only ever held the final weights, on the same inputs: within 2e-6 of scale
(summation-order noise, tests/test_encoder_sizes_gpu.py), and bit for bit on every output on which two fresh handles agree bit for bit in
the same test.  The fresh handle is held to the binary64 oracle at the tolerances tests/test_encoder_sizes_gpu.py uses for random weights.
tests/test_weight_reload_cpu.py shows that a tensor, or a derived image, left stale moves an output by at least 1e-3 of scale.
Which path runs is asked of the library (check(), gin_launches(), gin_res_kernel_name(), fused_launches()), never assumed."""
import contextlib
import time
from importlib import import_module

import numpy as np
import pytest

import weight_reload_ref as R

pytestmark = pytest.mark.gpu


def _mods():
    import torch
    import mtfjsp_amd  # noqa: F401
    return (torch, import_module("e2e-mappo-for-mt-fjsp_amd.encoder"), import_module("e2e-mappo-for-mt-fjsp_amd.capi"),
            import_module("e2e-mappo-for-mt-fjsp_amd.rollout"))


@pytest.fixture(scope="module")
def sets():
    return R.weight_sets()


@pytest.fixture(scope="module")
def inputs():
    return {"j6m6": R.fixture_inputs(), "j10m10": R.synthetic_inputs()}


def _device(inp):
    import torch
    B, T, M = inp["B"], inp["T"], inp["M"]
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()
    return dict(tfea=t(inp["tfea"]), col=t(inp["col"].reshape(B * T, 2)), val=t(inp["val"].reshape(B * T, 2)), cand=t(inp["cand"]), mask=t(inp["mask"]),
                hm=t(inp["hm"]), mfea1=t(inp["mfea1"].reshape(B * M, 6)), mfea2=t(inp["mfea2"].reshape(B * M, 8)), mmask=t(inp["mmask"]), h_o=t(inp["h_o"]))


def _enqueue(enc, d, f):
    """one forward of kind f, enqueued only -> its output tensors"""
    if f in ("first", "later"):
        prob, h_o, job_v = enc.job_actor_forward(d["tfea"], d["col"], d["val"], d["cand"], d["mask"], d["hm"] if f == "later" else None)
        return {"prob": prob, "h_pooled_o": h_o, "job_v": job_v}
    if f == "machine":
        prob, h_m, mach_v = enc.machine_actor_forward(d["mfea1"], d["mfea2"], d["h_o"], d["mmask"])
        return {"mch_prob": prob, "h_pooled_m": h_m, "mach_v": mach_v}
    return {"global_v": enc.global_critic_forward(d["tfea"], d["col"], d["val"], d["mfea1"], d["mfea2"])}


def _run(enc, d, which=None):
    """{forward: {tensor: host array}} (each forward read back before the next one reuses the handle's output tensors)"""
    return {f: {k: v.cpu().numpy().copy() for k, v in _enqueue(enc, d, f).items()} for f in which or R.FORWARDS}


def _handle(enc_mod, inp, w, mode=0, bn=False):
    e = enc_mod.Encoder(inp["J"], inp["M"], inp["B"], obs_dtype="f32")
    e.load_weights(*w)
    e.set_product_mode(mode)
    e.set_bn_mode(bn)
    return e


def _bitwise_outputs(a, b):
    return {(f, t) for f in a for t in a[f] if np.array_equal(a[f][t], b[f][t])}


def _same(got, want, bitwise, what):
    """the reload rule: every output within RELOAD_BOUND of scale, and bit for bit on those in `bitwise`"""
    d = R.distances(got, want)
    print(what, {f"{f}.{t}": f"{v:.1e}" for (f, t), v in d.items()})
    for (f, t), v in d.items():
        assert np.isfinite(got[f][t]).all(), (what, f, t)
        assert v <= R.RELOAD_BOUND, (what, f, t, v)
        if (f, t) in bitwise:
            assert np.array_equal(got[f][t], want[f][t]), (what, f, t, "not bit for bit", v)


def _against_oracle(got, want, what, per_instance=False):
    """tolerances of tests/test_encoder_sizes_gpu.py (random weights); global_v: 1e-3 relative, as tests/test_encoder_hip.py"""
    print(what, "vs oracle", {f"{f}.{t}": f"{v:.1e}" for (f, t), v in R.distances(got, want).items()})
    for f in got:
        g, w = got[f], want[f]
        if f in ("first", "later"):
            np.testing.assert_allclose(g["h_pooled_o"], w["h_pooled_o"], rtol=0, atol=2e-4 * max(1.0, float(np.abs(w["h_pooled_o"]).max())), err_msg=what)
            np.testing.assert_allclose(g["prob"], w["prob"], rtol=0, atol=2e-4, err_msg=what)
            np.testing.assert_allclose(g["job_v"], w["job_v"], rtol=2e-3, atol=2e-3, err_msg=what)
        elif f == "machine":
            htol = 5e-3 if per_instance else 2e-4
            np.testing.assert_allclose(g["mch_prob"], w["mch_prob"], rtol=0, atol=5e-4, err_msg=what)
            dh = np.abs(g["h_pooled_m"] - w["h_pooled_m"])
            assert dh.max() < htol * 4 and np.median(dh) < htol / 4, (what, dh.max(), np.median(dh))
            np.testing.assert_allclose(g["mach_v"], w["mach_v"], rtol=5e-3, atol=5e-3, err_msg=what)
        else:
            assert R.distance("global_v", g["global_v"], w["global_v"]) <= 1e-3, what


# name: (inputs, product mode, per-instance BatchNorm, job actor's GIN path, global critic's GIN path)
PATHS = {
    "single_launch": ("j6m6", 0, False, "single_launch", "single_launch"),
    "single_launch_f32_products": ("j6m6", 15, False, "streaming", "streaming"),     # (f32-instruction products run as streaming launches)
    "streaming_by_mode": ("j6m6", 16, False, "streaming", "streaming"),
    "per_instance_bn": ("j6m6", 0, True, "per_instance", "single_launch"),
    "per_instance_bn_f32_products": ("j6m6", 15, True, "per_instance", "streaming"),
    "streaming_by_shape": ("j10m10", 0, False, "streaming", "streaming"),
    "streaming_by_shape_f32_products": ("j10m10", 15, False, "streaming", "streaming"),
}


def _assert_path(torch, capi, e, inp, mode, bn, job_path, critic_path, d):
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for f, critic, want in (("later", False, job_path), ("critic", True, critic_path)):
        _enqueue(e, d, f)
        plan = e.gin_launches()
        assert plan["path"] == want, (f, plan)
        rule = capi.gin_launches_for(inp["B"], inp["J"], inp["M"], num_cu, critic=critic, per_instance=bn, product_mode=mode)
        assert (plan["pool"], [s[:2] for s in plan["steps"]]) == (rule["pool"], [s[:2] for s in rule["steps"]]), (f, plan, rule)
        if want == "single_launch":
            assert e.gin_res_kernel_name() == "k_gin_res"
    assert e.check() == (mode == 0 and inp["T"] <= 65)              # the single launch is in use for this shape and mode
    assert e.range_fallbacks() == (0, mode)


@pytest.mark.parametrize("path", list(PATHS))
def test_full_and_idempotent_reload(path, sets, inputs):
    """two rounds of every forward under W1, load W2 on the same handle: every forward equals a fresh W2 handle's; loading W2 once more changes nothing;
    loading W1 again gives the first outputs again"""
    torch, enc_mod, capi, _ = _mods()
    W1, W2 = sets
    shape, mode, bn, job_path, critic_path = PATHS[path]
    inp = inputs[shape]
    d = _device(inp)
    used = _handle(enc_mod, inp, W1, mode, bn)
    _assert_path(torch, capi, used, inp, mode, bn, job_path, critic_path, d)
    _run(used, d)
    first = _run(used, d)
    n_alloc = used.device_allocations()
    fresh = [_handle(enc_mod, inp, W2, mode, bn) for _ in range(2)]
    want, again = _run(fresh[0], d), _run(fresh[1], d)
    bitwise = _bitwise_outputs(want, again)
    print(path, "bit for bit between two fresh handles:", sorted(f"{f}.{t}" for f, t in bitwise))
    _same(again, want, bitwise, "fresh/fresh")
    _against_oracle(want, R.oracle_outputs(W2, inp, per_instance=bn), path + " W2", bn)
    _against_oracle(first, R.oracle_outputs(W1, inp, per_instance=bn), path + " W1", bn)
    assert min(R.distances(first, want).values()) >= R.OBSERVABLE_AT          # (the two sets are told apart on every output, on the device too)

    used.load_weights(*W2)
    reloaded = _run(used, d)
    _same(reloaded, want, bitwise, "reloaded/fresh")
    used.load_weights(*W2)
    _same(_run(used, d), reloaded, bitwise, "idempotent")
    used.load_weights(*W1)
    _same(_run(used, d), first, bitwise, "back to W1")
    assert used.device_allocations() == n_alloc                               # nothing allocated by three reloads
    for e in [used] + fresh:
        assert e.range_fallbacks() == (0, mode)
        e.check()
        e.close()


@pytest.mark.parametrize("mode", [0, 15, 16])
def test_single_key_walk(mode, sets, inputs):
    """one tensor after another loaded ALONE on a used handle (perturbed, cumulative), then the forwards that read it: held to the oracle of the mixed set;
    where several tensors feed one derived image (the fused GAT projections), and after the last step, to a fresh handle of the mixed set as well"""
    torch, enc_mod, capi, _ = _mods()
    W1, _ = sets
    inp = inputs["j6m6"]
    d = _device(inp)
    used = _handle(enc_mod, inp, W1, mode)
    assert used.check() == (mode == 0)
    _run(used, d)
    _run(used, d)
    steps, w = 0, W1
    for key, w in R.walk(W1):
        prefix = next(p for p in R.PREFIXES if key.startswith(p))
        one = {key[len(prefix):]: R.get(w, key)}
        used.load_weights(*[one if p == prefix else {} for p in R.PREFIXES])
        fs = R.forwards_reading(key)
        got = _run(used, d, fs)
        _against_oracle(got, R.oracle_outputs(w, inp, fs), f"mode {mode} after {key}")
        if key.endswith(("gat_layer.W", "m_fea_1_fcl.weight", "m_fea_2_fcl.weight")):
            fresh = _handle(enc_mod, inp, w, mode)
            _same(got, _run(fresh, d, fs), set(), f"mode {mode} after {key} vs fresh")
            fresh.close()
        steps += 1
    assert steps == len(R.all_keys(W1)) - (len(R.UNOBSERVABLE) - 1)
    fresh = _handle(enc_mod, inp, w, mode)
    _same(_run(used, d), _run(fresh, d), set(), f"mode {mode} end of the walk vs fresh")
    assert used.range_fallbacks() == (0, mode) and fresh.range_fallbacks() == (0, mode)
    used.check()


def test_reload_at_the_fixed_instantiation_and_in_the_three_in_one_launch(sets):
    """B = 16 x compute units at J6M6: the GIN kernel compiled for that shape (no node output) and the three-in-one heads launch of a rollout step.  One full
    reload on a handle that has stepped, against a fresh handle: the plain forwards on the environment's observation, then two joint decisions through
    ActorPair.act (selection, log-probabilities, values) — fused_launches() tells that they took the three-in-one launch"""
    torch, enc_mod, capi, rollout = _mods()
    W1, W2 = sets
    J, M, E = 6, 6, 2
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * num_cu
    assert capi.gin_res_kernel_for(B, J, M, num_cu)[0] == "k_gin_res_t36j6x16" and capi.fused3_kernel_for(B, J, M, num_cu)[0] is not None
    ro = rollout.Rollout(J, M, E, B, policy="actor", obs_dtype="f32", weights=W1, collect=False, seed=77)
    for _ in range(5):
        ro.step()
    env, used = ro.env, ro.actor.enc
    assert used.check() and used.gin_res_kernel_name() == "k_gin_res_t36j6x16" and used.fused_launches() == 5
    # the observation of a fresh episode (mid-episode this environment leaves one job unmasked in most instances: a one-hot prob, whatever o_policy holds)
    env.scaler_reset_returns(); env.reset(ro._episode_w3()); ro.actor.begin_episode()
    env.observe_mfea1(env.candidate[:, 0].contiguous())
    torch.cuda.synchronize()
    assert int((env.job_mask == 0).sum(1).min()) >= 3 and float(((env.mmask == 0).sum(1) >= 2).float().mean()) > 0.5
    d = dict(tfea=env.tasks_fea, col=env.ell_col, val=env.ell_val, cand=env.candidate, mask=env.job_mask, hm=used.h_pooled_m.clone(),
             mfea1=env.m_fea1.clone(), mfea2=env.m_fea2, mmask=env.mmask.clone(), h_o=used.h_pooled_o.clone())
    under_w1 = _run(used, d)
    fresh = [enc_mod.ActorPair(J, M, B, obs_dtype="f32", weights=W2, seed=ro.seed) for _ in range(2)]
    want, again = _run(fresh[0].enc, d), _run(fresh[1].enc, d)
    assert min(R.distances(under_w1, want).values()) >= R.OBSERVABLE_AT       # the two sets are told apart on every output of this observation
    bitwise = _bitwise_outputs(want, again)
    print("bit for bit between two fresh handles:", sorted(f"{f}.{t}" for f, t in bitwise))
    used.load_weights(*W2)
    _same(_run(used, d, ("first",)), {"first": want["first"]}, bitwise, "first forward after the reload")
    assert used.gin_res_kernel_name() == "k_gin_res_t36j6x16"
    _same(_run(used, d), want, bitwise, "reloaded/fresh")

    def decisions(pair):
        """two joint decisions on the same observation: the first with the learned `_input`, the second with the pair's own machine embedding"""
        n0 = pair.enc.fused_launches()
        pair.begin_episode()
        out = {}
        for c in (100, 101):
            task, mach, job = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
            pair.act(env, c, task, mach, job)
            torch.cuda.synchronize()
            out[c] = dict(task=task.cpu().numpy(), mach=mach.cpu().numpy(), job=job.cpu().numpy(), job_logp=pair.job_logp.cpu().numpy().copy(),
                          mch_logp=pair.mch_logp.cpu().numpy().copy(), job_v=pair.enc.job_v.cpu().numpy().copy(), mach_v=pair.enc.mach_v.cpu().numpy().copy())
        assert pair.enc.fused_launches() == n0 + 2 and pair.enc.fused3_kernel_name() is not None
        return out

    a, b, c = decisions(ro.actor), decisions(fresh[0]), decisions(fresh[1])
    for step in a:
        exact = {k for k in a[step] if np.array_equal(b[step][k], c[step][k])}
        for k in ("task", "mach", "job"):
            assert k in exact and np.array_equal(a[step][k], b[step][k]), (step, k)
        for k in ("job_logp", "mch_logp", "job_v", "mach_v"):
            v = R.distance(k, a[step][k], b[step][k])
            assert v <= R.RELOAD_BOUND and (k not in exact or np.array_equal(a[step][k], b[step][k])), (step, k, v)
    for e in (used, fresh[0].enc, fresh[1].enc):
        assert e.check() and e.range_fallbacks()[0] == 0


def _episode(ro, steps):
    """-> per step (task, machine, job, job log-probability, machine log-probability, job values, machine values, step info) of `steps` rollout steps"""
    import torch
    rec = []
    for _ in range(steps):
        ro.step()
        e = ro.actor.enc
        rec.append([x.clone() for x in (ro.task, ro.mach, ro.job, ro.actor.job_logp, ro.actor.mch_logp, e.job_v, e.mach_v, ro.env.info)])
    torch.cuda.current_stream().synchronize()
    return [np.stack([r[i].cpu().numpy() for r in rec]) for i in range(8)]


def _same_episode(got, want, exact_values, what):
    names = ("task", "machine", "job", "job_logp", "mch_logp", "job_v", "mach_v", "info")
    for i, k in enumerate(names):
        if i < 3:
            assert np.array_equal(got[i], want[i]), (what, k)
        elif i < 7:
            v = R.distance(k, got[i], want[i])
            assert v <= R.RELOAD_BOUND and (k not in exact_values or np.array_equal(got[i], want[i])), (what, k, v)


def test_rollout_episode_after_a_reload(sets):
    """Rollout.step (ActorPair.act: selection, m_fea1 and the GAT passes riding in the job heads' launch) at J6M6 x 32, seeded: the episode after
    load_weights(W2) on a handle that ran an episode under W1 equals the same episode of a fresh Rollout that was given W2 — decisions exactly,
    log-probabilities and values by the reload rule.  (Rewards are not compared: the reward scaler's running statistics belong to the environment's
    history, not to the weights.)"""
    torch, enc_mod, capi, rollout = _mods()
    W1, W2 = sets
    J, M, E, B = 6, 6, 2, 32
    T = J * M
    mk = lambda w: rollout.Rollout(J, M, E, B, policy="actor", obs_dtype="f32", weights=w, collect=False, seed=4321)
    used = mk(W1)
    _episode(used, T)
    kernels = [used.actor.enc.heads_kernel(i)[0] for i in (0, 1)]
    used.actor.enc.load_weights(*W2)
    got = _episode(used, T)
    fresh = []
    for _ in range(2):
        ro = mk(W2)
        ro.episode, ro.nsteps = 1, T                                 # the same reward-weight draw and the same selection counters as the used one's second episode
        fresh.append(_episode(ro, T))
        assert [ro.actor.enc.heads_kernel(i)[0] for i in (0, 1)] == kernels and ro.actor.enc.check()
    names = ("task", "machine", "job", "job_logp", "mch_logp", "job_v", "mach_v")
    exact = {k for i, k in enumerate(names) if np.array_equal(fresh[0][i], fresh[1][i])}
    print("heads launches:", kernels, "bit for bit between two fresh rollouts:", sorted(exact))
    assert {"task", "machine", "job"} <= exact
    _same_episode(got, fresh[0], exact, "episode after the reload")
    assert used.actor.enc.check() and used.actor.enc.range_fallbacks()[0] == 0 and used.n_resident_failures == 0
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert used.actor.enc.fused_launches() == (2 * T if capi.fused3_kernel_for(B, J, M, num_cu)[0] else 0)


def test_reloads_allocate_nothing(sets, inputs):
    """200 updates of the machine actor's and the global critic's GAT projection inputs, each followed by the forwards that rebuild the fused
    projections: the handle owns as many device buffers, and bytes, after cycle 200 as after cycle 2"""
    torch, enc_mod, capi, _ = _mods()
    W1, W2 = sets
    inp = inputs["j6m6"]
    d = _device(inp)
    e = _handle(enc_mod, inp, W1)
    keys = ("gat_layer.W", "m_fea_1_fcl.weight", "m_fea_2_fcl.weight")
    counts = {}
    for cycle in range(1, 201):
        w = W2 if cycle % 2 else W1
        e.load_weights({}, {k: w[1][k] for k in keys}, {k: w[2][k] for k in keys})
        _enqueue(e, d, "machine")
        _enqueue(e, d, "critic")
        if cycle in (2, 200):
            counts[cycle] = e.device_allocations()
    print("device allocations (buffers, bytes) after cycle 2 and after cycle 200:", counts)
    assert counts[200] == counts[2], counts
    fresh = _handle(enc_mod, inp, W1)                                # cycle 200 loaded W1's tensors
    fs = ("machine", "critic")
    _same(_run(e, d, fs), _run(fresh, d, fs), set(), "after 200 reloads vs fresh")
    e.check()


# ---- ordering on a caller-owned, non-blocking stream

def _spin_cycles_per_second(torch):
    """torch.cuda._sleep spins for a number of device clock ticks: the tick rate, measured"""
    s = torch.cuda.current_stream()
    torch.cuda._sleep(1000); s.synchronize()
    n = 20_000_000
    t0 = time.perf_counter(); torch.cuda._sleep(n); s.synchronize()
    return n / (time.perf_counter() - t0)


def test_reload_behind_a_queued_forward_on_a_side_stream(sets, inputs):
    """Under torch.cuda.stream(torch.cuda.Stream()) the handle enqueues on a non-blocking stream, which the null stream does not order.  A delay, a job
    actor forward and a machine actor forward under W1 are enqueued, then load_weights(W2) is called from the host: the queued forwards must give the
    outputs of W1 (those of the same forwards without the delay), forwards enqueued after the load those of W2.
    The delay is sized in the test: max(10 x the measured host time of load_weights on the idle handle, 0.2 s) of torch.cuda._sleep at its measured
    tick rate.  Chosen value on the MI355X this was written on: 0.2 s (load_weights of the whole set took 4.8 ms there; 2.39e9 ticks per second).  It
    precedes correct work and runs once.  (Before the library ordered the load against the handle's stream, load_weights returned after 4.7 ms here and
    the queued forwards gave W2's outputs: 3.4e-2 from W1's in prob, 0.9 of scale in h_pooled_o.)"""
    torch, enc_mod, capi, _ = _mods()
    W1, W2 = sets
    inp = inputs["j6m6"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        d = _device(inp)
        e = _handle(enc_mod, inp, W1)                                # takes the current stream: the side stream
        fs = ("later", "machine")
        ref1, ref1b = _run(e, d, fs), _run(e, d, fs)
        bitwise = _bitwise_outputs(ref1, ref1b)
        fresh2 = _handle(enc_mod, inp, W2)
        ref2 = _run(fresh2, d, fs)
        assert min(R.distances(ref2, ref1).values()) >= R.OBSERVABLE_AT
        side.synchronize()
        t0 = time.perf_counter(); e.load_weights(*W1); t_load = time.perf_counter() - t0
        delay = max(10.0 * t_load, 0.2)
        rate = _spin_cycles_per_second(torch)
        print(f"load_weights on the idle handle {t_load * 1e3:.1f} ms, delay {delay:.3f} s, {rate / 1e6:.0f} M ticks/s")
        out = {f: {k: torch.empty_like(v) for k, v in _enqueue(e, d, f).items()} for f in fs}      # (shapes; W1 outputs, discarded)
        side.synchronize()
        t0 = time.perf_counter()
        torch.cuda._sleep(int(delay * rate))
        for f in fs:
            for k, v in _enqueue(e, d, f).items():
                out[f][k].copy_(v, non_blocking=True)
        t_enq = time.perf_counter() - t0
        e.load_weights(*W2)
        t_loaded = time.perf_counter() - t0
        side.synchronize()
        print(f"enqueued after {t_enq * 1e3:.1f} ms, load_weights returned after {t_loaded * 1e3:.1f} ms")
        assert t_enq < delay / 2                                     # the forwards were still behind the delay when the load was called
        queued = {f: {k: v.cpu().numpy() for k, v in out[f].items()} for f in fs}
        _same(queued, ref1, bitwise, "forwards queued before the load (want: W1)")
        _same(_run(e, d, fs), ref2, set(), "forwards enqueued after the load (want: W2)")
        e.check()


def test_rollout_on_a_side_stream_behind_a_delayed_producer():
    """One J6M6 x 32 rollout episode whose environment and encoder handles are created under a side stream, and whose instances are produced on that stream
    behind a delay (device copies, taken by load_instances_device), equals the same episode on the default stream: actions and step info (rewards, done)
    exactly, log-probabilities and values by the reload rule.  Until the delayed copy has run, the source tensors hold OTHER instances: an environment that
    read them on another stream would play those."""
    torch, enc_mod, capi, rollout = _mods()
    inst_mod = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    J, M, E, B = 6, 6, 2, 32
    T = J * M
    weights = enc_mod.random_init_weights(5)
    real, other = (inst_mod.generate_instances(B, J, M, E, seed=s) for s in (0, 99))

    def arrays(inst):
        t, p, tt, edge = inst
        return [np.ascontiguousarray(t, np.float64), np.ascontiguousarray(p, np.float64), np.ascontiguousarray(tt, np.float64),
                np.ascontiguousarray(batch_env.shop_of_machine(edge), np.int32)]

    def episode(side):
        with (torch.cuda.stream(torch.cuda.Stream()) if side else contextlib.nullcontext()):
            stream = torch.cuda.current_stream()
            assert (stream.cuda_stream != 0) == side
            ro = rollout.Rollout(J, M, E, B, policy="actor", obs_dtype="f32", weights=weights, collect=False, seed=99, instances=other)
            src = [torch.as_tensor(a).cuda() for a in arrays(real)]
            dev = [torch.as_tensor(a).cuda() for a in arrays(other)]
            stream.synchronize()
            if side:
                torch.cuda._sleep(int(0.2 * _spin_cycles_per_second(torch)))
            for x, s in zip(dev, src):
                x.copy_(s, non_blocking=True)                        # the producer: on this stream, behind the delay
            ro.env.load_instances_device(*dev)
            ro.env.scaler_init()
            rec = _episode(ro, T)
            assert ro.actor.enc.check() and ro.n_resident_failures == 0 and bool(ro.env.info[:, 1].all())
            return rec

    want, again, got = episode(False), episode(False), episode(True)
    names = ("task", "machine", "job", "job_logp", "mch_logp", "job_v", "mach_v", "info")
    exact = {k for i, k in enumerate(names) if np.array_equal(want[i], again[i])}
    assert {"task", "machine", "job", "info"} <= exact
    _same_episode(got, want, exact, "side stream")
    assert np.array_equal(got[7], want[7])                           # rewards and done flags of every step
