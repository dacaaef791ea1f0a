"""GPU: what a FREE-RUNNING Rollout(collect="full") leaves in its device TrajectoryBuffer, slot by slot, against the host model
(tests/trajectory_replay_ref.py, pinned by tests/test_trajectory_replay_cpu.py) — on every launch form that writes the record in
place: the fused selection (indices and log-probabilities into slot views), the job heads' launch (m_fea1 and the machine mask into
the slot, read back from there by the machine actor), the heads launches (both critics' values into the T + 1 aliased value slots,
the post-terminal pair into the terminal slot), the step kernel or the step riding as the tail of a heads launch (r4 and done into
the slot) and mtfjsp_snapshot_obs2 (post-decision fields, the next slot's pre-decision fields, the scalar reward).

Every case
  * proves it ran the launch form it is about (Encoder.heads_kernel against capi.heads_kernel_for's answer for this device's CU
    count, fused_launches(), ActorPair.n_env_fused, the GIN path against capi.gin_launches_for) and prints it;
  * fills every tensor the buffer owns with a sentinel before the first step and finds none afterwards;
  * holds the environment half of every slot to the model with env_parity._same (trajectory_replay_ref.compare_slot), the recorded
    actions legal, no ST_INVALID;
  * holds the selection into the slots to the host model of the random streams (selection_check.assert_selection_exact);
  * holds probabilities, critic values and exp(log-probability) to the float32 oracle under the existing tensor classes of
    tests/error_budget.py, never looser than a class's hard cap unless the float32 oracle itself is further than half of that from a
    binary64 evaluation of the same network (`at_least`, the module's rule).  At B = 4096 the binary64 evaluation is made only for a
    figure beyond the hard cap — the same bound max(cap, 2 x |float32 oracle - binary64|), evaluated lazily — and the oracle forwards
    run on one of an episode's first, second and last slot per case and on the terminal pair (CASES); every smaller case runs every
    slot in both precisions;
  * prints its worst normalised error per tensor class.

The embeddings a slot's forwards consumed are the DEVICE's (cloned after every step; an episode's last slot and the terminal pair
take the clones a hook on ActorPair.terminal_values makes before that pair overwrites them), so round-off does not compound along
an episode.  The critics read pooled embeddings only, hence no stored value depends on the job mask of the post-terminal forward:
the mask that forward was GIVEN is cloned by the same hook and held to the model's pre-decision mask of the last slot.

Beyond a hard cap, taken against binary64 under the `at_least` rule (one GPU run; every other figure is inside its class's cap, the
largest 2.5e-5 for mch_prob and 1.3e-5 for mach_v at J6M6 x 96): the first decision of an episode at J6M6E2 x 4096, the machine
actor only — mch_prob 5.49e-5 from the float32 oracle (cap 4e-5) where that oracle is 5.36e-5 from binary64 and the kernel 1.92e-5;
exp(a_logprob) 4.99e-5 (5.13e-5, 1.92e-5); mach_v 2.06e-5 (cap 2e-5; 2.33e-5, 6.6e-6).  The kernel is the closer of the two.  The
figures of that run are in profiles/r05_encoder_errors.json under "trajectory:...".  GIN path per case: the handle's own answer is held
to capi.gin_launches_for and printed (on 256 CUs only (3, 4, 2, 7) takes the streaming launches; (13, 5, 1, 2), T = 65, is served by
the single launch)."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trajectory_replay_ref as ref  # noqa: E402
from env_parity import _same  # noqa: E402
from error_budget import DEFAULT_CAP, HARD_CAP, bound, check as budget, normalised  # noqa: E402
from selection_check import assert_selection_exact  # noqa: E402
from test_handoff_rollout_gpu import _perturb  # noqa: E402

pytestmark = pytest.mark.gpu

BLANKET = {"job_prob": 1e-4, "mch_prob": 1e-4, "job_v": 1e-3, "mach_v": 1e-3}       # tests/test_encoder_limits_gpu.py's
RELATIVE = ("job_v", "mach_v")
X, X10 = "k_headsx", "k_headsx10"
NO3, UNFUSED = {"MTFJSP_NO_FUSED_MHEADS": "1"}, {"MTFJSP_NO_FUSED_SELECT": "1"}
ENV2, ENV3 = {"MTFJSP_FUSED_ENV": "1"}, {"MTFJSP_FUSED_ENV3": "1"}
SENTINEL_INT, SENTINEL_BYTE = -7, 2
# (J, M, E, B), episodes per buffer, observation dtype, switches, greedy, (job, machine) heads launches on a 256-CU device, buffers,
# slots of the oracle forwards (None: every slot; -1: an episode's last).  At B = 4096 one job forward of the oracle takes more than a
# second, so each case there runs one of an episode's first (the learned `_input`), second (the first carried embedding) and last
# slot, the four cases together all three; the terminal pair is evaluated in every case
CASES = [
    ((3, 4, 2, 7), 3, "f32", {}, False, (X, X), 2, None),
    ((5, 7, 1, 19), 2, "f64", {}, False, (X, X), 1, None),
    ((13, 5, 1, 2), 1, "f32", {}, False, (X10, X), 1, None),
    ((4, 16, 2, 19), 1, "f32", {}, False, (X, X10), 1, None),
    ((6, 4, 2, 336), 1, "f32", NO3, False, ("k_headsx_gat3x", X), 1, None),
    ((6, 6, 2, 96), 2, "f32", UNFUSED, False, (X, X), 1, None),
    ((6, 6, 2, 96), 2, "f32", UNFUSED, True, (X, X), 1, None),
    ((6, 6, 2, 4096), 1, "f32", {}, False, ("three_in_one", "three_in_one"), 1, (0,)),
    ((7, 5, 1, 4096), 1, "f32", {}, False, ("three_in_one", "three_in_one"), 1, (1,)),
    ((6, 6, 2, 4096), 1, "f32", ENV2, False, ("k_headsx_gat3x", "k_headsx_envstep"), 1, (-1,)),
    ((6, 6, 2, 4096), 1, "f32", ENV3, False, ("three_in_one_env", "three_in_one_env"), 1, (1,)),
]


def _case_id(c):
    (J, M, E, B), eps, obs, env, greedy, _, _, _ = c
    sw = "+".join(k.replace("MTFJSP_", "") for k in env) or "default"
    return f"J{J}M{M}E{E}x{B}x{eps}-{obs}-{sw}" + ("-greedy" if greedy else "")


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.encoder"), import_module("e2e-mappo-for-mt-fjsp_amd.rollout"),
            import_module("e2e-mappo-for-mt-fjsp_amd.capi"), import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"))


def _kernel_of(form):
    return "k_headsx_gat3x_headsx" if form.startswith("three_in_one") else form


def _rule(capi, J, M, B, num_cu, env, f64):
    """-> ((job kernel, group, grid), (machine ...)) of a recording step by the handle-free rule, from what ActorPair.act arms under
    the case's switches (tests/test_selection_exact_gpu._asks, with the unfused path and the observation dtype added)"""
    fused = not env.get("MTFJSP_NO_FUSED_SELECT")
    handle = dict(gat_ok=True, mheads_ok=not env.get("MTFJSP_NO_FUSED_MHEADS"), obs_f64=f64)
    mheads = fused and not env.get("MTFJSP_FUSED_ENV")
    kj = capi.heads_kernel_for(B, J, M, num_cu=num_cu, gat=fused, mheads=mheads, env_tail=bool(mheads and env.get("MTFJSP_FUSED_ENV3")), **handle)
    if kj[0].startswith("k_headsx_gat3x_headsx"):
        return kj, kj                                   # the machine forward rode in the job launch
    return kj, capi.heads_kernel_for(B, J, M, which=1, num_cu=num_cu, env_tail=bool(env.get("MTFJSP_FUSED_ENV")), **handle)


def _owned(tb):
    return {k: v for k, v in vars(tb).items() if torch.is_tensor(v) and v._base is None}


def _sentinel(tb):
    """every tensor the buffer owns: NaN in floats, -7 in integers, byte 2 in masks (the kernels write bytes 0 and 1)"""
    for v in _owned(tb).values():
        if v.dtype == torch.bool:
            v.view(torch.uint8).fill_(SENTINEL_BYTE)
        elif v.dtype.is_floating_point:
            v.fill_(float("nan"))
        else:
            v.fill_(SENTINEL_INT)


def _assert_no_sentinel(tb):
    names = set(_owned(tb))
    assert {"_jv", "_mv", "r4", "random_weight", "a_logprob", "a_logprob_operation", "mask_machine_", "machine_fea1"} <= names, names
    for k, v in _owned(tb).items():
        if v.dtype == torch.bool:
            left = int((v.view(torch.uint8) > 1).sum().item())
        elif v.dtype.is_floating_point:
            left = int((~torch.isfinite(v)).sum().item())
        else:
            left = int((v == SENTINEL_INT).sum().item())
        if left:
            bad = (v.view(torch.uint8) > 1) if v.dtype == torch.bool else (~torch.isfinite(v)) if v.dtype.is_floating_point else (v == SENTINEL_INT)
            first = tuple(int(x) for x in bad.nonzero()[0])
            raise AssertionError(f"{k}: {left} of {v.numel()} elements were never written (or are not finite), first at {first} of {tuple(v.shape)}")


def _fill(ro, capi, forms, rule):
    """one buffer of the free-running rollout over sentinelled storage, the last step with the hand-off held back
    -> (clones per slot, release()) — release runs the held-back hand-off and the buffer's reset"""
    tb, env, act, enc = ro.traj, ro.env, ro.actor, ro.actor.enc
    S, T = ro.S, ro.T
    three = forms[0].startswith("three_in_one")
    _sentinel(tb)
    got = dict(job_prob=[], mch_prob=[], h_o=[], h_m=[], task=[], cand=[], jmask=[], term_mask=[], n0=ro.nsteps)
    flags = torch.zeros(ro.B, dtype=torch.int32, device=env.device)
    keep = {}
    terminal = act.terminal_values

    def hooked(env_, prev_job_mask, jv_out, mv_out):
        # the decision's own outputs, before the post-terminal pair runs over them, and the mask that pair is given
        keep["last"] = [x.clone() for x in (enc.job_prob, enc.mch_prob, enc.h_pooled_o, enc.h_pooled_m)]
        got["term_mask"].append(prev_job_mask.clone())
        return terminal(env_, prev_job_mask, jv_out, mv_out)

    act.terminal_values = hooked
    held = {}
    try:
        for s in range(S):
            if s == S - 1:
                held["finish"], held["reset"] = ro.finish_buffer, tb.reset
                ro.finish_buffer, tb.reset = (lambda: None), (lambda: None)
            got["cand"].append(env.candidate.clone()); got["jmask"].append(env.job_mask.clone())
            assert tb.count_operation == s
            ro.step()
            flags |= env.status
            last = s % T == T - 1
            outs = keep.pop("last") if last else [x.clone() for x in (enc.job_prob, enc.mch_prob, enc.h_pooled_o, enc.h_pooled_m)]
            for k, x in zip(("job_prob", "mch_prob", "h_o", "h_m"), outs):
                got[k].append(x)
            got["task"].append(ro.task.clone())
            if not last:                                   # (after a terminal step the last forwards are the values-only pair's)
                for which in (0, 1):
                    name, group, grid = enc.heads_kernel(which)
                    want = _kernel_of(forms[which])
                    assert name is not None and (name.startswith(want) if three else name == want), f"step {s}: forward {which} ran {name}, expected {want}"
                    assert (group, grid) == rule[which][1:], f"step {s}: forward {which}: groups of {group} in {grid} workgroups, the rule says {rule[which][1:]}"
    finally:
        act.terminal_values = terminal
    torch.cuda.synchronize()
    assert tb.full and ro.n_resident_failures == 0 and not ro.tainted
    assert int((flags & capi.ST_INVALID).ne(0).sum().item()) == 0, "ST_INVALID"

    def release():
        ro.finish_buffer, tb.reset = held["finish"], held["reset"]
        ro.finish_buffer(); tb.reset()
        torch.cuda.synchronize()
        assert tb.count_operation == 0
    return got, release


class _Worst:
    def __init__(self):
        self.w = {}

    def add(self, tensor, err):
        self.w[tensor] = max(self.w.get(tensor, 0.0), err)


def _held(worst, case, tensor, hip, f32, f64):
    """hip against the float32 oracle within max(bound of (case, tensor), 2 x |float32 oracle - binary64|); f64: the binary64
    evaluation, or a function that makes it (called only for a figure beyond the bound without it).  A figure beyond the class's
    hard cap is printed with the two distances that admit it"""
    rel = tensor in RELATIVE
    hip = hip.detach().cpu().numpy() if torch.is_tensor(hip) else np.asarray(hip)
    e_hip = normalised(hip, f32, None, rel)
    at_least = 0.0
    if not callable(f64) or e_hip > bound(case, tensor, BLANKET[tensor]):
        f64 = f64() if callable(f64) else f64
        at_least = 2 * normalised(f32, f64, None, rel)
    if e_hip > HARD_CAP[tensor]:
        print(f"{case} {tensor}: beyond the hard cap {HARD_CAP[tensor]:.1g}: HIP vs float32 oracle {e_hip:.3g}, float32 oracle vs binary64 {at_least / 2:.3g}, "
              f"HIP vs binary64 {normalised(hip, f64, None, rel):.3g}")
    worst.add(tensor, budget(case, tensor, hip, f32, BLANKET[tensor], None, rel, at_least=at_least))


def _check_buffer(case, model, ro, got, weights, forms, greedy, seed, net_slots, lazy64, worst):
    tb = ro.traj
    J, M, B, T, S = ro.J, ro.M, ro.B, ro.T, ro.S
    eps = S // T
    from oracle import encoder_oracle as eo
    ja, ma = weights
    n = lambda x: x.cpu().numpy()
    rows = np.arange(B)
    _assert_no_sentinel(tb)
    # ---- the aliased value slots: v_ of a slot IS v of the next one inside an episode, the terminal slot at its end
    jv, mv, jv_, mv_ = tb.local_values()
    for e in range(eps):
        o = e * T
        assert torch.equal(jv_[o:o + T - 1], jv[o + 1:o + T]) and torch.equal(mv_[o:o + T - 1], mv[o + 1:o + T])
        assert torch.equal(jv_[o + T - 1], tb._jv[e, T]) and torch.equal(mv_[o + T - 1], tb._mv[e, T])
    out = tb.numpy_to_tensor_operation()
    assert len(out) == 27 and all(torch.equal(a, b) for a, b in zip(out[23:], (jv, mv, jv_, mv_)))
    assert len(got["term_mask"]) == eps
    a_op, a_m = n(tb.a_operation), n(tb.a)
    logp_o, logp_m = n(tb.a_logprob_operation), n(tb.a_logprob)
    dev = lambda s: {k: n(getattr(tb, k)[s]) for k in ref.FIELDS}
    f64 = torch.float64
    state = {}

    def _check_slot_network(s):
        want, (e, t) = state["want"], divmod(s, T)
        pick = lambda fn: fn if lazy64 else fn()
        hm_prev = None if t == 0 else n(got["h_m"][s - 1])
        h_o = n(got["h_o"][s])
        j32, m32 = ref.slot_forward(ja, ma, want, hm_prev, h_o=h_o)
        memo = {}

        def job64():
            if "j" not in memo:
                memo["j"] = eo.job_actor_forward(ja, want["tasks_fea"], want["ell_col"], want["ell_val"], want["candidate"], want["mask_operation"], hm_prev, B, T, dtype=f64)
            return memo["j"]

        def mach64():
            if "m" not in memo:
                memo["m"] = eo.machine_actor_forward(ma, want["machine_fea1"], want["machine_fea2"], h_o, want["mask_machine_"], B, M, dtype=f64)
            return memo["m"]

        _held(worst, case, "job_prob", got["job_prob"][s], j32["prob"], pick(lambda: job64()["prob"]))
        _held(worst, case, "mch_prob", got["mch_prob"][s], m32["prob"], pick(lambda: mach64()["prob"]))
        _held(worst, case, "job_v", tb._jv[e, t], j32["job_v"], pick(lambda: job64()["job_v"]))
        _held(worst, case, "mach_v", tb._mv[e, t], m32["mach_v"], pick(lambda: mach64()["mach_v"]))
        # exp(stored log-probability) against the oracle's probability of the recorded action
        _held(worst, case + ":logp", "job_prob", np.exp(logp_o[s].astype(np.float64)), j32["prob"][rows, a_op[s]], pick(lambda: job64()["prob"][rows, a_op[s]]))
        _held(worst, case + ":logp", "mch_prob", np.exp(logp_m[s].astype(np.float64)), m32["prob"][rows, a_m[s]], pick(lambda: mach64()["prob"][rows, a_m[s]]))

    def _check_terminal_pair(s):
        # the terminal slot against the model's pair, on the device's machine embedding of the last decision
        want, e = state["want"], s // T
        pick = lambda fn: fn if lazy64 else fn()
        hm_last = n(got["h_m"][s])
        tj32, tm32 = ref.terminal_pair(ja, ma, want, hm_last)
        memo = {}

        def term64():
            if "x" not in memo:
                memo["x"] = ref.terminal_pair(ja, ma, want, hm_last, dtype=f64)
            return memo["x"]

        _held(worst, case + ":term", "job_v", tb._jv[e, T], tj32["job_v"], pick(lambda: term64()[0]["job_v"]))
        _held(worst, case + ":term", "mach_v", tb._mv[e, T], tm32["mach_v"], pick(lambda: term64()[1]["mach_v"]))

    count = 0
    for s, want in enumerate(model.slots(a_op, a_m, eps)):
        e, t = divmod(s, T)
        count += 1
        state["want"] = want
        # ---- environment half
        ref.compare_slot(dev(s), want, s)
        assert np.array_equal(n(got["task"][s]), want["task"]), f"slot {s}: the task the step was given is not candidate[job]"
        if t > 0:                                        # (an episode's first decision sees the reset made inside its step)
            assert np.array_equal(n(got["cand"][s]), want["candidate"]) and np.array_equal(n(got["jmask"][s]) != 0, want["mask_operation"]), s
        # ---- the selection, into the slot
        k = got["n0"] + s
        assert_selection_exact(got["job_prob"][s], a_op[s], logp_o[s], seed, 2 * k, greedy, gather_from=want["candidate"], gathered=got["task"][s],
                               mask=want["mask_operation"], form=forms[0])
        assert_selection_exact(got["mch_prob"][s], a_m[s], logp_m[s], seed, 2 * k + 1, greedy, mask=want["mask_machine_"].reshape(B, M), form=forms[1])
        if t == T - 1:
            _same(n(got["term_mask"][e]) != 0, want["mask_operation"], f"slot {s} term_mask (the job mask of the post-terminal forward)")
        # ---- network half: the float32 oracle (and binary64) on the slot's own fields and the device's embeddings
        if s in net_slots:
            _check_slot_network(s)
        if t == T - 1:
            _check_terminal_pair(s)
    assert count == S, f"the model's replay ended after {count} of {S} slots"


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_free_running_rollout_records_what_the_model_replays(c, monkeypatch):
    (J, M, E, B), eps, obs, env_sw, greedy, forms, buffers, oracle_slots = c
    for k in ("MTFJSP_NO_FUSED_MHEADS", "MTFJSP_NO_FUSED_SELECT", "MTFJSP_FUSED_ENV", "MTFJSP_FUSED_ENV3", "MTFJSP_NO_VALUES_ONLY", "MTFJSP_NO_RESET_EPISODE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env_sw.items():
        monkeypatch.setenv(k, v)
    enc_mod, rollout, capi, batch_env = _mods()
    T, S = J * M, eps * J * M
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rule = _rule(capi, J, M, B, num_cu, env_sw, obs == "f64")
    routed = tuple(r[0] for r in rule)
    assert all(r.startswith(_kernel_of(f)) if f.startswith("three_in_one") else r == f for r, f in zip(routed, forms)), \
        f"on {num_cu} CUs this shape is routed to {routed}: choose another shape"
    three, stepping, fused = forms[0].startswith("three_in_one"), forms[1] in ("k_headsx_envstep", "three_in_one_env"), not env_sw.get("MTFJSP_NO_FUSED_SELECT")
    sel_forms = forms if fused else ("k_sample", "k_sample")
    # B distinct instances drawn on the device and read back: the model's and the rollout's
    gen = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype=obs)
    gen.generate_instances(seed=J * 1000 + M * 10 + E)
    ins = gen.read_instances()
    gen.close()
    weights = enc_mod.random_init_weights(seed=J * 100 + M, with_critic=False)
    _perturb(weights, 3)
    seed = (1 << 32) + 4321 + B
    ro = rollout.Rollout(J, M, E, B, policy="actor", collect="full", obs_dtype=obs, buffer_episodes=eps, weights=weights, instances=ins, seed=seed,
                         greedy=greedy)
    enc = ro.actor.enc
    assert ro.S == S and ro.traj.obs_dtype == (torch.float32 if obs == "f32" else torch.float64) and ro.seed == seed
    single = enc.check()
    if three:
        assert single, "the three-in-one launch needs the single-launch GIN kernel's census"
    model = ref.TrajectoryModel(ins, seed, obs_dtype=obs, left_shift=ro.env.left_shift, w_cfg=ro.env.w_cfg, divisor=ro.env.scaling_divisor, gamma=ro.gamma)
    case = "trajectory:" + _case_id(c)
    big = oracle_slots is not None                       # (B = 4096)
    worst = _Worst()
    for fill in range(buffers):
        got, release = _fill(ro, capi, forms, rule)
        # the launch form, from the library's own counters
        done = (fill + 1) * S
        assert enc.fused_launches() == (done if three else 0), (enc.fused_launches(), done, three)
        assert ro.actor.n_env_fused == (done if stepping else 0), (ro.actor.n_env_fused, done, stepping)
        plan = enc.gin_launches()
        want_plan = capi.gin_launches_for(B, J, M, num_cu=num_cu, obs_f64=obs == "f64", single_ok=single)
        assert plan is not None and plan["path"] == want_plan["path"], (plan, want_plan)
        assert ro.nsteps == done and ro.episode == (fill + 1) * eps and ro.n_handoffs == fill
        net_slots = set(range(S)) if oracle_slots is None else {e * T + k % T for e in range(eps) for k in oracle_slots}
        _check_buffer(case, model, ro, got, weights, sel_forms, greedy, seed, net_slots, big, worst)
        assert enc.check() == single
        release()
        assert ro.n_handoffs == fill + 1 and ro.last_adv is not None
        ro.check_finished_cleanly()
    print(f"{case}: job heads {routed[0]} (groups of {rule[0][1]}, {rule[0][2]} workgroups), machine heads {routed[1]} ({rule[1][1]}, {rule[1][2]}), "
          f"three-in-one launches {enc.fused_launches()}, steps inside a heads launch {ro.actor.n_env_fused}, selection {sel_forms[0]} / {sel_forms[1]}, "
          f"GIN {plan['path']}, step kernel {ro.env.step_kernel_name()}, {buffers} buffer(s) of {S} slots, oracle forwards on {len(net_slots)} slots")
    print(f"{case}: worst normalised error per tensor class: " + ", ".join(f"{k} {v:.3g} (cap {HARD_CAP.get(k, DEFAULT_CAP):.1g})" for k, v in sorted(worst.w.items())))
