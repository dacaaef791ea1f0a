"""The six one-shot arms of an encoder handle (mtfjsp_encoder_arm_selection(0 / 1), _arm_mfea1, _arm_machine_heads, _arm_env_step,
_arm_values_only) after a forward that FAILED or was SKIPPED.  The contract (include/mtfjsp.h, "One-shot arms"): an arm belongs to the
next call of the forward it names and to no later call — a forward that returns an error, and mtfjsp_encoder_check when it reports
MTFJSP_ERR_RETRY, leave nothing armed; mtfjsp_encoder_env_step_fused() speaks of the last forward pair only.

How a forward is made to fail, host-only: MTFJSP_RANGE_FAIL_AT=1 (read when the handle is created) lets the handle's FIRST job forward
raise the host-mapped range word after its own entry poll — no kernel misbehaves, nothing waits — and the next forward entry on the
handle returns MTFJSP_ERR_RETRY and switches it to product mode 15; set_product_mode(0) is the documented way back, taken before the
forwards under test.  The other failing returns need no switch: an m_fea1 arm without a selection (MTFJSP_ERR_STATE), a null output
(MTFJSP_ERR_ARG).

What is observed: every buffer an arm could write through is pre-filled with a sentinel (selection outputs, the redirected m_fea1 /
machine mask, the armed machine-heads outputs, the handle's own prob tensors), the environment's state signature, the launches
(Encoder.heads_kernel, fused_launches).  Reference: fresh handles with the same weights that never failed, running the same un-armed
forwards — bit for bit wherever two fresh handles agree bit for bit (the rule of tests/test_weight_reload_gpu.py), else within the bounds
tests/test_encoder_hip.py holds the kernels to (probabilities 1e-4, embeddings 1e-4 of scale, values 1e-3)."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from selection_check import assert_selection_exact  # noqa: E402

pytestmark = pytest.mark.gpu
SENT, ISENT, BSENT = -7.0, -7, 0xAA
SEED = 4242
SWITCHES = ("MTFJSP_RANGE_FAIL_AT", "MTFJSP_FUSED_ENV", "MTFJSP_FUSED_ENV3", "MTFJSP_NO_FUSED_SELECT", "MTFJSP_NO_FUSED_MHEADS", "MTFJSP_NO_FUSED_GAT",
            "MTFJSP_NO_VALUES_ONLY", "MTFJSP_NO_RESIDENT_GIN")


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.encoder"), import_module("e2e-mappo-for-mt-fjsp_amd.rollout"),
            import_module("e2e-mappo-for-mt-fjsp_amd.capi"))


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _shape(name):
    """J6M6E2 at the smallest batch whose job forward can carry the whole machine forward (heads_gat_ride_shape decides: one workgroup of 16
    instances per compute unit) / J10M10E2 x 16 (T = 100: streaming GIN launches, nothing rides in the heads launch)"""
    capi = _mods()[2]
    if name == "stream":
        return 10, 10, 16
    for b in range(16, 16 * 1024 + 1, 16):
        if capi.heads_kernel_for(b, 6, 6, num_cu=_num_cu(), gat=True, mheads=True)[0].startswith("k_headsx_gat3x_headsx"):
            return 6, 6, b
    raise AssertionError("no batch up to 16384 takes the three-in-one launch at J6M6 on this device")


def _weights(enc_mod, seed=77):
    ja, ma = enc_mod.random_init_weights(seed=seed)
    rs = np.random.RandomState(seed)
    for d in (ja, ma):
        for k in d:
            if "batch_norms" in k or k.startswith("bn."):
                d[k] = (rs.uniform(0.5, 1.5, d[k].shape) if k.endswith("weight") else rs.uniform(-0.5, 0.5, d[k].shape)).astype(np.float32)
    return ja, ma


class State:
    """a rollout stepped to mid-episode and the inputs of one forward pair on its state, CLONED (a stale environment step must not change what the
    reference is computed from): the machine actor's inputs are those of every instance's first selectable candidate"""

    def __init__(self, monkeypatch, shape, obs_dtype="f32", rollout_too=False, **switches):
        """switches: set for the handles made afterwards (a handle reads them when it is created) — rollout_too: and for the rollout's own"""
        enc_mod, rollout, _ = _mods()
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in switches.items() if rollout_too else ():
            monkeypatch.setenv(k, v)
        self.J, self.M, self.B = self.shape = _shape(shape)
        self.obs_dtype, self.W = obs_dtype, _weights(enc_mod)
        self.ro = rollout.Rollout(self.J, self.M, 2, self.B, policy="actor", obs_dtype=obs_dtype, weights=self.W, collect=False, seed=3)
        for _ in range(self.J * self.M // 2 + 3):
            self.ro.step()
        for k, v in switches.items():
            monkeypatch.setenv(k, v)
        self.env = self.ro.env
        self.inputs()

    def inputs(self, hm=True):
        env = self.env
        torch.cuda.synchronize()
        mask = env.job_mask.clone()
        first = (mask == 0).int().argmax(1, keepdim=True)
        assert bool((mask.gather(1, first) == 0).all())               # every instance still has a selectable job
        self.task = env.candidate.gather(1, first).reshape(-1).int().contiguous()
        env.observe_mfea1(self.task)
        torch.cuda.synchronize()
        self.d = dict(tfea=env.tasks_fea.clone(), col=env.ell_col.clone(), val=env.ell_val.clone(), cand=env.candidate.clone(), mask=mask,
                      hm=self.ro.actor.enc.h_pooled_m.clone() if hm else None, mfea1=env.m_fea1.clone(), mfea2=env.m_fea2.clone(), mmask=env.mmask.clone())
        return self.d

    def handle(self, monkeypatch, fail_at=None):
        """a handle with the weights of the rollout's; fail_at: its n-th job forward raises the range word"""
        enc_mod = _mods()[0]
        if fail_at is None:
            monkeypatch.delenv("MTFJSP_RANGE_FAIL_AT", raising=False)
        else:
            monkeypatch.setenv("MTFJSP_RANGE_FAIL_AT", str(fail_at))
        e = enc_mod.Encoder(self.J, self.M, self.B, obs_dtype=self.obs_dtype)
        e.load_weights(*self.W)
        monkeypatch.delenv("MTFJSP_RANGE_FAIL_AT", raising=False)
        return e

    def signature(self):
        torch.cuda.synchronize()
        return self.env.state_signature().cpu().numpy().copy()


def _job(e, d):
    return e.job_actor_forward(d["tfea"], d["col"], d["val"], d["cand"], d["mask"], d["hm"])


def _machine(e, d):
    return e.machine_actor_forward(d["mfea1"], d["mfea2"], e.h_pooled_o, d["mmask"])


def _outputs(e):
    torch.cuda.synchronize()
    return {k: getattr(e, k).cpu().numpy().copy() for k in ("job_prob", "h_pooled_o", "job_v", "mch_prob", "h_pooled_m", "mach_v")}


def _pair(e, d):
    """one plain (job, machine) forward pair, nothing armed -> (outputs, the heads kernel of each forward, the GIN path)"""
    e.job_prob.fill_(SENT); e.mch_prob.fill_(SENT)
    _job(e, d)
    k0 = e.heads_kernel(0)[0]
    _machine(e, d)
    return _outputs(e), (k0, e.heads_kernel(1)[0]), e.gin_launches()["path"]


def _reference(st, monkeypatch):
    """two fresh handles' plain pair on the same inputs -> (outputs, outputs, kernels, path)"""
    a, ka, pa = _pair(st.handle(monkeypatch), st.d)
    b, kb, pb = _pair(st.handle(monkeypatch), st.d)
    assert ka == kb and pa == pb
    for k in a:
        assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), k
    assert not (a["job_prob"] == SENT).any() and not (a["mch_prob"] == SENT).any()
    return a, b, ka, pa


def _same_as_fresh(got, ref, what):
    a, b = ref[0], ref[1]
    for k in a:
        d = float(np.abs(got[k].astype(np.float64) - a[k]).max())
        print(what, k, f"max |difference| {d:.2e}", "fresh handles agree bit for bit" if np.array_equal(a[k], b[k]) else "")
    for k in a:
        assert np.isfinite(got[k]).all(), (what, k)
        if k.endswith("prob"):
            assert not (got[k] == SENT).any(), (what, k, "left unwritten")
        if np.array_equal(a[k], b[k]):
            assert np.array_equal(got[k], a[k]), (what, k, "not bit for bit")
        elif k.endswith("prob"):
            np.testing.assert_allclose(got[k], a[k], rtol=0, atol=1e-4, err_msg=f"{what} {k}")
        elif k.startswith("h_pooled"):
            np.testing.assert_allclose(got[k], a[k], rtol=0, atol=1e-4 * max(1.0, float(np.abs(a[k]).max())), err_msg=f"{what} {k}")
        else:
            np.testing.assert_allclose(got[k], a[k], rtol=1e-3, atol=1e-3, err_msg=f"{what} {k}")


class Arms:
    """sentinel-filled buffers for everything an arm can write through, and the arming calls"""

    def __init__(self, st, e):
        self.st, self.e = st, e
        B, M, dev = st.B, st.M, e.device
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.job_idx, self.task, self.mach_idx = (torch.full((B,), ISENT, **i32) for _ in range(3))
        self.job_logp, self.mch_logp = (torch.full((B,), SENT, **f32) for _ in range(2))
        self.mfea1 = torch.full((B, M, 6), SENT, dtype=torch.float32 if st.obs_dtype == "f32" else torch.float64, device=dev)
        self.mmask = torch.full((B, M), BSENT, dtype=torch.uint8, device=dev)
        self.mprob, self.mh, self.mv = torch.full((B, M), SENT, **f32), torch.full((B, 128), SENT, **f32), torch.full((B, 2), SENT, **f32)
        self.step_armed = False

    def selection0(self):
        self.e.arm_selection(0, False, SEED, 10, self.job_idx, self.job_logp, self.st.d["cand"], self.task)

    def mfea1_redirected(self):
        self.ctx = self.st.env.mfea1_context()
        assert self.ctx.m_fea2                                        # (the context that lets the GAT passes ride)
        self.ctx.m_fea1_out, self.ctx.mmask_out = self.mfea1.data_ptr(), self.mmask.data_ptr()
        self.e.arm_mfea1(self.ctx)

    def selection1(self):
        self.e.arm_selection(1, False, SEED, 11, self.mach_idx, self.mch_logp)

    def machine_heads(self):
        self.e.arm_machine_heads(self.mprob, self.mh, self.mv)

    def env_step(self, task=None):
        params = self.st.env.step_params(self.task if task is None else task, self.mach_idx)
        if params is not None:                                        # (None: this shape's step cannot ride in a heads launch at all)
            self.e.arm_env_step(params)
            self.step_armed = True

    def everything(self):
        """what ActorPair.act arms for a decision under MTFJSP_FUSED_ENV3, the m_fea1 outputs redirected as a trajectory slot's are"""
        self.selection0(); self.mfea1_redirected(); self.selection1(); self.machine_heads(); self.env_step()
        return self

    def assert_intact(self, what):
        torch.cuda.synchronize()
        for k in ("job_idx", "task", "mach_idx"):
            assert bool((getattr(self, k) == ISENT).all()), (what, k, "written through a stale arm")
        for k in ("job_logp", "mch_logp", "mfea1", "mprob", "mh", "mv"):
            assert bool((getattr(self, k) == SENT).all()), (what, k, "written through a stale arm")
        assert bool((self.mmask == BSENT).all()), (what, "mmask", "written through a stale arm")


def _retry(capi, call):
    with pytest.raises(capi.MtfjspError) as ex:
        call()
    assert ex.value.code == capi.ERR_RETRY, ex.value
    return ex


def _as_if_never_armed(st, e, arms, before, monkeypatch, what):
    """the plain pair after the failure: every sentinel intact, no three-in-one launch, no step reported or taken, outputs those of fresh handles"""
    n3, sig = before
    arms.assert_intact(what + ": the failed forward")
    got, kern, path = _pair(e, st.d)
    arms.assert_intact(what + ": the plain pair after it")
    assert e.fused_launches() == n3, (what, "a stale machine-heads arm took the three-in-one launch")
    assert not e.env_step_fused(), (what, "a step is reported that no forward of this pair was armed with")
    assert np.array_equal(st.signature(), sig), (what, "a stale arm stepped the environment")
    ref = _reference(st, monkeypatch)
    assert (kern, path) == (ref[2], ref[3]) and "k_headsx_values" not in kern, (what, kern, path, ref[2:])
    _same_as_fresh(got, ref, what)
    e.check()


def _forms(st, e):
    """the launch forms the shape is here for, asserted: J6M6 — the job forward of an armed decision can take the three-in-one launch (and the GIN
    encoder its single launch); J10M10 x 16 — streaming GIN launches, nothing rides"""
    capi = _mods()[2]
    three = capi.heads_kernel_for(st.B, st.J, st.M, num_cu=_num_cu(), gat=True, mheads=True, obs_f64=st.obs_dtype != "f32")[0].startswith("k_headsx_gat3x_headsx")
    path = capi.gin_launches_for(st.B, st.J, st.M, num_cu=_num_cu(), obs_f64=st.obs_dtype != "f32", single_ok=e.check())["path"]
    assert (three, path) == ((True, "single_launch") if st.J == 6 else (False, "streaming")), (st.shape, three, path)


# ---- A: values-only outlives a failed job forward
@pytest.mark.parametrize("shape", ["three", "stream"])
def test_values_only_arm_is_gone_after_the_job_forward_it_was_made_for_failed(shape, monkeypatch):
    capi = _mods()[2]
    st = State(monkeypatch, shape)
    e = st.handle(monkeypatch, fail_at=1)
    _forms(st, e)
    _job(e, st.d)                                                  # (the handle's first job forward: raises the range word behind its own poll)
    e.arm_values_only()
    _retry(capi, lambda: _job(e, st.d))                            # the armed forward fails at its entry
    assert e.range_fallbacks() == (1, 15)
    e.set_product_mode(0)
    full, kern, path = _pair(e, st.d)
    ref = _reference(st, monkeypatch)
    assert (kern, path) == (ref[2], ref[3]) and "k_headsx_values" not in kern, (kern, path, ref[2:])
    _same_as_fresh(full, ref, "A")
    # ... and the arm itself still works: a later armed pair leaves prob untouched and gives the full pair's values bit for bit
    e.job_prob.fill_(SENT); e.mch_prob.fill_(SENT)
    e.arm_values_only()
    _job(e, st.d); k0 = e.heads_kernel(0)[0]
    _machine(e, st.d)
    only = _outputs(e)
    assert (k0, e.heads_kernel(1)[0]) == ("k_headsx_values", "k_headsx_values")
    assert (only["job_prob"] == SENT).all() and (only["mch_prob"] == SENT).all()
    for k in ("h_pooled_o", "job_v", "h_pooled_m", "mach_v"):
        assert np.array_equal(only[k], full[k]), k
    again, kern2, _ = _pair(e, st.d)                               # one pair only
    assert kern2 == kern and all(np.array_equal(again[k], full[k]) for k in full)
    e.check()


# ---- B: the same through ActorPair with the selection as separate launches
def test_terminal_values_failure_does_not_cost_the_next_episode_its_first_decision(monkeypatch):
    enc_mod, _, capi = _mods()
    st = State(monkeypatch, "three")
    monkeypatch.setenv("MTFJSP_NO_FUSED_SELECT", "1"); monkeypatch.setenv("MTFJSP_RANGE_FAIL_AT", "1")
    pair = enc_mod.ActorPair(st.J, st.M, st.B, obs_dtype="f32", weights=st.W, seed=SEED)
    monkeypatch.delenv("MTFJSP_RANGE_FAIL_AT")
    e, env, ro = pair.enc, st.env, st.ro
    assert not pair.fused and pair.values_only_terminal
    _job(e, st.d)                                                  # (raises the range word)
    jv, mv = torch.zeros(st.B, 2, device=e.device), torch.zeros(st.B, 2, device=e.device)
    _retry(capi, lambda: pair.terminal_values(env, st.d["mask"], jv, mv))   # fails at its job forward, values-only armed
    e.set_product_mode(0)
    pair.begin_episode()
    env.scaler_reset_returns(); env.reset(ro._episode_w3())
    torch.cuda.synchronize()
    e.job_prob.fill_(SENT); e.mch_prob.fill_(SENT)
    task, mach, job = (torch.full((st.B,), ISENT, dtype=torch.int32, device=e.device) for _ in range(3))
    assert pair.act(env, 5, task, mach, job) is False
    got = _outputs(e)
    assert not (got["job_prob"] == SENT).any() and not (got["mch_prob"] == SENT).any(), "the first decision of the episode ran without its scorers"
    assert_selection_exact(got["job_prob"], job, pair.job_logp, SEED, 10, False, gather_from=env.candidate, gathered=task, mask=env.job_mask, form="k_sample")
    assert_selection_exact(got["mch_prob"], mach, pair.mch_logp, SEED, 11, False, mask=env.mmask, form="k_sample")
    # ... probabilities of THIS state: those of fresh handles on the reset environment and the m_fea1 of the task just selected
    d = dict(tfea=env.tasks_fea, col=env.ell_col, val=env.ell_val, cand=env.candidate, mask=env.job_mask, hm=None, mfea1=env.m_fea1, mfea2=env.m_fea2, mmask=env.mmask)
    st.d = {k: (v.clone() if v is not None else None) for k, v in d.items()}
    monkeypatch.delenv("MTFJSP_NO_FUSED_SELECT")
    _same_as_fresh(got, _reference(st, monkeypatch), "B")
    e.check()


# ---- C: everything a decision arms, before a job forward that fails at its entry
@pytest.mark.parametrize("shape,obs_dtype", [("three", "f32"), ("three", "f64"), ("stream", "f32")])
def test_arms_of_a_failed_job_forward_do_not_fire_in_the_next_pair(shape, obs_dtype, monkeypatch):
    capi = _mods()[2]
    st = State(monkeypatch, shape, obs_dtype, MTFJSP_FUSED_ENV3="1")
    e = st.handle(monkeypatch, fail_at=1)
    _forms(st, e)
    _job(e, st.d)                                                  # (raises the range word)
    before = (e.fused_launches(), st.signature())
    arms = Arms(st, e).everything()
    assert arms.step_armed or shape == "stream"
    _retry(capi, lambda: _job(e, st.d))
    e.set_product_mode(0)
    _as_if_never_armed(st, e, arms, before, monkeypatch, "C")


# ---- D: the machine forward fails at its entry (the word raised by the same pair's job forward)
@pytest.mark.parametrize("shape", ["three", "stream"])
def test_machine_selection_and_step_of_a_failed_machine_forward_do_not_fire_in_the_next_one(shape, monkeypatch):
    capi = _mods()[2]
    st = State(monkeypatch, shape, MTFJSP_FUSED_ENV="1")
    e = st.handle(monkeypatch, fail_at=1)
    _forms(st, e)
    before = (e.fused_launches(), st.signature())
    e.job_prob.fill_(SENT); e.mch_prob.fill_(SENT)
    _job(e, st.d); k0 = e.heads_kernel(0)[0]                       # (raises the range word behind its own poll: a good forward)
    arms = Arms(st, e)
    arms.selection1(); arms.env_step(task=st.task)
    _retry(capi, lambda: _machine(e, st.d))
    arms.assert_intact("D: the failed machine forward")
    e.set_product_mode(0)
    _machine(e, st.d)
    got, kern = _outputs(e), (k0, e.heads_kernel(1)[0])
    arms.assert_intact("D: the plain machine forward after it")     # no index written
    assert not e.env_step_fused() and e.fused_launches() == before[0]
    assert np.array_equal(st.signature(), before[1]), "a stale arm stepped the environment"
    ref = _reference(st, monkeypatch)
    assert kern == ref[2], (kern, ref[2])
    _same_as_fresh(got, ref, "D")
    e.check()


# ---- E: MTFJSP_ERR_STATE (an m_fea1 arm without a selection), other arms beside it
def test_arms_beside_an_mfea1_arm_without_selection_do_not_outlive_the_error(monkeypatch):
    capi = _mods()[2]
    st = State(monkeypatch, "three", MTFJSP_FUSED_ENV3="1")
    e = st.handle(monkeypatch)
    _forms(st, e)
    before = (e.fused_launches(), st.signature())
    arms = Arms(st, e)
    arms.mfea1_redirected(); arms.machine_heads(); arms.selection1(); e.arm_values_only()
    with pytest.raises(capi.MtfjspError) as ex:
        _job(e, st.d)
    assert ex.value.code == capi.ERR_STATE, ex.value
    _as_if_never_armed(st, e, arms, before, monkeypatch, "E")


# ---- F: MTFJSP_ERR_ARG (a null output), everything armed
def test_arms_do_not_outlive_a_job_forward_refused_for_its_arguments(monkeypatch):
    capi = _mods()[2]
    st = State(monkeypatch, "three", MTFJSP_FUSED_ENV3="1")
    e = st.handle(monkeypatch)
    _forms(st, e)
    before = (e.fused_launches(), st.signature())
    arms = Arms(st, e).everything()
    assert arms.step_armed
    d = st.d
    rc = e.L.mtfjsp_job_actor_forward(e.h, d["tfea"].data_ptr(), d["col"].data_ptr(), d["val"].data_ptr(), d["cand"].data_ptr(), d["mask"].data_ptr(),
                                      d["hm"].data_ptr(), None, e.h_pooled_o.data_ptr(), e.job_v.data_ptr(), None)
    assert rc == capi.ERR_ARG
    _as_if_never_armed(st, e, arms, before, monkeypatch, "F")


# ---- G: deferred poll — the failure is reported by check(), no forward returned an error
def test_check_reporting_a_failure_leaves_nothing_armed(monkeypatch):
    capi = _mods()[2]
    st = State(monkeypatch, "three", MTFJSP_FUSED_ENV3="1")
    e = st.handle(monkeypatch, fail_at=1)
    _forms(st, e)
    e.set_deferred_poll(True)
    _job(e, st.d)                                                  # (raises the range word; no forward entry polls it)
    before = (e.fused_launches(), st.signature())
    arms = Arms(st, e).everything()
    assert arms.step_armed
    _retry(capi, e.check)
    e.set_deferred_poll(False)
    e.set_product_mode(0)
    _as_if_never_armed(st, e, arms, before, monkeypatch, "G")


# ---- H: env_step_fused() after a pair that had no armed step
def test_env_step_fused_speaks_of_the_last_pair_only(monkeypatch):
    st = State(monkeypatch, "three", rollout_too=True, MTFJSP_FUSED_ENV3="1")
    ro, env = st.ro, st.env
    pair, e = ro.actor, ro.actor.enc
    assert pair.fuse_env3 and e.check()
    n0 = e.fused_launches()
    assert pair.act(env, ro.nsteps, ro.task, ro.mach, ro.job, env_step=()) is True and e.env_step_fused()     # the step rode in the three-in-one launch
    assert e.fused_launches() == n0 + 1 and e.heads_kernel(0)[0].startswith("k_headsx_gat3x_headsx")
    sig = st.signature()
    assert pair.act(env, ro.nsteps + 1, ro.task, ro.mach, ro.job, env_step=None) is False
    assert e.fused_launches() == n0 + 2, "the second decision did not take the three-in-one launch"
    assert np.array_equal(st.signature(), sig)                     # no step was armed, none ran ...
    assert not e.env_step_fused(), "... and none may be reported"
    e.check()


def test_values_only_count_does_not_outlive_a_pair_served_by_one_launch(monkeypatch):
    """The machine forward that finds itself done by the job forward's three-in-one launch still is the second forward of the pair the values-only
    arm was made for (ignored by both: selections were armed): the pair after it is a full one."""
    st = State(monkeypatch, "three")
    ro, env = st.ro, st.env
    pair, e = ro.actor, ro.actor.enc
    n0 = e.fused_launches()
    e.arm_values_only()
    pair.act(env, ro.nsteps, ro.task, ro.mach, ro.job)
    assert e.fused_launches() == n0 + 1                            # (one launch served both forwards)
    st.inputs()
    got, kern, path = _pair(e, st.d)
    ref = _reference(st, monkeypatch)
    assert (kern, path) == (ref[2], ref[3]) and "k_headsx_values" not in kern, (kern, path, ref[2:])
    _same_as_fresh(got, ref, "values-only after a one-launch pair")
    e.check()
