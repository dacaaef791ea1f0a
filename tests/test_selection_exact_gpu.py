"""GPU: every selecting launch picks what the host model (tests/device_streams_ref.py) picks from the probabilities that same launch
stored — all instances, equality (tests/selection_check.py) — for the standalone sampler on rows built by hand and for every form the
fused selection is launched in, at the first, a middle and the last decision of an episode, and along whole rollouts (which pins the
(seed, counter) schedule).  Only the log-probability has a bound (binary32 ulps, tests/selection_check.py)."""
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


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.encoder"), import_module("e2e-mappo-for-mt-fjsp_amd.rollout"),
            import_module("e2e-mappo-for-mt-fjsp_amd.capi"))


# ---------------------------------------------------------------------------------------------------------------------------------
# standalone k_sample on rows built by hand
def _hand_rows(B, n, rs):
    """-> list of (name, prob [B,n] f32)"""
    out = []
    z = rs.normal(0, 2, (B, n))
    soft = np.exp(z - z.max(1, keepdims=True))
    dead = rs.uniform(size=(B, n)) < 0.3
    dead[np.arange(B), rs.randint(0, n, B)] = False
    soft[dead] = 0.0
    soft = (soft / soft.sum(1, keepdims=True)).astype(np.float32)
    out.append(("softmax rows with masked zeros", soft))
    for name, col in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        one = np.zeros((B, n), np.float32)
        one[:, col] = rs.choice([1.0, 0.37, 2.5], B).astype(np.float32)
        out.append((f"single positive entry in the {name} column", one))
    out.append(("rows scaled by 0.5", (soft * np.float32(0.5)).astype(np.float32)))
    out.append(("rows scaled by 3", (soft * np.float32(3.0)).astype(np.float32)))
    tiny = np.where(rs.uniform(size=(B, n)) < 0.5, np.float32(1e-30), np.float32(0.5)).astype(np.float32)
    tiny[:, rs.randint(0, n)] = 0.5
    out.append(("entries of 1e-30 beside entries of 0.5", tiny))
    zero = soft.copy()
    zero[::3] = 0.0                                                       # every third row all zero (every row for B = 1)
    out.append(("all-zero rows among ordinary ones", zero))
    return out


def _tie_rows(B, n, rs, k):
    """greedy rows whose maximum occurs k times (fewer where n < k)"""
    p = rs.uniform(0.0, 0.5, (B, n)).astype(np.float32)
    for b in range(B):
        cols = rs.choice(n, min(k, n), replace=False)
        p[b, cols] = np.float32(0.75)
    return p


@pytest.mark.parametrize("B", [1, 17, 4096])
@pytest.mark.parametrize("n", [1, 2, 5, 6, 7, 10, 16, 17, 20, 33])
def test_standalone_sampler_on_hand_built_rows(n, B):
    enc_mod, _, _ = _mods()
    enc = enc_mod.Encoder(6, 6, B)
    rs = np.random.RandomState(1000 * n + B)
    idx = torch.full((B,), -7, dtype=torch.int32, device="cuda"); got = torch.full_like(idx, -7)
    logp = torch.zeros(B, device="cuda")
    src = torch.as_tensor(rs.randint(0, 1000, (B, n)).astype(np.int32), device="cuda")
    runs = [(0, 5), (1, (1 << 32) + 5), (1 << 32, 5), ((1 << 40) + 9, (1 << 63) + 11)]          # (counter, seed)
    for name, rows in _hand_rows(B, n, rs):
        p = torch.as_tensor(rows, device="cuda").contiguous()
        # sampling with EVERY (counter, seed) pair — k_sample forms its uniform number itself (pick_action), apart from pick_uniform;
        # greedy reads neither seed nor counter: once
        for greedy, (counter, seed) in [(False, r) for r in runs] + [(True, runs[1])]:
            enc.sample(p, greedy, seed, counter, idx, logp, src, got)
            torch.cuda.synchronize()
            assert_selection_exact(p, idx, logp, seed, counter, greedy, gather_from=src, gathered=got, form="k_sample")
            if name.startswith("all-zero"):                               # the code's answer for a row without a positive entry
                i, lp = idx.cpu().numpy()[::3], logp.cpu().numpy()[::3]
                assert (i == 0).all() and np.isneginf(lp).all(), name
    for ties in (2, 3):
        rows = _tie_rows(B, n, rs, ties)
        p = torch.as_tensor(rows, device="cuda").contiguous()
        enc.sample(p, True, 5, ties, idx, logp, src, got)
        torch.cuda.synchronize()
        assert_selection_exact(p, idx, logp, 5, ties, True, gather_from=src, gathered=got, form="k_sample")
        assert np.array_equal(idx.cpu().numpy(), np.argmax(rows, 1)), "greedy: the first of equal maxima wins"
    # every word of seed and counter reaches the draw
    p = torch.as_tensor(_hand_rows(max(B, 64), n, rs)[0][1][:B], device="cuda").contiguous()
    if n >= 5 and B >= 17:
        picks = []
        for counter, seed in ((3, 9), (3 + (1 << 32), 9), (3, 9 + (1 << 32)), (4, 9), (3, 10)):
            enc.sample(p, False, seed, counter, idx)
            picks.append(idx.cpu().numpy().copy())
        assert all(not np.array_equal(picks[0], x) for x in picks[1:])
    enc.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# fused selection: which kernel a decision's two heads launches are.  The library reports it — the kernel, its group size and its grid per forward
# (Encoder.heads_kernel), three-in-one or not (fused_launches()), the environment step inside the launch (act's return value), the heads family
# of each launch (timing families heads / heads_gat3 / heads_gat3_heads) and the product mode — and states its rule without a handle
# (capi.heads_kernel_for, csrc/mtfjsp_heads_select.h).  _asks is what ActorPair.act arms under a case's switches and modes: the rule's input.
def _asks(env, mode, stepping):
    """-> (job, machine): keyword arguments of capi.heads_kernel_for for the two forwards of one decision"""
    handle = dict(f32=mode.get("product") == 15, gat_ok=not mode.get("bn") and not mode.get("product"), mheads_ok=not env.get("MTFJSP_NO_FUSED_MHEADS"))
    mheads = not (env.get("MTFJSP_FUSED_ENV") and stepping)
    job = dict(handle, gat=True, mheads=mheads, env_tail=bool(mheads and env.get("MTFJSP_FUSED_ENV3") and stepping))
    return job, dict(handle, which=1, env_tail=bool(env.get("MTFJSP_FUSED_ENV") and stepping))


def _kernel_of(form):
    return "k_headsx_gat3x_headsx" if form.startswith("three_in_one") else form


def _rule(capi, J, M, B, num_cu, env, mode, stepping):
    """-> ((job kernel, group, grid), (machine ...)) by the handle-free rule; a machine forward the job launch ran is that launch"""
    job, mach = _asks(env, mode, stepping)
    kj = capi.heads_kernel_for(B, J, M, num_cu=num_cu, **job)
    return kj, (kj if kj[0].startswith("k_headsx_gat3x_headsx") else capi.heads_kernel_for(B, J, M, num_cu=num_cu, **mach))


HG16, NO10, BOTH = {"MTFJSP_NO_HEADS_HG8": "1"}, {"MTFJSP_NO_HEADS10": "1"}, {"MTFJSP_NO_HEADS_HG8": "1", "MTFJSP_NO_HEADS10": "1"}
NO3 = {"MTFJSP_NO_FUSED_MHEADS": "1"}
X, X10 = "k_headsx", "k_headsx10"
CASES = [
    # (J, M, E, B), environment switches, mode, the (job, machine) heads launches this must be on a 256-CU device
    ((6, 6, 2, 4096), {}, {}, ("three_in_one", "three_in_one")),
    ((4, 8, 2, 4096), {}, {}, ("three_in_one", "three_in_one")),
    ((7, 5, 1, 4096), {}, {}, ("three_in_one", "three_in_one")),
    ((6, 6, 2, 4096), NO3, {}, ("k_headsx_gat3x", X)),
    ((6, 6, 2, 333), NO3, {}, (X, X)),                  # (333 instances are no whole groups of 16: no GAT passes in the job launch ...
    ((6, 4, 2, 336), NO3, {}, ("k_headsx_gat3x", X)),   #  ... this batch of about that size takes them)
    ((6, 6, 2, 333), {}, {}, (X, X)), ((6, 6, 2, 333), HG16, {}, (X, X)),
    ((3, 4, 2, 7), {}, {}, (X, X)), ((3, 4, 2, 7), HG16, {}, (X, X)),
    ((13, 5, 1, 2), {}, {}, (X10, X)), ((13, 5, 1, 2), HG16, {}, (X, X)),
    ((10, 10, 2, 96), {}, {}, (X, X)), ((10, 10, 2, 96), HG16, {}, (X10, X10)), ((10, 10, 2, 96), BOTH, {}, (X, X)),
    ((10, 6, 2, 37), {}, {}, (X, X)), ((10, 6, 2, 37), HG16, {}, (X10, X)), ((10, 6, 2, 37), BOTH, {}, (X, X)),
    ((8, 4, 2, 53), {}, {}, (X, X)), ((8, 4, 2, 53), HG16, {}, (X10, X)), ((8, 4, 2, 53), BOTH, {}, (X, X)),
    ((16, 4, 2, 19), {}, {}, (X10, X)), ((4, 16, 2, 19), {}, {}, (X, X10)), ((17, 4, 1, 5), {}, {}, (X10, X)), ((20, 20, 4, 9), {}, {}, (X10, X10)),
    ((16, 4, 2, 19), NO10, {}, (X, X)), ((17, 4, 1, 5), NO10, {}, (X, X)), ((20, 20, 4, 9), NO10, {}, (X, X)),
    ((6, 6, 2, 333), {}, {"product": 15}, ("k_heads", "k_heads")), ((20, 20, 4, 9), {}, {"product": 15}, ("k_heads", "k_heads")),
    ((6, 6, 2, 4096), {"MTFJSP_FUSED_ENV": "1"}, {}, ("k_headsx_gat3x", "k_headsx_envstep")),
    ((6, 6, 2, 4096), {"MTFJSP_FUSED_ENV3": "1"}, {}, ("three_in_one_env", "three_in_one_env")),
    ((6, 6, 2, 100), {}, {"bn": True}, (X, X)), ((10, 10, 2, 24), {}, {"bn": True}, (X, X)),
]
FAMILY = {"three_in_one": "heads_gat3_heads", "three_in_one_env": "heads_gat3_heads", "k_headsx_gat3x": "heads_gat3"}


def _case_id(c):
    (J, M, E, B), env, mode, _ = c
    sw = "+".join(k.replace("MTFJSP_", "") for k in env) or "default"
    return f"J{J}M{M}E{E}x{B}-{sw}" + ("-f32" if mode.get("product") else "") + ("-bn" if mode.get("bn") else "")


def _check_decision(ro, forms, greedy, stepping, last, capi, rule):
    """one ActorPair.act at the rollout's current state (with the environment step only where the form carries it) and everything it
    wrote checked; -> True when the environment took the step inside the launch"""
    env, act, e = ro.env, ro.actor, ro.actor.enc
    cand, jmask = env.candidate.clone(), env.job_mask.clone()
    n, have_hm, was_greedy = ro.nsteps, act.have_hm, act.greedy
    act.greedy = greedy
    n3 = e.fused_launches()
    if not stepping:
        e.timing_begin()
    stepped = act.act(env, n, ro.task, ro.mach, ro.job, env_step=() if stepping else None)
    torch.cuda.synchronize()
    fams = {} if stepping else e.timing_end()
    act.greedy = was_greedy
    three = forms[0].startswith("three_in_one")
    assert e.fused_launches() - n3 == (1 if three else 0), "three-in-one launch " + ("did not run" if three else "ran")
    for which in (0, 1):
        name, group, grid = e.heads_kernel(which)
        want = _kernel_of(forms[which])
        assert name is not None and (name.startswith(want) if three else name == want), f"forward {which} ran {name}, expected {want}"
        assert (group, grid) == rule[which][1:], f"forward {which}: groups of {group} in {grid} workgroups, the rule says {rule[which][1:]}"
    assert bool(stepped) == stepping, "the environment step did not ride in the heads launch"
    if not stepping:
        want = {}
        for f in forms[:1] if three else forms:
            k = FAMILY.get(f, "heads")
            want[k] = want.get(k, 0) + 1
        got = {k: fams.get(k, {}).get("launches", 0) for k in ("heads", "heads_gat3", "heads_gat3_heads")}
        assert got == {k: want.get(k, 0) for k in got}, f"heads launches {got}, expected {want}"
        assert ("sample" not in fams), "the selection must be the fused one"
    assert_selection_exact(e.job_prob, ro.job, act.job_logp, act.seed, 2 * n, greedy, gather_from=cand, gathered=ro.task, mask=jmask, form=forms[0])
    mf1, mm = env.m_fea1.clone(), env.mmask.clone()
    env.observe_mfea1(ro.task)
    torch.cuda.synchronize()
    assert torch.equal(mf1, env.m_fea1) and torch.equal(mm, env.mmask), "m_fea1 / machine mask of the selected task"
    assert_selection_exact(e.mch_prob, ro.mach, act.mch_logp, act.seed, 2 * n + 1, greedy, mask=mm, form=forms[1])
    if last:
        free = jmask.cpu().numpy() == 0
        assert (free.sum(1) == 1).all(), "the last decision has one job left"
        assert np.array_equal(ro.job.cpu().numpy(), np.argmax(free, 1)), "every instance must pick its last job"
    if stepped:                                                           # what Rollout._step does after a decision
        ro.nsteps += 1
        ro.t_in_ep += 1
    else:
        act.have_hm = have_hm                                             # the decision is taken again by ro.step()
    return stepped


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fused_selection_of_every_launch_form(case, monkeypatch):
    (J, M, E, B), env_sw, mode, forms = case
    for k, v in env_sw.items():
        monkeypatch.setenv(k, v)
    enc_mod, rollout, capi = _mods()
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    stepping = forms[1] in ("k_headsx_envstep", "three_in_one_env")
    rule = _rule(capi, J, M, B, num_cu, env_sw, mode, stepping)
    routed = tuple(r[0] for r in rule)
    assert all(r.startswith(_kernel_of(f)) if f.startswith("three_in_one") else r == f for r, f in zip(routed, forms)), \
        f"on {num_cu} CUs this shape is routed to {routed}: choose another shape"
    T = J * M
    only_greedy = bool(mode.get("bn"))
    ro = rollout.Rollout(J, M, E, B, policy="actor", obs_dtype="f32", weights=enc_mod.random_init_weights(seed=J * 100 + M), collect=False,
                         seed=(1 << 32) + 77, greedy=only_greedy)
    e = ro.actor.enc
    if mode.get("product"):
        e.set_product_mode(mode["product"])
    if mode.get("bn"):
        e.set_bn_mode(True)
    if forms[0].startswith("three_in_one"):
        assert e.check(), "the three-in-one launch needs the single-launch GIN kernel's census"
    if mode.get("product"):
        assert e.range_fallbacks()[1] == mode["product"]
    # an episode's first decision (the learned `_input` in place of the machine embedding), as Rollout._step begins an episode
    ro.env.scaler_reset_returns(); ro.env.reset(ro._episode_w3()); ro.actor.begin_episode()
    flags = torch.zeros(B, dtype=torch.int32, device="cuda")

    def advance_to(t):
        while ro.t_in_ep < t:
            ro.step()                                                     # (its first call repeats the reset above: the same episode, the same weights)
            flags.bitwise_or_(ro.env.status)

    if stepping:
        # the step rides in the launch: a decision is taken once, so sampling and greedy alternate over neighbouring decisions
        plan = [(0, False), (1, True), (T // 2, False), (T // 2 + 1, True), (T - 2, True), (T - 1, False)]
    else:
        plan = [(t, g) for t in (0, T // 2, T - 1) for g in ((True,) if only_greedy else (False, True))]
    for t, greedy in plan:
        advance_to(t)
        assert ro.t_in_ep == t and ro.nsteps == t
        _check_decision(ro, forms, greedy, stepping, t == T - 1, capi, rule)
        flags.bitwise_or_(ro.env.status)
    assert int((flags & capi.ST_INVALID).ne(0).sum().item()) == 0
    e.check()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,M,E,B,rank", [(6, 6, 2, 4096, 0), (10, 10, 2, 333, 1)])
def test_whole_rollout_selects_exactly_and_keeps_its_counter_schedule(J, M, E, B, rank):
    """two full episodes plus three steps of Rollout(policy="actor", collect=False): both actors' selections after every step, with
    counter 2 n / 2 n + 1 for the n-th step of the RUN (continuing across the episode boundary) and seed + rank"""
    enc_mod, rollout, capi = _mods()
    T = J * M
    seed = (1 << 32) + 1234
    ro = rollout.Rollout(J, M, E, B, policy="actor", obs_dtype="f32", weights=enc_mod.random_init_weights(seed=3), collect=False,
                         seed=seed, rank=rank, world=rank + 1)
    env, act, e = ro.env, ro.actor, ro.actor.enc
    three = (J, M, B) == (6, 6, 4096)
    assert act.seed == seed + rank
    used = []
    flags = torch.zeros(B, dtype=torch.int32, device="cuda")
    for n in range(2 * T + 3):
        first = ro.t_in_ep == 0                                           # the reset of this step happens inside ro.step()
        cand, jmask = env.candidate.clone(), env.job_mask.clone()
        assert ro.nsteps == n
        ro.step()
        torch.cuda.synchronize()
        flags |= env.status
        form = "three_in_one" if three else "k_headsx"
        if first:
            # what the decision saw is what a reset leaves — every job's first operation, no job masked — and the step moved only the
            # selected job's entry: checked on the state after the step, then used as the gather source and the mask
            cand = (torch.arange(J, dtype=torch.int32, device="cuda") * M).repeat(B, 1)
            jmask = torch.zeros(B, J, dtype=torch.uint8, device="cuda")
            moved = env.candidate != cand
            assert bool((moved.sum(1) <= 1).all().item()) and bool((moved.long().argmax(1)[moved.any(1)] == ro.job[moved.any(1)]).all().item())
            assert not bool(((env.job_mask != 0) & ~moved).any().item()), "only the selected job's mask byte may be set after one step"
        assert_selection_exact(e.job_prob, ro.job, act.job_logp, seed + rank, 2 * n, False, gather_from=cand, gathered=ro.task, mask=jmask, form=form)
        assert_selection_exact(e.mch_prob, ro.mach, act.mch_logp, seed + rank, 2 * n + 1, False, mask=env.mmask, form=form)
        used += [(seed + rank, 2 * n), (seed + rank, 2 * n + 1)]
    assert len(set(used)) == len(used) == 2 * (2 * T + 3) and ro.episode == 2 and ro.t_in_ep == 3
    assert e.fused_launches() == (2 * T + 3 if three else 0)
    assert int((flags & capi.ST_INVALID).ne(0).sum().item()) == 0
    ro.check_finished_cleanly()
