"""GPU: the device's beam search (mtfjsp_lookahead_expand / the ordinary step / mtfjsp_state_signature / mtfjsp_beam_select /
mtfjsp_fork / mtfjsp_beam_backtrack, baselines.BeamSearch and beam_baselines) EQUALS the host model of tests/beam_ref.py — parent,
source slot, task, machine and the score's bits on every slot at every step of the episode; no tolerance anywhere.  The shapes are
the smallest that reach each path of the selection: fewer candidates than a wave, a ragged second pass, more slots than children
(empty ranks), more than one pass per wave, T > 64, and tie-rich data on which merging duplicates changes the survivors."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import beam_ref as ref
from env_parity import _same

pytestmark = pytest.mark.gpu

# name: (J, M, E, N, W, tie-rich data, left shift)
CASES = {
    "J3M3_W1": (3, 3, 3, 5, 1, False, True),            # degenerate: the look-ahead with a running score
    "J3M3_W3": (3, 3, 3, 5, 3, False, True),            # 27 candidates: less than a wave
    "J3M3_W8": (3, 3, 3, 5, 8, False, True),            # 72 candidates: a ragged second wave
    "J3M3_W16": (3, 3, 3, 5, 16, False, True),          # more slots than children for the first steps: empty ranks
    "J6M6_W4": (6, 6, 2, 3, 4, False, True),            # 144 candidates
    "J9M8_W2": (9, 8, 2, 2, 2, False, True),            # T > 64
    "J6M6_W8": (6, 6, 2, 3, 8, False, True),            # 288 candidates: a wave's second pass
    "ties_J3M3_W4": (3, 3, 3, 5, 4, True, False),       # where merging changes the survivors
    "J6M6_W4_no_left_shift": (6, 6, 2, 3, 4, False, False),
}
ALL_COLUMNS = "J6M6_W4_no_left_shift"


def _mods():
    import mtfjsp_amd  # noqa: F401
    return (import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.baselines"),
            import_module("e2e-mappo-for-mt-fjsp_amd.capi"))


def _env(batch_env, data, J, M, E, left_shift, obs_dtype="f32"):
    t, p, tt, edge, w3 = data
    env = batch_env.DeviceBatchEnv(J, M, E, t.shape[0], left_shift=left_shift, obs_dtype=obs_dtype, w_cfg=ref.CONFIG_W)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(w3)
    return env


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _check_row(bs, s, rec, tag):
    for k in ("parent", "from_slot", "task", "mach"):
        _same(bs.hist[k][s].cpu().numpy(), rec[k], f"{tag} {k}")
    _same(_bits(bs.score.cpu().numpy()), _bits(rec["score"]), f"{tag} score (bits)")


def _episode(case, column, dedupe):
    batch_env, baselines, capi = _mods()
    J, M, E, N, W, ties, left_shift = CASES[case]
    data, recs = ref.cached_episode(J, M, E, N, W, column, dedupe, left_shift, ties)
    env = _env(batch_env, data, J, M, E, left_shift)
    bs = baselines.BeamSearch(env, W, dedupe=dedupe)
    return env, bs, data, recs


# every shape with and without merging on columns 0 and 2; one shape runs all five columns
EPISODES = [(case, column, dedupe) for case in CASES for column in range(5) for dedupe in (True, False)
            if column in (0, 2) or (case == ALL_COLUMNS and dedupe)]


@pytest.mark.parametrize("case,column,dedupe", EPISODES, ids=[f"{c}-column{k}-{'dedupe' if d else 'plain'}" for c, k, d in EPISODES])
def test_every_step_of_the_episode_equals_the_model(case, column, dedupe):
    J, M = CASES[case][:2]
    env, bs, data, recs = _episode(case, column, dedupe)
    for s in range(J * M):
        assert bs.advance(column) == s
        _check_row(bs, s, recs[s], f"{case} column {column} step {s}")
    if "W16" in case:
        assert (recs[0]["parent"] < 0).any(), "this case has empty ranks"
    bs.close(); env.close()


def test_merging_changes_the_survivors_on_the_tie_rich_data():
    """the model's two episodes differ (so the case above compares the device on both sides of the difference), and the device's
    merged beam never holds one signature twice"""
    case = "ties_J3M3_W4"
    J, M, E, N, W, ties, left_shift = CASES[case]
    _, plain = ref.cached_episode(J, M, E, N, W, 2, False, left_shift, ties)
    env, bs, data, merged = _episode(case, 2, True)
    assert any(not np.array_equal(a["parent"], b["parent"]) for a, b in zip(plain, merged))
    for s in range(J * M):
        bs.advance(2)
        sig = bs.beam.state_signature().cpu().numpy().reshape(N, W)
        live = np.isfinite(bs.score.cpu().numpy()).reshape(N, W)
        for n in range(N):
            assert len(set(sig[n][live[n]])) == live[n].sum(), f"step {s} instance {n}: two slots with one signature"
    bs.close(); env.close()


@pytest.mark.parametrize("column", [0, 2])
def test_a_finished_instance_beside_running_ones_keeps_its_beam(column):
    batch_env, baselines, capi = _mods()
    J, M, E, N, W, _, left_shift = CASES["J3M3_W3"]
    T = J * M
    data, recs = ref.cached_episode(J, M, E, N, W, column, True, left_shift, False)
    task, mach = ref.plan_arrays(recs[-1]["prefixes"], T)
    env = _env(batch_env, data, J, M, E, left_shift, "f64")
    # instance 2 alone plays the model's best plan to the end: the others get task -1, which the step rejects and leaves untouched
    only = np.arange(N) == 2
    for s in range(T):
        a = torch.as_tensor(np.where(only, task[::W, s], -1).astype(np.int32), device=env.device)
        m = torch.as_tensor(np.where(only, mach[::W, s], 0).astype(np.int32), device=env.device)
        env.step(a, m)
    assert env.info.cpu().numpy()[2, 1] == 1.0
    bs = baselines.BeamSearch(env, W)
    before = bs.score.cpu().numpy().copy()
    bs.advance(column)
    got = {k: bs.hist[k][0].cpu().numpy().reshape(N, W) for k in bs.hist}
    score = bs.score.cpu().numpy().reshape(N, W)
    assert (got["parent"][2] == -1).all() and (got["task"][2] == -1).all() and (got["mach"][2] == -1).all()
    _same(got["from_slot"][2], np.arange(W, dtype=np.int32), "finished: every slot stays where it is")
    _same(_bits(score[2]), _bits(before.reshape(N, W)[2]), "finished: scores unchanged")
    rec = recs[0]
    for k in ("parent", "from_slot", "task", "mach"):
        _same(got[k][~only], rec[k].reshape(N, W)[~only], f"running instances: {k}")
    _same(_bits(score[~only]), _bits(rec["score"].reshape(N, W)[~only]), "running instances: score (bits)")
    bs.close(); env.close()


def test_plans_of_empty_slots_are_minus_one():
    """two decisions at W = 16 on J3M3: the first leaves ranks empty, the second fills them from fewer parents"""
    case, column = "J3M3_W16", 2
    J, M, E, N, W, ties, left_shift = CASES[case]
    env, bs, data, recs = _episode(case, column, True)
    for steps in (1, 2):
        bs.advance(column)
        want_t, want_m = ref.plan_arrays(recs[steps - 1]["prefixes"], steps)
        if steps == 1:
            assert (want_t == -1).any() and (want_t[::W] >= 0).all(), "the first decision leaves empty ranks, never rank 0"
        for k in range(W):
            tk, mk = bs.plans(np.full(N, k, np.int32))
            _same(tk.cpu().numpy(), want_t[k::W], f"{steps} step(s), slot {k}: tasks"); _same(mk.cpu().numpy(), want_m[k::W], f"{steps} step(s), slot {k}: machines")
    # a start slot outside the beam reads as an empty one
    tk, mk = bs.plans(np.array([-1, W, 0, 1, W + 7], np.int32))
    assert (tk.cpu().numpy()[[0, 1, 4]] == -1).all() and (mk.cpu().numpy()[[0, 1, 4]] == -1).all() and (tk.cpu().numpy()[[2, 3]] >= 0).all()
    bs.close(); env.close()


@pytest.mark.parametrize("case", ["J3M3_W16", "J6M6_W4", "ties_J3M3_W4"])
def test_run_reads_out_the_models_plans_and_the_best_one_replays_to_its_score(case):
    batch_env, baselines, capi = _mods()
    J, M, E, N, W, ties, left_shift = CASES[case]
    T, column = J * M, 2
    env, bs, data, recs = _episode(case, column, True)
    task0, mach0, score = bs.run(column)
    want_t, want_m = ref.plan_arrays(recs[-1]["prefixes"], T)
    _same(_bits(score.cpu().numpy().reshape(-1)), _bits(recs[-1]["score"]), "final scores (bits)")
    for k in range(W):
        tk, mk = bs.plans(np.full(N, k, np.int32))
        _same(tk.cpu().numpy(), want_t[k::W], f"slot {k}: tasks"); _same(mk.cpu().numpy(), want_m[k::W], f"slot {k}: machines")
    _same(task0.cpu().numpy(), want_t[0::W], "run: tasks of the best slot"); _same(mach0.cpu().numpy(), want_m[0::W], "run: machines of the best slot")
    plain = _env(batch_env, data, J, M, E, left_shift)
    total = np.zeros(N)
    ts, ms = task0.t().contiguous(), mach0.t().contiguous()
    for s in range(T):
        plain.step(ts[s], ms[s])
        assert not (plain.status.cpu().numpy() & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any(), f"step {s}"
        total = total + plain.raw.cpu().numpy()[:, column]
    assert bool(plain.info[:, 1].all().item())
    _same(_bits(total), _bits(score.cpu().numpy()[:, 0]), "the replayed plan's running sum is the beam's score (bits)")
    plain.close(); bs.close(); env.close()


def test_beam_baselines_equal_the_oracle_driven_by_the_models_plans():
    from oracle.env_oracle import OracleBatch
    _, baselines, _ = _mods()
    J, M, E, N, W, _, left_shift = CASES[ALL_COLUMNS]
    T = J * M
    assert baselines.BEAM_RULES == [("BS_IT", 2), ("BS_TT", 4), ("BS_MK", 1), ("BS_EC", 3), ("BS_R", 0)]
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=ref.CONFIG_W[0], weight_ec=ref.CONFIG_W[1], weight_tt=ref.CONFIG_W[2])
    t, p, tt, edge, w3 = ref.cached_data(J, M, E, N)
    res = baselines.beam_baselines(t, p, tt, edge, args, width=W)
    one = baselines.beam_baselines(t, p, tt, edge, args, width=W, chunk=1)
    assert sorted(res) == sorted([r[0] for r in baselines.BEAM_RULES] + [baselines.PLANS]) == sorted(one)
    for name, column in baselines.BEAM_RULES:
        _, recs = ref.cached_episode(J, M, E, N, W, column, True, left_shift, False)
        task, mach = ref.plan_arrays(recs[-1]["prefixes"], T)
        task, mach = np.ascontiguousarray(task[::W]), np.ascontiguousarray(mach[::W])
        _same(res[baselines.PLANS][name][0], task, f"{name} plan: tasks"); _same(res[baselines.PLANS][name][1], mach, f"{name} plan: machines")
        orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(w3)
        cum = np.zeros((N, 5))
        for s in range(T):
            cum += orc.step(task[:, s], mach[:, s])[1]
        prev = orc.state()["prev"]
        cost, final4, obj = res[name]
        for k, key in enumerate(("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")):
            _same(cost[key], cum[:, k], f"{name} {key}")
            _same(one[name][0][key], cost[key], f"{name} {key}: chunk=1")
        want4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
        _same(final4, want4, f"{name} Final_4cost")
        w = ref.CONFIG_W
        _same(obj, w[0] * want4[:, 0] + w[1] * (want4[:, 1] + want4[:, 3]) + w[2] * want4[:, 2], f"{name} Objective")
        _same(one[name][1], final4, f"{name} Final_4cost: chunk=1"); _same(one[name][2], obj, f"{name} Objective: chunk=1")
        _same(one[baselines.PLANS][name][0], task, f"{name} plan: tasks, chunk=1"); _same(one[baselines.PLANS][name][1], mach, f"{name} plan: machines, chunk=1")


def test_beam_and_scratch_handles_inherit_reward_weights_off_the_default():
    """BS_R (raw[0], the weighted total) at W = 2 with the configuration's weights at (0.55, 0.15, 0.30), divisor 1 (the host model
    takes none), on the smallest shape of this file: the children are stepped by the scratch handle and the winners live in the beam
    handle, which must both have taken their source's weights (baselines.BeamSearch)"""
    from oracle.env_oracle import OracleBatch
    _, baselines, _ = _mods()
    J, M, E, N = CASES["J3M3_W3"][:4]
    T, W, W_A, left_shift = J * M, 2, (0.55, 0.15, 0.30), True
    assert min(v[0] * v[1] for v in CASES.values()) == T
    args = dict(n_job=J, n_machine=M, n_edge=E, weight_mk=W_A[0], weight_ec=W_A[1], weight_tt=W_A[2])
    (t, p, tt, edge, w3), recs = ref.cached_episode(J, M, E, N, W, 0, True, left_shift, False, W_A)
    _same(w3, np.tile(np.array([W_A]), (N, 1)), "the model's weights")
    _, default = ref.cached_episode(J, M, E, N, W, 0, True, left_shift, False)
    assert not np.array_equal(_bits(default[-1]["score"]), _bits(recs[-1]["score"])), "the weights must change the model's scores"
    res = baselines.beam_baselines(t, p, tt, edge, args, rules=[("BS_R", 0)], width=W, left_shift=left_shift)
    task, mach = ref.plan_arrays(recs[-1]["prefixes"], T)
    task, mach = np.ascontiguousarray(task[::W]), np.ascontiguousarray(mach[::W])
    _same(res[baselines.PLANS]["BS_R"][0], task, "BS_R plan: tasks"); _same(res[baselines.PLANS]["BS_R"][1], mach, "BS_R plan: machines")
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=W_A); orc.scaler_init(); orc.reset(w3)
    cum, total = np.zeros((N, 5)), np.zeros(N)
    for s in range(T):
        raw = orc.step(task[:, s], mach[:, s])[1]
        cum += raw
        total = total + raw[:, 0]
    _same(_bits(total), _bits(recs[-1]["score"][::W]), "the best plan's running sum is the model's best score (bits)")
    prev = orc.state()["prev"]
    cost, final4, obj = res["BS_R"]
    for k, key in enumerate(("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")):
        _same(cost[key], cum[:, k], f"BS_R {key}")
    want4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
    _same(final4, want4, "BS_R Final_4cost")
    _same(obj, W_A[0] * want4[:, 0] + W_A[1] * (want4[:, 1] + want4[:, 3]) + W_A[2] * want4[:, 2], "BS_R Objective")
    # the device's own scores, every slot at every step, through the class the baseline drives
    batch_env = _mods()[0]
    env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=left_shift, obs_dtype="f32", w_cfg=W_A)
    env.load_instances(t, p, tt, edge=edge); env.scaler_init(); env.reset(w3)
    bs = baselines.BeamSearch(env, W)
    assert bs.beam.w_cfg == W_A and bs.scratch.w_cfg == W_A
    for s in range(T):
        assert bs.advance(0) == s
        _check_row(bs, s, recs[s], f"weights {W_A} step {s}")
    bs.close(); env.close()


def test_argument_errors_write_nothing():
    batch_env, baselines, capi = _mods()
    J, M, E, N, W, _, left_shift = CASES["J3M3_W3"]
    T = J * M
    data = ref.cached_data(J, M, E, N)
    env = _env(batch_env, data, J, M, E, left_shift)
    bs = baselines.BeamSearch(env, W)
    bs.advance(2)                                                       # both handles hold a state; a valid call is possible
    dev, NW, L = env.device, N * W, env.L
    ints = [torch.full((NW,), -77, dtype=torch.int32, device=dev) for _ in range(4)]
    out = torch.full((NW,), float("nan"), dtype=torch.float64, device=dev)
    score = bs.score

    def call(scratch, beam, width, column, score_out):
        return L.mtfjsp_beam_select(scratch.h, beam.h, width, column, score.data_ptr(), C.c_void_p(None), *[x.data_ptr() for x in ints], score_out.data_ptr())

    other = batch_env.DeviceBatchEnv(J, M, E, NW * T + 1, left_shift=left_shift, obs_dtype="f32", w_cfg=ref.CONFIG_W)
    before = score.cpu().numpy().copy()
    assert call(bs.scratch, bs.beam, 0, 2, out) == capi.ERR_ARG
    assert call(bs.scratch, bs.beam, 65, 2, out) == capi.ERR_ARG
    assert call(bs.scratch, bs.beam, 2, 2, out) == capi.ERR_ARG         # 15 slots are no multiple of 2
    assert call(other, bs.beam, W, 2, out) == capi.ERR_ARG              # scratch batch != beam batch * T
    assert b"batch" in L.mtfjsp_last_error(other.h)
    assert call(bs.scratch, bs.beam, W, 5, out) == capi.ERR_ARG
    assert call(bs.scratch, bs.beam, W, -1, out) == capi.ERR_ARG
    assert call(bs.scratch, bs.beam, W, 2, score) == capi.ERR_ARG       # score_out == score_in
    assert b"score_out" in L.mtfjsp_last_error(bs.scratch.h)
    # W * T > 8192: J13M10 (T = 130) at W = 64
    big_beam = batch_env.DeviceBatchEnv(13, 10, 2, 64, left_shift=left_shift, obs_dtype="f32", w_cfg=ref.CONFIG_W)
    big_scratch = batch_env.DeviceBatchEnv(13, 10, 2, 64 * 130, left_shift=left_shift, obs_dtype="f32", w_cfg=ref.CONFIG_W)
    ints64 = [torch.full((64,), -77, dtype=torch.int32, device=dev) for _ in range(4)]
    in64 = torch.zeros(64, dtype=torch.float64, device=dev)
    out64 = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    assert L.mtfjsp_beam_select(big_scratch.h, big_beam.h, 64, 2, in64.data_ptr(), C.c_void_p(None), *[x.data_ptr() for x in ints64], out64.data_ptr()) == capi.ERR_ARG
    assert b"8192" in L.mtfjsp_last_error(big_scratch.h)
    with pytest.raises(ValueError):
        baselines.BeamSearch(env, 65)
    torch.cuda.synchronize()
    for x in ints + ints64:
        assert (x.cpu().numpy() == -77).all()
    assert np.isnan(out.cpu().numpy()).all() and np.isnan(out64.cpu().numpy()).all()
    _same(_bits(score.cpu().numpy()), _bits(before), "the input scores")
    # and the same buffers take a valid call
    assert call(bs.scratch, bs.beam, W, 2, out) == capi.OK
    torch.cuda.synchronize()
    assert not np.isnan(out.cpu().numpy()).any() and (ints[0].cpu().numpy() != -77).all()
    for e in (other, big_beam, big_scratch):
        e.close()
    bs.close(); env.close()


@pytest.mark.parametrize("with_sig", [True, False], ids=["dedupe", "plain"])
def test_selection_at_the_size_limit_on_synthetic_children(with_sig):
    """J13M10 at W = 63: 8 190 candidates per instance, 128 KB of (value, signature) pairs in LDS — no episode's model is affordable
    there, so the children are synthetic: status words, raw rewards (few distinct values: ties; NaN and -inf among them), signatures
    (few distinct: many duplicates) and parent scores (some slots empty) are written straight into the scratch handle's bound
    buffers, and the selection rule of tests/beam_ref.py is applied to the same arrays.  A third instance has its maximum at zeros
    of both signs: a score is its own candidate's sum, bit for bit, never the other zero"""
    batch_env, baselines, capi = _mods()
    J, M, E, N, W, column = 13, 10, 2, 3, 63, 3
    T = J * M
    mk = lambda b: batch_env.DeviceBatchEnv(J, M, E, b, left_shift=False, obs_dtype="f32", w_cfg=ref.CONFIG_W)      # noqa: E731
    beam, scratch = mk(N * W), mk(N * W * T)
    for e in (beam, scratch):
        e.generate_instances(3); e.scaler_init()
        e.reset(torch.tensor([ref.CONFIG_W], dtype=torch.float64, device=e.device).repeat(e.B, 1))
    rng = np.random.RandomState(8)
    R2 = 2 * W * T                                                      # instances 0 and 1
    raw = rng.randint(-6, 7, (R2, 5)).astype(np.float64) * 0.375
    raw[rng.rand(R2) < 0.01, column] = np.nan
    raw[rng.rand(R2) < 0.01, column] = -np.inf
    status = np.where(rng.rand(R2) < 0.3, capi.ST_INVALID, 0) | np.where(rng.rand(R2) < 0.2, capi.ST_INFEASIBLE, 0) | rng.randint(0, 8, R2)
    score = rng.randint(-4, 5, 2 * W).astype(np.float64) * 0.75
    score[rng.rand(2 * W) < 0.25] = -np.inf
    score[W:W + 40] = -np.inf                                           # instance 1: few live slots ...
    sig = rng.randint(0, 2 if with_sig else 1 << 30, R2).astype(np.uint64)
    sig[W * T:] = rng.randint(0, 40, R2 - W * T)                         # ... and 40 signatures: ranks run out
    # instance 2: nothing above zero, and the zeros carry both signs — the top ranks are ties between -0.0 and +0.0, taken in index
    # order, and every rank's score is its own candidate's sum (-0.0 only from -0.0 + -0.0).  Signatures all differ: every rank is filled
    rng = np.random.RandomState(9)
    raw2 = -np.abs(rng.randint(-6, 7, (W * T, 5)).astype(np.float64)) * 0.375
    score2 = -np.abs(rng.randint(-4, 5, W).astype(np.float64)) * 0.75
    raw2[raw2 == 0] = np.where(rng.rand((raw2 == 0).sum()) < 0.5, -0.0, 0.0)
    score2[score2 == 0] = np.where(rng.rand((score2 == 0).sum()) < 0.5, -0.0, 0.0)
    status2 = np.where(rng.rand(W * T) < 0.3, capi.ST_INVALID, 0) | np.where(rng.rand(W * T) < 0.2, capi.ST_INFEASIBLE, 0) | rng.randint(0, 8, W * T)
    score2[0], raw2[7, column], status2[7] = -0.0, -0.0, 0              # the lowest index of the maximum: -0.0 + -0.0
    score2[W - 1], raw2[(W - 1) * T + 70, column], status2[(W - 1) * T + 70] = -0.0, 0.0, 0     # tied with it, from a later pass of another wave: +0.0
    raw2[:7, column] = -0.375
    raw, status, score = np.concatenate([raw, raw2]), np.concatenate([status, status2]), np.concatenate([score, score2])
    sig = np.concatenate([sig, rng.permutation(W * T).astype(np.uint64)])
    R = N * W * T
    dev = beam.device
    scratch.raw.copy_(torch.as_tensor(raw, device=dev)); scratch.status.copy_(torch.as_tensor(status.astype(np.int32), device=dev))
    d_score = torch.as_tensor(score, device=dev)
    d_sig = torch.as_tensor(sig.view(np.int64), device=dev)
    ints = [torch.full((N * W,), -77, dtype=torch.int32, device=dev) for _ in range(4)]
    out = torch.full((N * W,), float("nan"), dtype=torch.float64, device=dev)
    capi.check(beam.L.mtfjsp_beam_select(scratch.h, beam.h, W, column, d_score.data_ptr(), C.c_void_p(d_sig.data_ptr() if with_sig else None),
                                         *[x.data_ptr() for x in ints], out.data_ptr()), scratch.h)
    parent, from_slot, task, mach = (x.cpu().numpy() for x in ints)
    got = out.cpu().numpy()
    values = np.repeat(score, T) + raw[:, column]
    eligible = np.repeat(score != -np.inf, T) & ((status & (capi.ST_INVALID | capi.ST_INFEASIBLE)) == 0)
    empty = 0
    for n in range(N):
        lo = n * W * T
        picks = ref.select(values[lo:lo + W * T], eligible[lo:lo + W * T], sig[lo:lo + W * T] if with_sig else None, W)
        for k, c in enumerate(picks):
            i = n * W + k
            if c is None:
                empty += 1
                assert (parent[i], from_slot[i], task[i], mach[i]) == (-1, -1, -1, -1) and got[i] == -np.inf, f"instance {n} rank {k}"
                continue
            w, r = divmod(c, T)
            assert (parent[i], from_slot[i], task[i], mach[i]) == (lo + c, w, r // M * M, r % M), f"instance {n} rank {k}"
            assert got[i].view(np.int64) == values[lo + c].view(np.int64), f"instance {n} rank {k}: value bits"
    assert empty > 0 if with_sig else empty == 0
    top = got[2 * W:]                                                   # instance 2: the picks at zero, in rank order
    zeros = top[top == 0]
    assert parent[2 * W] == 2 * W * T + 7 and np.signbit(zeros[0]) and len(zeros) >= 4 and not np.signbit(zeros).all(), "rank 0 is the -0.0, later ranks hold +0.0"
    scratch.close(); beam.close()
