"""GPU: the dispatch-rule planner (k_pdr_plan, mtfjsp_pdr_plan) and the batched baselines driver (baselines.pdr_baselines).

Yardsticks: the reference's own lists and costs (tests/golden/pdr_*.npz), and at full size tests/pdr_rules_ref.py — the numpy
restatement that tests/test_pdr_rules_cpu.py pins to those fixtures — plus the CPU environment with left shift off.  Plans are
compared integer for integer on EVERY instance: both sides do the same binary64 operations in the same order, so there is no tie
allowance; costs are compared with np.array_equal like every other environment float of this project.
"""
import os
import sys
from importlib import import_module

import numpy as np
import pytest

import mtfjsp_amd  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pdr_rules_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
baselines = import_module("e2e-mappo-for-mt-fjsp_amd.baselines")
instances = import_module("e2e-mappo-for-mt-fjsp_amd.instances")

FIXTURES = ["pdr_j6m6e2_eval16", "pdr_j10m10e2_b4"]
COST_KEYS = ["opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT"]


def load(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    J, M, E, N = [int(x) for x in g["meta"]]
    return g, J, M, E, N


def rep12(x):
    x = np.asarray(x)
    return np.tile(x, (12,) + (1,) * (x.ndim - 1))


def all_rules(N):
    return (np.repeat(np.array([r[1] for r in ref.RULES], np.int32), N), np.repeat(np.array([r[2] for r in ref.RULES], np.int32), N))


def env_with(t, p, tt, edge, J, M, E, **kw):
    env = batch_env.DeviceBatchEnv(J, M, E, len(t), **kw)
    env.load_instances(t, p, tt, edge=edge)
    return env


@pytest.mark.parametrize("name", FIXTURES)
def test_plan_matches_the_reference_lists(name):
    """(4) task_out, mach_out against the reference's operation_lst / machine_lst: all 12 pairs in one batch."""
    g, J, M, E, N = load(name)
    env = env_with(rep12(g["t"]), rep12(g["p"]), rep12(g["tt"]), rep12(g["edge"]), J, M, E, left_shift=False)
    o, m = all_rules(N)
    task, mach = baselines.pdr_plan(env, o, m, mor_order=rep12(g["mor_order"]))
    task, mach = task.cpu().numpy(), mach.cpu().numpy()
    assert np.array_equal(task, g["task"].reshape(12 * N, -1))
    assert np.array_equal(mach, np.take_along_axis(g["machine_lst"], g["task"], 2).reshape(12 * N, -1))
    env.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_baselines_match_the_reference_costs(name):
    """(5) Final_4cost, Objective and the cumulative sums equal the reference's; f32 and f64 observation handles agree."""
    g, J, M, E, N = load(name)
    w = [float(x) for x in g["cfg_w"]]
    args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": w[0], "weight_ec": w[1], "weight_tt": w[2]}
    res = {dt: baselines.pdr_baselines(g["t"], g["p"], g["tt"], g["edge"], args, mor_order=g["mor_order"], obs_dtype=dt) for dt in ("f32", "f64")}
    for dt, out in res.items():
        assert list(out)[:12] == [r[0] for r in baselines.RULES] and baselines.PLANS in out
        for r, (rule, _, _) in enumerate(baselines.RULES):
            cost, final4, obj = out[rule]
            f4 = g["final4"][r]
            print(dt, rule, "max |final4 - ref|", np.abs(final4 - f4).max(), "max |cum - ref|", max(np.abs(cost[k] - g["cum"][r][:, i]).max() for i, k in enumerate(COST_KEYS)))
            assert np.array_equal(final4, f4), f"{dt} {rule}: final costs"
            assert np.array_equal(obj, w[0] * f4[:, 0] + w[1] * (f4[:, 1] + f4[:, 3]) + w[2] * f4[:, 2]), f"{dt} {rule}: objective"
            for i, k in enumerate(COST_KEYS):
                assert np.array_equal(cost[k], g["cum"][r][:, i]), f"{dt} {rule}: {k}"
            task, mach = out[baselines.PLANS][rule]
            assert np.array_equal(task, g["task"][r])
    for rule, _, _ in baselines.RULES:
        assert np.array_equal(res["f32"][rule][1], res["f64"][rule][1]) and np.array_equal(res["f32"][rule][2], res["f64"][rule][2])


@pytest.mark.parametrize("J,M,E,N", [(6, 6, 2, 4096), (10, 10, 2, 1024), (20, 20, 4, 128)], ids=["J6M6E2", "J10M10E2", "J20M20E4"])
def test_full_size_all_rules_in_one_batch(J, M, E, N):
    """(6) host-generated instances (with infeasible machines), B = 12 N: plans equal the restatement on every instance, every
    planned machine is feasible, no invalid / infeasible status, done after exactly T steps; every 8th instance's final costs
    and path words equal the CPU environment without left shift."""
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
    _all_rules_in_one_batch(J, M, E, N, t, p, tt, edge, every=8)


def test_integer_times_break_argmin_and_argmax_ties_at_the_first_index():
    """small-integer times (env_parity.integer_data): the minimum of a task's row is shared by several machines in about half of
    all rows, and some jobs start with the same total work, so SPT / SEC and the work-remaining rules decide by "first index" —
    which generated times, products of uniform doubles, never ask of them.  J6M6 x 64, all 12 rules, every instance against the
    restatement and the CPU environment (no reference fixture: the restatement is the yardstick, as at full size)"""
    from env_parity import integer_data
    J, M, E, N = 6, 6, 2, 64
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=31)
    t, p, tt = integer_data(t, p, tt)
    for x in (np.where(t < 0, np.inf, t), np.where(t < 0, np.inf, t * np.abs(p))):         # SPT, SEC: a shared row minimum
        assert ((x == x.min(-1, keepdims=True)).sum(-1) > 1).mean() > 0.1
    refer = np.sum(ref.task_values(t, p, 2).reshape(N, J, M), axis=2)                       # jobs with the same total work
    assert any(len(set(r)) < J for r in refer.tolist())
    _all_rules_in_one_batch(J, M, E, N, t, p, tt, edge, every=1)


def _all_rules_in_one_batch(J, M, E, N, t, p, tt, edge, every):
    import torch
    from oracle.env_oracle import OracleBatch          # checker
    T, B = J * M, 12 * N
    assert (t < 0).any(), "the set must contain infeasible machines"
    rng = np.random.RandomState(5)
    mor = np.stack([np.stack([rng.permutation(J) for _ in range(M)]) for _ in range(N)]).astype(np.int32)
    tb, pb, ttb, eb = rep12(t), rep12(p), rep12(tt), rep12(edge)
    o, m = all_rules(N)
    env = env_with(tb, pb, ttb, eb, J, M, E, left_shift=False, obs_dtype="f32")
    env.scaler_init()
    w3 = np.tile(np.array([[0.4, 0.4, 0.2]]), (B, 1))
    env.reset(torch.as_tensor(w3, device=env.device))
    task_d, mach_d = baselines.pdr_plan(env, o, m, mor_order=rep12(mor))
    task, mach = task_d.cpu().numpy(), mach_d.cpu().numpy()
    rt, rm = ref.plan_batch(tb, pb, J, M, o, m, rep12(mor))
    bad = np.flatnonzero((task != rt).any(1) | (mach != rm).any(1))
    print(f"J{J}M{M}: {len(bad)} of {B} plans differ from the restatement", bad[:8])
    assert len(bad) == 0
    assert np.array_equal(np.sort(task, 1), np.tile(np.arange(T), (B, 1))), "every task exactly once"
    assert (tb[np.arange(B)[:, None], task, mach] > 0).all(), "a planned machine cannot process its task"
    sub = np.arange(0, B, every)
    orc = OracleBatch(tb[sub], pb[sub], ttb[sub], eb[sub], left_shift=False)
    orc.scaler_init()
    orc.reset(w3[sub])
    ts, ms = task_d.t().contiguous(), mach_d.t().contiguous()
    flags = torch.zeros(B, dtype=torch.int32, device=env.device)
    words = set()
    for s in range(T):
        if s == T - 1:
            assert not bool(env.info[:, 1].any().item()), "an episode finished before step T"
        env.step(ts[s], ms[s])
        flags |= env.status
        _, _, paths = orc.step(task[sub, s], mach[sub, s])
        st = env.status.cpu().numpy()[sub]
        assert np.array_equal(st & capi.PATH_MASK, paths & capi.PATH_MASK), f"step {s}: path words differ"
        words |= set(int(x) for x in st & capi.PATH_MASK)
    assert int((flags & (capi.ST_INVALID | capi.ST_INFEASIBLE)).ne(0).sum().item()) == 0
    assert bool(env.info[:, 1].all().item()), "every instance is done after exactly T steps"
    assert words <= {0, 3}, f"only empty / append may occur without left shift: {sorted(words)}"
    assert np.array_equal(env.read_state(capi.STATE_PREV_COSTS)[sub], orc.state()["prev"])
    env.close()


def test_more_jobs_than_lanes():
    """the planner's J > 64 path (jobs scanned in strides of the wave) against the restatement"""
    J, M, E, N = 70, 4, 2, 8
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=32)
    rng = np.random.RandomState(6)
    mor = np.stack([np.stack([rng.permutation(J) for _ in range(M)]) for _ in range(N)]).astype(np.int32)
    o, m = all_rules(N)
    env = env_with(rep12(t), rep12(p), rep12(tt), rep12(edge), J, M, E, left_shift=False)
    task, mach = baselines.pdr_plan(env, o, m, mor_order=rep12(mor))
    rt, rm = ref.plan_batch(rep12(t), rep12(p), J, M, o, m, rep12(mor))
    assert np.array_equal(task.cpu().numpy(), rt) and np.array_equal(mach.cpu().numpy(), rm)
    drawn, _ = baselines.pdr_plan(env, 1, 0, seed=3)
    d = drawn.cpu().numpy().reshape(12 * N, M, J)
    assert np.array_equal(d % M, np.broadcast_to(np.arange(M)[None, :, None], d.shape))
    assert np.array_equal(np.sort(d // M, 2), np.broadcast_to(np.arange(J), d.shape))
    env.close()


def test_sixty_four_machines():
    """J4M64: the machine rule walks a full wave of entries, a planned machine is a byte up to 63, and the job sums of the restatement
    are numpy's 8-way unrolled loop over exactly eight blocks — the order the kernel has to add in.  All 12 pairs against the restatement"""
    J, M, E, N = 4, 64, 2, 8
    t, p, tt, edge = instances.generate_instances(N, J, M, E, seed=35)
    assert (t < 0).any(), "the set must contain infeasible machines"
    rng = np.random.RandomState(7)
    mor = np.stack([np.stack([rng.permutation(J) for _ in range(M)]) for _ in range(N)]).astype(np.int32)
    o, m = all_rules(N)
    env = env_with(rep12(t), rep12(p), rep12(tt), rep12(edge), J, M, E, left_shift=False)
    task, mach = baselines.pdr_plan(env, o, m, mor_order=rep12(mor))
    task, mach = task.cpu().numpy(), mach.cpu().numpy()
    rt, rm = ref.plan_batch(rep12(t), rep12(p), J, M, o, m, rep12(mor))
    bad = np.flatnonzero((task != rt).any(1) | (mach != rm).any(1))
    print(f"J{J}M{M}: {len(bad)} of {12 * N} plans differ from the restatement", bad[:8])
    assert np.array_equal(task, rt) and np.array_equal(mach, rm)
    assert np.array_equal(np.sort(task, 1), np.tile(np.arange(J * M), (12 * N, 1))), "every task exactly once"
    assert (rep12(t)[np.arange(12 * N)[:, None], task, mach] > 0).all(), "a planned machine cannot process its task"
    assert mach.max() > 32 and len(np.unique(mach)) > 32, "machines of the upper half of the wave are planned"
    env.close()


def test_device_generated_instances_need_no_host_copy():
    """(7) planned straight after mtfjsp_generate_instances == the same instances read back and loaded again"""
    J, M, E, B = 6, 6, 2, 256
    a = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=False)
    a.generate_instances(seed=77, first_instance=5)
    o = np.arange(B, dtype=np.int32) % 6
    m = (np.arange(B, dtype=np.int32) // 6) % 2
    ta, ma = baselines.pdr_plan(a, o, m, seed=9)
    t, p, tt, edge = a.read_instances()
    b = env_with(t, p, tt, edge, J, M, E, left_shift=False)
    tb, mb = baselines.pdr_plan(b, o, m, seed=9)
    assert np.array_equal(ta.cpu().numpy(), tb.cpu().numpy()) and np.array_equal(ma.cpu().numpy(), mb.cpu().numpy())
    keep = o != 1                                                    # MOR's order is drawn; the other rules have a restatement
    rt, rm = ref.plan_batch(t[keep], p[keep], J, M, o[keep], m[keep])
    assert np.array_equal(ta.cpu().numpy()[keep], rt) and np.array_equal(ma.cpu().numpy()[keep], rm)
    a.close(); b.close()


def test_mor_order_drawn_on_the_device():
    """(8) permutation per column, same seed same bits, another seed another order, the static rules ignore the seed"""
    J, M, E, B = 10, 10, 2, 256
    t, p, tt, edge = instances.generate_instances(B, J, M, E, seed=33)
    env = env_with(t, p, tt, edge, J, M, E, left_shift=False)
    t1, m1 = [x.cpu().numpy() for x in baselines.pdr_plan(env, 1, 0, seed=1)]
    t1b, m1b = [x.cpu().numpy() for x in baselines.pdr_plan(env, 1, 0, seed=1)]
    t2, _ = [x.cpu().numpy() for x in baselines.pdr_plan(env, 1, 0, seed=2)]
    assert np.array_equal(t1, t1b) and np.array_equal(m1, m1b)
    d = t1.reshape(B, M, J)
    assert np.array_equal(d % M, np.broadcast_to(np.arange(M)[None, :, None], d.shape)), "block c holds column c's tasks"
    assert np.array_equal(np.sort(d // M, 2), np.broadcast_to(np.arange(J), d.shape)), "each block is a permutation of the J jobs"
    assert (t1 != t2).any(1).sum() >= 1, "a different seed changes the order in at least one of 256 instances"
    assert len({tuple(x) for x in (d // M).reshape(-1, J)}) > B, "columns and instances draw their own orders"
    assert np.array_equal(m1, ref.machine_rule(t, p, 0)[np.arange(B)[:, None], t1])
    for o in (0, 2, 3, 4, 5):
        x = [y.cpu().numpy() for y in baselines.pdr_plan(env, o, 1, seed=1)]
        y = [y.cpu().numpy() for y in baselines.pdr_plan(env, o, 1, seed=2)]
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    env.close()


@pytest.mark.parametrize("o_bad,m_bad", [(6, 0), (-1, 1), (2, 2), (0, -1)])
def test_bad_rule_id_is_an_error_and_writes_nothing(o_bad, m_bad):
    """(9)"""
    import torch
    J, M, E, B = 6, 6, 2, 16
    t, p, tt, edge = instances.generate_instances(B, J, M, E, seed=34)
    env = env_with(t, p, tt, edge, J, M, E, left_shift=False)
    o = np.zeros(B, np.int32); m = np.zeros(B, np.int32)
    o[11], m[11] = o_bad, m_bad
    od, md = torch.as_tensor(o, device=env.device), torch.as_tensor(m, device=env.device)
    task = torch.full((B, J * M), -7, dtype=torch.int32, device=env.device); mach = torch.full_like(task, -7)
    rc = env.L.mtfjsp_pdr_plan(env.h, od.data_ptr(), md.data_ptr(), None, 0, task.data_ptr(), mach.data_ptr())
    torch.cuda.synchronize()
    assert rc == capi.ERR_ARG
    assert b"rule id out of range" in env.L.mtfjsp_last_error(env.h)
    assert bool((task == -7).all().item()) and bool((mach == -7).all().item()), "outputs must stay untouched"
    with pytest.raises(capi.MtfjspError):
        baselines.pdr_plan(env, o, m)
    ok_t, _ = baselines.pdr_plan(env, 0, 0)                          # the handle stays usable
    assert np.array_equal(ok_t.cpu().numpy(), np.tile(np.arange(J * M), (B, 1)))
    env.close()


def test_baselines_on_a_generated_device_batch():
    """env=: the rules run one after another on an already generated batch; same numbers as the same instances passed from the host"""
    J, M, E, N = 6, 6, 2, 64
    args = {"n_job": J, "n_machine": M, "n_edge": E, "weight_mk": 0.4, "weight_ec": 0.4, "weight_tt": 0.2}
    env = batch_env.DeviceBatchEnv(J, M, E, N, left_shift=False, obs_dtype="f32")
    env.generate_instances(seed=78)
    a = baselines.pdr_baselines(None, None, None, None, args, env=env, seed=4)
    t, p, tt, edge = env.read_instances()
    mor = a[baselines.PLANS]["MOR+SPT"][0].reshape(N, M, J) // M
    b = baselines.pdr_baselines(t, p, tt, edge, args, mor_order=mor)
    for rule, _, _ in baselines.RULES:
        assert np.array_equal(a[rule][1], b[rule][1]) and np.array_equal(a[rule][2], b[rule][2]), rule
        assert all(np.array_equal(a[rule][0][k], b[rule][0][k]) for k in COST_KEYS), rule
    with pytest.raises(ValueError):
        baselines.pdr_baselines(None, None, None, None, args, env=batch_env.DeviceBatchEnv(J, M, E, N))   # left shift on
    env.close()
