"""Shared parity driver (plain module): a DeviceBatchEnv against the C oracle on the same host-generated instances and random valid
actions, compared in FULL after the reset and after EVERY step.

A step rewrites only the rows its decision changes (at most M feature rows, at most 4 ELL rows, one machine row), so a wrong or skipped
row stays wrong until that job acts again: a comparison at a few steps can miss it, a comparison at every step cannot.

The dtype contract (tests/test_env_hip_golden.py): with obs_dtype="f32" tasks_fea, m_fea2 and m_fea1 are float32 and np.array_equal to
oracle_f64.astype(np.float32) — round to nearest, what actor_critic.py:143's `.float()` does; everything else stays f64 / integer and
bit-equal.  With "f64" every float is bit-equal.  No tolerance appears anywhere.

Two parameters choose what the kernels are shown.  policy: "mask" draws the job from the unmasked jobs — the round-robin job mask
keeps all jobs in lockstep, so an operation almost never fits before or between the operations already on its machine; "blocks" and
"jobseq" ignore the mask (any job with operations left, as the reference's `free` traces do) and send 4 to 13 % of all steps down the
front insertion and 21 to 50 % down the gap insertion.  data: "generated" times are products of uniform doubles and never equal;
"integer" times (integer_data) tie everywhere, which is the only input on which `<=` differs from `<` in the three comparisons that
choose the scheduling path.  oracle_walk runs the oracle alone over the same instances and actions: tests/test_env_insertions_cpu.py
uses it to prove that a case reaches what it is about.

adjacency: "dense" reads the whole [B, T, T] adjacency after every step — 100 MB per step at T = 2048.  "sparse" compares what the
kernels write, the two in-edge slots of every row (ell_col / ell_val), with the oracle's own ELL (observe(dense=False)) after every
step, each row as the SET of its (column, value) pairs with column -1 = an empty slot, and the dense form after the reset and at the
episode's end only.  tests/test_env_large_shapes_cpu.py proves on the CPU that the oracle's ELL is its dense adjacency in this sense,
so the sparse comparison is as strong as the dense one.
"""
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import torch

_SELECTION_VARS = ("MTFJSP_ENV_KERNEL", "MTFJSP_ENV_LDS", "MTFJSP_ENV_STEP_G")


def dispatch_kernel(J, M, B, force=None):
    """the step kernel mtfjsp_step launches for this shape: Rollout.env_kernel_name (the library's own launch selection, no handle
    needed) on a stand-in carrying T, M, J, B, with MTFJSP_ENV_KERNEL = force (None: the default dispatch)"""
    import mtfjsp_amd  # noqa: F401
    rollout = import_module("e2e-mappo-for-mt-fjsp_amd.rollout")
    saved = {k: os.environ.pop(k, None) for k in _SELECTION_VARS}
    try:
        if force:
            os.environ["MTFJSP_ENV_KERNEL"] = force
        return rollout.Rollout.env_kernel_name(SimpleNamespace(J=J, M=M, T=J * M, B=B))
    finally:
        for k in _SELECTION_VARS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def create_lds_bytes(J, M, f32):
    """csrc/mtfjsp_env_select.h's env_step_lds_bytes and mtfjsp_env.hip's env_reset_lds_bytes restated: the dynamic LDS of k_env_step
    (one instance per workgroup) and of k_env_reset, and the larger of the two — what mtfjsp_create holds against the device's limit"""
    T = J * M
    Tp = (T + 7) & ~7
    up16 = lambda x: (x + 15) & ~15
    step = up16(up16((4 * T + Tp + M * M + 3 * M + 2 * J + 28 + 8) * 8) + M * 12 * (4 if f32 else 8)) + (3 * T + J + 4 * M + 1 + 4) * 4
    reset = 3 * T * 8 + min(T, 64) * 12 * 8 + 16
    return step, reset, max(step, reset)


def random_valid(rs, cand, mask, feas):
    """one uniformly drawn valid (job, task, machine) per instance, on the host"""
    B = cand.shape[0]
    job = np.array([rs.choice(np.flatnonzero(mask[b] == 0)) for b in range(B)], np.int32)
    task = cand[np.arange(B), job].astype(np.int32)
    mach = np.array([rs.choice(np.flatnonzero(feas[b, task[b]])) for b in range(B)], np.int32)
    return job, task, mach


POLICIES = ("mask", "blocks", "jobseq")
DATA = ("generated", "integer")


def integer_data(t, p, tt):
    """small-integer times from a generated instance: durations 1..9 and powers with the sign (negative = infeasible machine)
    kept, transport floor(tt/7) — still symmetric with a zero diagonal, zero between some different machines.  Every value is
    exact in float32"""
    ti = np.sign(t) * np.ceil(np.abs(t) * 9 / 120)
    pi = np.sign(p) * np.ceil(np.abs(p) / 6)
    return ti, pi, np.floor(tt / 7)


def parity_instances(J, M, E, B, seed, data="generated"):
    """the instances of a run_parity case: -> t, p, tt, edge"""
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    assert data in DATA
    t, p, tt, edge = inst.generate_instances(B, J, M, E, seed=1000 * seed + J * 100 + M)
    if data == "integer":
        t, p, tt = integer_data(t, p, tt)
    return t, p, tt, edge


class Actions:
    """the action stream of one episode.  "mask": random_valid on the shared RandomState, as before.  The mask-free policies keep
    their own per-job counters (task = job * M + done[job]) and take all randomness from one array U[T, B, 3] of random_sample drawn
    up front — column 0 the redraw decision, 1 the job, 2 the machine, index = int(U * len(choices)) — so that no instance's state
    reaches another instance's actions (rs.choice consumes a state-dependent number of words).
    "blocks": the previous job is kept while it has operations left, except with probability 0.3, or at step 0, a job is drawn
    uniformly among the unfinished ones.  "jobseq": a per-instance random permutation of the jobs, each finished before the next"""

    def __init__(self, policy, rs, J, M, B, feas):
        assert policy in POLICIES
        self.policy, self.rs, self.J, self.M, self.B, self.feas = policy, rs, J, M, B, feas
        if policy != "mask":
            self.U = rs.random_sample((J * M, B, 3))
            self.done = np.zeros((B, J), np.int64)
            self.prev = np.full(B, -1, np.int64)
            self.order = np.argsort(self.U[:J, :, 1], axis=0, kind="stable").T     # [B, J]: jobseq's permutations

    def next(self, s, cand, mask):
        """-> job, task, machine [B] int32 of step s; cand, mask: the oracle's candidate and job mask (read by "mask" only)"""
        if self.policy == "mask":
            return random_valid(self.rs, cand, mask, self.feas)
        B, M, U, done = self.B, self.M, self.U[s], self.done
        job = np.zeros(B, np.int32)
        for b in range(B):
            if self.policy == "jobseq":
                job[b] = self.order[b, s // M]
            elif s == 0 or done[b, self.prev[b]] == M or U[b, 0] < 0.3:
                ok = np.flatnonzero(done[b] < M)
                job[b] = ok[int(U[b, 1] * len(ok))]
            else:
                job[b] = self.prev[b]
        ar = np.arange(B)
        task = (job * M + done[ar, job]).astype(np.int32)
        mach = np.zeros(B, np.int32)
        for b in range(B):
            fm = np.flatnonzero(self.feas[b, task[b]])
            mach[b] = fm[int(U[b, 2] * len(fm))]
        done[ar, job] += 1
        self.prev = job.astype(np.int64)
        return job, task, mach


def config_kwargs(config):
    """config = (w_mk, w_ec, w_tt, divisor, gamma) or None (both sides' defaults: 0.4, 0.4, 0.2, 1, 0.99) -> the keywords of
    DeviceBatchEnv and of OracleBatch"""
    if config is None:
        return {}, {}
    w_mk, w_ec, w_tt, divisor, gamma = (float(x) for x in config)
    return (dict(w_cfg=(w_mk, w_ec, w_tt), scaling_divisor=divisor, gamma=gamma),
            dict(w_cfg=(w_mk, w_ec, w_tt), divisor=divisor, gamma=gamma))


def oracle_walk(J, M, E, B, left_shift=True, episodes=1, seed=0, policy="mask", data="generated", config=None):
    """the oracle alone over run_parity's instances and actions (no device, no reset_episode): -> dict of paths [episodes, T, B],
    ties [episodes, B, 3] (OracleBatch.ties at each episode's end), actions [episodes, T, B, 3] = job, task, machine, and info
    [episodes, T, B, 6], raw [episodes, T, B, 5] of every step.  config: config_kwargs"""
    from oracle.env_oracle import OracleBatch
    T = J * M
    t, p, tt, edge = parity_instances(J, M, E, B, seed, data)
    feas = t >= 0
    rs = np.random.RandomState(seed)
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, **config_kwargs(config)[1])
    orc.scaler_init()
    paths, ties, actions, infos, raws = [], [], [], [], []
    for ep in range(episodes):
        w3 = rs.dirichlet([1, 1, 1], B)
        if ep > 0:
            orc.scaler_reset_returns()
        orc.reset(w3)
        cand, mask = orc.job_mask_state()
        act = Actions(policy, rs, J, M, B, feas)
        for s in range(T):
            job, task, mach = act.next(s, cand, mask)
            info, raw, pth = orc.step(task, mach)
            cand, mask = orc.job_mask_update(job)
            paths.append(pth); actions.append(np.stack([job, task, mach], 1)); infos.append(info); raws.append(raw)
        assert info[:, 1].all()
        ties.append(orc.ties())
    return dict(paths=np.array(paths).reshape(episodes, T, B), ties=np.array(ties),
                actions=np.array(actions, np.int32).reshape(episodes, T, B, 3),
                info=np.array(infos).reshape(episodes, T, B, 6), raw=np.array(raws).reshape(episodes, T, B, 5))


def ell_rows(col, val):
    """[.., 2] slots of every row in a canonical order (by column, then value), values as float64: two ELL forms hold the same set of
    (column, value) pairs per row, -1 = empty, exactly when these arrays are equal"""
    col = np.asarray(col).reshape(-1, 2).astype(np.int32); val = np.asarray(val).reshape(-1, 2).astype(np.float64)
    swap = (col[:, 0] > col[:, 1]) | ((col[:, 0] == col[:, 1]) & (val[:, 0] > val[:, 1]))
    col[swap] = col[swap][:, ::-1]; val[swap] = val[swap][:, ::-1]
    return col, val


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, expected {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {i}: {got[i]!r}, expected {want[i]!r}")


def run_parity(J, M, E, B, obs_dtype, left_shift=True, episodes=1, seed=0, force=None, monkeypatch=None, expect_kernel=None,
               second_reset="reset", policy="mask", data="generated", adjacency="dense", expect_launch=None, config=None):
    """-> number of compared steps.  policy, data: the action stream and the instance times (module docstring).
    force: MTFJSP_ENV_KERNEL for the handle's launches (needs monkeypatch).  expect_kernel: the kernel
    the case is about; asserted against the dispatch.  second_reset: how episodes after the first begin — "reset" (scaler_reset_returns
    + reset with fresh weights) or "reset_episode" (the one-launch form; the weights it draws are fed to the oracle's reset).  Every
    later reset runs over the terminal state of the episode before: it must rewrite every row of a dirty observation buffer.
    adjacency: "dense" or "sparse" (module docstring).  expect_launch: (instances per workgroup[, dynamic LDS bytes]) of the live
    handle's step launch.  config: (w_mk, w_ec, w_tt, divisor, gamma) for the handle and the oracle (config_kwargs); None = the
    defaults of both."""
    import mtfjsp_amd  # noqa: F401
    batch_env = import_module("e2e-mappo-for-mt-fjsp_amd.batch_env")
    capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
    from oracle.env_oracle import OracleBatch
    assert obs_dtype in ("f32", "f64") and second_reset in ("reset", "reset_episode") and policy in POLICIES and data in DATA
    assert adjacency in ("dense", "sparse")
    if monkeypatch is not None:
        for k in _SELECTION_VARS:
            monkeypatch.delenv(k, raising=False)
        if force:
            monkeypatch.setenv("MTFJSP_ENV_KERNEL", force)
    else:
        assert not force and not any(os.environ.get(k) for k in _SELECTION_VARS), "forcing a kernel needs monkeypatch"
    T = J * M
    odt = np.float32 if obs_dtype == "f32" else np.float64
    case = f"J{J}M{M}E{E} B={B} {obs_dtype} force={force} left_shift={left_shift} policy={policy} data={data}"
    if config is not None:
        case += f" config={tuple(config)}"
    env_kw, orc_kw = config_kwargs(config)

    def obs(x):                                      # the oracle's f64 observation in the handle's observation type
        return np.asarray(x, np.float64).astype(odt)

    t, p, tt, edge = parity_instances(J, M, E, B, seed, data)
    feas = t >= 0
    rs = np.random.RandomState(seed)
    env = batch_env.DeviceBatchEnv(J, M, E, B, left_shift=left_shift, obs_dtype=obs_dtype, **env_kw)
    if expect_kernel is not None:                    # the live handle's own answer: this device's LDS, the switches as set above
        assert env.step_kernel_name() == expect_kernel, (env.step_kernel_name(), expect_kernel)
    if expect_launch is not None:
        assert env.step_launch_info()[:len(expect_launch)] == tuple(expect_launch), (env.step_launch_info(), expect_launch)
    env.load_instances(t, p, tt, edge=edge)
    env.scaler_init()
    orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, **orc_kw)
    orc.scaler_init()

    sparse = adjacency == "sparse"

    def check_observation(o, tag):
        _same(env.tasks_fea.cpu().numpy(), obs(o["tfea"]), tag + " tasks_fea")
        _same(env.m_fea2.cpu().numpy(), obs(o["mfea2"]), tag + " m_fea2")
        if sparse:
            got, want = ell_rows(env.ell_col.cpu().numpy(), env.ell_val.cpu().numpy()), ell_rows(o["ell_col"], o["ell_val"])
            _same(got[0], want[0], tag + " ell_col (rows as sets)"); _same(got[1], want[1], tag + " ell_val (rows as sets)")
        if "adj" in o:
            _same(env.dense_adj().cpu().numpy(), o["adj"], tag + " dense_adj")
        _same(env.valid_action_mask().cpu().numpy(), orc.valid_action_mask(), tag + " valid_action_mask")

    n = 0
    for ep in range(episodes):
        tag = f"{case} episode {ep} reset"
        if ep > 0 and second_reset == "reset_episode":
            w3 = env.reset_episode(77 + seed, ep).cpu().numpy()
            assert w3.shape == (B, 3) and (w3 > 0).all()
            orc.scaler_reset_returns()
        else:
            w3 = rs.dirichlet([1, 1, 1], B)
            if ep > 0:
                env.scaler_reset_returns(); orc.scaler_reset_returns()
            env.reset(w3)
        o = orc.reset(w3)
        _same(env.read_state(capi.STATE_W3), w3, tag + " reward weights")
        check_observation(o, tag)
        cand, mask = orc.job_mask_state()
        _same(env.candidate.cpu().numpy(), cand, tag + " candidate"); _same(env.job_mask.cpu().numpy(), mask, tag + " job_mask")
        act = Actions(policy, rs, J, M, B, feas)
        for s in range(T):
            tag = f"{case} episode {ep} step {s}"
            job, task, mach = act.next(s, cand, mask)
            mm = ~feas[np.arange(B), task]
            mf1 = env.observe_mfea1(task, mm).cpu().numpy()               # before the step, with the machine mask (run:258-259)
            _same(mf1, obs(orc.mfea1(task, mm, o["tfea"])), tag + " m_fea1")
            _same(env.mmask.cpu().numpy(), mm.astype(np.uint8), tag + " machine mask")
            # the rows a step is to rewrite in full — the acting task .. the end of its job (env:2245-2277) — are poisoned first:
            # columns 8..11 (job number, reward weights) do not change within an episode, so a store the kernel skips there would
            # leave the right value behind and show in no comparison.  Observations are outputs only: no kernel reads them back
            rows = np.concatenate([b * T + np.arange(task[b], (task[b] // M + 1) * M) for b in range(B)])
            env.tasks_fea[torch.as_tensor(rows, device=env.tasks_fea.device)] = float("nan")
            env.step(task, mach)                                          # host variant: raises on an invalid action
            info, raw, paths = orc.step(task, mach)
            cand, mask = orc.job_mask_update(job)
            o = orc.observe(dense=not sparse or s == T - 1)
            st = env.status.cpu().numpy()
            assert not (st & (capi.ST_INVALID | capi.ST_INFEASIBLE)).any(), tag + " status flags"
            _same(st & capi.PATH_MASK, paths, tag + " scheduling path")
            _same(env.info.cpu().numpy(), info, tag + " info"); _same(env.raw.cpu().numpy(), raw, tag + " raw")
            check_observation(o, tag)
            _same(env.candidate.cpu().numpy(), cand, tag + " candidate"); _same(env.job_mask.cpu().numpy(), mask, tag + " job_mask")
            n += 1
        assert info[:, 1].all(), tag + ": the episode must be over"
        tag = f"{case} episode {ep} end"
        so = orc.state()
        _same(env.read_state(capi.STATE_SCALER), so["scaler"], tag + " scaler")
        _same(env.read_state(capi.STATE_START), so["st"], tag + " start times"); _same(env.read_state(capi.STATE_FINISH), so["ft"], tag + " finish times")
        _same(env.read_state(capi.STATE_MACHINE), so["mach"], tag + " machines"); _same(env.read_state(capi.STATE_ROUTES), so["routes"], tag + " routes")
        _same(env.read_state(capi.STATE_PREV_COSTS), so["prev"], tag + " previous costs")
    env.close()
    return n
