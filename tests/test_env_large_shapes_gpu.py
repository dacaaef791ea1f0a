"""PARITY (GPU): the environment beyond J20M20, up to the largest shape mtfjsp_create accepts, against the C oracle after the reset and
after EVERY step (tests/env_parity.py), by the default dispatch only.

mtfjsp_create takes any n_job >= 1, 2 <= n_machine <= 64 and T = n_job * n_machine <= 32767 whose single instance fits a workgroup's
LDS.  Every other every-step comparison stops at T = 400, J = 20, M = 20, and runs k_env_step_grp with 8 instances per workgroup and
k_env_step only where it is forced.  The rows below reach what lies beyond: the group size falling from 8 to 4 to 2 and then to
k_env_step as one instance's LDS region grows (csrc/mtfjsp_env_select.h), more than 64 jobs (more than one job per lane), 64 machines
(the largest transport matrix and machine rows), a pairwise energy sum of 8 and of 32 leaves, a group launch 2.7 KB under the device's
limit whose float64 twin no longer fits, and the largest accepted shape.  Beyond it stands the refusal, and two live handles of
different size share the kernels whose LDS limit mtfjsp_create sets.

The table states the plan of every row where a workgroup may use 163840 bytes of LDS (gfx950); tests/test_step_dispatch_cpu.py holds
the library's rule to the same figures without a GPU.  The GPU test asks the device for its limit, takes the expectation from
mtfjsp_step_kernel_name_for with that limit — never from the handle under test — and asserts the live handle's kernel, group size and
launched LDS bytes against it.  Every batch ends in a partly filled group wherever a group holds more than one instance.

Shapes with T > 600 compare the adjacency in its sparse form (env_parity: as strong as the dense one, proven on the CPU), in one
episode of mask-respecting actions.  The smaller shapes also run without left shift, and with mask-free "blocks" actions over two
episodes, the second begun by reset_episode; tests/test_env_large_shapes_cpu.py proves on the oracle that those reach the front and the
gap insertion.
"""
import functools
from collections import namedtuple
from importlib import import_module

import numpy as np
import pytest

from env_parity import _same, create_lds_bytes, ell_rows, parity_instances, random_valid, run_parity

LDS_GFX950 = 163840
Plan = namedtuple("Plan", "kernel G region launch")          # region: bytes of one instance's k_env_step_grp region; launch: dynamic LDS
Row = namedtuple("Row", "J M E B f32 f64 also_f64 what")


def _grp(G, region):
    return Plan("k_env_step_grp", G, region, G * region)


def _one(region, launch):
    return Plan("k_env_step", 1, region, launch)


ROWS = (
    Row(65, 2, 1, 11, _grp(8, 6976), _grp(8, 7072), False, "smallest J > 64, T = 130"),
    Row(70, 8, 2, 7, _grp(4, 23984), _grp(4, 24368), False, "G = 4 by LDS, 8 leaves, J > 64"),
    Row(4, 64, 4, 11, _grp(8, 16448), _grp(8, 19520), True, "M = 64 at small T; 8 regions fill 156160 B in f64"),
    Row(64, 16, 2, 3, _grp(2, 42272), _grp(2, 43040), False, "G = 2, T = 1024"),
    Row(30, 64, 4, 3, _grp(2, 80304), _one(83376, 142220), True, "group launch of 160608 B; the dtype flips the kernel"),
    Row(64, 32, 4, 3, _one(82784, 119092), _one(84320, 120628), False, "k_env_step by default, T = 2048"),
    Row(36, 64, 4, 2, _one(95152, 159236), _one(98224, 162308), True, "largest accepted, 32 leaves"),
)
SPARSE_ABOVE = 600                                            # T
VARIANTS = ("noleftshift", "blocks_reset_episode")            # of the rows with T <= SPARSE_ABOVE, in f32
Case = namedtuple("Case", "row obs_dtype variant")
CASES = ([Case(r, "f32", "plain") for r in ROWS] + [Case(r, "f64", "plain") for r in ROWS if r.also_f64]
         + [Case(r, "f32", v) for r in ROWS if r.J * r.M <= SPARSE_ABOVE for v in VARIANTS])
SEED = 3


def case_id(c):
    r = c.row
    return f"J{r.J}M{r.M}E{r.E}-B{r.B}-{c.obs_dtype}-{c.variant}"


def case_arguments(c):
    """-> keyword arguments of run_parity / oracle_walk that the variant sets, and the adjacency form"""
    kw = {"plain": dict(left_shift=True, episodes=1, policy="mask"), "noleftshift": dict(left_shift=False, episodes=1, policy="mask"),
          "blocks_reset_episode": dict(left_shift=True, episodes=2, policy="blocks")}[c.variant]
    return kw, "sparse" if c.row.J * c.row.M > SPARSE_ABOVE else "dense"


def _lib():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.batch_env"), import_module("e2e-mappo-for-mt-fjsp_amd.capi")


@functools.lru_cache(maxsize=None)
def device_lds():
    """the LDS a workgroup may use on this device, asked through a handle of another shape than any under test"""
    batch_env, _ = _lib()
    env = batch_env.DeviceBatchEnv(6, 6, 2, 1)
    lds = env.step_launch_info()[2]
    env.close()
    return lds


def expected_plan(r, obs_dtype, lds_max):
    """(kernel, G, launched bytes) from the handle-free rule; on gfx950's 160 KiB it must be the table's"""
    batch_env, _ = _lib()
    f32 = obs_dtype == "f32"
    kernel, G, region, overridden = batch_env.step_kernel_for(r.J, r.M, r.B, f32, lds_max)
    assert not overridden
    launch = G * region if kernel == "k_env_step_grp" else create_lds_bytes(r.J, r.M, f32)[0]
    if lds_max == LDS_GFX950:
        want = r.f32 if f32 else r.f64
        assert (kernel, G, region, launch) == tuple(want), (r, obs_dtype)
    return kernel, G, launch


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_step_and_reset_equal_the_oracle(case, monkeypatch):
    r = case.row
    kernel, G, launch = expected_plan(r, case.obs_dtype, device_lds())
    kw, adjacency = case_arguments(case)
    print(f"{case_id(case)}: {kernel}, G = {G}, {launch} bytes of LDS per launch, adjacency {adjacency}")
    n = run_parity(r.J, r.M, r.E, r.B, case.obs_dtype, seed=SEED, monkeypatch=monkeypatch, expect_kernel=kernel, expect_launch=(G, launch),
                   second_reset="reset_episode", adjacency=adjacency, **kw)
    assert n == kw["episodes"] * r.J * r.M


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
def test_create_refuses_one_instance_that_does_not_fit_and_takes_the_largest_that_does(obs_dtype):
    """J40M64 needs 172628 B (f32) for k_env_step: MTFJSP_ERR_ARG, "too large"; J36M64 is created; the handle-free rule says the same on
    both sides of the device's limit"""
    batch_env, capi = _lib()
    lds, f32 = device_lds(), obs_dtype == "f32"
    assert create_lds_bytes(40, 64, True)[2] == 172628
    for J in (36, 37, 40):
        fits = create_lds_bytes(J, 64, f32)[2] <= lds
        if lds == LDS_GFX950:
            assert fits == (J == 36 or (J == 37 and f32)), (J, obs_dtype)
        if fits:
            env = batch_env.DeviceBatchEnv(J, 64, 4, 2, obs_dtype=obs_dtype)
            assert env.step_kernel_name() == batch_env.step_kernel_for(J, 64, 2, f32, lds)[0]
            env.close()
        else:
            with pytest.raises(capi.MtfjspError, match="too large") as e:
                batch_env.DeviceBatchEnv(J, 64, 4, 2, obs_dtype=obs_dtype)
            assert e.value.code == capi.ERR_ARG
            with pytest.raises(ValueError):
                batch_env.step_kernel_for(J, 64, 2, f32, lds)


class Live:
    """one handle and its oracle, stepped by the caller: everything run_parity compares per step, the adjacency in its sparse form"""

    def __init__(self, J, M, E, B, obs_dtype, seed):
        batch_env, self.capi = _lib()
        from oracle.env_oracle import OracleBatch
        self.J, self.M, self.T, self.B = J, M, J * M, B
        self.tag = f"J{J}M{M} B={B}"
        self.odt = np.float32 if obs_dtype == "f32" else np.float64
        t, p, tt, edge = parity_instances(J, M, E, B, seed)
        self.feas = t >= 0
        self.rs = np.random.RandomState(seed)
        self.env = batch_env.DeviceBatchEnv(J, M, E, B, obs_dtype=obs_dtype)
        self.env.load_instances(t, p, tt, edge=edge)
        self.env.scaler_init()
        self.orc = OracleBatch(t, p, tt, edge)
        self.orc.scaler_init()

    def observation(self, o, tag):
        env = self.env
        _same(env.tasks_fea.cpu().numpy(), np.asarray(o["tfea"], np.float64).astype(self.odt), tag + " tasks_fea")
        _same(env.m_fea2.cpu().numpy(), np.asarray(o["mfea2"], np.float64).astype(self.odt), tag + " m_fea2")
        got, want = ell_rows(env.ell_col.cpu().numpy(), env.ell_val.cpu().numpy()), ell_rows(o["ell_col"], o["ell_val"])
        _same(got[0], want[0], tag + " ell_col"); _same(got[1], want[1], tag + " ell_val")
        _same(env.valid_action_mask().cpu().numpy(), self.orc.valid_action_mask(), tag + " valid_action_mask")
        _same(env.candidate.cpu().numpy(), self.cand, tag + " candidate"); _same(env.job_mask.cpu().numpy(), self.mask, tag + " job_mask")

    def reset(self):
        w3 = self.rs.dirichlet([1, 1, 1], self.B)
        self.env.reset(w3)
        self.orc.reset(w3)
        self.cand, self.mask = self.orc.job_mask_state()
        self.observation(self.orc.observe(dense=False), self.tag + " reset")

    def step(self, s):
        tag = f"{self.tag} step {s}"
        job, task, mach = random_valid(self.rs, self.cand, self.mask, self.feas)
        self.env.step(task, mach)
        info, raw, paths = self.orc.step(task, mach)
        self.cand, self.mask = self.orc.job_mask_update(job)
        st = self.env.status.cpu().numpy()
        assert not (st & (self.capi.ST_INVALID | self.capi.ST_INFEASIBLE)).any(), tag
        _same(st & self.capi.PATH_MASK, paths, tag + " scheduling path")
        _same(self.env.info.cpu().numpy(), info, tag + " info"); _same(self.env.raw.cpu().numpy(), raw, tag + " raw")
        self.observation(self.orc.observe(dense=False), tag)


@pytest.mark.gpu
def test_a_small_handle_created_later_does_not_take_the_large_ones_lds():
    """hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel, not to a handle.  J64M32 launches k_env_step with 119092 bytes of
    dynamic LDS and k_env_reset with 55312; J6M6 and J20M20, created after it, need 3 KB and 20 KB of the same kernels.  mtfjsp_create
    once set the attribute to the size of the handle being created, which lowered it under the large handle (the runtime of the MI355X
    this was written on did not enforce the lower value: the launches went through and were right); it now sets the device's limit.  The
    large handle resets and steps first after both small ones exist, then the three take turns for 20 steps, each against its oracle"""
    large = Live(64, 32, 4, 3, "f32", SEED)
    assert large.env.step_kernel_name() == "k_env_step"
    small = [Live(6, 6, 2, 4, "f32", SEED), Live(20, 20, 4, 3, "f32", SEED)]
    handles = [large] + small
    for h in handles:
        h.reset()
    for s in range(20):
        for h in handles:
            h.step(s)
    for h in handles:
        h.env.close()
