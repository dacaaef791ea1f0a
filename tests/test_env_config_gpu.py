"""PARITY (GPU): every step kernel against the C oracle with the reward weights, the divisor and gamma OFF their defaults, after the
reset and after EVERY step (tests/env_parity.py), and the rollout's own environment under a configuration of the caller's.

Every step kernel reads five words of EnvParams — w_mk, w_ec, w_tt, divisor, gamma (env:1164, pt:54-124) — and every other test of
the suite shows them (0.4, 0.4, 0.2), 1.0 and 0.99.  With those a kernel may swap w_mk and w_ec, never take the second arm of
`divisor == 1.0 ? tot_n : tot_n / divisor` (or take it as a multiplication by the reciprocal), or keep 0.99 as the scaler's gamma,
and pass everything.  The two configurations here, as (w_mk, w_ec, w_tt, divisor, gamma):

  A = (0.55, 0.15, 0.30, 7.0, 0.9)   three different weights, a divisor whose reciprocal is not exact, another gamma
  B = (0.0, 1.0, 0.0, -3.0, 1.0)     zero weights, a negative divisor (mtfjsp_create refuses 0 only), an undiscounted return

The oracle is pinned to the reference under both by tests/golden/trace_j6m6e2_cfg{A,B}_*.npz (tests/test_oracle_golden.py).

The table names the kernel every row is about; the GPU test asserts that the dispatch reaches it, the first CPU test walks the table
through the dispatch, and the second proves on the oracle alone that every row's instances and actions tell the three defects apart.
Shapes are the smallest that reach each kernel; every batch ends in a partly filled group; the actions are "blocks" (insertions
occur); every row runs two episodes, the second begun with reset_episode: the scaler's mean and S carry over, its returns do not.
"""
from collections import namedtuple
from importlib import import_module

import numpy as np
import pytest

from env_parity import _same, dispatch_kernel, oracle_walk, run_parity

CONFIG_A = (0.55, 0.15, 0.30, 7.0, 0.9)
CONFIG_B = (0.0, 1.0, 0.0, -3.0, 1.0)
CONFIGS = {"A": CONFIG_A, "B": CONFIG_B}

Case = namedtuple("Case", "config obs_dtype force J M E B kernel")

J6M6, J3M11, J5M12 = (6, 6, 2), (3, 11, 1), (5, 12, 2)
SEED = 5

CASES = (
    # A, float32 observations: every step kernel.  B = 19: one full group of 16 + 3, four full groups of 4 + 3; 11: one full group
    # of 8 + 3; 3 workgroups of the one-instance kernel
    Case("A", "f32", "grp16", *J6M6, 19, "k_env_grp16"),
    Case("A", "f32", "grp4", *J6M6, 19, "k_env_grp4"),
    Case("A", "f32", "reg1", *J6M6, 19, "k_env_reg"),
    Case("A", "f32", "grp16", *J3M11, 19, "k_env_grp16x2"),
    Case("A", "f32", "grp4", *J3M11, 19, "k_env_grp4x2"),
    Case("A", "f32", "lds", *J6M6, 11, "k_env_step_grp"),
    Case("A", "f32", None, *J5M12, 11, "k_env_step_grp"),
    Case("A", "f32", "lds1", *J6M6, 3, "k_env_step"),
    # B: one kernel of each of the three bodies that hold the reward code
    Case("B", "f32", "grp16", *J6M6, 19, "k_env_grp16"),
    Case("B", "f32", None, *J5M12, 11, "k_env_step_grp"),
    Case("B", "f32", "lds1", *J6M6, 3, "k_env_step"),
    # A, float64 observations
    Case("A", "f64", "grp16", *J6M6, 19, "k_env_grp16"),
    Case("A", "f64", None, *J5M12, 11, "k_env_step_grp"),
)
GROUP = {"k_env_grp16": 16, "k_env_grp16x2": 16, "k_env_grp4": 4, "k_env_grp4x2": 4, "k_env_reg": 1, "k_env_step_grp": 8, "k_env_step": 1}


def _id(c):
    return f"{c.config}-{c.obs_dtype}-{c.force or 'default'}-J{c.J}M{c.M}E{c.E}-B{c.B}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_step_equals_the_oracle_off_the_default_configuration(case, monkeypatch):
    c = case
    n = run_parity(c.J, c.M, c.E, c.B, c.obs_dtype, episodes=2, seed=SEED, force=c.force, monkeypatch=monkeypatch,
                   expect_kernel=c.kernel, second_reset="reset_episode", policy="blocks", config=CONFIGS[c.config])
    assert n == 2 * c.J * c.M


@pytest.mark.gpu
def test_rollout_hands_its_configuration_to_its_environment():
    """Rollout's gamma is the discount of the advantages and of the reward scaler (pe:82: both are args['GAMMA']), and its w_cfg and
    scaling_divisor are the environment's: the rollout's own environment, stepped by the rollout, against the oracle built with the
    same five numbers — rewards after every step of two episodes, the scaler's state at each episode's end"""
    import mtfjsp_amd  # noqa: F401
    rollout = import_module("e2e-mappo-for-mt-fjsp_amd.rollout")
    capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
    from oracle.env_oracle import OracleBatch
    J, M, E, B = 6, 6, 2, 19
    A = CONFIG_A
    ro = rollout.Rollout(J, M, E, B, policy="random", gamma=0.9, w_cfg=A[:3], scaling_divisor=7.0, w3="host")
    env = ro.env
    t, p, tt, edge = env.read_instances()
    orc = OracleBatch(t, p, tt, edge, w_cfg=A[:3], divisor=7.0, gamma=0.9)
    orc.scaler_init()
    for ep in range(2):
        for s in range(J * M):
            tag = f"episode {ep} step {s}"
            ro.step()                                                    # (its first step of an episode resets the environment)
            if s == 0:
                orc.scaler_reset_returns()
                orc.reset(env.read_state(capi.STATE_W3))
            task, mach = ro.task.cpu().numpy(), ro.mach.cpu().numpy()
            info, raw, _ = orc.step(task, mach)
            _same(env.raw.cpu().numpy(), raw, tag + " raw")
            _same(env.info.cpu().numpy(), info, tag + " info")
        assert info[:, 1].all(), tag + ": the episode must be over"
        _same(env.read_state(capi.STATE_SCALER), orc.state()["scaler"], f"episode {ep} end: scaler")


def test_the_table_reaches_every_step_kernel_under_A_and_every_reward_body_under_B():
    """no GPU: the dispatch sends every row to the kernel it names; the batches end in a partly filled group"""
    for c in CASES:
        assert dispatch_kernel(c.J, c.M, c.B, c.force) == c.kernel, _id(c)
        g = GROUP[c.kernel]
        assert c.M % c.E == 0 and c.B > g and (g == 1 or c.B % g != 0), _id(c)     # a full group and a ragged last one
    reached = {(c.config, c.obs_dtype, c.kernel) for c in CASES}
    kernels = ("k_env_grp16", "k_env_grp4", "k_env_grp16x2", "k_env_grp4x2", "k_env_reg", "k_env_step_grp", "k_env_step")
    assert {("A", "f32", k) for k in kernels} <= reached
    # the three bodies: mtfjsp_env_grp.h (register kernels), mtfjsp_env.hip's grouped LDS kernel and its one-instance kernel
    assert {("B", "f32", k) for k in ("k_env_grp16", "k_env_step_grp", "k_env_step")} <= reached
    assert {("A", "f64", k) for k in ("k_env_grp16", "k_env_step_grp")} <= reached
    # the LDS kernel both forced on a register-kernel shape and by the default dispatch
    assert {c.force for c in CASES if c.kernel == "k_env_step_grp" and c.config == "A" and c.obs_dtype == "f32"} == {"lds", None}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def test_every_row_tells_swapped_weights_a_unit_divisor_and_a_frozen_gamma_apart():
    """no GPU, the oracle alone: conditions on the INPUTS of the GPU test.  The first episode of oracle_walk is the first episode of
    run_parity word for word (instances, weights, actions; the raw rewards do not depend on the weights the second reset draws), so
    what shows here shows there.  Per row: the configuration with w_mk and w_ec swapped, with divisor 1 and with gamma 0.99 each
    changes `raw` or `info` at some step; raw[:, 0] is tot_n / divisor to the bit, tot_n restated from raw[:, 1:5] in env:1164's
    order; and under A (divisor 7) the multiplication by the reciprocal gives other bits at some step"""
    seen = {}
    for c in CASES:
        key = (c.config, c.J, c.M, c.E, c.B)
        if key in seen:
            continue
        seen[key] = True
        w_mk, w_ec, w_tt, d, gamma = cfg = CONFIGS[c.config]

        def walk(config):
            return oracle_walk(c.J, c.M, c.E, c.B, seed=SEED, policy="blocks", config=config)
        ref = walk(cfg)
        for what, other in (("swapped weights", (w_ec, w_mk, w_tt, d, gamma)), ("divisor 1", (w_mk, w_ec, w_tt, 1.0, gamma)),
                            ("gamma 0.99", (w_mk, w_ec, w_tt, d, 0.99))):
            assert other != cfg, (_id(c), what)
            got = walk(other)
            assert np.array_equal(got["actions"], ref["actions"]) and np.array_equal(got["raw"][..., 1:], ref["raw"][..., 1:])
            assert not (np.array_equal(got["raw"], ref["raw"]) and np.array_equal(got["info"], ref["info"])), (_id(c), what)
        raw = ref["raw"]                                                   # [1, T, B, 5]: total, r_t, r_idle, r_pt, r_tt
        r_t, r_idle, r_pt, r_tt = (raw[..., i] for i in (1, 2, 3, 4))
        tot_n = w_mk * r_t + w_ec * (r_pt + 1 * r_idle) + w_tt * r_tt * 1      # env:1164
        assert np.array_equal(_bits(tot_n / d), _bits(raw[..., 0])), _id(c)
        if c.config == "A":
            assert d == 7.0 and (_bits(tot_n * (1 / d)) != _bits(raw[..., 0])).any(), _id(c)
    assert len(seen) >= 5
