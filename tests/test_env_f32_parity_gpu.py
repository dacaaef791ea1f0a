"""PARITY (GPU): float32 observations of every step and reset kernel against the C oracle, after the reset and after EVERY step
(tests/env_parity.py), beside the same case with float64 observations as the control: the f64 leg separates a defect of the float
instantiation (its 48-byte row pitch and 16-byte word copies, its LDS layout, its own casts) from a defect of the shape.

Every rollout the project measures runs with obs_dtype="f32"; before this file the float instantiations were held to the oracle at
two traces, at the recorded steps, through k_env_grp16<float> with one full group and k_env_grp16x2<float> with 2 of 16 slots.

The table names the kernel every case is about; the GPU test asserts that the dispatch reaches it, and the CPU test at the end walks
the table so that a later change of the dispatch thresholds cannot silently empty one of its rows.  Shapes are the smallest that
reach each path; every batch ends in a partly filled group.
"""
from collections import namedtuple

import pytest

from env_parity import dispatch_kernel, run_parity

Case = namedtuple("Case", "family force J M E B kernel left_shift episodes second_reset")


def _c(family, force, J, M, E, B, kernel, left_shift=True, episodes=1, second_reset="reset"):
    return Case(family, force, J, M, E, B, kernel, left_shift, episodes, second_reset)


def _family(name, forces, shapes, B, variants):
    """every (kernel, shape) of the family once, then the three variants every family has, on `variants` = three (force, shape) pairs:
    left_shift=False; two episodes (the second reset runs over the terminal state: scaler_reset_returns + reset with fresh weights);
    two episodes with the second reset through reset_episode (one launch; the weights it draws go to the oracle)"""
    rows = [_c(name, f, *s, B, k) for f, k in forces for s in shapes]
    kern = dict(forces)
    (f0, s0), (f1, s1), (f2, s2) = variants
    rows.append(_c(name, f0, *s0, B, kern[f0], left_shift=False))
    rows.append(_c(name, f1, *s1, B, kern[f1], episodes=2))
    rows.append(_c(name, f2, *s2, B, kern[f2], episodes=2, second_reset="reset_episode"))
    return rows


J6M6, J8M8, J3M2 = (6, 6, 2), (8, 8, 2), (3, 2, 1)
J10M10, J16M8, J11M11, J7M9, J3M11 = (10, 10, 2), (16, 8, 2), (11, 11, 1), (7, 9, 1), (3, 11, 1)
J5M12, J13M10, J20M15, J20M20 = (5, 12, 2), (13, 10, 2), (20, 15, 3), (20, 20, 4)

CASES = (
    # one task slot per lane (T <= 64, M*M <= 64): J8M8 is T = 64 and M*M = 64, J3M2 has no full block of 8 tasks;
    # B = 19: one full group of 16 + 3, four full groups of 4 + 3
    _family("one_slot", [("grp16", "k_env_grp16"), ("grp4", "k_env_grp4"), ("reg1", "k_env_reg")], [J6M6, J8M8, J3M2], 19,
            [("grp4", J6M6), ("reg1", J6M6), ("grp16", J8M8)])
    # two task slots per lane: T = 100, 128, 121, and the shapes that fail the one-slot test on M*M > 64 only — J7M9 (T = 63,
    # M*M = 81) and J3M11 (T = 33): the second slot of every lane is empty
    + _family("two_slot", [("grp16", "k_env_grp16x2"), ("grp4", "k_env_grp4x2")], [J10M10, J16M8, J11M11, J7M9, J3M11], 19,
              [("grp4", J3M11), ("grp16", J3M11), ("grp4", J7M9)])
    # the grouped LDS kernel forced on register-kernel shapes; B = 11: one full group of 8 + 3
    + _family("lds_forced", [("lds", "k_env_step_grp")], [J6M6, J10M10], 11, [("lds", J6M6), ("lds", J10M10), ("lds", J6M6)])
    # the grouped LDS kernel by the default dispatch: J5M12 (T = 60 but M*M = 144: a single, partly filled wave of tasks),
    # J13M10 (T = 130: pairwise leaves 64 | 66), J20M15 (T = 300: two levels), J20M20 (T = 400: the production shape)
    + _family("lds_default", [(None, "k_env_step_grp")], [J5M12, J13M10, J20M15, J20M20], 11,
              [(None, J5M12), (None, J5M12), (None, J13M10)])
    # one instance per workgroup
    + _family("lds1", [("lds1", "k_env_step")], [J6M6, J20M20], 3, [("lds1", J6M6), ("lds1", J6M6), ("lds1", J6M6)])
)
FAMILIES = ("one_slot", "two_slot", "lds_forced", "lds_default", "lds1")
GROUP = {"k_env_grp16": 16, "k_env_grp16x2": 16, "k_env_grp4": 4, "k_env_grp4x2": 4, "k_env_step_grp": 8}


def _id(c):
    v = "noleftshift" if not c.left_shift else "plain" if c.episodes == 1 else "two_episodes" if c.second_reset == "reset" else "reset_episode"
    return f"{c.family}-{c.force or 'default'}-J{c.J}M{c.M}E{c.E}-B{c.B}-{v}"


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_step_and_reset_equal_the_oracle(case, obs_dtype, monkeypatch):
    c = case
    n = run_parity(c.J, c.M, c.E, c.B, obs_dtype, left_shift=c.left_shift, episodes=c.episodes, seed=3, force=c.force,
                   monkeypatch=monkeypatch, expect_kernel=c.kernel, second_reset=c.second_reset)
    assert n == c.episodes * c.J * c.M


def test_the_table_reaches_every_kernel_in_both_dtypes_and_both_new_routing_edges():
    """no GPU: the dispatch restated by Rollout.env_kernel_name sends every case to the kernel its row names; the rows cover the
    seven step kernels (each runs as <float> and as <double>: fourteen instantiations), end in a partly filled group, and hold the
    two routing edges no other test reaches — the two-slot register kernels and the LDS kernel at T <= 64"""
    for c in CASES:
        assert dispatch_kernel(c.J, c.M, c.B, c.force) == c.kernel, _id(c)
        assert c.M % c.E == 0 and c.B <= 19, _id(c)
        if c.kernel in GROUP:
            assert c.B > GROUP[c.kernel] and c.B % GROUP[c.kernel] != 0, _id(c)       # at least one full group and a ragged last one
    dtypes = ("f32", "f64")                          # the GPU test's parametrisation: every case in both
    reached = {(c.kernel, d) for c in CASES for d in dtypes}
    wanted = {(k, d) for k in ("k_env_grp16", "k_env_grp4", "k_env_grp16x2", "k_env_grp4x2", "k_env_reg", "k_env_step_grp", "k_env_step")
              for d in dtypes}
    assert wanted <= reached, wanted - reached
    for k in ("k_env_grp16x2", "k_env_grp4x2"):      # second task slot of every lane empty
        assert any(c.kernel == k and c.J * c.M <= 64 for c in CASES), k
    # LDS kernel by the default dispatch with a single, partly filled wave of tasks
    assert any(c.kernel == "k_env_step_grp" and c.force is None and c.J * c.M < 64 and c.M * c.M > 128 for c in CASES)
    # the default dispatch of the production shape
    assert any(c.kernel == "k_env_step_grp" and c.force is None and (c.J, c.M, c.E) == (20, 20, 4) for c in CASES)
    for fam in FAMILIES:
        rows = [c for c in CASES if c.family == fam]
        assert any(not c.left_shift for c in rows), fam
        assert any(c.episodes == 2 and c.second_reset == "reset" for c in rows), fam
        assert any(c.episodes == 2 and c.second_reset == "reset_episode" for c in rows), fam
    assert {c.family for c in CASES} == set(FAMILIES)
