"""CPU: which heads kernel serves an actor forward, with which group size and grid — the library's one statement of the rule
(csrc/mtfjsp_heads_select.h, asked through the handle-free entry mtfjsp_heads_kernel_name_for) on 256 compute units, against literals: every
launch form tests/test_selection_exact_gpu.py runs on the device, the groups of 8 instances, and each boundary of the rule from both sides.
No handle, no device."""
import os
import sys
from importlib import import_module

import pytest

import mtfjsp_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_selection_exact_gpu import CASES, _asks, _case_id  # noqa: E402

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
X, X10, GAT, ENV, VAL, F32 = "k_headsx", "k_headsx10", "k_headsx_gat3x", "k_headsx_envstep", "k_headsx_values", "k_heads"
THREE = "k_headsx_gat3x_headsx"
FIXED = "k_headsx_gat3x_headsx<0, true, H3ShapeFixed<6, 6, 16>>"
SWITCHES = ("MTFJSP_NO_HEADS_HG8", "MTFJSP_NO_HEADS10", "MTFJSP_FUSED3_NODES_HBM", "MTFJSP_FUSED3_GENERIC")


@pytest.fixture
def no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def ask(B, J, M, **kw):
    return capi.heads_kernel_for(B, J, M, num_cu=kw.pop("num_cu", 256), **kw)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_launch_form_of_the_device_test(no_switch, case):
    (J, M, E, B), env, mode, forms = case
    for k, v in env.items():
        if k in SWITCHES:
            no_switch.setenv(k, v)
    stepping = forms[1] in (ENV, "three_in_one_env")
    job, mach = _asks(env, mode, stepping)
    kj, km = ask(B, J, M, **job)[0], ask(B, J, M, **mach)[0]
    if forms[0].startswith("three_in_one"):
        assert kj == (FIXED if (J, M, B) == (6, 6, 4096) and not stepping else THREE)        # (the machine forward is that launch)
        assert ask(B, J, M, **job)[1:] == (16, B // 16)
    else:
        assert (kj, km) == forms


def test_groups_of_eight_where_nothing_rides_and_half_the_units_would_idle(no_switch):
    assert ask(7, 3, 4) == (X, 8, 1) and ask(7, 3, 4, which=1) == (X, 8, 1)
    assert ask(333, 6, 6) == (X, 8, 42) and ask(333, 6, 6, which=1) == (X, 8, 42)
    assert ask(96, 10, 10) == (X, 8, 12) and ask(96, 10, 10, which=1) == (X, 8, 12)           # (5 tiles per group of 8)
    assert ask(96, 10, 10, values_only=True) == (VAL, 8, 12)                                    # the values alone are no ride
    # something rides: groups of 16
    assert ask(96, 10, 10, which=1, env_tail=True) == (ENV, 16, 6)
    assert ask(336, 6, 4, gat=True) == (GAT, 16, 21)
    assert ask(4096, 6, 6, gat=True, mheads=True) == (FIXED, 16, 256)
    assert ask(333, 6, 6, f32=True) == (F32, 16, 21)
    no_switch.setenv("MTFJSP_NO_HEADS_HG8", "1")
    assert ask(7, 3, 4) == (X, 16, 1)
    assert ask(333, 6, 6) == (X, 16, 21)
    assert ask(96, 10, 10) == (X10, 16, 6) and ask(96, 10, 10, values_only=True) == (VAL, 16, 6)


def test_groups_of_eight_end_where_twice_the_groups_of_16_exceed_the_units(no_switch):
    assert ask(2048, 6, 6) == (X, 8, 256)                                                      # 2 * 128 == 256
    assert ask(2049, 6, 6) == (X, 16, 129)                                                     # 2 * 129 > 256
    assert ask(2048, 6, 6, num_cu=255) == (X, 16, 128)
    assert ask(2049, 6, 6, num_cu=258) == (X, 8, 257)


@pytest.mark.parametrize("rows,kernel", [(6, X), (7, X10), (10, X10), (11, X)])
def test_ten_tiles_per_chunk_for_full_groups_of_7_to_10_tiles(no_switch, rows, kernel):
    # groups of 16 (a batch that fills the device): a full group has `rows` tiles; groups of 8: ceil(rows / 2) — 2 rows - 1 and 2 rows tiles' worth of rows
    assert ask(4095, rows, 4) == (kernel, 16, 256) and ask(4095, 4, rows, which=1) == (kernel, 16, 256)
    assert ask(24, 2 * rows, 4) == (kernel, 8, 3) and ask(24, 2 * rows - 1, 4) == (kernel, 8, 3)
    no_switch.setenv("MTFJSP_NO_HEADS10", "1")
    assert ask(4095, rows, 4)[0] == X and ask(24, 2 * rows, 4)[0] == X


def test_the_gat_passes_ride_on_whole_groups_in_one_round_as_wide_as_their_own_grid(no_switch):
    # M = 4: B / 2 row tiles, a GAT grid of B / 16 — every whole number of groups up to one round rides
    assert ask(4080, 8, 4, gat=True) == (GAT, 16, 255)
    assert ask(4095, 8, 4, gat=True) == (X10, 16, 256)                                          # not whole groups of 16
    assert ask(4096, 8, 4, gat=True) == (GAT, 16, 256)
    assert ask(4112, 8, 4, gat=True) == (X10, 16, 257)                                          # a second round of workgroups
    # M = 6: the GAT launch would fill all 256 units from B = 2731: only 4096 is as wide
    assert ask(4080, 6, 6, gat=True) == (X, 16, 255)
    assert ask(4096, 6, 6, gat=True) == (GAT, 16, 256)
    # asked for or not, allowed or not
    assert ask(4096, 6, 6) == (X, 16, 256)
    assert ask(4096, 6, 6, gat=True, gat_ok=False) == (X, 16, 256)
    assert ask(4096, 6, 6, gat=True, mheads=True, gat_ok=False) == (X, 16, 256)
    assert ask(4096, 6, 6, gat=True, f32=True) == (F32, 16, 256)
    assert ask(4096, 6, 6, which=1, env_tail=True, f32=True) == (F32, 16, 256)


def test_the_machine_heads_ride_with_at_most_eight_machines(no_switch):
    assert ask(4096, 4, 8, gat=True, mheads=True) == (THREE, 16, 256)
    assert ask(4096, 4, 9, gat=True, mheads=True) == (GAT, 16, 256)
    assert ask(4096, 4, 8, gat=True, mheads=True, mheads_ok=False) == (GAT, 16, 256)
    assert ask(4096, 4, 8, gat=True) == (GAT, 16, 256)
    assert ask(4096, 4, 8, mheads=True) == (X, 16, 256)                                         # (no machine heads without the GAT passes)
    # an environment tail rides behind the machine selection: not in a launch that carries the GAT passes alone
    assert ask(4096, 4, 8, gat=True, mheads=True, env_tail=True) == (THREE, 16, 256)
    assert ask(4096, 4, 9, gat=True, mheads=True, env_tail=True) == (GAT, 16, 256)
    assert ask(4096, 4, 8, which=1, env_tail=True) == (ENV, 16, 256)


def test_each_switch_is_read_per_call(no_switch):
    assert ask(7, 3, 4)[1] == 8
    no_switch.setenv("MTFJSP_NO_HEADS_HG8", "1")
    assert ask(7, 3, 4)[1] == 16
    no_switch.delenv("MTFJSP_NO_HEADS_HG8")
    assert ask(7, 3, 4)[1] == 8
    assert ask(19, 16, 4)[0] == X10
    no_switch.setenv("MTFJSP_NO_HEADS10", "1")
    assert ask(19, 16, 4)[0] == X
    no_switch.delenv("MTFJSP_NO_HEADS10")
    assert ask(19, 16, 4)[0] == X10
    for k in ("MTFJSP_FUSED3_NODES_HBM", "MTFJSP_FUSED3_GENERIC"):
        assert ask(4096, 6, 6, gat=True, mheads=True)[0] == FIXED
        no_switch.setenv(k, "1")
        assert ask(4096, 6, 6, gat=True, mheads=True)[0] == THREE
        no_switch.delenv(k)
    assert ask(4096, 6, 6, gat=True, mheads=True)[0] == FIXED


@pytest.mark.parametrize("shape", [(6, 6), (4, 8), (7, 5), (8, 4)])
@pytest.mark.parametrize("obs_f64", [False, True])
@pytest.mark.parametrize("env_tail", [False, True])
def test_the_three_in_one_name_is_the_one_its_own_rule_gives(no_switch, shape, obs_f64, env_tail):
    j, m = shape
    for generic in (None, "1"):
        if generic:
            no_switch.setenv("MTFJSP_FUSED3_GENERIC", generic)
        name, grid = capi.fused3_kernel_for(4096, j, m, 256, obs_f64=obs_f64, env_tail=env_tail)
        assert name is not None and ask(4096, j, m, gat=True, mheads=True, obs_f64=obs_f64, env_tail=env_tail) == (name, 16, grid)


def test_sizes_below_one_have_no_kernel():
    assert ask(0, 6, 6)[0] is None and ask(16, 0, 6)[0] is None and ask(16, 6, 0, which=1)[0] is None and ask(16, 6, 6, num_cu=0)[0] is None
