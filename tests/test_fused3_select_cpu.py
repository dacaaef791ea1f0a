"""CPU: which instantiation of the three-in-one heads launch (k_headsx_gat3x_headsx) serves a rollout step — the library's one statement of the
rule (csrc/mtfjsp_fused3_select.h, asked through the handle-free entry mtfjsp_fused3_kernel_name_for).  The fixed-shape instantiation serves
exactly J6M6 x 4096 on 256 compute units with f32 observations, node rows in LDS and no environment tail; everything else the launch is eligible
for runs the run-time kernel; MTFJSP_FUSED3_GENERIC=1 forces the run-time kernel; where the launch is not eligible the answer is None.
No handle, no device."""
from importlib import import_module

import pytest

import mtfjsp_amd  # noqa: F401

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
GENERIC = "k_headsx_gat3x_headsx"
FIXED = "k_headsx_gat3x_headsx<0, true, H3ShapeFixed<6, 6, 16>>"


@pytest.fixture
def no_switch(monkeypatch):
    monkeypatch.delenv("MTFJSP_FUSED3_GENERIC", raising=False)
    monkeypatch.delenv("MTFJSP_FUSED3_NODES_HBM", raising=False)
    return monkeypatch


def test_the_headline_shape_takes_the_fixed_instantiation(no_switch):
    assert capi.fused3_kernel_for(4096, 6, 6, 256) == (FIXED, 256)


@pytest.mark.parametrize("shape", [(4, 8), (7, 5), (8, 4)])
def test_neighbouring_shapes_at_4096_run_the_run_time_kernel(no_switch, shape):
    j, m = shape
    assert capi.fused3_kernel_for(4096, j, m, 256) == (GENERIC, 256)


def test_another_batch_runs_the_run_time_kernel(no_switch):
    # J6M6 on 256 compute units is eligible at B = 4096 only (B / 16 >= min(12 B / 128, CUs) and B / 16 <= CUs); on 128 units it is at B = 2048, and
    # with M = 4 (8 B / 128 = B / 16 row-tile groups) every multiple of 16 up to 4096 is
    assert capi.fused3_kernel_for(2048, 6, 6, 128) == (GENERIC, 128)
    assert capi.fused3_kernel_for(4096, 6, 6, 128)[0] is None
    assert capi.fused3_kernel_for(2048, 8, 4, 256) == (GENERIC, 128)
    assert capi.fused3_kernel_for(4080, 8, 4, 256) == (GENERIC, 255)


def test_f64_observations_hbm_nodes_and_an_environment_tail_run_the_run_time_kernel(no_switch):
    assert capi.fused3_kernel_for(4096, 6, 6, 256, obs_f64=True)[0] == GENERIC
    assert capi.fused3_kernel_for(4096, 6, 6, 256, env_tail=True)[0] == GENERIC
    assert capi.fused3_kernel_for(4096, 6, 6, 256, obs_f64=True, env_tail=True)[0] == GENERIC
    no_switch.setenv("MTFJSP_FUSED3_NODES_HBM", "1")
    assert capi.fused3_kernel_for(4096, 6, 6, 256)[0] == GENERIC
    no_switch.delenv("MTFJSP_FUSED3_NODES_HBM")
    assert capi.fused3_kernel_for(4096, 6, 6, 256)[0] == FIXED


def test_the_switch_forces_the_run_time_kernel_and_is_read_per_call(no_switch):
    assert capi.fused3_kernel_for(4096, 6, 6, 256)[0] == FIXED
    no_switch.setenv("MTFJSP_FUSED3_GENERIC", "1")
    assert capi.fused3_kernel_for(4096, 6, 6, 256) == (GENERIC, 256)
    no_switch.setenv("MTFJSP_FUSED3_GENERIC", "0")
    assert capi.fused3_kernel_for(4096, 6, 6, 256)[0] == FIXED
    no_switch.delenv("MTFJSP_FUSED3_GENERIC")
    assert capi.fused3_kernel_for(4096, 6, 6, 256)[0] == FIXED


def test_both_names_keep_the_prefix_the_profile_readers_match_on():
    assert FIXED.startswith(GENERIC)


def test_shapes_the_launch_is_not_eligible_for_have_no_kernel(no_switch):
    assert capi.fused3_kernel_for(4095, 6, 6, 256)[0] is None              # not whole groups of 16 instances
    assert capi.fused3_kernel_for(8192, 6, 6, 256)[0] is None              # two rounds of workgroups
    assert capi.fused3_kernel_for(2048, 6, 6, 256)[0] is None              # fewer workgroups than the GAT launch's own grid
    assert capi.fused3_kernel_for(8192, 10, 10, 256)[0] is None
    assert capi.fused3_kernel_for(2048, 20, 20, 256)[0] is None
    assert capi.fused3_kernel_for(4096, 4, 9, 256)[0] is None              # more than 8 machines
