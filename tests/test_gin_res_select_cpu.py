"""CPU: which instantiation of the single-launch GIN kernel serves a forward — the library's one statement of the rule
(csrc/mtfjsp_gin_res_select.h, asked through the handle-free entry mtfjsp_gin_res_kernel_name_for).  The fixed-shape instantiation
(T = 36, J = 6, 16 instances in every workgroup, no node output) serves exactly that shape; everything else eligible runs the
run-time kernel; MTFJSP_GIN_RES_GENERIC=1 forces the run-time kernel.  No handle, no device."""
from importlib import import_module

import pytest

import mtfjsp_amd  # noqa: F401

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")
FIXED, GENERIC = "k_gin_res_t36j6x16", "k_gin_res"


@pytest.fixture
def no_switch(monkeypatch):
    monkeypatch.delenv("MTFJSP_GIN_RES_GENERIC", raising=False)
    return monkeypatch


# (batch, n_job, n_machine, node output requested) -> kernel, instances per workgroup, workgroups; 256 compute units
TABLE = [
    ((4096, 6, 6, False), (FIXED, 16, 256)),
    ((3856, 6, 6, False), (FIXED, 16, 241)),            # 241 full workgroups
    ((4095, 6, 6, False), (GENERIC, 16, 256)),          # partial last workgroup
    ((4096, 6, 6, True), (GENERIC, 16, 256)),           # node output requested
    ((4096, 5, 7, False), (GENERIC, 16, 256)),          # T = 35 (and J = 5)
    ((4096, 7, 5, False), (GENERIC, 16, 256)),          # T = 35 (J = 7)
    ((2048, 6, 6, False), (GENERIC, 8, 256)),           # 8 instances per workgroup
    ((16, 6, 6, False), (GENERIC, 1, 16)),
    ((9216, 4, 4, False), (GENERIC, 36, 256)),          # T = 16, the fewest rows per instance: 36 instances = 576 rows per workgroup
    ((2048, 5, 13, False), (GENERIC, 8, 256)),          # T = 65, the most (tests/gin_res_edges.py has the shapes in between)
]


@pytest.mark.parametrize("shape,expect", TABLE)
def test_the_rule_over_the_case_table(no_switch, shape, expect):
    B, J, M, nodes = shape
    assert capi.gin_res_kernel_for(B, J, M, 256, node_output=nodes) == expect


def test_a_forward_with_other_candidates_than_six_per_instance_runs_the_run_time_kernel(no_switch):
    # T = 36 with J = 5 candidates per instance asked for (and none: the global critic's forward)
    assert capi.gin_res_kernel_for(4096, 6, 6, 256, candidates=5)[0] == GENERIC
    assert capi.gin_res_kernel_for(4096, 6, 6, 256, candidates=0)[0] == GENERIC
    assert capi.gin_res_kernel_for(4096, 6, 6, 256, candidates=6)[0] == FIXED


def test_the_switch_forces_the_run_time_kernel_and_is_read_per_call(no_switch):
    assert capi.gin_res_kernel_for(4096, 6, 6, 256)[0] == FIXED
    no_switch.setenv("MTFJSP_GIN_RES_GENERIC", "1")
    assert capi.gin_res_kernel_for(4096, 6, 6, 256) == (GENERIC, 16, 256)
    assert capi.gin_res_kernel_for(3856, 6, 6, 256) == (GENERIC, 16, 241)
    no_switch.setenv("MTFJSP_GIN_RES_GENERIC", "0")
    assert capi.gin_res_kernel_for(4096, 6, 6, 256)[0] == FIXED
    no_switch.delenv("MTFJSP_GIN_RES_GENERIC")
    assert capi.gin_res_kernel_for(4096, 6, 6, 256)[0] == FIXED


def test_both_names_keep_the_prefix_the_profile_readers_match_on():
    assert FIXED.startswith(GENERIC)


def test_shapes_outside_the_single_launch_have_no_kernel(no_switch):
    assert capi.gin_res_kernel_for(4096, 3, 3, 256)[0] is None             # T = 9 < 16
    assert capi.gin_res_kernel_for(4096, 10, 10, 256)[0] is None           # T = 100 > 65
    assert capi.gin_res_kernel_for(8192, 6, 6, 256)[0] is None             # 32 instances x 36 rows > 576 rows per workgroup
    # fewer compute units: 4096 instances no longer fit one workgroup per unit
    assert capi.gin_res_kernel_for(4096, 6, 6, 128)[0] is None
