"""CPU: which path a GIN forward takes, who pools, and for the streaming path every launch it makes — the library's one statement of the rule
(csrc/mtfjsp_gin_select.h, asked through the handle-free entry mtfjsp_gin_launches_for) against literals written from the code the rule
replaced: the path condition of the two forwards, the heads-pool decision of the job actor's forward and the conditions, launches and
row orders of run_gin as they stood before the header.  256 compute units.  No handle, no device."""
from importlib import import_module

import pytest

import mtfjsp_amd  # noqa: F401
import gin_res_edges as edges

capi = import_module("e2e-mappo-for-mt-fjsp_amd.capi")

SWITCHES = ("MTFJSP_FUSE_PAIR", "MTFJSP_FUSE_GIN0", "MTFJSP_FUSE_POOL", "MTFJSP_NO_STREAM_ORDER", "MTFJSP_STREAM_NT", "MTFJSP_POOL_S",
            "MTFJSP_FUSE_POOL_MAXT", "MTFJSP_NO_RESIDENT_GIN", "MTFJSP_GIN_RES_GENERIC")
X6, P16 = "k_gemm_x6<%s>", "k_gemm16p<%s>"
# (family, kernel, rev, nt, a reduction follows)
MOMENTS = ("gin0_moments", "k_gin0_moments", 0, 0, 1)
GIN0BN = ("gin0_bn_gemm", X6 % "PRO_GIN0BN", 0, 0, 1)
AGG = ("gin_gemm_agg", X6 % "PRO_AGG", 0, 0, 1)
FIXUP = ("cand_fixup", "k_cand_fixup", 0, 0, 0)


def bn(rev, nt, kernel=X6 % "PRO_BNRELU"):
    return ("gin_gemm_bn_relu", kernel, rev, nt, 1)


def stats_only(rev, nt):
    return ("gin_gemm_stats_only", X6 % "PRO_BNRELU", rev, nt, 1)


def pool(rev, nt):
    return ("gin_gemm_pool", X6 % "PRO_BNRELU", rev, nt, 0)


def gin0(family, rev):
    return (family, X6 % "PRO_GIN0", rev, 0, 1)


def gather(nt):
    return ("job_pool_gather", "k_job_pool_gather<%d>" % nt, 0, nt, 0)


# the default forward beyond the single launch: moments, the fused first launch, ..., the last product twice, the candidates' fix-up
DEFAULT = [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), stats_only(0, 0), pool(1, 1), FIXUP]
DEFAULT_FAMILIES = ["gin0_moments", "gin0_bn_gemm", "gin_gemm_bn_relu", "gin_gemm_agg", "gin_gemm_bn_relu", "gin_gemm_stats_only", "gin_gemm_pool", "cand_fixup"]
SINGLE = {"path": "single_launch", "pool": "gin_kernel", "rpr": 0, "pool_grid": 0}


@pytest.fixture
def env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def families(plan):
    return [s[0] for s in plan["steps"]]


def ragged(**kw):
    """J10M10 x 333: 33 300 rows = 2082 tiles of 16 over 256 workgroups, nine tiles (144 rows) in the longest range"""
    return capi.gin_launches_for(333, 10, 10, 256, **kw)


def test_the_default_sequence_at_the_two_streaming_sizes(env):
    for B, J, M in ((8192, 10, 10), (2048, 20, 20)):
        plan = capi.gin_launches_for(B, J, M, 256)
        assert (plan["path"], plan["pool"]) == ("streaming", "epilogue")
        assert families(plan) == DEFAULT_FAMILIES
        assert plan["steps"] == DEFAULT
        critic = capi.gin_launches_for(B, J, M, 256, critic=True)
        assert (critic["path"], critic["pool"], critic["steps"]) == ("streaming", "epilogue", DEFAULT[:-1])


def test_the_headline_size_takes_the_single_launch(env):
    assert capi.gin_launches_for(4096, 6, 6, 256) == dict(SINGLE, steps=[("gin_resident", "k_gin_res_t36j6x16", 0, 0, 0)])
    assert capi.gin_launches_for(4096, 6, 6, 256, critic=True) == dict(SINGLE, steps=[("gin_resident", "k_gin_res", 0, 0, 0)])
    assert capi.gin_launches_for(4096, 6, 6, 256, node_output=True) == dict(SINGLE, steps=[("gin_resident", "k_gin_res", 0, 0, 0)])
    env.setenv("MTFJSP_GIN_RES_GENERIC", "1")
    assert capi.gin_launches_for(4096, 6, 6, 256)["steps"] == [("gin_resident", "k_gin_res", 0, 0, 0)]
    env.setenv("MTFJSP_NO_RESIDENT_GIN", "1")
    assert capi.gin_launches_for(4096, 6, 6, 256)["path"] == "streaming"


def test_the_handle_s_census_a_reduction_and_product_mode_bits_1_8_16_bar_the_single_launch(env):
    heads_pooled = [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1)]          # T = 36: the job actor's heads launch pools
    plan = capi.gin_launches_for(4096, 6, 6, 256, single_ok=False)
    assert (plan["path"], plan["pool"], plan["steps"]) == ("streaming", "heads", heads_pooled)
    assert capi.gin_launches_for(4096, 6, 6, 256, product_mode=16) == plan
    assert capi.gin_launches_for(4096, 6, 6, 256, reduce=True)["path"] == "streaming"
    for bit in (1, 8):
        assert capi.gin_launches_for(4096, 6, 6, 256, product_mode=bit)["path"] == "streaming"
    for bits in (2, 4, 6):
        assert capi.gin_launches_for(4096, 6, 6, 256, product_mode=bits)["path"] == "single_launch"


def test_per_instance_mode_is_the_job_actor_s_alone(env):
    inst = {"path": "per_instance", "pool": "gin_kernel", "rpr": 0, "pool_grid": 0}
    assert capi.gin_launches_for(4096, 6, 6, 256, per_instance=True) == dict(inst, steps=[("gin_inst", "k_gin_inst<float>", 0, 0, 0)])
    assert capi.gin_launches_for(333, 10, 10, 256, per_instance=True, obs_f64=True) == dict(inst, steps=[("gin_inst", "k_gin_inst<double>", 0, 0, 0)])
    assert capi.gin_launches_for(4096, 6, 6, 256, per_instance=True, critic=True)["path"] == "single_launch"
    assert capi.gin_launches_for(333, 10, 10, 256, per_instance=True, critic=True) == capi.gin_launches_for(333, 10, 10, 256, critic=True)


def test_fused_first_launch_from_eight_rows_per_instance(env):
    # T = 7 | 8, the job actor (its heads launch pools)
    seven = capi.gin_launches_for(333, 7, 1, 256)
    assert (seven["pool"], seven["steps"]) == ("heads", [gin0("gin0_agg_linear12", 1), bn(0, 1), bn(1, 1), AGG, bn(1, 1), bn(0, 1)])
    eight = capi.gin_launches_for(333, 4, 2, 256)
    assert (eight["pool"], eight["steps"]) == ("heads", [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1)])


def test_pooling_epilogue_from_sixteen_rows_per_instance(env):
    # T = 15 | 16, the global critic (nobody else pools for it), a handle without the single launch
    fifteen = capi.gin_launches_for(333, 5, 3, 256, critic=True, single_ok=False)
    assert (fifteen["pool"], fifteen["steps"]) == ("pool_gather", [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1), gather(1)])
    assert (fifteen["rpr"], fifteen["pool_grid"]) == (128, 160)               # 4995 rows = 313 tiles over 40 workgroups: 8 tiles each, 4 blocks per range
    sixteen = capi.gin_launches_for(333, 4, 4, 256, critic=True, single_ok=False)
    assert (sixteen["pool"], sixteen["steps"]) == ("epilogue", DEFAULT[:-1])


def test_heads_pool_up_to_64_rows_then_the_epilogue(env):
    # T = 64 | 65, a handle without the single launch
    p64 = capi.gin_launches_for(333, 8, 8, 256, single_ok=False)
    assert (p64["pool"], p64["steps"]) == ("heads", [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1)])
    p65 = capi.gin_launches_for(333, 5, 13, 256, single_ok=False)
    assert (p65["pool"], p65["steps"]) == ("epilogue", DEFAULT)
    for J, M in ((8, 8), (5, 13)):                                              # the global critic takes the epilogue at either
        c = capi.gin_launches_for(333, J, M, 256, critic=True, single_ok=False)
        assert (c["pool"], c["steps"]) == ("epilogue", DEFAULT[:-1])
    env.setenv("MTFJSP_FUSE_POOL_MAXT", "63")
    assert capi.gin_launches_for(333, 8, 8, 256, single_ok=False)["pool"] == "epilogue"


def test_the_single_launch_ends_at_65_rows_per_instance(env):
    assert capi.gin_launches_for(2048, 5, 13, 256) == dict(SINGLE, steps=[("gin_resident", "k_gin_res", 0, 0, 0)])
    p66 = capi.gin_launches_for(2048, 6, 11, 256)
    assert (p66["path"], p66["pool"], p66["steps"]) == ("streaming", "epilogue", DEFAULT)


def test_candidates_that_do_not_divide_the_rows_leave_the_epilogue(env):
    plan = ragged(candidates=7)
    assert (plan["pool"], plan["steps"]) == ("pool_gather", [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1), gather(1)])
    assert (plan["rpr"], plan["pool_grid"]) == (144, 1024)
    assert ragged(candidates=5)["pool"] == "epilogue"


def test_f64_observations_have_no_fused_first_launch(env):
    assert ragged(obs_f64=True)["steps"] == [gin0("gin0_agg_linear12", 1), bn(0, 1), bn(1, 1), AGG, bn(1, 1), stats_only(0, 0), pool(1, 1), FIXUP]


def test_a_reduction_takes_the_sums_of_the_first_linear_not_the_moments(env):
    plan, with_reduce = ragged(), ragged(reduce=True)
    assert with_reduce["steps"] == [gin0("gin0_stats_only", 1)] + DEFAULT[1:]
    assert sum(s[4] for s in with_reduce["steps"]) == sum(s[4] for s in plan["steps"]) == 6


def test_product_mode_bits_one_at_a_time(env):
    b16 = X6 % "PRO_BNRELU"
    f32 = P16 % "PRO_BNRELU"
    # 1: the f32 instruction — no fused first launch, no epilogue, k_gemm16p (the first Linear keeps its exact split)
    assert ragged(product_mode=1)["steps"] == [gin0("gin0_agg_linear12", 1), bn(0, 1, f32), bn(1, 1, f32), ("gin_gemm_agg", P16 % "PRO_AGG", 0, 0, 1),
                                               bn(1, 1, f32), bn(0, 1, f32), gather(1)]
    assert ragged(product_mode=1)["pool"] == "pool_gather"
    # 8: the first Linear on the vector ALU
    assert ragged(product_mode=8)["steps"] == [("gin0_agg_linear12", "k_gin0<float>", 0, 0, 1), bn(0, 1, b16), bn(1, 1), AGG, bn(1, 1),
                                               stats_only(0, 0), pool(1, 1), FIXUP]
    assert ragged(product_mode=8, obs_f64=True)["steps"][0] == ("gin0_agg_linear12", "k_gin0<double>", 0, 0, 1)
    # 16 (and the GAT / heads bits) change nothing in the streaming launches
    for bits in (16, 2, 4):
        assert ragged(product_mode=bits) == ragged()
    assert all(sum(s[4] for s in ragged(product_mode=m)["steps"]) == 6 for m in (0, 1, 8, 9, 16))


def test_node_output_is_written_by_the_gather_kernel(env):
    plan = ragged(node_output=True)
    assert (plan["pool"], plan["steps"]) == ("pool_gather", [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1), gather(1)])
    small = capi.gin_launches_for(7, 4, 6, 256, single_ok=False, node_output=True)
    assert (small["pool"], small["rpr"], small["pool_grid"]) == ("pool_gather", 96, 8)         # 168 rows = 11 tiles over 2 workgroups: 6 tiles each
    assert capi.gin_launches_for(7, 4, 6, 256, single_ok=False)["pool"] == "heads"


def test_ragged_shape_defaults_written_out(env):
    plan = ragged()
    assert plan == {"path": "streaming", "pool": "epilogue", "rpr": 0, "pool_grid": 0, "steps": DEFAULT}


@pytest.mark.parametrize("value,first", [("0", [gin0("gin0_agg_linear12", 1), bn(0, 1)]), ("1", [MOMENTS, GIN0BN]), ("2", [gin0("gin0_stats_only", 1), GIN0BN])])
def test_switch_fuse_gin0(env, value, first):
    env.setenv("MTFJSP_FUSE_GIN0", value)
    assert ragged()["steps"] == first + DEFAULT[2:]


def test_switch_fuse_pool(env):
    env.setenv("MTFJSP_FUSE_POOL", "0")
    plan = ragged()
    assert plan == {"path": "streaming", "pool": "pool_gather", "rpr": 144, "pool_grid": 1024,
                    "steps": [MOMENTS, GIN0BN, bn(1, 1), AGG, bn(1, 1), bn(0, 1), gather(1)]}
    assert ragged(critic=True) == plan                                          # (the kernel's J is an argument, not another launch)
    env.setenv("MTFJSP_FUSE_POOL", "1")
    assert ragged()["steps"] == DEFAULT


def test_switch_fuse_pair(env):
    pair = [gin0("gin0_agg_linear12", 1), stats_only(0, 1), ("gin_gemm_pair", "k_gemm_x6f", 1, 1, 1), AGG, stats_only(1, 1), ("gin_gemm_pair", "k_gemm_x6f", 0, 1, 1),
            gather(1)]
    env.setenv("MTFJSP_FUSE_PAIR", "1")
    plan = ragged()
    assert plan == {"path": "streaming", "pool": "pool_gather", "rpr": 144, "pool_grid": 1024, "steps": pair}
    assert capi.gin_launches_for(7, 4, 6, 256, single_ok=False)["steps"] == pair[:-1]          # (the heads launch pools behind a pair too)
    assert ragged(product_mode=1)["steps"][1][0] == "gin_gemm_bn_relu"                         # split products only
    env.setenv("MTFJSP_FUSE_PAIR", "0")
    assert ragged()["steps"] == DEFAULT
    # -1: where the activation matrix ([rows,128] f32) exceeds the 256 MB memory-side cache — 524 288 rows
    env.setenv("MTFJSP_FUSE_PAIR", "-1")
    assert ragged()["steps"] == DEFAULT
    assert capi.gin_launches_for(5242, 10, 10, 256)["steps"] == DEFAULT                       # 524 200 rows
    assert capi.gin_launches_for(5243, 10, 10, 256)["steps"] == pair                          # 524 300 rows
    assert capi.gin_launches_for(8192, 10, 10, 256)["steps"] == pair


def test_switch_no_stream_order(env):
    env.setenv("MTFJSP_NO_STREAM_ORDER", "1")
    assert ragged()["steps"] == [MOMENTS, GIN0BN, bn(0, 0), AGG, bn(0, 0), stats_only(0, 0), pool(0, 0), FIXUP]
    env.setenv("MTFJSP_FUSE_GIN0", "0")
    env.setenv("MTFJSP_FUSE_POOL", "0")
    assert ragged() == {"path": "streaming", "pool": "pool_gather", "rpr": 0, "pool_grid": 333,     # plain instance order: a workgroup per instance
                        "steps": [gin0("gin0_agg_linear12", 0), bn(0, 0), bn(0, 0), AGG, bn(0, 0), bn(0, 0), gather(0)]}
    assert capi.gin_launches_for(8192, 10, 10, 256)["pool_grid"] == 2048                            # ... up to eight per compute unit


def test_switch_stream_nt(env):
    agg_nt = ("gin_gemm_agg", X6 % "PRO_AGG", 0, 1, 1)
    env.setenv("MTFJSP_STREAM_NT", "2")
    assert ragged()["steps"] == [MOMENTS, GIN0BN, bn(1, 0), agg_nt, bn(1, 0), stats_only(0, 0), pool(1, 0), FIXUP]
    env.setenv("MTFJSP_FUSE_POOL", "0")
    assert ragged()["steps"] == [MOMENTS, GIN0BN, bn(1, 0), agg_nt, bn(1, 0), bn(0, 0), gather(0)]
    env.setenv("MTFJSP_STREAM_NT", "7")
    assert ragged()["steps"] == [MOMENTS, GIN0BN, bn(1, 1), agg_nt, bn(1, 1), bn(0, 1), gather(1)]
    env.setenv("MTFJSP_STREAM_NT", "0")
    plan = ragged()
    assert plan["steps"] == [MOMENTS, GIN0BN, bn(1, 0), AGG, bn(1, 0), bn(0, 0), gather(0)]
    assert (plan["rpr"], plan["pool_grid"]) == (144, 1024)


def test_switch_pool_s(env):
    env.setenv("MTFJSP_FUSE_POOL", "0")
    for value, expect in (("0", (0, 333)), ("1", (144, 256)), ("2", (144, 512)), ("4", (144, 1024))):
        env.setenv("MTFJSP_POOL_S", value)
        plan = ragged()
        assert (plan["rpr"], plan["pool_grid"]) == expect
        assert plan["steps"][-1] == gather(1)


EXTRA = [(4096, 3, 3), (4096, 10, 10), (8192, 6, 6), (4096, 6, 6), (3856, 6, 6), (16, 6, 6)]


@pytest.mark.parametrize("B,J,M", [(c[0][3], c[0][0], c[0][1]) for c in edges.CASES] + EXTRA)
def test_the_path_follows_the_single_launch_kernel_s_eligibility(env, B, J, M):
    for critic in (False, True):
        kernel = capi.gin_res_kernel_for(B, J, M, 256, candidates=0 if critic else J)[0]
        plan = capi.gin_launches_for(B, J, M, 256, critic=critic)
        if kernel is None:
            assert plan["path"] == "streaming"
        else:
            assert plan == dict(SINGLE, steps=[("gin_resident", kernel, 0, 0, 0)])
    assert capi.gin_launches_for(B, J, M, 128)["path"] == ("single_launch" if capi.gin_res_kernel_for(B, J, M, 128)[0] else "streaming")


def test_sizes_out_of_range_have_no_plan(env):
    assert capi.gin_launches_for(0, 6, 6, 256) is None
    assert capi.gin_launches_for(16, 6, 6, 0) is None
    assert capi.gin_launches_for(16, 6, 6, 256, product_mode=32) is None
