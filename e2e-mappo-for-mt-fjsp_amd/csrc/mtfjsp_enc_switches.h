// mtfjsp_enc_switches.h — the run-time switches of the encoder unit (mtfjsp_encoder.hip), stated ONCE: every environment variable that steers a plan or a
// launch has its name, its default and what it changes on ONE line here, and nothing else in the unit reads the environment for them.  The table of
// DESIGN.md ("Encoder switches") lists the same names and defaults (tests/test_enc_switches_cpu.py holds the two together).  Plain C++17, no HIP header;
// included by mtfjsp_encoder.hip only.
//
// When a switch is read:
//   * Create-time — every field of EncSwitches.  enc_switches_read() runs once in mtfjsp_encoder_create, into e->sw, and the handle keeps those values
//     for life.  What the device does not grant lowers three of them there, after the read: sw.fuse_pair, sw.heads10, sw.fuse_mheads.  sw.f32_products
//     is only the INITIAL product mode: the handle's own f32_products is what mtfjsp_encoder_set_product_mode and the range fallback change.
//     The handle-free entries (mtfjsp_gin_launches_for, mtfjsp_heads_kernel_name_for, mtfjsp_fused3_kernel_name_for) read a fresh EncSwitches per call.
//   * Per forward / per call — enc_gin_res_generic(), enc_fused3_generic(): as the variable is NOW, by the forwards and the handle-free entries alike.
//     enc_no_resident_gin(): at create, at every mtfjsp_encoder_check that could bring the single launch back, and per call of mtfjsp_gin_launches_for.
//   * MTFJSP_FUSE_POOL_MAXT — the one oddity: handles take it once per PROCESS (enc_heads_pool_maxT_once, at the first GIN forward of any handle),
//     mtfjsp_gin_launches_for per call like the rest (include/mtfjsp.h documents it, tests/test_gin_select_cpu.py relies on the per-call half).
//   * Left where they are used, beside or behind compile-time diagnostics: MTFJSP_STAMP_PRINT (every use), MTFJSP_GEMM_DBG (once per process).
#pragma once
#include <stdlib.h>
#include "mtfjsp_gin_select.h"
#include "mtfjsp_heads_select.h"

static inline bool sw_set(const char *name) { return getenv(name) != nullptr; }
static inline int sw_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
static inline long long sw_ll(const char *name, long long dflt) { const char *v = getenv(name); return v ? atoll(v) : dflt; }
static inline double sw_f64(const char *name, double dflt) { const char *v = getenv(name); return v ? atof(v) : dflt; }

// The values of one reading of the environment (the initialisers ARE the reading: make one through enc_switches_read() only).
struct EncSwitches {
    // which products run with the f32 matrix instruction instead of the exact bf16 split (A/B reference; bits: 1 GIN products,
    // 2 GAT passes, 4 heads, 8 first GIN Linear on the VALU): the product mode a handle starts with
    int f32_products = (sw_set("MTFJSP_GEMM_F32MFMA") ? 1 : 0) | (sw_set("MTFJSP_GAT_F32MFMA") ? 2 : 0) |
                       (sw_set("MTFJSP_HEADS_F32MFMA") ? 4 : 0) | (sw_set("MTFJSP_GIN0_VALU") ? 8 : 0);
    bool fuse_gat = !sw_set("MTFJSP_NO_FUSED_GAT");                // the machine path's GAT passes in the job actor's heads launch
    bool fuse_mheads = !sw_set("MTFJSP_NO_FUSED_MHEADS");          // the machine heads in the job heads + GAT launch behind an in-launch exchange of the node statistics (three launches per rollout step)
    bool heads_hg8 = !sw_set("MTFJSP_NO_HEADS_HG8");               // groups of 8 instances in k_headsx when groups of 16 fill at most half the CUs
    bool heads10 = !sw_set("MTFJSP_NO_HEADS10");                   // k_headsx10 (ten tiles per chunk) for groups of 7..10 tiles
    // the environment step as the tail of the machine heads' launch (mtfjsp_encoder_arm_env_step).  OFF unless MTFJSP_FUSED_ENV is set:
    // bit-identical (tests/test_fused_env_step_gpu.py) and one launch less per step, but measured SLOWER at the headline shape —
    // 220.4 against 217.6 us per step, three alternating runs on one box — because the heads' 8 waves take the 16 instances in two
    // rounds where k_env_grp16's 16 waves take them in one: the second round costs more than the launch boundary saves
    bool fuse_env = sw_set("MTFJSP_FUSED_ENV");
    // Round 6: the step as the tail of the THREE-in-one launch (k_headsx_gat3x_headsx<1|2>) with its state lines requested 13 us ahead:
    // two launches per rollout step, bit-identical (tests/test_fused_env_step_gpu.py).  OFF unless MTFJSP_FUSED_ENV3 is set: measured
    // SLOWER again — 0.1772-0.1786 against 0.1750-0.1751 ms per step, three alternating runs on one box (tools/ab_bench_env3.sh,
    // profiles/r06_ab_env3.txt): the launch's 8 waves take the 16 instances in two rounds behind one another, which costs about 3 us
    // more than the launch boundary and the separate kernel's dispatch ramp together, warm state lines or not.
    bool fuse_env3 = sw_set("MTFJSP_FUSED_ENV3");
    bool nodes_lds = !sw_set("MTFJSP_FUSED3_NODES_HBM");           // three-in-one launch: the GAT part's node rows stay in LDS for the machine part (round 6)
    bool warm_heads = !sw_set("MTFJSP_NO_WARM_HEADS");             // k_gin_res requests the heads launch's weight lines in its last phase
    // streaming GIN launches: the two inner Linears of an MLP in one launch behind a statistics-only pass (mtfjsp_gemm_pair.h).
    // MTFJSP_FUSE_PAIR=1: always; -1: where the activation matrix exceeds the 256 MB memory-side cache; 0 (default): never —
    // measured (round 5, J10M10 x 8192 / J20M20 x 2048): statistics-only pass 102 us + pair launch 203 us against 2 x 148 us for the two
    // launches: a consumer wave runs BOTH products of a step's four tiles back to back (8 tile products, ~10 k cycles per step) and
    // is the critical path; the 25 % of HBM traffic saved does not show because these launches are bound by the SIMDs' instruction
    // issue (~100 us per launch even with no output at all), not by memory
    int fuse_pair = sw_int("MTFJSP_FUSE_PAIR", 0);
    int stream_order = sw_set("MTFJSP_NO_STREAM_ORDER") ? 0 : 1;   // streaming GIN launches: alternating row direction + non-temporal input reads (A/B switch)
    // (what each of these switches changes in a forward's launches: gin_plan, mtfjsp_gin_select.h — this struct only holds their values)
    int fuse_pool = sw_int("MTFJSP_FUSE_POOL", 1);                 // the last Linear's output pooled / gathered in a second pass' epilogue instead of stored
    int fuse_gin0 = sw_int("MTFJSP_FUSE_GIN0", 1);                 // the first Linear's output formed again by the second launch's producers instead of stored
    int pool_s = sw_int("MTFJSP_POOL_S", 4);                       // k_job_pool_gather: blocks per row range of the last product (0: plain instance order)
    int stream_nt = sw_int("MTFJSP_STREAM_NT", 5);                 // which readers use non-temporal loads: 1 BatchNorm+ReLU products, 2 aggregation product, 4 pool / gather
    int heads_pool_maxT = sw_int("MTFJSP_FUSE_POOL_MAXT", 64);     // the job actor's heads launch pools up to this many rows per instance (J10M10 x 8192: 264 us pooled in the heads launch, 240 us apart); handles: enc_heads_pool_maxT_once
    // diagnostics (tests)
    long long res_fail_at = sw_ll("MTFJSP_GIN_RES_FAIL_AT", 0);    // this single-launch forward's barriers time out
    long long range_fail_at = sw_ll("MTFJSP_RANGE_FAIL_AT", 0);    // the n-th job-actor forward raises the range word (as a NaN output would)
    long long fused3_fail_at = sw_ll("MTFJSP_FUSED3_FAIL_AT", 0);  // this three-in-one launch waits for a workgroup that does not exist
    double xchg_fine_limit = sw_f64("MTFJSP_XCHG_FINE_LIMIT", 2147483648.0);   // a lower limit sends ordinary contributions through the wide-range words
};
static inline EncSwitches enc_switches_read() { return EncSwitches{}; }

// read at every use
static inline const char *enc_gin_res_generic() { return getenv("MTFJSP_GIN_RES_GENERIC"); }   // a value other than 0 forces the run-time k_gin_res where the fixed-shape one would serve
static inline const char *enc_fused3_generic() { return getenv("MTFJSP_FUSED3_GENERIC"); }     // the same for the three-in-one heads launch
static inline bool enc_no_resident_gin() { return sw_set("MTFJSP_NO_RESIDENT_GIN"); }          // no single-launch GIN kernel: every handle takes the streaming launches
// handles only: the first reading of the process holds
static inline int enc_heads_pool_maxT_once() { static const int v = enc_switches_read().heads_pool_maxT; return v; }

// The ONE mapping from the switches to a request's switch fields: a handle passes e->sw (and then takes heads_pool_maxT from enc_heads_pool_maxT_once), a
// handle-free entry a fresh enc_switches_read(); each caller sets the shape and its own answers besides.
static inline void gin_request_switches(GinRequest &q, const EncSwitches &sw)
{
    q.fuse_pair = sw.fuse_pair; q.fuse_gin0 = sw.fuse_gin0; q.fuse_pool = sw.fuse_pool;
    q.stream_order = sw.stream_order; q.stream_nt = sw.stream_nt; q.pool_s = sw.pool_s; q.heads_pool_maxT = sw.heads_pool_maxT;
    q.force_generic = enc_gin_res_generic();
}
static inline void heads_request_switches(HeadsRequest &q, const EncSwitches &sw)
{
    q.hg8 = sw.heads_hg8; q.heads10 = sw.heads10; q.nodes_hbm = !sw.nodes_lds;
    q.force_generic = enc_fused3_generic();
}
static inline Fused3Plan fused3_plan_switches(int B, int J, int M, int T, int num_cu, bool obs_f64, bool env_tail, const EncSwitches &sw)
{
    return fused3_plan(B, J, M, T, num_cu, obs_f64, sw.nodes_lds ? nullptr : "1", env_tail, enc_fused3_generic());
}
