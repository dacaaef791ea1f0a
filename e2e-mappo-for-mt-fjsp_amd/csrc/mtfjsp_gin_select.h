// mtfjsp_gin_select.h — which path a GIN forward takes (per-instance kernel, single launch, streaming launches), which of the pooling forms serves it,
// and for the streaming path every launch it makes, in order, stated ONCE: both forwards of mtfjsp_encoder.hip build this plan and run_gin only
// executes its steps; mtfjsp_encoder_check asks gin_single_launch_ok; mtfjsp_gin_launches_for reports the plan without a GPU.  Plain C++17, no HIP
// header: a host-only program can include it.
#pragma once
#include <stddef.h>
#include "mtfjsp_gin_res_select.h"

enum GinPath { GIN_PATH_INST = 0, GIN_PATH_SINGLE, GIN_PATH_STREAM, GIN_PATH_COUNT };
static const char *const GIN_PATH_NAME[GIN_PATH_COUNT] = {"per_instance", "single_launch", "streaming"};
// who forms the graph mean pool and the candidates' rows
enum GinPool {
    GIN_POOL_KERNEL = 0,                  // the per-instance / single-launch kernel itself
    GIN_POOL_HEADS,                       // the job actor's heads launch: BatchNorm + ReLU, pool and gather of the last product's stored output
    GIN_POOL_EPILOGUE,                    // the epilogue of a second pass of the last product (+ k_cand_fixup): that product's output is never stored
    GIN_POOL_GATHER,                      // k_job_pool_gather behind the last product
    GIN_POOL_COUNT
};
static const char *const GIN_POOL_NAME[GIN_POOL_COUNT] = {"gin_kernel", "heads", "epilogue", "pool_gather"};

enum GinKernel {
    GIN_K_INST_F32 = 0, GIN_K_INST_F64, GIN_K_RES,                 // (GIN_K_RES: the instantiation GinPlan::res names)
    GIN_K_X6_GIN0, GIN_K_X6_GIN0BN, GIN_K_X6_BNRELU, GIN_K_X6_AGG, GIN_K_16P_BNRELU, GIN_K_16P_AGG,
    GIN_K_GIN0_F32, GIN_K_GIN0_F64, GIN_K_MOMENTS, GIN_K_X6F, GIN_K_FIXUP, GIN_K_GATHER, GIN_K_GATHER_NT, GIN_K_COUNT
};
static const char *const GIN_KERNEL_NAME[GIN_K_COUNT] = {
    "k_gin_inst<float>", "k_gin_inst<double>", "k_gin_res",
    "k_gemm_x6<PRO_GIN0>", "k_gemm_x6<PRO_GIN0BN>", "k_gemm_x6<PRO_BNRELU>", "k_gemm_x6<PRO_AGG>", "k_gemm16p<PRO_BNRELU>", "k_gemm16p<PRO_AGG>",
    "k_gin0<float>", "k_gin0<double>", "k_gin0_moments", "k_gemm_x6f", "k_cand_fixup", "k_job_pool_gather<0>", "k_job_pool_gather<1>"};

// What a step launches and which arguments it needs beyond the common ones of its layer (run_gin dispatches on this alone)
enum GinStepKind {
    GIN_STEP_INST = 0,                    // the whole encoder, one workgroup per instance
    GIN_STEP_RES,                         // the whole encoder in one launch
    GIN_STEP_MOMENTS,                     // second moments of the 12 aggregated features: the first BatchNorm's sums without forming the first Linear
    GIN_STEP_GIN0_VALU,                   // first Linear on the vector ALU (product mode bit 8)
    GIN_STEP_GIN0,                        // first Linear with the aggregation of the raw features in its producers (dst none: its BatchNorm sums only)
    GIN_STEP_GIN0BN,                      // second Linear whose producers form the first Linear's output again from the raw features
    GIN_STEP_GEMM,                        // BatchNorm + ReLU of src, then the Linear (dst none: the BatchNorm sums of the product only)
    GIN_STEP_AGG,                         // ... with the neighbour aggregation between them
    GIN_STEP_STATS_ZERO,                  // GIN_STEP_GEMM without output that also clears the pooled means the next step adds into
    GIN_STEP_POOL,                        // the product again, pooled and gathered in the epilogue
    GIN_STEP_PAIR,                        // two Linears in one launch (mtfjsp_gemm_pair.h): layer and layer + 1, the BatchNorm between them from slot `layer`
    GIN_STEP_FIXUP,                       // k_cand_fixup: the candidates' rows of the pooled product
    GIN_STEP_GATHER                       // k_job_pool_gather
};
enum GinBuf { GIN_BUF_NONE = 0, GIN_BUF_FEATURES, GIN_BUF_ZA, GIN_BUF_ZB };

// Layer l = 0..5 is the l-th Linear of the encoder and the BatchNorm behind it (one six-entry table of weight names, mtfjsp_encoder.hip: GIN_LIN / GIN_BN);
// statistics slot l holds the column sums of Linear l's output.
struct GinStep {
    GinStepKind kind;
    GinKernel kernel;
    const char *family;                   // timing family (mtfjsp_encoder_timing_query; bench.py, encoder.py and the profile readers match on these strings)
    int layer;
    int sin, sout;                        // slot (and BatchNorm) applied to the input / slot the output's sums go to; -1: none
    GinBuf src, dst;
    int rev, nt;                          // GemmArgs::rev (the workgroup walks its rows backwards), GemmArgs::nt (non-temporal input reads)
    bool from_moments;                    // GIN_STEP_GIN0BN: slot `sin` holds the features' moments (the producers need the first Linear's f32 weight)
    bool reduce;                          // a reduce_stats of slot `sout` follows the launch
};
#define GIN_MAX_STEPS 12
struct GinPlan {
    GinPath path;
    GinPool pool;
    GinResPlan res;                       // path == GIN_PATH_SINGLE: the instantiation, instances per workgroup and workgroups
    int pool_rpr, pool_grid, pool_s;      // pool == GIN_POOL_GATHER: k_job_pool_gather's rows per range (0: plain instance order), workgroups, blocks per range
    int nsteps;
    GinStep step[GIN_MAX_STEPS];
};

struct GinRequest {
    int B, T, n_job, J;                   // instances; rows per instance; candidates per instance the handle can be asked for; candidates of THIS forward (0: none)
    int num_cu;
    bool obs_f64;
    bool job_actor;                       // the job actor asks (its heads launch can pool); otherwise the global critic
    bool h_nodes;                         // the node embeddings are requested
    bool per_instance;                    // per-instance BatchNorm mode
    // the handle's answers
    bool res_ok;                          // the census of co-resident workgroups passed and no launch has timed out since
    bool reduce;                          // a statistics reduction over several shards is installed
    int f32_products;                     // product mode (mtfjsp_encoder_set_product_mode)
    bool last_wx6;                        // the last Linear has its split-product weight image
    // the switches, by value (names' defaults and when each is read: mtfjsp_enc_switches.h, which fills these fields)
    int fuse_pair, fuse_gin0, fuse_pool;  // MTFJSP_FUSE_PAIR, MTFJSP_FUSE_GIN0, MTFJSP_FUSE_POOL
    int stream_order, stream_nt, pool_s;  // !MTFJSP_NO_STREAM_ORDER, MTFJSP_STREAM_NT, MTFJSP_POOL_S
    int heads_pool_maxT;                  // MTFJSP_FUSE_POOL_MAXT
    const char *force_generic;            // the value of MTFJSP_GIN_RES_GENERIC or nullptr
};

// The single launch serves a handle whose census passed, unless a cross-shard reduction is installed (it cannot happen inside the launch) or the
// product mode asks for the f32 instruction in the GIN products (1), the first Linear on the vector ALU (8) or the streaming launches (16).
static inline bool gin_single_launch_ok(bool res_ok, bool reduce, int f32_products) { return res_ok && !reduce && !(f32_products & (1 | 8 | 16)); }

static inline const char *gin_kernel_name(const GinPlan &pl, const GinStep &s) { return s.kernel == GIN_K_RES ? GIN_RES_KERNEL_NAME[pl.res.kernel] : GIN_KERNEL_NAME[s.kernel]; }

// The rule.
static inline GinPlan gin_plan(const GinRequest &q)
{
    GinPlan pl{};
    pl.res = gin_res_plan(q.B, q.T, q.n_job, q.J, q.num_cu, q.h_nodes, q.force_generic);
    auto add = [&pl](GinStepKind kind, GinKernel kernel, const char *family, int layer, int sin, int sout, GinBuf src, GinBuf dst, int rev, int nt, bool reduce) {
        pl.step[pl.nsteps++] = GinStep{kind, kernel, family, layer, sin, sout, src, dst, rev, nt, false, reduce};
    };
    // ---- the path.  Per-instance BatchNorm is a mode of the two actor forwards: the global critic keeps the whole-batch statistics
    if (q.job_actor && q.per_instance) {
        pl.path = GIN_PATH_INST; pl.pool = GIN_POOL_KERNEL;
        add(GIN_STEP_INST, q.obs_f64 ? GIN_K_INST_F64 : GIN_K_INST_F32, "gin_inst", 0, -1, -1, GIN_BUF_FEATURES, GIN_BUF_NONE, 0, 0, false);
        return pl;
    }
    if (gin_single_launch_ok(q.res_ok, q.reduce, q.f32_products) && pl.res.eligible) {      // (a handle's census only ever passes for an eligible shape)
        pl.path = GIN_PATH_SINGLE; pl.pool = GIN_POOL_KERNEL;
        add(GIN_STEP_RES, GIN_K_RES, "gin_resident", 0, -1, -1, GIN_BUF_FEATURES, GIN_BUF_NONE, 0, 0, false);
        return pl;
    }
    pl.path = GIN_PATH_STREAM;
    const size_t N = (size_t)q.B * (size_t)q.T;
    const bool f32 = q.f32_products & 1;                           // the products run the f32 instruction (k_gemm16p) instead of the split products (k_gemm_x6)
    const int so = q.stream_order ? 1 : 0;
    // ---- the launch forms
    // Two Linears per launch (mtfjsp_gemm_pair.h), split products only.  MTFJSP_FUSE_PAIR=1: always; -1: where the [N,128] f32 activation matrix
    // exceeds the 256 MB memory-side cache (below that the second launch finds its input there and the pair saves no traffic); 0 (default): never.
    const bool pair = !f32 && (q.fuse_pair > 0 || (q.fuse_pair < 0 && N * 128 * 4 > ((size_t)256 << 20)));
    // The first Linear's output is not stored (MTFJSP_FUSE_GIN0=0 switches it off): its BatchNorm sums come from the second moments of the 12 aggregated
    // features (k_gin0_moments) and the producers of the second launch form it again from the raw features (PRO_GIN0BN).  f32 observations, split
    // products, no pair.  Row -> instance is an f32 reciprocal + one correction in k_gin0_moments and the PRO_GIN0BN producers — right for quotients
    // below 2^21, hence fewer than 2^24 rows of at least 8 per instance.
    const bool fuse0 = q.fuse_gin0 && !(q.f32_products & 9) && !pair && !q.obs_f64 && N < ((size_t)1 << 24) && q.T >= 8;
    // MTFJSP_FUSE_GIN0=2: the sums by a statistics-only PRO_GIN0 launch instead — the two-launch form's bits (A/B and tests).  So too with a statistics
    // reduction over several ranks: slot 0 must hold the SAME quantities on every rank, and a rank that has left the split products after a range
    // failure sums the first Linear's output itself — no moments then.
    const bool mom0 = fuse0 && q.fuse_gin0 != 2 && !q.reduce;
    // ---- who pools.  The heads kernel does BatchNorm + ReLU, graph pool and candidate gather itself while T is small: a workgroup pools 16 instances
    // with 512 threads, too little parallelism for 100- or 400-row instances (measured: J20M20 x 2048 199 vs 81 + 113 us; J10M10 x 8192 job + machine
    // heads 264 us fused vs 110 + 130 us with the stand-alone kernel).  Otherwise the last Linear's output is not stored either (MTFJSP_FUSE_POOL=0
    // switches it off): a statistics-only pass leaves its BatchNorm sums, a second pass forms it again and keeps only what the heads read — the
    // per-instance means and the candidates' rows — in its epilogue.  That epilogue takes a 16-row tile to hold rows of at most two instances
    // (T >= 16), finds a row's candidate slot as row / (T / J) with a reciprocal that is exact below 65536 (T < 65536; candidate j's row is one of
    // rows [j T / J, (j + 1) T / J): T % J == 0), maps row -> instance through an f32 quotient that is off by at most one below 2^24 rows, and
    // exists in the split-product kernel only (the last Linear's weight image, product mode bit 1 clear).
    const bool heads_pool = q.job_actor && !q.h_nodes && q.T <= q.heads_pool_maxT;
    const bool epilogue = !heads_pool && !pair && q.fuse_pool && !q.h_nodes && q.T >= 16 && q.T < 65536 && (q.J == 0 || q.T % q.J == 0) &&
                          N < ((size_t)1 << 24) && q.last_wx6 && !f32;
    pl.pool = heads_pool ? GIN_POOL_HEADS : epilogue ? GIN_POOL_EPILOGUE : GIN_POOL_GATHER;
    // ---- the steps.  The launches alternate the direction in which a workgroup walks its rows: each starts on the part of its input that is still in
    // the memory-side cache.  The aggregation product walks FORWARD (a row's job predecessor is the row before it: read a moment ago and still in L2;
    // backward it was measured 251 against 234 us), which fixes the others.  MTFJSP_STREAM_NT: which readers use non-temporal loads — 1 the
    // BatchNorm + ReLU products, 2 the aggregation product, 4 pool / gather.  MTFJSP_NO_STREAM_ORDER switches both off.
    const GinKernel k_bn = f32 ? GIN_K_16P_BNRELU : GIN_K_X6_BNRELU, k_agg = f32 ? GIN_K_16P_AGG : GIN_K_X6_AGG;
    const int nt1 = so && (q.stream_nt & 1), nt2 = so && (q.stream_nt & 2), nt4 = so && (q.stream_nt & 4);
    // (every form of the first Linear is followed by a reduction: the same number of reductions per forward in every product mode)
    if (mom0) add(GIN_STEP_MOMENTS, GIN_K_MOMENTS, "gin0_moments", 0, -1, 0, GIN_BUF_FEATURES, GIN_BUF_NONE, 0, 0, true);
    else if (!(q.f32_products & 8))
        add(GIN_STEP_GIN0, GIN_K_X6_GIN0, fuse0 ? "gin0_stats_only" : "gin0_agg_linear12", 0, -1, 0, GIN_BUF_FEATURES, fuse0 ? GIN_BUF_NONE : GIN_BUF_ZA, so, 0, true);
    else add(GIN_STEP_GIN0_VALU, q.obs_f64 ? GIN_K_GIN0_F64 : GIN_K_GIN0_F32, "gin0_agg_linear12", 0, -1, 0, GIN_BUF_FEATURES, GIN_BUF_ZA, 0, 0, true);
    // a pair: pass 1 = the first product without output (the sums of slot `layer`), pass 2 = both products, in the opposite direction (it starts on
    // what pass 1 read last)
    auto add_pair = [&](int layer, GinBuf src, GinBuf dst, int rev) {
        add(GIN_STEP_GEMM, k_bn, "gin_gemm_stats_only", layer, layer - 1, layer, src, GIN_BUF_NONE, so ? rev : 0, nt1, true);
        add(GIN_STEP_PAIR, GIN_K_X6F, "gin_gemm_pair", layer, layer - 1, layer + 1, src, dst, so ? rev ^ 1 : 0, nt1, true);
    };
    if (pair) add_pair(1, GIN_BUF_ZA, GIN_BUF_ZB, 0);
    else {
        if (fuse0) {
            add(GIN_STEP_GIN0BN, GIN_K_X6_GIN0BN, "gin0_bn_gemm", 1, 0, 1, GIN_BUF_FEATURES, GIN_BUF_ZB, 0, 0, true);
            pl.step[pl.nsteps - 1].from_moments = mom0;
        } else add(GIN_STEP_GEMM, k_bn, "gin_gemm_bn_relu", 1, 0, 1, GIN_BUF_ZA, GIN_BUF_ZB, 0, nt1, true);
        add(GIN_STEP_GEMM, k_bn, "gin_gemm_bn_relu", 2, 1, 2, GIN_BUF_ZB, GIN_BUF_ZA, so, nt1, true);
    }
    const GinBuf z2 = pair ? GIN_BUF_ZB : GIN_BUF_ZA, z3 = pair ? GIN_BUF_ZA : GIN_BUF_ZB;   // where the first MLP's output is / the aggregation product goes
    add(GIN_STEP_AGG, k_agg, "gin_gemm_agg", 3, 2, 3, z2, z3, 0, nt2, true);
    if (pair) add_pair(4, z3, GIN_BUF_ZB, 1);
    else {
        add(GIN_STEP_GEMM, k_bn, "gin_gemm_bn_relu", 4, 3, 4, GIN_BUF_ZB, GIN_BUF_ZA, so, nt1, true);
        if (epilogue) {
            // (the first pass reads with plain loads: its input is read twice; the second walks back from the end)
            add(GIN_STEP_STATS_ZERO, k_bn, "gin_gemm_stats_only", 5, 4, 5, GIN_BUF_ZA, GIN_BUF_NONE, 0, 0, true);
            add(GIN_STEP_POOL, k_bn, "gin_gemm_pool", 5, 4, -1, GIN_BUF_ZA, GIN_BUF_NONE, so, nt1, false);
            if (q.J > 0) add(GIN_STEP_FIXUP, GIN_K_FIXUP, "cand_fixup", 5, 4, -1, GIN_BUF_ZA, GIN_BUF_NONE, 0, 0, false);
        } else add(GIN_STEP_GEMM, k_bn, "gin_gemm_bn_relu", 5, 4, 5, GIN_BUF_ZA, GIN_BUF_ZB, 0, nt1, true);
    }
    if (pl.pool == GIN_POOL_GATHER) {
        // row ranges = the last product's partition (launch_gemm's grid and k_gemm_x6's tiles per workgroup), MTFJSP_POOL_S workgroups per range
        const int ntiles = (int)((N + 15) / 16), ggrid = (ntiles + 7) / 8 < q.num_cu ? (ntiles + 7) / 8 : q.num_cu;
        pl.pool_s = q.pool_s;
        pl.pool_rpr = so && q.pool_s > 0 ? ((ntiles + ggrid - 1) / ggrid) * 16 : 0;
        pl.pool_grid = pl.pool_rpr ? ggrid * q.pool_s : (q.B < q.num_cu * 8 ? q.B : q.num_cu * 8);
        add(GIN_STEP_GATHER, nt4 ? GIN_K_GATHER_NT : GIN_K_GATHER, "job_pool_gather", 5, 5, -1, GIN_BUF_ZB, GIN_BUF_NONE, 0, nt4, false);
    }
    return pl;
}
