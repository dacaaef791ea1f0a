// mtfjsp_heads_select.h — which heads kernel serves an actor forward, with how many instances per workgroup and how many workgroups, stated ONCE:
// both forwards of mtfjsp_encoder.hip build this plan before anything of the launch is timed or assembled (the timing family, HeadArgs::hg, the grid,
// the launch and the handle's record of it all come from it), and mtfjsp_heads_kernel_name_for reports it without a GPU.  Plain C++17, no HIP header:
// a host-only program can include it.
#pragma once
#include "mtfjsp_fused3_select.h"

enum HeadsKernel {
    HEADS_K_F32 = 0,                      // k_heads: the f32 matrix instruction (product mode bit 4), the A/B reference
    HEADS_K_X,                            // k_headsx: the split products, six scorer tiles per chunk
    HEADS_K_X10,                          // k_headsx10: ten tiles per chunk
    HEADS_K_VALUES,                       // k_headsx_values: the critic values alone
    HEADS_K_GAT3X,                        // k_headsx_gat3x: + the machine path's GAT passes of the same 16 instances
    HEADS_K_ENVSTEP,                      // k_headsx_envstep<OBS>: + the environment step of the same 16 instances
    HEADS_K_FUSED3,                       // k_headsx_gat3x_headsx<ENV, NLDS, SH>: + the GAT passes + the machine actor's heads (mtfjsp_fused3_select.h)
    HEADS_K_COUNT
};
static const char *const HEADS_KERNEL_NAME[HEADS_K_COUNT] = {"k_heads", "k_headsx", "k_headsx10", "k_headsx_values", "k_headsx_gat3x", "k_headsx_envstep",
                                                             "k_headsx_gat3x_headsx"};   // (the last: FUSED3_KERNEL_NAME[the instantiation], heads_kernel_name)
// the timing family of each (mtfjsp_encoder_timing_query; bench.py and the profile readers match on these strings)
static const char *const HEADS_KERNEL_FAMILY[HEADS_K_COUNT] = {"heads", "heads", "heads", "heads", "heads_gat3", "heads", "heads_gat3_heads"};

// (the shape condition of a launch that carries the GAT passes: heads_gat_ride_shape, mtfjsp_fused3_select.h — fused3_plan needs it too)
struct HeadsRequest {
    int B, R, M, T, num_cu;               // instances; rows per instance (J for the job actor, M for the machine actor); machines; task rows; compute units
    // what the caller asks to ride along
    bool gat;                             // the machine path's GAT passes (a job forward with an armed m_fea1 context that has m_fea2)
    bool mheads;                          // ... and the machine actor's heads (armed outputs and an armed machine selection)
    bool env_tail;                        // an armed environment step that reads the last selection made in this launch
    bool values_only;                     // the critic values alone
    // the handle's answers
    bool f32;                             // product mode bit 4: the heads run the f32 matrix instruction
    bool gat_ok, mheads_ok;               // the handle's half of gat_fusable / mheads_fusable (switches, modes, weight images, the census) holds
    bool hg8, heads10;                    // !MTFJSP_NO_HEADS_HG8; !MTFJSP_NO_HEADS10 and the device grants k_headsx10 its LDS (read in mtfjsp_enc_switches.h, like the two below)
    bool nodes_hbm;                       // MTFJSP_FUSED3_NODES_HBM
    bool obs_f64;                         // the observation dtype the riding parts read
    const char *force_generic;            // the value of MTFJSP_FUSED3_GENERIC or nullptr
};
struct HeadsPlan {
    HeadsKernel kernel;
    int hg, grid;                         // instances per workgroup (HeadArgs::hg), workgroups
    int env;                              // 0: no environment tail in the launch, 1 / 2: the step behind the launch's last selection (f32 / f64 observations)
    Fused3Plan three;                     // kernel == HEADS_K_FUSED3: the instantiation's rule; otherwise only .eligible means anything
};
// The rule, in the order of precedence.  Nothing rides with the f32 instruction or with the values alone; an environment tail rides behind the
// machine selection, so in a launch that carries the GAT passes only the three-in-one form takes it; groups of 8 instances (the grid twice as wide,
// the LDS layout that of 16) only where nothing rides and groups of 16 would leave at least half the compute units without a workgroup.
static inline HeadsPlan heads_plan(const HeadsRequest &q)
{
    HeadsPlan pl{HEADS_K_X, F3_HG, 0, 0, fused3_plan(q.B, q.R, q.M, q.T, q.num_cu, q.obs_f64, q.nodes_hbm ? "1" : nullptr, q.env_tail, q.force_generic)};
    const int g16 = (q.B + F3_HG - 1) / F3_HG;
    pl.grid = g16;
    if (q.f32) { pl.kernel = HEADS_K_F32; return pl; }
    const bool gat = q.gat && !q.values_only && q.gat_ok && heads_gat_ride_shape(q.B, q.M, q.num_cu);
    if (gat && q.mheads && q.mheads_ok && pl.three.eligible) { pl.kernel = HEADS_K_FUSED3; pl.env = pl.three.env; return pl; }
    if (gat) { pl.kernel = HEADS_K_GAT3X; return pl; }
    if (q.env_tail) { pl.kernel = HEADS_K_ENVSTEP; pl.env = q.obs_f64 ? 2 : 1; return pl; }
    if (q.hg8 && 2 * g16 <= q.num_cu) { pl.hg = F3_HG / 2; pl.grid = (q.B + pl.hg - 1) / pl.hg; }
    if (q.values_only) { pl.kernel = HEADS_K_VALUES; return pl; }
    const int ntl = (pl.hg * q.R + 15) / 16;                      // tiles of a full group
    if (q.heads10 && ntl > 6 && ntl <= 10) pl.kernel = HEADS_K_X10;
    return pl;
}
static inline const char *heads_kernel_name(const HeadsPlan &pl) { return pl.kernel == HEADS_K_FUSED3 ? FUSED3_KERNEL_NAME[pl.three.kernel] : HEADS_KERNEL_NAME[pl.kernel]; }
