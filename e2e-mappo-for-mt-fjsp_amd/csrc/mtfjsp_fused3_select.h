// mtfjsp_fused3_select.h — which instantiation of the three-in-one heads launch (k_headsx_gat3x_headsx, mtfjsp_encoder.hip: job heads + the machine
// path's GAT passes + machine heads) serves a job forward, stated ONCE: the heads launch's plan (mtfjsp_heads_select.h) holds this one, and
// mtfjsp_fused3_kernel_name_for reports it without a GPU.  Plain C++17, no HIP header: a host-only program can include it.
#pragma once
#include <stdlib.h>

#define F3_HG 16                          // instances per workgroup (HG of the heads kernels)
#define F3_HCH 6                          // scorer tiles per chunk (HCH): the machine part stages its rows by instance where M <= HCH
#define F3_MAXM 8                         // the pool rows are requested ahead of the exchange (mtfjsp_headsx_body.h)
// the fixed-shape instantiation: the headline workload (J6M6 x 4096 on 256 compute units)
#define FUSED3_FX_J 6
#define FUSED3_FX_M 6
#define FUSED3_FX_IPC 16
#define FUSED3_FX_B 4096                  // (the kernel itself does not depend on the batch: the rule names the one shape whose bits the tests pin)

enum Fused3Kernel { FUSED3_K_ANY = 0, FUSED3_K_J6M6X16, FUSED3_K_COUNT };
static const char *const FUSED3_KERNEL_NAME[FUSED3_K_COUNT] = {"k_headsx_gat3x_headsx", "k_headsx_gat3x_headsx<0, true, H3ShapeFixed<6, 6, 16>>"};   // (as a profile shows the fixed one; the first prefixes both and every <ENV, NLDS, H3ShapeAny>: the profile readers match on it)

// Can the machine path's GAT passes ride in a heads launch over B instances of M machines on num_cu compute units?  Whole groups of 16 instances, one
// round of workgroups, and a grid (B / 16) as wide as the GAT launch would make its own — min(row tiles / 8, CUs).  Measured, J6M6 x 4096: 47.7 us
// against 24.6 + 26.8.  Fewer workgroups than the GAT's own grid leave CUs idle during the GAT part (J20M20 x 2048, 128 workgroups: 110 against
// 53 + 38), two rounds of workgroups gain nothing (J10M10 x 8192: 130 against 128).
static inline bool heads_gat_ride_shape(int B, int M, int num_cu)
{
    const int hgrid = B / F3_HG, gtiles = (2 * B * M + 15) / 16, ggrid = (gtiles + 7) / 8 < num_cu ? (gtiles + 7) / 8 : num_cu;
    return B % F3_HG == 0 && hgrid <= num_cu && hgrid >= ggrid;
}

struct Fused3Plan {
    bool eligible;                        // the shape can take the three-in-one launch at all
    Fused3Kernel kernel;
    int grid;                             // workgroups
    bool nodes_lds;                       // the GAT part's node rows stay in LDS for the machine part
    int env;                              // 0: no environment tail, 1 / 2: the step of the workgroup's instances behind the machine part (f32 / f64 observations)
};
// The rule.  B instances of J candidates, M machines and T task rows each on num_cu compute units; obs_f64: the observation dtype; nodes_hbm: the value
// of MTFJSP_FUSED3_NODES_HBM or nullptr; env_tail: an armed environment step rides in the launch; force_generic: the value of MTFJSP_FUSED3_GENERIC or
// nullptr, read by the caller.  Eligibility is the shape's half of mheads_fusable (the handle's half — switches, weights, the census of co-resident
// workgroups — is its own): the shape on which the GAT passes ride at all, every workgroup resident at once, at most 8 machines.  The fixed
// instantiation serves exactly the shape it was compiled for: f32 observations, node rows in LDS, no environment tail.
static inline Fused3Plan fused3_plan(int B, int J, int M, int T, int num_cu, bool obs_f64, const char *nodes_hbm, bool env_tail, const char *force_generic)
{
    Fused3Plan pl{false, FUSED3_K_ANY, 0, false, 0};
    if (B < 1 || J < 1 || M < 1 || T < 1 || num_cu < 1) return pl;
    const int hgrid = B / F3_HG, gtiles = (2 * B * M + 15) / 16;
    pl.grid = hgrid;
    pl.eligible = heads_gat_ride_shape(B, M, num_cu) && (hgrid + 7) / 8 <= 63 && M <= F3_MAXM;   // (a count field of the exchange words holds the arrivals of one dispatch group in 6 bits)
    if (!pl.eligible) return pl;
    const int gper = (gtiles + hgrid - 1) / hgrid;                // GAT row tiles per workgroup: each has an LDS buffer of its own up to 12
    pl.nodes_lds = !nodes_hbm && gper <= 12 && M <= F3_HCH;
    pl.env = !env_tail ? 0 : obs_f64 ? 2 : 1;
    const bool forced = force_generic && atoi(force_generic) != 0;
    if (!forced && J == FUSED3_FX_J && M == FUSED3_FX_M && T == FUSED3_FX_J * FUSED3_FX_M && B == FUSED3_FX_B && !obs_f64 && pl.nodes_lds && pl.env == 0)
        pl.kernel = FUSED3_K_J6M6X16;
    return pl;
}
