// mtfjsp_gin_res_select.h — which instantiation of the single-launch GIN kernel (mtfjsp_gin_resident.h) serves a forward, stated ONCE: every
// launch (the forwards and the co-residency census of mtfjsp_encoder.hip) goes through this plan, and mtfjsp_gin_res_kernel_name_for reports
// it without a GPU.  Plain C++17, no HIP header: a host-only program can include it.
#pragma once
#include <stdlib.h>

#define GR_NT 18                          // row tiles per workgroup (576 rows)
#define GR_ROWS (32 * GR_NT)
#define GR_MAXCAND 384
#define GR_MAXT 65                        // rows per instance: the in-edge sources of a tile lie within two tiles of it
#define GR_MINT 16                        // ... and a 16-row run spans at most two instances (pooling)
#define GR_MAXIPC 64                      // instances per workgroup (u8 instance ids; pool accumulators in the ring area)
// the fixed-shape instantiation: the headline workload (J6M6 x 4096 on 256 compute units), 16 instances = 576 rows in every workgroup
#define GIN_RES_FX_T 36
#define GIN_RES_FX_J 6
#define GIN_RES_FX_IPC 16

enum GinResKernel { GIN_RES_K_ANY = 0, GIN_RES_K_T36J6X16, GIN_RES_K_COUNT };
static const char *const GIN_RES_KERNEL_NAME[GIN_RES_K_COUNT] = {"k_gin_res", "k_gin_res_t36j6x16"};    // ("k_gin_res" prefixes both: the profile readers match on it)

struct GinResPlan {
    bool eligible;                        // the shape can run in one launch at all (whole instances per workgroup, one workgroup per compute unit)
    GinResKernel kernel;
    int ipc, grid;                        // instances per workgroup, workgroups
};
// The rule.  B instances of T rows; n_job: candidates per instance the handle can be asked for (bounds the candidate table); J: candidates
// per instance of THIS forward (0: none — the global critic); h_nodes: the node embeddings are requested; force_generic: the value of
// MTFJSP_GIN_RES_GENERIC or nullptr, read by the caller.  The fixed instantiation serves exactly the shape it was compiled for with every
// workgroup full (B % ipc == 0) and no node output; everything else eligible runs the run-time kernel.
static inline GinResPlan gin_res_plan(int B, int T, int n_job, int J, int num_cu, bool h_nodes, const char *force_generic)
{
    GinResPlan pl{false, GIN_RES_K_ANY, 0, 0};
    if (B < 1 || num_cu < 1 || T < GR_MINT || T > GR_MAXT) return pl;
    pl.ipc = (B + num_cu - 1) / num_cu;
    pl.grid = (B + pl.ipc - 1) / pl.ipc;
    // (grid + 7) / 8 <= 63: a count-carrying statistics word holds the arrivals of one dispatch group in 6 bits (gr_fix_encode)
    pl.eligible = pl.ipc * T <= GR_ROWS && pl.ipc <= GR_MAXIPC && pl.grid <= num_cu && (pl.grid + 7) / 8 <= 63 && pl.ipc * n_job <= GR_MAXCAND;
    const bool forced = force_generic && atoi(force_generic) != 0;
    if (pl.eligible && !forced && T == GIN_RES_FX_T && J == GIN_RES_FX_J && pl.ipc == GIN_RES_FX_IPC && B % pl.ipc == 0 && !h_nodes)
        pl.kernel = GIN_RES_K_T36J6X16;
    return pl;
}
