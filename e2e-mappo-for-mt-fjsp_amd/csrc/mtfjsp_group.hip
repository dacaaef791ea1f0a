// mtfjsp_group.hip — reductions over groups of copies of one instance (best-of-K evaluation on the device fork: K sampled schedules
// per instance in one handle of N*K copies, copy c of instance n = element n*K + c).
//   mtfjsp_final_costs    k_final_costs: one thread per instance, the finished schedule's four costs and whether it finished.  The
//                         reference forms them on the host from the *_previous_step state (validate.py:277-287, here
//                         evaluate.py's Final_4cost): makespan, processing energy / T, transport time, idle time
//   mtfjsp_group_reduce   k_group_reduce: one workgroup per group — every copy's objective (test_all.py:536-538, evaluate.py's
//                         Objective), the copy with the smallest one and the non-dominated copies in (makespan, energy, transport)
// Arithmetic: ONE binary64 division in k_final_costs; in k_group_reduce the objective's (the rule: mtfjsp_copy_costs.h), never contracted.
// Everything else is comparisons: both must equal a host model bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_copy_costs.h"
#include "mtfjsp_env_dev.h"
#include "mtfjsp_wave_select.h"

#define GRP_WAVES 4
#define GRP_THREADS (GRP_WAVES * WAVE)
#define GRP_MAX_K 4096                 // 128 KB of (mk, ec, tt, obj) in a workgroup's 160 KB

// ---------------------------------------------------------------- final costs
struct FinalArgs {
    int B, T;
    const double *scal;                // [B,SCAL_N]
    double *cost4;                     // [B,4]
    uint8_t *done;                     // [B] or null
};

__global__ __launch_bounds__(256) void k_final_costs(FinalArgs A)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const double *s = A.scal + (size_t)(i < A.B ? i : A.B - 1) * SCAL_N;
    const double mk = s[S_MK_PREV], e1 = s[S_E1_PREV], tr = s[S_TR_PREV], id = s[S_ID_PREV], ns = s[S_NSCHED];
    if (i >= A.B) return;
    double *o = A.cost4 + (size_t)i * 4;
    o[0] = mk; o[1] = e1 / (double)A.T; o[2] = tr; o[3] = id;
    if (A.done) A.done[i] = ns == (double)A.T ? 1 : 0;
}

extern "C" int mtfjsp_final_costs(mtfjsp_handle_t h, double *cost4_out, uint8_t *done_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!cost4_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_final_costs: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.was_reset)
        return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, v.replayed ? "mtfjsp_final_costs: the handle holds replayed plans (mtfjsp_replay_plans wrote their costs), not a state: reset first"
                                                               : "mtfjsp_final_costs: the handle has never been reset");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_final_costs")) return rc;
    FinalArgs A{};
    A.B = v.B; A.T = v.T; A.scal = v.scal; A.cost4 = cost4_out; A.done = done_out;
    hipLaunchKernelGGL(k_final_costs, dim3((unsigned)(((size_t)v.B + 255) / 256)), dim3(256), 0, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_final_costs");
}

// ---------------------------------------------------------------- group reduction
struct GroupArgs {
    int K;
    CopyWeights w;
    const double *cost4;               // [N*K,4]
    const uint8_t *done;               // [N*K]
    double *obj;                       // [N*K] or null
    int *best;                         // [N] or null
    double *best_obj;                  // [N] or null
    uint8_t *front;                    // [N*K] or null
};

// Copy c of group n lives in LDS as its record; thread tid owns copies tid, tid + 256, ... (OWN of them at most: 1, 4 or 16 by K), keeps them
// in registers and alone writes their flags; the minimum runs over the owned copies (all of it: mtfjsp_copy_costs.h).
// The dominance loop reads copy c' at one address for the whole workgroup (a broadcast read: no bank conflict at any pitch).
template <int OWN>
__global__ __launch_bounds__(GRP_THREADS) void k_group_reduce(GroupArgs A)
{
    extern __shared__ __align__(32) unsigned char smem[];
    __shared__ double part_v[GRP_WAVES];
    __shared__ int part_i[GRP_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, K = A.K;
    const size_t g0 = (size_t)blockIdx.x * K;
    double4 *cp = reinterpret_cast<double4 *>(smem);
    // every load of this thread first (a copy past K reads the group's last one again and is ignored)
    double c0[OWN], c1[OWN], c2[OWN], c3[OWN];
    uint8_t dn[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * GRP_THREADS;
        const size_t g = g0 + (c < K ? c : K - 1);
        c0[i] = A.cost4[g * 4]; c1[i] = A.cost4[g * 4 + 1]; c2[i] = A.cost4[g * 4 + 2]; c3[i] = A.cost4[g * 4 + 3];
        dn[i] = A.done[g];
    }
    double mk[OWN], ec[OWN], tt[OWN], ob[OWN];
    bool el[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * GRP_THREADS;
        const double m = c0[i], e = c1[i] + c3[i], t = c2[i];
        const double o = (A.w.mk * m + A.w.ec * e) + A.w.tt * t;
        el[i] = c < K && dn[i] != 0 && m == m && e == e && t == t;
        mk[i] = el[i] ? m : (double)NAN; ec[i] = e; tt[i] = t; ob[i] = el[i] ? o : (double)NAN;
        if (c < K) {
            cp[c] = make_double4(mk[i], ec[i], tt[i], ob[i]);
            if (A.obj) A.obj[g0 + c] = ob[i];
        }
    }
    __syncthreads();
    // ---- the smallest objective, lowest copy on ties (an eligible copy whose objective is NaN — infinite costs — is never picked)
    WaveBest<false> mine;
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int cw = wave * WAVE + i * GRP_THREADS;                       // (wave-uniform)
        if (cw < K) mine.pass(ob[i] == ob[i], ob[i], cw);
    }
    if (lane == 0) { part_v[wave] = mine.v; part_i[wave] = mine.i; }
    __syncthreads();
    if (tid == 0) {
        const int gi = wave_best_combine<false, GRP_WAVES>(part_v, part_i).i;
        if (A.best) A.best[blockIdx.x] = gi < 0 ? -1 : (int)(g0 + gi);
        if (A.best_obj) A.best_obj[blockIdx.x] = gi < 0 ? (double)NAN : cp[gi].w;   // the copy's own word (the minimum may be a zero of the other sign)
    }
    // ---- the front: copy c is dominated by c' iff c' is nowhere worse and somewhere better, or equal throughout with c' < c (copy_dominates,
    // written out: through the function the loop's code changes and K > 256 is slower, profiles/HISTORY.md)
    if (!A.front) return;
    bool dom[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) dom[i] = false;
    for (int q = 0; q < K; q++) {
        const double4 o = cp[q];
#pragma unroll
        for (int i = 0; i < OWN; i++) {
            const int c = tid + i * GRP_THREADS;
            const bool le = o.x <= mk[i] && o.y <= ec[i] && o.z <= tt[i];
            const bool lt = o.x < mk[i] || o.y < ec[i] || o.z < tt[i];
            dom[i] = dom[i] || (le && (lt || q < c));
        }
    }
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * GRP_THREADS;
        if (c < K) A.front[g0 + c] = (el[i] && !dom[i]) ? 1 : 0;
    }
}

template <int OWN>
static int group_launch(mtfjsp_handle_t h, const EnvHostView &v, int N, const GroupArgs &A)
{
    const size_t lds = (size_t)A.K * 32;
    if (int rc = mtfjsp_env_dyn_lds(h, (const void *)k_group_reduce<OWN>, lds, "mtfjsp_group_reduce")) return rc;
    hipLaunchKernelGGL(k_group_reduce<OWN>, dim3((unsigned)N), dim3(GRP_THREADS), lds, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_group_reduce");
}

extern "C" int mtfjsp_group_reduce(mtfjsp_handle_t h, int32_t N, int32_t K, const double *cost4, const uint8_t *done, const double *w3cfg_host,
                                   double *obj_out, int32_t *best_out, double *best_obj_out, uint8_t *front_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!cost4 || !done || !w3cfg_host) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_group_reduce: null argument");
    if (K < 1 || K > GRP_MAX_K || N < 1 || (long)N * K > INT_MAX)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_group_reduce: 1 <= K <= 4096, N >= 1 and N*K must fit 31 bits");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_group_reduce")) return rc;
    GroupArgs A{};
    A.K = K; A.w = copy_weights(w3cfg_host); A.cost4 = cost4; A.done = done;
    A.obj = obj_out; A.best = best_out; A.best_obj = best_obj_out; A.front = front_out;
    if (K <= GRP_THREADS) return group_launch<1>(h, v, N, A);
    if (K <= 4 * GRP_THREADS) return group_launch<4>(h, v, N, A);
    return group_launch<16>(h, v, N, A);
}
