// mtfjsp_walk.hip — the acceptance step of a search on plans that may leave a local optimum: in the round of the local search
// (mtfjsp_plan_neighbours, replay, mtfjsp_final_costs) it takes the place of mtfjsp_group_reduce.
//   mtfjsp_walk_accept    k_walk_accept: one workgroup per group — every copy's objective (mtfjsp_copy_costs.h has the rule), the candidates
//                         (not the incumbent's own schedule again, not a schedule of the tabu ring), the best of them, whether the walk
//                         moves there (strictly better | within the slack | not above the late ring's entry), both rings' updates and
//                         the best plan seen so far: the incumbent may get worse, so the best is kept beside it
// Arithmetic: the objective's (the rule: mtfjsp_copy_costs.h), never contracted, and ONE addition cur + slack. Everything else is comparisons of
// binary64 and of 64-bit signatures: the kernel must equal a host model bit for bit (tests/walk_ref.py).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_copy_costs.h"
#include "mtfjsp_env_dev.h"
#include "mtfjsp_plan_dev.h"
#include "mtfjsp_wave_select.h"

#define WALK_WAVES 4
#define WALK_THREADS (WALK_WAVES * WAVE)
#define WALK_MAX_K 4096
#define WALK_MAX_LATE 4096
#define WALK_MAX_TABU 1024             // 8 KB of LDS

struct WalkArgs {
    int N, K, T, first, late_len, tabu_len, late_slot;
    CopyWeights w;
    double slack;
    const double *cost4;               // [N*K,4]
    const uint8_t *done;               // [N*K]
    const uint64_t *sig;               // [N*K] or null
    const int *task, *mach;            // [T,N*K]
    double *late;                      // [N,late_len]
    uint64_t *tabu;                    // [N,tabu_len]
    int *tabu_n;                       // [N]
    double *best_obj;                  // [N]
    int *best_task, *best_mach;        // [T,N]
    int *next_col;                     // [N]
    double *cur_out, *best_out;        // [N] or null
    int *pick_out;                     // [N] or null
    int8_t *why_out;                   // [N] or null
    int *barred_out;                   // [N] or null
    double *obj_out;                   // [N*K] or null
};

// Thread tid owns copies tid, tid + 256, ... (OWN of them at most: 1, 4 or 16 by K) and keeps their objectives and signatures in registers, as
// k_group_reduce does: pass i of wave w over the minimum is its i-th owned copy.  The valid entries of the group's tabu ring go to LDS once;
// every thread tests its own copies against entry q, which the whole workgroup reads at one address (a broadcast).  Thread 0 owns copy 0, the
// incumbent: it combines the waves' results, decides, writes the scalars of the state and leaves (source column of the best plan, cur, new
// cur) in LDS; behind the barrier the workgroup copies that column, rows over threads, and on a first call fills the late ring.
// Reads before writes: the ring is in LDS and late's entry and best_obj in thread 0's registers before the first barrier; the first write
// to any of them comes after the second.
template <int OWN>
__global__ __launch_bounds__(WALK_THREADS) void k_walk_accept(WalkArgs A)
{
    __shared__ uint64_t ring[WALK_MAX_TABU];
    __shared__ double part_v[WALK_WAVES];
    __shared__ int part_i[WALK_WAVES], part_b[WALK_WAVES];
    __shared__ double dec_cur[2];      // cur, new cur
    __shared__ int dec_col;            // the column that becomes the best plan, -1: it stays
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, K = A.K, n = blockIdx.x;
    const size_t g0 = (size_t)n * K;
    // every load of this thread first (a copy past K reads the group's last one again and is ignored)
    double c0[OWN], c1[OWN], c2[OWN], c3[OWN];
    uint64_t sg[OWN];
    uint8_t dn[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * WALK_THREADS;
        const size_t g = g0 + (c < K ? c : K - 1);
        c0[i] = A.cost4[g * 4]; c1[i] = A.cost4[g * 4 + 1]; c2[i] = A.cost4[g * 4 + 2]; c3[i] = A.cost4[g * 4 + 3];
        dn[i] = A.done[g];
        sg[i] = A.sig ? A.sig[g] : 0;
    }
    const uint64_t sig0 = A.sig ? A.sig[g0] : 0;
    int tn = 0, n_ring = 0;
    if (A.tabu_len > 0) {
        tn = A.first ? 0 : A.tabu_n[n];
        n_ring = tn < A.tabu_len ? (tn > 0 ? tn : 0) : A.tabu_len;
        for (int e = tid; e < n_ring; e += WALK_THREADS) ring[e] = A.tabu[(size_t)n * A.tabu_len + e];
    }
    double late_v = 0.0, best_v = 0.0;
    if (tid == 0) {
        if (A.late_len > 0 && !A.first) late_v = A.late[(size_t)n * A.late_len + A.late_slot];
        if (!A.first) best_v = A.best_obj[n];
    }
    double ob[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * WALK_THREADS;
        const double m = c0[i], e = c1[i] + c3[i], t = c2[i];
        const double o = (A.w.mk * m + A.w.ec * e) + A.w.tt * t;
        const bool el = c < K && dn[i] != 0 && m == m && e == e && t == t;
        ob[i] = el ? o : (double)NAN;
        if (c < K && A.obj_out) A.obj_out[g0 + c] = ob[i];
    }
    __syncthreads();
    // ---- the candidates: copies c >= 1 with an objective, minus the incumbent's own schedule and the schedules of the ring
    bool hit[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) hit[i] = A.sig && sg[i] == sig0;
    for (int q = 0; q < n_ring; q++) {
        const uint64_t r = ring[q];
#pragma unroll
        for (int i = 0; i < OWN; i++) hit[i] = hit[i] || sg[i] == r;
    }
    WaveBest<false> mine;
    int barred = 0;
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int cw = wave * WAVE + i * WALK_THREADS;                      // (wave-uniform)
        const int c = tid + i * WALK_THREADS;
        const bool has = c >= 1 && c < K && ob[i] == ob[i];
        if (cw < K) {
            barred += __popcll(__ballot(has && hit[i]));
            mine.pass(has && !hit[i], ob[i], cw);
        }
    }
    if (lane == 0) { part_v[wave] = mine.v; part_i[wave] = mine.i; part_b[wave] = barred; }
    __syncthreads();
    // ---- the decision
    if (tid == 0) {
        const WaveBest<false> g = wave_best_combine<false, WALK_WAVES>(part_v, part_i);
        const int pick = g.i;
        const double cur = ob[0];
        if (A.first) { late_v = cur; best_v = cur; }
        int why = 0;
        if (pick >= 0) {
            if (cur != cur || g.v < cur) why = 2;
            else if (A.slack >= 0 && g.v <= cur + A.slack) why = 3;
            else if (A.late_len > 0 && g.v <= late_v) why = 4;
            else why = 1;
        }
        const bool move = why >= 2;
        const double now = move ? g.v : cur;                                // the copy's own word
        if (move && A.tabu_len > 0) {
            const int slot = ((tn % A.tabu_len) + A.tabu_len) % A.tabu_len;
            A.tabu[(size_t)n * A.tabu_len + slot] = sig0;
            tn += 1;
        }
        if (A.tabu_len > 0 && (move || A.first)) A.tabu_n[n] = tn;
        A.next_col[n] = move ? (int)(g0 + pick) : (cur == cur ? (int)g0 : -1);
        const bool better = move && (best_v != best_v || now < best_v);
        if (better) { best_v = now; why += 8; }
        if (better || A.first) A.best_obj[n] = best_v;
        dec_cur[0] = cur; dec_cur[1] = now;
        dec_col = better ? (int)(g0 + pick) : (A.first ? (int)g0 : -1);
        if (A.cur_out) A.cur_out[n] = now;
        if (A.best_out) A.best_out[n] = best_v;
        if (A.pick_out) A.pick_out[n] = pick;
        if (A.why_out) A.why_out[n] = (int8_t)why;
        if (A.barred_out) A.barred_out[n] = part_b[0] + part_b[1] + part_b[2] + part_b[3];
    }
    __syncthreads();
    // ---- the late ring: a first call fills it with cur; the round's entry takes the new cur
    if (A.late_len > 0) {
        double *lt = A.late + (size_t)n * A.late_len;
        if (A.first)
            for (int e = tid; e < A.late_len; e += WALK_THREADS) lt[e] = dec_cur[e == A.late_slot ? 1 : 0];
        else if (tid == 0)
            lt[A.late_slot] = dec_cur[1];
    }
    // ---- the best plan: column dec_col of this round's plans, row by row
    const int col = dec_col;
    if (col < 0) return;
    const size_t NK = (size_t)A.N * K;
    for (int s = tid; s < A.T; s += WALK_THREADS) {
        A.best_task[(size_t)s * A.N + n] = A.task[(size_t)s * NK + col];
        A.best_mach[(size_t)s * A.N + n] = A.mach[(size_t)s * NK + col];
    }
}

template <int OWN>
static int walk_launch(mtfjsp_handle_t h, const EnvHostView &v, const WalkArgs &A)
{
    hipLaunchKernelGGL(k_walk_accept<OWN>, dim3((unsigned)A.N), dim3(WALK_THREADS), 0, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_walk_accept");
}

extern "C" int mtfjsp_walk_accept(mtfjsp_handle_t h, int32_t N, int32_t K, const double *cost4, const uint8_t *done, const double *w3cfg_host,
                                  const uint64_t *sig, const int32_t *task, const int32_t *mach, uint64_t round, int32_t first, double slack,
                                  int32_t late_len, int32_t tabu_len, double *late, uint64_t *tabu, int32_t *tabu_n, double *best_obj,
                                  int32_t *best_task, int32_t *best_mach, int32_t *next_col, double *cur_obj_out, double *best_obj_out,
                                  int32_t *pick_out, int8_t *why_out, int32_t *barred_out, double *obj_out)
{
    const char *who = "mtfjsp_walk_accept";
    if (!h) return MTFJSP_ERR_ARG;
    if (!cost4 || !done || !w3cfg_host || !task || !mach || !best_obj || !best_task || !best_mach || !next_col)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_walk_accept: null argument");
    if (K < 1 || K > WALK_MAX_K || N < 1 || (long)N * K > INT_MAX)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_walk_accept: 1 <= K <= 4096, N >= 1 and N*K must fit 31 bits");
    if (late_len < 0 || late_len > WALK_MAX_LATE || tabu_len < 0 || tabu_len > WALK_MAX_TABU)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_walk_accept: 0 <= late_len <= 4096 and 0 <= tabu_len <= 1024");
    if ((late_len > 0 && !late) || (tabu_len > 0 && (!tabu || !tabu_n || !sig)))
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_walk_accept: late_len > 0 needs late, tabu_len > 0 needs tabu, tabu_n and sig");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    const unsigned __int128 n = (unsigned __int128)N, nk = n * (unsigned)K, T4 = (unsigned __int128)v.T * 4;
    const PlanSpan srcs[5] = {{cost4, nk * 32}, {done, nk}, {sig, nk * 8}, {task, T4 * nk}, {mach, T4 * nk}};
    const PlanSpan outs[13] = {{late_len ? late : nullptr, n * (unsigned)late_len * 8}, {tabu_len ? tabu : nullptr, n * (unsigned)tabu_len * 8},
                               {tabu_len ? tabu_n : nullptr, n * 4}, {best_obj, n * 8}, {best_task, T4 * n}, {best_mach, T4 * n}, {next_col, n * 4},
                               {cur_obj_out, n * 8}, {best_obj_out, n * 8}, {pick_out, n * 4}, {why_out, n}, {barred_out, n * 4}, {obj_out, nk * 8}};
    if (int rc = plan_check_overlap(h, who, 13, outs, 5, srcs)) return rc;
    if (int rc = mtfjsp_env_set_device(h, v.device_id, who)) return rc;
    WalkArgs A{};
    A.N = N; A.K = K; A.T = v.T; A.first = first != 0; A.late_len = late_len; A.tabu_len = tabu_len;
    A.late_slot = late_len > 0 ? (int)(round % (uint64_t)late_len) : 0;
    A.w = copy_weights(w3cfg_host); A.slack = slack;
    A.cost4 = cost4; A.done = done; A.sig = sig; A.task = task; A.mach = mach;
    A.late = late; A.tabu = tabu; A.tabu_n = tabu_n; A.best_obj = best_obj; A.best_task = best_task; A.best_mach = best_mach;
    A.next_col = next_col; A.cur_out = cur_obj_out; A.best_out = best_obj_out; A.pick_out = pick_out; A.why_out = why_out;
    A.barred_out = barred_out; A.obj_out = obj_out;
    if (K <= WALK_THREADS) return walk_launch<1>(h, v, A);
    if (K <= 4 * WALK_THREADS) return walk_launch<4>(h, v, A);
    return walk_launch<16>(h, v, A);
}
