// mtfjsp_nsga.hip — multi-front selection over groups of candidates (Pareto-front evolutionary search: parents and children of one
// instance are ranked together and the first P of the selection order are the next population; candidate c of group n = element
// n*Ka + c of the first array pair for c < Ka, element n*Kb + (c - Ka) of the second, so the two need no concatenation).
//   mtfjsp_front_rank       k_front_rank: one workgroup per group — the front index of every candidate by peeling (rank 0 =
//                           mtfjsp_group_reduce's front, then the front of what is left, ...), the crowding distance inside its front,
//                           the group's selection order, the size of front 0 and the smallest objective
//   mtfjsp_plan_survivors   k_plan_survivors: the first P candidates of every group's order, gathered into a population in history
//                           layout with their costs, ranks and the position as the fitness the next tournaments compare
// Arithmetic: the additions and products of the objective (the rule: mtfjsp_copy_costs.h), and per candidate and axis one subtraction, one subtraction
// and one division of the crowding distance and two additions of the three axes, never contracted.  Everything else is comparisons:
// both must equal a host model bit for bit.
// Cost of the peeling: 2 K dominance tests per candidate whatever the number of fronts (one pass counts every candidate's dominators,
// every ranked candidate is taken off the counts once), plus per front a barrier and a scan of the K ranks, 64 at a time.  A totally
// ordered group — every candidate a front of its own — is the slow extreme: K rounds of that scan.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_copy_costs.h"
#include "mtfjsp_env_dev.h"
#include "mtfjsp_plan_dev.h"
#include "mtfjsp_wave_select.h"

#define NSGA_WAVES 4                   // of a workgroup; one for a group of at most 64 candidates
#define NSGA_MAX_K 2048                // 88 KB of (mk, ec, tt, obj), crowd and rank in a workgroup's 160 KB
#define NSGA_BYTES 44                  // of LDS per candidate
#define NSGA_UNRANKED INT_MAX

// ---------------------------------------------------------------- front ranks, crowding distance, selection order
struct FrontArgs {
    int Ka, Kb;
    CopyWeights w;
    const double *cost4_a, *cost4_b;   // [N*Ka,4], [N*Kb,4] or null
    const uint8_t *done_a, *done_b;    // [N*Ka], [N*Kb] or null
    int *rank;                         // [N*K] or null
    double *crowd;                     // [N*K] or null
    int *order;                        // [N*K] or null
    int *front_size;                   // [N] or null
    double *best_obj;                  // [N] or null
};

// candidate q comes before candidate c of the same rank with crowding distances dq, dc: the larger distance, a NaN after every number,
// the lower index among equal ones or two NaNs
__device__ __forceinline__ bool nsga_crowd_first(double dq, double dc) { return dq > dc || (dq == dq && dc != dc); }

// Candidate c of group n lives in LDS as its record (mtfjsp_copy_costs.h) with its rank (NSGA_UNRANKED while the peeling has not reached it, -1 for an ineligible one) and its
// crowding distance beside it.  A workgroup has WAVES waves (one for K <= 64: four times as many groups per compute unit; else four);
// thread tid owns candidates tid, tid + 64*WAVES, ... (OWN at most: 1, 4 or 8 by K): it alone writes their rank and distance.  Every loop over q reads one LDS address for the whole workgroup (a broadcast).
template <int OWN, int WAVES>
__global__ __launch_bounds__(WAVES * WAVE) void k_front_rank(FrontArgs A)
{
    constexpr int THREADS = WAVES * WAVE;
    extern __shared__ __align__(32) unsigned char smem[];
    __shared__ double part_v[WAVES];
    __shared__ int part_i[WAVES], part_n[WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, Ka = A.Ka, Kb = A.Kb, K = Ka + Kb;
    const size_t g0 = (size_t)blockIdx.x * K;
    double4 *cp = reinterpret_cast<double4 *>(smem);
    double *cr = reinterpret_cast<double *>(smem + (size_t)K * 32);
    int *rk = reinterpret_cast<int *>(smem + (size_t)K * 40);
    // every load of this thread first (a candidate past K reads the group's last one again and is ignored)
    double c0[OWN], c1[OWN], c2[OWN], c3[OWN];
    uint8_t dn[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * THREADS, cc = c < K ? c : K - 1;
        const bool in_a = cc < Ka;
        const size_t g = in_a ? (size_t)blockIdx.x * Ka + cc : (size_t)blockIdx.x * Kb + (cc - Ka);
        const double *src = in_a ? A.cost4_a : A.cost4_b;
        c0[i] = src[g * 4]; c1[i] = src[g * 4 + 1]; c2[i] = src[g * 4 + 2]; c3[i] = src[g * 4 + 3];
        dn[i] = (in_a ? A.done_a : A.done_b)[g];
    }
    double mk[OWN], ec[OWN], tt[OWN], ob[OWN];
    int my[OWN];                                                        // the owned candidates' ranks (-1 also past K)
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * THREADS;
        const double m = c0[i], e = c1[i] + c3[i], t = c2[i];
        const double o = (A.w.mk * m + A.w.ec * e) + A.w.tt * t;
        const bool el = c < K && dn[i] != 0 && m == m && e == e && t == t;
        mk[i] = el ? m : (double)NAN; ec[i] = e; tt[i] = t; ob[i] = el ? o : (double)NAN;
        my[i] = el ? NSGA_UNRANKED : -1;
        if (c < K) {
            cp[c] = make_double4(mk[i], ec[i], tt[i], ob[i]);
            rk[c] = my[i];
        }
    }
    __syncthreads();
    // ---- the smallest objective, lowest candidate on ties (k_group_reduce's)
    WaveBest<false> mine;
#pragma unroll
    for (int i = 0; i < OWN; i++) {
        const int cw = wave * WAVE + i * THREADS;                      // (wave-uniform)
        if (cw < K) mine.pass(ob[i] == ob[i], ob[i], cw);
    }
    // ---- phase 1, the peeling: rank r holds the unranked candidates that no unranked candidate dominates.  One pass over q counts the dominators of every owned
    // candidate; round r ranks the unranked candidates whose count is zero (a strict partial order: there is one while any is left),
    // and every wave then takes them off the counts of its own candidates: it scans the ranks 64 at a time and tests only the new
    // members.  Every candidate is tested against every other twice in all, however many fronts there are; a round costs K / 64 steps
    // of the scan on top.  No barrier after the scan: the only writes it can meet turn NSGA_UNRANKED into r + 1, never into r
    int cnt[OWN];
#pragma unroll
    for (int i = 0; i < OWN; i++) cnt[i] = 0;
    for (int q = 0; q < K; q++) {
        const double4 o = cp[q];
#pragma unroll
        for (int i = 0; i < OWN; i++) cnt[i] += copy_dominates(o, q, mk[i], ec[i], tt[i], tid + i * THREADS) ? 1 : 0;
    }
    for (int r = 0; r < K; r++) {
        bool left = false;
#pragma unroll
        for (int i = 0; i < OWN; i++) {
            if (my[i] != NSGA_UNRANKED) continue;
            if (cnt[i] != 0) { left = true; continue; }
            my[i] = r;
            rk[tid + i * THREADS] = r;
        }
        if (!__syncthreads_or(left ? 1 : 0)) break;
        for (int q0 = 0; q0 < K; q0 += WAVE) {
            const int qq = q0 + lane;
            unsigned long long m = __ballot(qq < K && rk[qq < K ? qq : K - 1] == r);
            while (m) {                                                     // (wave-uniform)
                const int q = q0 + (int)__builtin_ctzll(m);
                m &= m - 1;
                const double4 o = cp[q];
#pragma unroll
                for (int i = 0; i < OWN; i++) cnt[i] -= copy_dominates(o, q, mk[i], ec[i], tt[i], tid + i * THREADS) ? 1 : 0;
            }
        }
    }
    // ---- the members of rank 0; the partial minima
    int n0 = 0;
#pragma unroll
    for (int i = 0; i < OWN; i++) n0 += __popcll(__ballot(my[i] == 0));
    if (lane == 0) { part_v[wave] = mine.v; part_i[wave] = mine.i; part_n[wave] = n0; }
    // ---- phase 2, the crowding distance of c among the members of its rank: per axis the neighbours below and above in (value, index)
    // order and the rank's extremes; and whether a member of the rank has a better objective (smaller, or equal with a lower index)
#pragma unroll 1
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * THREADS;
        if (c >= K) break;
        const int rc = rk[c];
        const double4 me = cp[c];
        const double x[3] = {me.x, me.y, me.z};
        double pred[3], succ[3], lo[3], hi[3];
        bool hp[3], hs[3];
#pragma unroll
        for (int a = 0; a < 3; a++) { pred[a] = succ[a] = 0.0; lo[a] = hi[a] = x[a]; hp[a] = hs[a] = false; }
        bool beaten = !(me.w == me.w);                                     // an objective that is NaN never is the rank's best
        for (int q = 0; q < K; q++) {
            if (rk[q] != rc || q == c || rc < 0) continue;
            const double4 o = cp[q];
            const double y[3] = {o.x, o.y, o.z};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const bool below = y[a] < x[a] || (y[a] == x[a] && q < c);
                if (below) {
                    if (!hp[a] || y[a] > pred[a]) pred[a] = y[a];
                    hp[a] = true;
                } else {
                    if (!hs[a] || y[a] < succ[a]) succ[a] = y[a];
                    hs[a] = true;
                }
                lo[a] = y[a] < lo[a] ? y[a] : lo[a];
                hi[a] = y[a] > hi[a] ? y[a] : hi[a];
            }
            beaten = beaten || o.w < me.w || (o.w == me.w && q < c);
        }
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!hp[a] || !hs[a]) d[a] = (double)INFINITY;
            else if (hi[a] == lo[a]) d[a] = 0.0;
            else d[a] = (succ[a] - pred[a]) / (hi[a] - lo[a]);
        }
        double crowd = (d[0] + d[1]) + d[2];
        if (!beaten) crowd = (double)INFINITY;                              // the rank's best objective is never crowded out
        if (rc < 0) crowd = (double)NAN;
        cr[c] = crowd;
        if (A.rank) A.rank[g0 + c] = rc;
        if (A.crowd) A.crowd[g0 + c] = crowd;
    }
    __syncthreads();
    if (tid == 0) {
        const int gi = wave_best_combine<false, WAVES>(part_v, part_i).i;
        int n0all = 0;
#pragma unroll
        for (int k = 0; k < WAVES; k++) n0all += part_n[k];
        if (A.best_obj) A.best_obj[blockIdx.x] = gi < 0 ? (double)NAN : cp[gi].w;   // the candidate's own word
        if (A.front_size) A.front_size[blockIdx.x] = n0all;
    }
    // ---- phase 3, the selection order: the position of c is the number of candidates that come before it — eligible before ineligible,
    // ascending rank, descending distance (a NaN last), ascending index: a strict total order, so the positions are a permutation
    if (!A.order) return;
#pragma unroll 1
    for (int i = 0; i < OWN; i++) {
        const int c = tid + i * THREADS;
        if (c >= K) break;
        const int rc = rk[c];
        const double dc = cr[c];
        int pos = 0;
        for (int q = 0; q < K; q++) {
            const int rq = rk[q];
            const double dq = cr[q];
            bool first;
            if (rc < 0) first = rq >= 0 || q < c;
            else first = rq >= 0 && (rq < rc || (rq == rc && (nsga_crowd_first(dq, dc) || (!nsga_crowd_first(dc, dq) && q < c))));
            pos += first ? 1 : 0;
        }
        A.order[g0 + pos] = c;
    }
}

template <int OWN, int WAVES>
static int front_launch(mtfjsp_handle_t h, const EnvHostView &v, int N, const FrontArgs &A)
{
    void (*fn)(FrontArgs) = k_front_rank<OWN, WAVES>;
    const size_t lds = (size_t)(A.Ka + A.Kb) * NSGA_BYTES;
    if (int rc = mtfjsp_env_dyn_lds(h, (const void *)fn, lds, "mtfjsp_front_rank")) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)N), dim3(WAVES * WAVE), lds, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_front_rank");
}

extern "C" int mtfjsp_front_rank(mtfjsp_handle_t h, int32_t N, int32_t Ka, int32_t Kb, const double *cost4_a, const uint8_t *done_a,
                                 const double *cost4_b, const uint8_t *done_b, const double *w3cfg_host, int32_t *rank_out, double *crowd_out,
                                 int32_t *order_out, int32_t *front_size_out, double *best_obj_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!cost4_a || !done_a || !w3cfg_host || (Kb != 0 && (!cost4_b || !done_b)))
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_front_rank: null argument");
    if (Ka < 1 || Kb < 0 || (long)Ka + Kb > NSGA_MAX_K || N < 1 || (long)N * ((long)Ka + Kb) > INT_MAX)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_front_rank: Ka >= 1, Kb >= 0, Ka + Kb <= 2048, N >= 1 and N*(Ka + Kb) must fit 31 bits");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_front_rank")) return rc;
    FrontArgs A{};
    A.Ka = Ka; A.Kb = Kb; A.w = copy_weights(w3cfg_host);
    A.cost4_a = cost4_a; A.done_a = done_a; A.cost4_b = cost4_b; A.done_b = done_b;
    A.rank = rank_out; A.crowd = crowd_out; A.order = order_out; A.front_size = front_size_out; A.best_obj = best_obj_out;
    const int K = Ka + Kb;
    if (K <= WAVE) return front_launch<1, 1>(h, v, N, A);
    if (K <= NSGA_WAVES * WAVE) return front_launch<1, NSGA_WAVES>(h, v, N, A);
    if (K <= 4 * NSGA_WAVES * WAVE) return front_launch<4, NSGA_WAVES>(h, v, N, A);
    return front_launch<8, NSGA_WAVES>(h, v, N, A);
}

// ---------------------------------------------------------------- survivors
struct SurvArgs {
    int B, T, N, Ka, Kb, P;
    const int *order, *rank;           // [N*K]
    const int *task_a, *mach_a, *task_b, *mach_b;   // [T,N*Ka], [T,N*Kb] or null
    const double *cost4_a, *cost4_b;
    const uint8_t *done_a, *done_b;
    int *task_out, *mach_out;          // [T,B], B = N*P
    double *cost4;                     // [B,4] or null
    uint8_t *done;                     // [B] or null
    int *rank_out, *src_out;           // [B] or null
    double *fit;                       // [B] or null
};

// one thread per (row, output column): blockIdx.y = the row s, so a wave writes 64 consecutive words of row s and reads inside the
// columns of one or two groups; the threads of row 0 also write what a column has once
__global__ __launch_bounds__(256) void k_plan_survivors(SurvArgs A)
{
    const long col = (long)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (col >= A.B) return;
    const int K = A.Ka + A.Kb, n = (int)(col / A.P), i = (int)(col - (long)n * A.P);
    const int c = A.order[(size_t)n * K + i];
    const bool ok = (unsigned)c < (unsigned)K, in_a = !ok || c < A.Ka;
    const size_t width = in_a ? (size_t)A.N * A.Ka : (size_t)A.N * A.Kb;
    const size_t g = !ok ? 0 : (in_a ? (size_t)n * A.Ka + c : (size_t)n * A.Kb + (c - A.Ka));
    int tk = -1, mc = -1;
    if (ok) {
        tk = (in_a ? A.task_a : A.task_b)[(size_t)s * width + g];
        mc = (in_a ? A.mach_a : A.mach_b)[(size_t)s * width + g];
    }
    A.task_out[(size_t)s * A.B + col] = tk;
    A.mach_out[(size_t)s * A.B + col] = mc;
    if (s != 0) return;
    const int rc = ok ? A.rank[(size_t)n * K + c] : -1;
    if (A.cost4) {
        const double *src = (in_a ? A.cost4_a : A.cost4_b) + g * 4;
#pragma unroll
        for (int k = 0; k < 4; k++) A.cost4[(size_t)col * 4 + k] = ok ? src[k] : (double)NAN;
    }
    if (A.done) A.done[col] = ok ? (in_a ? A.done_a : A.done_b)[g] : 0;
    if (A.rank_out) A.rank_out[col] = rc;
    if (A.src_out) A.src_out[col] = c;
    if (A.fit) A.fit[col] = rc >= 0 ? (double)i : (double)NAN;
}

extern "C" int mtfjsp_plan_survivors(mtfjsp_handle_t h, int32_t N, int32_t Ka, int32_t Kb, int32_t P, const int32_t *order, const int32_t *rank,
                                     const int32_t *task_a, const int32_t *mach_a, const double *cost4_a, const uint8_t *done_a,
                                     const int32_t *task_b, const int32_t *mach_b, const double *cost4_b, const uint8_t *done_b,
                                     int32_t *task_out, int32_t *mach_out, double *cost4_out, uint8_t *done_out, int32_t *rank_out,
                                     int32_t *src_out, double *fit_out)
{
    const char *who = "mtfjsp_plan_survivors";
    if (!h) return MTFJSP_ERR_ARG;
    if (!order || !rank || !task_a || !mach_a || !cost4_a || !done_a || !task_out || !mach_out ||
        (Kb != 0 && (!task_b || !mach_b || !cost4_b || !done_b)))
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_survivors: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    const long K = (long)Ka + Kb;
    if (Ka < 1 || Kb < 0 || N < 1 || (long)N * K > INT_MAX || P < 1 || P > K || (long)N * P != (long)v.B || v.T > 65535)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_survivors: Ka >= 1, Kb >= 0, N >= 1, 1 <= P <= Ka + Kb, N*(Ka + Kb) must fit 31 bits and N*P must be the handle's batch");
    const unsigned __int128 T4 = (unsigned __int128)v.T * 4, na = (unsigned __int128)N * Ka, nb = (unsigned __int128)N * Kb, nk = (unsigned __int128)N * K,
                            np = (unsigned __int128)v.B;
    const PlanSpan srcs[10] = {{order, nk * 4}, {rank, nk * 4}, {task_a, T4 * na}, {mach_a, T4 * na}, {cost4_a, na * 32}, {done_a, na},
                               {Kb ? task_b : nullptr, T4 * nb}, {Kb ? mach_b : nullptr, T4 * nb}, {Kb ? cost4_b : nullptr, nb * 32}, {Kb ? done_b : nullptr, nb}};
    const PlanSpan outs[7] = {{task_out, T4 * np}, {mach_out, T4 * np}, {cost4_out, np * 32}, {done_out, np}, {rank_out, np * 4}, {src_out, np * 4}, {fit_out, np * 8}};
    if (int rc = plan_check_overlap(h, who, 7, outs, 10, srcs)) return rc;
    if (int rc = mtfjsp_env_set_device(h, v.device_id, who)) return rc;
    SurvArgs A{};
    A.B = v.B; A.T = v.T; A.N = N; A.Ka = Ka; A.Kb = Kb; A.P = P; A.order = order; A.rank = rank;
    A.task_a = task_a; A.mach_a = mach_a; A.cost4_a = cost4_a; A.done_a = done_a;
    A.task_b = task_b; A.mach_b = mach_b; A.cost4_b = cost4_b; A.done_b = done_b;
    A.task_out = task_out; A.mach_out = mach_out; A.cost4 = cost4_out; A.done = done_out; A.rank_out = rank_out; A.src_out = src_out; A.fit = fit_out;
    hipLaunchKernelGGL(k_plan_survivors, dim3((unsigned)(((size_t)v.B + 255) / 256), (unsigned)v.T), dim3(256), 0, v.stream, A);
    return mtfjsp_env_launched(h, who);
}
