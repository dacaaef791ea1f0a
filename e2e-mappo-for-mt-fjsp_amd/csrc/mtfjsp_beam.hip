// mtfjsp_beam.hip — beam search over (job, machine) decisions on the device fork.  A beam handle holds W partial schedules ("slots")
// for each of N source instances; a decision expands every slot into its T = J*M children exactly as the one-step look-ahead does
// (mtfjsp_lookahead_expand on (scratch, beam) and one ordinary step of the scratch handle: csrc/mtfjsp_lookahead.hip), keeps the W
// best of the W*T children per source instance and makes them the next beam with the explicit-index fork (mtfjsp_fork).
//   mtfjsp_state_signature   k_state_signature: one wavefront per instance, a 64-bit order-independent hash of its partial schedule
//   mtfjsp_beam_select       k_beam_select: one workgroup per source instance, W ranks over W*T candidates kept in LDS
//   mtfjsp_beam_backtrack    k_beam_backtrack: one thread per source instance walks the back-pointers
// A candidate's value is ONE binary64 addition (parent score + raw[column]); everything else is comparisons and integer arithmetic:
// the selection must equal a host model's bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_wave_select.h"

#define BEAM_WAVES 4
#define BEAM_THREADS (BEAM_WAVES * WAVE)
#define BEAM_MAX_W 64
#define BEAM_MAX_CAND 8192             // 128 KB of (value, signature) pairs in a workgroup's 160 KB

typedef unsigned long long u64;

// ---------------------------------------------------------------- signature
__device__ __forceinline__ u64 sig_mix(u64 z)                      // splitmix64's finaliser
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

struct SigArgs {
    int B, T;
    const TaskSD *sd;                  // [B,T]
    const TaskPL *pl;                  // [B,T]
    u64 *out;                          // [B]
};

// lanes over the tasks of one instance (64 at a time); the sum is an integer one: any order of addition gives the same word
__global__ __launch_bounds__(BEAM_THREADS) void k_state_signature(SigArgs A)
{
    const int lane = threadIdx.x & (WAVE - 1), T = A.T;
    const long i = (long)blockIdx.x * BEAM_WAVES + (threadIdx.x >> 6);
    const size_t base = (size_t)(i < A.B ? i : A.B - 1) * T;
    u64 acc = 0;
    for (int k0 = 0; k0 < T; k0 += WAVE) {
        const int k = k0 + lane, kk = k < T ? k : T - 1;
        const double st = A.sd[base + kk].st;
        const Link l = A.pl[base + kk].link;
        const u64 where = ((u64)(unsigned)k << 32) | ((u64)(unsigned short)l.mach << 16) | (u64)(unsigned short)l.pos;
        const u64 c = sig_mix(sig_mix((u64)__double_as_longlong(st)) + where);
        acc += (k < T && l.mach >= 0) ? c : 0ull;
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) acc += __shfl_xor(acc, d, WAVE);
    if (lane == 0 && i < A.B) A.out[i] = acc;
}

extern "C" int mtfjsp_state_signature(mtfjsp_handle_t h, uint64_t *sig_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!sig_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_state_signature: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.has_schedule()) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_state_signature: the handle holds no schedule (never reset, or plans replayed without MTFJSP_REPLAY_STATE)");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_state_signature")) return rc;
    SigArgs A{};
    A.B = v.B; A.T = v.T; A.sd = v.sd; A.pl = v.pl; A.out = (u64 *)sig_out;
    hipLaunchKernelGGL(k_state_signature, dim3((unsigned)(((size_t)v.B + BEAM_WAVES - 1) / BEAM_WAVES)), dim3(BEAM_THREADS), 0, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_state_signature");
}

// ---------------------------------------------------------------- selection
struct BeamArgs {
    int W, T, M, MJ, column;
    const MJRec *mj;                   // beam: [N*W,MJ], .cnt of element j = scheduled operations of job j
    const int *status;                 // scratch: [N*W*T]
    const double *raw;                 // scratch: [N*W*T,5]
    const double *score_in;            // [N*W], -inf = empty slot
    const u64 *sig;                    // scratch: [N*W*T] or null
    int *parent, *from_slot, *task, *mach;     // [N*W]
    double *score_out;                 // [N*W]
};

// Candidate c = w*T + r of source instance n (slot w, child r = j*M + m) lives in LDS as its value, NaN once it cannot be picked
// any more (not eligible, picked, or merged into a pick); thread c % 256 owns it — it alone reads and writes val[c] after the
// first barrier, so a rank needs one barrier: the one between the waves' partial results and their combination.  A wave takes its
// candidates 64 at a time in ascending c and a later pass wins only with a strictly larger value; the four partial results are
// combined by (value, then lower c): the lowest index of the maximum, whatever the number of waves (WaveBest, mtfjsp_wave_select.h).
__global__ __launch_bounds__(BEAM_THREADS) void k_beam_select(BeamArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double part_v[2][BEAM_WAVES];
    __shared__ int part_i[2][BEAM_WAVES];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int W = A.W, T = A.T, M = A.M, C = W * T;
    double *val = reinterpret_cast<double *>(smem);
    u64 *sg = reinterpret_cast<u64 *>(smem) + C;                            // (present only with A.sig)
    const size_t slot0 = (size_t)n * W;
    for (int c = tid; c < C; c += BEAM_THREADS) {
        const int w = c / T;
        const size_t g = slot0 * T + c;                                     // (slot0 + w) * T + r
        const double s = A.score_in[slot0 + w];
        const int st = A.status[g];
        const double v = s + A.raw[g * 5 + A.column];
        val[c] = (s != -INFINITY && !(st & (MTFJSP_ST_INVALID | MTFJSP_ST_INFEASIBLE))) ? v : (double)NAN;
        if (A.sig) sg[c] = A.sig[g];
    }
    __syncthreads();
    for (int k = 0; k < W; k++) {
        WaveBest<true> mine;
        for (int c0 = wave * WAVE; c0 < C; c0 += BEAM_THREADS) {
            const int c = c0 + lane;
            const double v = c < C ? val[c] : (double)NAN;
            mine.pass(v == v, v, c0);                                       // a NaN is never selected
        }
        if (lane == 0) { part_v[k & 1][wave] = mine.v; part_i[k & 1][wave] = mine.i; }
        __syncthreads();
        const WaveBest<true> all = wave_best_combine<true, BEAM_WAVES>(part_v[k & 1], part_i[k & 1]);
        const double gb = all.v;
        const int gi = all.i;
        if (gi < 0) {
            if (k == 0) {                                                   // nothing to pick at all (finished): the beam is kept
                for (int q = tid; q < W; q += BEAM_THREADS) {
                    A.parent[slot0 + q] = -1; A.from_slot[slot0 + q] = q; A.task[slot0 + q] = -1; A.mach[slot0 + q] = -1;
                    A.score_out[slot0 + q] = A.score_in[slot0 + q];
                }
                return;
            }
            if (tid == 0) {                                                 // exhausted rank: an empty slot
                A.parent[slot0 + k] = -1; A.from_slot[slot0 + k] = -1; A.task[slot0 + k] = -1; A.mach[slot0 + k] = -1;
                A.score_out[slot0 + k] = -INFINITY;
            }
            continue;
        }
        if (tid == 0) {
            const int w = gi / T, r = gi - w * T, j = r / M;
            const int cnt = A.mj[(slot0 + w) * A.MJ + j].cnt;
            A.parent[slot0 + k] = (int)(slot0 * T) + gi;
            A.from_slot[slot0 + k] = w;
            A.task[slot0 + k] = j * M + (cnt < M ? cnt : M - 1);
            A.mach[slot0 + k] = r - j * M;
            A.score_out[slot0 + k] = gb;
        }
        if (A.sig) {
            const u64 sw = sg[gi];
            for (int c = tid; c < C; c += BEAM_THREADS)
                if (sg[c] == sw) val[c] = (double)NAN;                      // the pick itself and every duplicate of it
        } else if (tid == (gi & (BEAM_THREADS - 1))) {
            val[gi] = (double)NAN;
        }
    }
}

extern "C" int mtfjsp_beam_select(mtfjsp_handle_t scratch, mtfjsp_handle_t beam, int32_t W, int32_t column, const double *score_in, const uint64_t *sig,
                                  int32_t *parent_out, int32_t *from_slot_out, int32_t *task_out, int32_t *mach_out, double *score_out)
{
    if (!scratch) return MTFJSP_ERR_ARG;
    if (!beam || !score_in || !parent_out || !from_slot_out || !task_out || !mach_out || !score_out)
        return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_beam_select: null argument");
    if (column < 0 || column > 4) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_beam_select: column must be 0..4 (reward, makespan, idle, energy, transport)");
    if (score_out == score_in) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_beam_select: score_out must not be score_in (every rank reads all parent scores)");
    EnvHostView sc, bm;
    int rc = mtfjsp_env_pair_views("mtfjsp_beam_select", "beam", scratch, beam, &sc, &bm);
    if (rc) return rc;
    if (W < 1 || W > BEAM_MAX_W || bm.B % W) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_beam_select: the width must be 1..64 and divide the beam handle's batch");
    if ((long)W * bm.T > BEAM_MAX_CAND) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_beam_select: width * n_job * n_machine must not exceed 8192 candidates");
    if (!sc.was_reset || !bm.was_reset) return mtfjsp_env_fail(scratch, MTFJSP_ERR_STATE, "mtfjsp_beam_select: both handles must hold a state (mtfjsp_lookahead_expand and a step first)");
    if (!sc.obs_bound || !sc.obs.raw) return mtfjsp_env_fail(scratch, MTFJSP_ERR_STATE, "mtfjsp_beam_select: the scratch handle needs bound observations with raw");
    if ((rc = mtfjsp_env_set_device(scratch, bm.device_id, "mtfjsp_beam_select"))) return rc;
    const size_t lds = (size_t)W * bm.T * (sig ? 16 : 8);
    if ((rc = mtfjsp_env_dyn_lds(scratch, (const void *)k_beam_select, lds, "mtfjsp_beam_select"))) return rc;
    BeamArgs A{};
    A.W = W; A.T = bm.T; A.M = bm.M; A.MJ = bm.MJ; A.column = column; A.mj = bm.mj; A.status = sc.obs.status; A.raw = sc.obs.raw;
    A.score_in = score_in; A.sig = (const u64 *)sig; A.parent = parent_out; A.from_slot = from_slot_out; A.task = task_out; A.mach = mach_out;
    A.score_out = score_out;
    hipLaunchKernelGGL(k_beam_select, dim3((unsigned)(bm.B / W)), dim3(BEAM_THREADS), lds, bm.stream, A);
    return mtfjsp_env_launched(scratch, "mtfjsp_beam_select");
}

// ---------------------------------------------------------------- back-pointers
struct BackArgs {
    int N, W, S;
    const int *from_slot, *task, *mach;        // [S,N*W]
    const int *start;                          // [N] or null
    int *task_plan, *mach_plan;                // [N,S]
};

__global__ __launch_bounds__(256) void k_beam_backtrack(BackArgs A)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= A.N) return;
    const size_t row = (size_t)A.N * A.W;
    int k = A.start ? A.start[n] : 0;
    for (int s = A.S - 1; s >= 0; s--) {
        if (k < 0 || k >= A.W) k = -1;                                      // an empty slot: nothing before it either
        const size_t at = (size_t)s * row + (size_t)n * A.W + (k < 0 ? 0 : k);
        A.task_plan[(size_t)n * A.S + s] = k < 0 ? -1 : A.task[at];
        A.mach_plan[(size_t)n * A.S + s] = k < 0 ? -1 : A.mach[at];
        k = k < 0 ? -1 : A.from_slot[at];
    }
}

extern "C" int mtfjsp_beam_backtrack(mtfjsp_handle_t h, int32_t W, int32_t S, const int32_t *hist_from_slot, const int32_t *hist_task,
                                     const int32_t *hist_mach, const int32_t *start_slot, int32_t *task_plan, int32_t *mach_plan)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!hist_from_slot || !hist_task || !hist_mach || !task_plan || !mach_plan) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_beam_backtrack: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (W < 1 || W > BEAM_MAX_W || v.B % W || S < 1) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_beam_backtrack: the width must be 1..64 and divide the handle's batch, steps >= 1");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_beam_backtrack")) return rc;
    BackArgs A{};
    A.N = v.B / W; A.W = W; A.S = S; A.from_slot = hist_from_slot; A.task = hist_task; A.mach = hist_mach; A.start = start_slot;
    A.task_plan = task_plan; A.mach_plan = mach_plan;
    hipLaunchKernelGGL(k_beam_backtrack, dim3((unsigned)((A.N + 255) / 256)), dim3(256), 0, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_beam_backtrack");
}
