// mtfjsp_policy_beam.hip — beam decoding of the trained policy on the device fork.  A beam handle holds W partial schedules
// ("slots") for each of N source instances, as in mtfjsp_beam.hip; here a slot's score is the running sum of the two actors' log
// probabilities, and only the W children that are kept are stepped.  The machine actor's distribution exists per chosen task, so a
// decision asks it about every job's candidate task at once:
//   mtfjsp_observe_mfea1_jobs   k_mfea1_jobs: thread = (instance, job, machine), the machine actor's first input for every job
//   mtfjsp_beam_select_policy   k_beam_select_policy: one workgroup per source instance, W ranks over W*T candidates kept in LDS
//   mtfjsp_beam_merge_slots     k_beam_merge_slots: one workgroup per source instance, later slots of one signature emptied
// A candidate's value is TWO binary64 additions, (score + log p(job)) + log p(machine | job), in that order; everything else is
// comparisons and integer arithmetic: the selection must equal a host model's bit for bit.  The logarithms are inputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_wave_select.h"

#define PB_WAVES 4
#define PB_THREADS (PB_WAVES * WAVE)
#define PB_MAX_W 64
#define PB_MAX_CAND 8192               // 64 KB of values in a workgroup's 160 KB: mtfjsp_beam_select's limit

typedef unsigned long long u64;

// ---------------------------------------------------------------- m_fea1 of every job's candidate task
// k_mfea1 (mtfjsp_env.hip; pe:152-214) with task_idx[b] = candidate[b][j] and no mask given: the same expressions on the same words
template <typename OBS>
__global__ __launch_bounds__(256) void k_mfea1_jobs(long n, int J, int T, int M, const double *t, const double *p, const double *tt, const double *mean3,
                                                    const int *shop, const TaskPL *pl, const int *cand, OBS *out, uint8_t *mmask_out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;               // (b*J + j)*M + m
    if (i >= n) return;
    const long bj = i / M;
    const int m = (int)(i - bj * M);
    const long b = bj / J;
    int a = cand[bj];
    if (a < 0 || a >= T) a = 0;
    const size_t row = (size_t)b * T + a;
    const double tv = t[row * M + m], pv = p[row * M + m];
    const double ptv = tv * fabs(pv);
    const uint8_t mk = (uint8_t)!(tv >= 0);                            // run:258-259 ~(t >= 0)
    double x = 0.0;
    if (a % M != 0) {
        int pm = pl[row - 1].link.mach;                                // == tasks_fea[a-1][5] - 1 (pe:206)
        if (pm < 0) pm += M;                                           // python negative index on an unscheduled predecessor
        x = tt[((size_t)b * M + pm) * M + m];
    }
    OBS *o = out + (size_t)i * 6;
    o[0] = (OBS)(tv > 0 ? tv : mean3[row * 3 + 0]);
    o[1] = (OBS)(ptv > 0 ? ptv : mean3[row * 3 + 1]);
    o[2] = (OBS)x;
    o[3] = (OBS)(1 - (int)mk);
    o[4] = (OBS)(pv > 0 ? pv : mean3[row * 3 + 2]);
    o[5] = (OBS)(shop[(size_t)b * M + m] + 1);
    if (mmask_out) mmask_out[i] = mk;
}

extern "C" int mtfjsp_observe_mfea1_jobs(mtfjsp_handle_t h, void *out, uint8_t *mmask_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_observe_mfea1_jobs: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.loaded || !v.obs_bound || !v.was_reset || !v.obs.candidate)
        return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_observe_mfea1_jobs: the handle needs a reset and bound observations with candidate");
    mtfjsp_mfea1_ctx_t cx;
    if (int rc = mtfjsp_get_mfea1_context(h, out, (uint8_t *)out, &cx)) return rc;         // the instance arrays k_mfea1 reads
    const size_t n = (size_t)v.B * v.J * v.M, osz = cx.obs_f32 ? 4 : 8;
    if (mmask_out) {
        const uintptr_t a0 = (uintptr_t)out, a1 = a0 + n * 6 * osz, b0 = (uintptr_t)mmask_out, b1 = b0 + n;
        if (a0 < b1 && b0 < a1) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_observe_mfea1_jobs: out and mmask_out overlap");
    }
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_observe_mfea1_jobs")) return rc;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (cx.obs_f32)
        hipLaunchKernelGGL((k_mfea1_jobs<float>), grid, dim3(256), 0, v.stream, (long)n, v.J, v.T, v.M, cx.t, cx.p, cx.tt, cx.mean3, cx.shop,
                           (const TaskPL *)cx.link, v.obs.candidate, (float *)out, mmask_out);
    else
        hipLaunchKernelGGL((k_mfea1_jobs<double>), grid, dim3(256), 0, v.stream, (long)n, v.J, v.T, v.M, cx.t, cx.p, cx.tt, cx.mean3, cx.shop,
                           (const TaskPL *)cx.link, v.obs.candidate, (double *)out, mmask_out);
    return mtfjsp_env_launched(h, "mtfjsp_observe_mfea1_jobs");
}

// ---------------------------------------------------------------- selection
struct PolicyBeamArgs {
    int W, T, M, J, MJ;
    const MJRec *mj;                   // beam: [N*W,MJ], .cnt of element j = scheduled operations of job j
    const uint8_t *job_mask;           // beam: [N*W,J]
    const double *score_in;            // [N*W], -inf = empty slot
    const double *logp_job;            // [N*W,J]
    const double *logp_mach;           // [N*W*J,M]
    const uint8_t *mmask;              // [N*W*J,M]
    int *parent, *from_slot, *job, *task, *mach, *child;       // [N*W]
    double *score_out;                 // [N*W]
};

// k_beam_select's ranks (mtfjsp_beam.hip) over another value: candidate c = w*T + j*M + m of source instance n lives in LDS as its
// value, NaN once it cannot be picked (not eligible, or picked); thread c % 256 owns it, so a rank needs one barrier: the one between
// the waves' partial results and their combination (WaveBest, mtfjsp_wave_select.h: the lowest index of the maximum).
__global__ __launch_bounds__(PB_THREADS) void k_beam_select_policy(PolicyBeamArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double part_v[2][PB_WAVES];
    __shared__ int part_i[2][PB_WAVES];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int W = A.W, T = A.T, M = A.M, J = A.J, C = W * T;
    double *val = reinterpret_cast<double *>(smem);
    const size_t slot0 = (size_t)n * W;
    for (int c = tid; c < C; c += PB_THREADS) {
        const int w = c / T, j = (c - w * T) / M;
        const size_t g = slot0 * T + c;                                     // ((slot0 + w)*J + j)*M + m
        const size_t sj = (slot0 + w) * J + j;
        const double s = A.score_in[slot0 + w];
        const double v = (s + A.logp_job[sj]) + A.logp_mach[g];
        const bool ok = s != -INFINITY && A.job_mask[sj] == 0 && A.mmask[g] == 0 && v == v && v != -INFINITY;
        val[c] = ok ? v : (double)NAN;
    }
    __syncthreads();
    for (int k = 0; k < W; k++) {
        WaveBest<true> mine;
        for (int c0 = wave * WAVE; c0 < C; c0 += PB_THREADS) {
            const int c = c0 + lane;
            const double v = c < C ? val[c] : (double)NAN;
            mine.pass(v == v, v, c0);                                       // a NaN is never selected
        }
        if (lane == 0) { part_v[k & 1][wave] = mine.v; part_i[k & 1][wave] = mine.i; }
        __syncthreads();
        const WaveBest<true> all = wave_best_combine<true, PB_WAVES>(part_v[k & 1], part_i[k & 1]);
        const int gi = all.i;
        if (gi < 0) {                                                       // exhausted rank: an empty slot
            if (tid == 0) {
                const size_t o = slot0 + k;
                A.parent[o] = -1; A.from_slot[o] = -1; A.job[o] = -1; A.task[o] = -1; A.mach[o] = -1; A.child[o] = -1;
                A.score_out[o] = -INFINITY;
            }
            continue;
        }
        if (tid == 0) {
            const int w = gi / T, r = gi - w * T, j = r / M;
            const int cnt = A.mj[(slot0 + w) * A.MJ + j].cnt;
            const size_t o = slot0 + k;
            A.parent[o] = (int)(slot0 + w);
            A.from_slot[o] = w;
            A.job[o] = j;
            A.task[o] = j * M + (cnt < M ? cnt : M - 1);
            A.mach[o] = r - j * M;
            A.child[o] = (int)((slot0 + w) * J + j);
            A.score_out[o] = all.v;
        }
        if (tid == (gi & (PB_THREADS - 1))) val[gi] = (double)NAN;
    }
}

extern "C" int mtfjsp_beam_select_policy(mtfjsp_handle_t beam, int32_t W, const double *score_in, const double *logp_job, const double *logp_mach,
                                         const uint8_t *mmask, int32_t *parent_out, int32_t *from_slot_out, int32_t *job_out, int32_t *task_out,
                                         int32_t *mach_out, int32_t *child_out, double *score_out)
{
    if (!beam) return MTFJSP_ERR_ARG;
    if (!score_in || !logp_job || !logp_mach || !mmask || !parent_out || !from_slot_out || !job_out || !task_out || !mach_out || !child_out || !score_out)
        return mtfjsp_env_fail(beam, MTFJSP_ERR_ARG, "mtfjsp_beam_select_policy: null argument");
    if (score_out == score_in) return mtfjsp_env_fail(beam, MTFJSP_ERR_ARG, "mtfjsp_beam_select_policy: score_out must not be score_in (every rank reads all parent scores)");
    EnvHostView bm;
    mtfjsp_env_host_view(beam, &bm);
    if (W < 1 || W > PB_MAX_W || bm.B % W) return mtfjsp_env_fail(beam, MTFJSP_ERR_ARG, "mtfjsp_beam_select_policy: the width must be 1..64 and divide the beam handle's batch");
    if ((long)W * bm.T > PB_MAX_CAND) return mtfjsp_env_fail(beam, MTFJSP_ERR_ARG, "mtfjsp_beam_select_policy: width * n_job * n_machine must not exceed 8192 candidates");
    if ((size_t)bm.B * bm.J >= (size_t)1 << 31) return mtfjsp_env_fail(beam, MTFJSP_ERR_ARG, "mtfjsp_beam_select_policy: batch * n_job must stay below 2^31 (child_out is int32)");
    if (!bm.was_reset) return mtfjsp_env_fail(beam, MTFJSP_ERR_STATE, "mtfjsp_beam_select_policy: the beam handle must hold a state");
    if (!bm.obs_bound || !bm.obs.job_mask) return mtfjsp_env_fail(beam, MTFJSP_ERR_STATE, "mtfjsp_beam_select_policy: the beam handle needs bound observations with job_mask");
    int rc;
    if ((rc = mtfjsp_env_set_device(beam, bm.device_id, "mtfjsp_beam_select_policy"))) return rc;
    const size_t lds = (size_t)W * bm.T * 8;
    if ((rc = mtfjsp_env_dyn_lds(beam, (const void *)k_beam_select_policy, lds, "mtfjsp_beam_select_policy"))) return rc;
    PolicyBeamArgs A{};
    A.W = W; A.T = bm.T; A.M = bm.M; A.J = bm.J; A.MJ = bm.MJ; A.mj = bm.mj; A.job_mask = bm.obs.job_mask;
    A.score_in = score_in; A.logp_job = logp_job; A.logp_mach = logp_mach; A.mmask = mmask;
    A.parent = parent_out; A.from_slot = from_slot_out; A.job = job_out; A.task = task_out; A.mach = mach_out; A.child = child_out;
    A.score_out = score_out;
    hipLaunchKernelGGL(k_beam_select_policy, dim3((unsigned)(bm.B / W)), dim3(PB_THREADS), lds, bm.stream, A);
    return mtfjsp_env_launched(beam, "mtfjsp_beam_select_policy");
}

// ---------------------------------------------------------------- merged slots
// thread k = slot k of source instance blockIdx.x; signatures and ENTRY scores are staged in LDS before anything is written
__global__ __launch_bounds__(PB_MAX_W) void k_beam_merge_slots(int W, const u64 *sig, double *score)
{
    __shared__ u64 sg[PB_MAX_W];
    __shared__ double sc[PB_MAX_W];
    const int k = threadIdx.x;
    const size_t slot0 = (size_t)blockIdx.x * W;
    if (k < W) { sg[k] = sig[slot0 + k]; sc[k] = score[slot0 + k]; }
    __syncthreads();
    if (k >= W) return;
    bool dup = false;
    for (int q = 0; q < k; q++) dup = dup || (sg[q] == sg[k] && sc[q] != -INFINITY);
    if (dup) score[slot0 + k] = -INFINITY;
}

extern "C" int mtfjsp_beam_merge_slots(mtfjsp_handle_t h, int32_t W, const uint64_t *sig, double *score_inout)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!sig || !score_inout) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_beam_merge_slots: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (W < 1 || W > PB_MAX_W || v.B % W) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_beam_merge_slots: the width must be 1..64 and divide the handle's batch");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_beam_merge_slots")) return rc;
    hipLaunchKernelGGL(k_beam_merge_slots, dim3((unsigned)(v.B / W)), dim3(PB_MAX_W), 0, v.stream, W, (const u64 *)sig, score_inout);
    return mtfjsp_env_launched(h, "mtfjsp_beam_merge_slots");
}
