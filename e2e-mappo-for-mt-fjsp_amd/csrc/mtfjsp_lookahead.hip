// mtfjsp_lookahead.hip — one-step look-ahead dispatch rules on the device fork (mtfjsp_fork, csrc/mtfjsp_env.hip).  The reference's
// idle-time rule (LWKR_IT_o_jointActor, tester/pdrs.py:465-540, "pdrs:") tries every candidate by env.reset() plus a replay of the
// whole prefix — O(T^2 J) environment steps per instance, which is why the reference ships it commented out (pdrs:695-700).  Here a
// decision is: fork the B source instances into B*T scratch copies (one per (job, machine)), one ordinary step of the scratch
// handle with the candidate actions, and a selection of the best copy per source instance.
//   mtfjsp_lookahead_expand   k_env_fork (STATE, implicit index i / T) + k_lookahead_actions
//   mtfjsp_lookahead_select   k_lookahead_select: one wavefront per source instance, lanes over its T copies
// Values are compared as binary64 and never computed with: the selection must equal a host model's bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_wave_select.h"

struct LaArgs {
    int B, J, M, T, MJ, column;
    const MJRec *mj;                   // source: [B,MJ], .cnt of element j = scheduled operations of job j
    const int *status;                 // scratch: [B*T]
    const double *raw;                 // scratch: [B*T,5]
    int *task, *mach, *job;            // expand: task, mach [B*T] | select: [B] (job may be null)
    double *best;                      // select: [B] or null
};

// candidate actions (pdrs:486-492: every job's next task; here times every machine): copy (b, j, m) = job j's next operation — the
// last one again for a finished job, which the step rejects — on machine m
__global__ __launch_bounds__(256) void k_lookahead_actions(LaArgs A)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x, n = (unsigned)A.B * (unsigned)A.T;
    const unsigned c = i < n ? i : n - 1;
    const unsigned b = c / (unsigned)A.T, r = c - b * (unsigned)A.T, j = r / (unsigned)A.M, m = r - j * (unsigned)A.M;
    const int cnt = A.mj[(size_t)b * A.MJ + j].cnt;
    if (i < n) {
        A.task[i] = (int)(j * (unsigned)A.M) + (cnt < A.M ? cnt : A.M - 1);
        A.mach[i] = (int)m;
    }
}

// ONE: T <= 64 — a single pass, straight-line.  Otherwise the copies are taken 64 at a time; a later pass wins only with a strictly
// larger value, so the lowest index of the maximum is kept (WaveBest, mtfjsp_wave_select.h).
template <bool ONE>
__global__ __launch_bounds__(64) void k_lookahead_select(LaArgs A)
{
    const int b = blockIdx.x, lane = threadIdx.x, T = A.T, M = A.M;
    const size_t base = (size_t)b * T;
    WaveBest<true> w;
    for (int c0 = 0; c0 < (ONE ? 1 : T); c0 += WAVE) {
        const int c = c0 + lane, cc = c < T ? c : T - 1;
        const int st = A.status[base + cc];
        const double v = A.raw[(base + cc) * 5 + A.column];
        w.pass(c < T && !(st & (MTFJSP_ST_INVALID | MTFJSP_ST_INFEASIBLE)), v, c0);
    }
    const int bi = w.i;
    const int j = bi < 0 ? 0 : bi / M;
    const int cnt = A.mj[(size_t)b * A.MJ + j].cnt;
    if (lane == 0) {
        A.task[b] = bi < 0 ? -1 : j * M + (cnt < M ? cnt : M - 1);
        A.mach[b] = bi < 0 ? -1 : bi - j * M;
        if (A.job) A.job[b] = bi < 0 ? -1 : j;
        if (A.best) A.best[b] = bi < 0 ? (double)NAN : w.v;
    }
}

extern "C" int mtfjsp_lookahead_expand(mtfjsp_handle_t scratch, mtfjsp_handle_t src, int32_t *task_c, int32_t *mach_c)
{
    if (!scratch) return MTFJSP_ERR_ARG;
    if (!src || !task_c || !mach_c) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_lookahead_expand: null argument");
    EnvHostView sc, so;
    int rc = mtfjsp_env_pair_views("mtfjsp_lookahead_expand", "source", scratch, src, &sc, &so);
    if (rc) return rc;
    rc = mtfjsp_env_fork_launch(scratch, src, nullptr, so.T, MTFJSP_FORK_STATE, "mtfjsp_lookahead_expand");
    if (rc) return rc;
    LaArgs A{};
    A.B = so.B; A.J = so.J; A.M = so.M; A.T = so.T; A.MJ = so.MJ; A.mj = so.mj; A.task = task_c; A.mach = mach_c;
    hipLaunchKernelGGL(k_lookahead_actions, dim3((unsigned)(((size_t)sc.B + 255) / 256)), dim3(256), 0, sc.stream, A);
    return mtfjsp_env_launched(scratch, "mtfjsp_lookahead_expand");
}

extern "C" int mtfjsp_lookahead_select(mtfjsp_handle_t scratch, mtfjsp_handle_t src, int32_t column, int32_t *task_out, int32_t *mach_out,
                                       int32_t *job_out, double *best_out)
{
    if (!scratch) return MTFJSP_ERR_ARG;
    if (!src || !task_out || !mach_out) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_lookahead_select: null argument");
    if (column < 0 || column > 4) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_lookahead_select: column must be 0..4 (reward, makespan, idle, energy, transport)");
    EnvHostView sc, so;
    int rc = mtfjsp_env_pair_views("mtfjsp_lookahead_select", "source", scratch, src, &sc, &so);
    if (rc) return rc;
    if (!sc.was_reset || !so.was_reset) return mtfjsp_env_fail(scratch, MTFJSP_ERR_STATE, "mtfjsp_lookahead_select: both handles must hold a state (mtfjsp_lookahead_expand and a step first)");
    if (!sc.obs_bound || !sc.obs.raw) return mtfjsp_env_fail(scratch, MTFJSP_ERR_STATE, "mtfjsp_lookahead_select: the scratch handle needs bound observations with raw");
    if ((rc = mtfjsp_env_set_device(scratch, so.device_id, "mtfjsp_lookahead_select"))) return rc;
    LaArgs A{};
    A.B = so.B; A.J = so.J; A.M = so.M; A.T = so.T; A.MJ = so.MJ; A.column = column; A.mj = so.mj;
    A.status = sc.obs.status; A.raw = sc.obs.raw; A.task = task_out; A.mach = mach_out; A.job = job_out; A.best = best_out;
    if (so.T <= WAVE) hipLaunchKernelGGL(k_lookahead_select<true>, dim3(so.B), dim3(WAVE), 0, so.stream, A);
    else hipLaunchKernelGGL(k_lookahead_select<false>, dim3(so.B), dim3(WAVE), 0, so.stream, A);
    return mtfjsp_env_launched(scratch, "mtfjsp_lookahead_select");
}
