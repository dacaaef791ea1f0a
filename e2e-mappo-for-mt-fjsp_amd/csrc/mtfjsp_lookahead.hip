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
#include <stdio.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"

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

// wave-wide maximum on the cross-lane data path (row shifts, then row_bcast:15 / :31: lane 63 holds the result), read back to every
// lane.  Lanes without a source keep their own value.  All 64 lanes must be active.  fmax returns one of its operands: a comparison.
#define LA_DPP(x, ctrl) __builtin_amdgcn_update_dpp((x), (x), (ctrl), 0xF, 0xF, false)
__device__ __forceinline__ double la_wave_max(double x)
{
#define STEP_(ctrl)                                                                                     \
    {                                                                                                  \
        const int lo = LA_DPP(__double2loint(x), ctrl), hi = LA_DPP(__double2hiint(x), ctrl);          \
        x = fmax(x, __hiloint2double(hi, lo));                                                         \
    }
    STEP_(0x111) STEP_(0x112) STEP_(0x114) STEP_(0x118) STEP_(0x142) STEP_(0x143)
#undef STEP_
    return rl_d(x, 63);
}

// ONE: T <= 64 — a single pass, straight-line.  Otherwise the copies are taken 64 at a time; a later pass wins only with a strictly
// larger value, so the lowest index of the maximum is kept.
template <bool ONE>
__global__ __launch_bounds__(64) void k_lookahead_select(LaArgs A)
{
    const int b = blockIdx.x, lane = threadIdx.x, T = A.T, M = A.M;
    const size_t base = (size_t)b * T;
    double best = 0.0;
    int bi = -1;
    for (int c0 = 0; c0 < (ONE ? 1 : T); c0 += WAVE) {
        const int c = c0 + lane, cc = c < T ? c : T - 1;
        const int st = A.status[base + cc];
        const double v = A.raw[(base + cc) * 5 + A.column];
        const bool ok = c < T && !(st & (MTFJSP_ST_INVALID | MTFJSP_ST_INFEASIBLE));
        const double mx = la_wave_max(ok ? v : -INFINITY);
        const unsigned long long eq = __ballot(ok && v == mx);
        if (eq && (bi < 0 || mx > best)) { best = mx; bi = c0 + __ffsll((long long)eq) - 1; }
    }
    const int j = bi < 0 ? 0 : bi / M;
    const int cnt = A.mj[(size_t)b * A.MJ + j].cnt;
    if (lane == 0) {
        A.task[b] = bi < 0 ? -1 : j * M + (cnt < M ? cnt : M - 1);
        A.mach[b] = bi < 0 ? -1 : bi - j * M;
        if (A.job) A.job[b] = bi < 0 ? -1 : j;
        if (A.best) A.best[b] = bi < 0 ? (double)NAN : best;
    }
}

static int la_views(const char *who, mtfjsp_handle_t scratch, mtfjsp_handle_t src, EnvHostView *sc, EnvHostView *so)
{
    mtfjsp_env_host_view(scratch, sc);
    mtfjsp_env_host_view(src, so);
    if (scratch == src || sc->J != so->J || sc->M != so->M || sc->device_id != so->device_id || (long)sc->B != (long)so->B * so->T) {
        char msg[200];
        snprintf(msg, sizeof msg, "%s: the scratch handle must be another handle of the same size on the same device with batch = source batch * T", who);
        return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, msg);
    }
    return MTFJSP_OK;
}

extern "C" int mtfjsp_lookahead_expand(mtfjsp_handle_t scratch, mtfjsp_handle_t src, int32_t *task_c, int32_t *mach_c)
{
    if (!scratch) return MTFJSP_ERR_ARG;
    if (!src || !task_c || !mach_c) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_lookahead_expand: null argument");
    EnvHostView sc, so;
    int rc = la_views("mtfjsp_lookahead_expand", scratch, src, &sc, &so);
    if (rc) return rc;
    rc = mtfjsp_env_fork_launch(scratch, src, nullptr, so.T, MTFJSP_FORK_STATE, "mtfjsp_lookahead_expand");
    if (rc) return rc;
    LaArgs A{};
    A.B = so.B; A.J = so.J; A.M = so.M; A.T = so.T; A.MJ = so.MJ; A.mj = so.mj; A.task = task_c; A.mach = mach_c;
    hipLaunchKernelGGL(k_lookahead_actions, dim3((unsigned)(((size_t)sc.B + 255) / 256)), dim3(256), 0, sc.stream, A);
    if (hipGetLastError() != hipSuccess) return mtfjsp_env_fail(scratch, MTFJSP_ERR_HIP, "mtfjsp_lookahead_expand: launch failed");
    return MTFJSP_OK;
}

extern "C" int mtfjsp_lookahead_select(mtfjsp_handle_t scratch, mtfjsp_handle_t src, int32_t column, int32_t *task_out, int32_t *mach_out,
                                       int32_t *job_out, double *best_out)
{
    if (!scratch) return MTFJSP_ERR_ARG;
    if (!src || !task_out || !mach_out) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_lookahead_select: null argument");
    if (column < 0 || column > 4) return mtfjsp_env_fail(scratch, MTFJSP_ERR_ARG, "mtfjsp_lookahead_select: column must be 0..4 (reward, makespan, idle, energy, transport)");
    EnvHostView sc, so;
    int rc = la_views("mtfjsp_lookahead_select", scratch, src, &sc, &so);
    if (rc) return rc;
    if (!sc.was_reset || !so.was_reset) return mtfjsp_env_fail(scratch, MTFJSP_ERR_STATE, "mtfjsp_lookahead_select: both handles must hold a state (mtfjsp_lookahead_expand and a step first)");
    if (!sc.obs_bound || !sc.obs.raw) return mtfjsp_env_fail(scratch, MTFJSP_ERR_STATE, "mtfjsp_lookahead_select: the scratch handle needs bound observations with raw");
    if (hipSetDevice(so.device_id) != hipSuccess) return mtfjsp_env_fail(scratch, MTFJSP_ERR_HIP, "mtfjsp_lookahead_select: hipSetDevice failed");
    LaArgs A{};
    A.B = so.B; A.J = so.J; A.M = so.M; A.T = so.T; A.MJ = so.MJ; A.column = column; A.mj = so.mj;
    A.status = sc.obs.status; A.raw = sc.obs.raw; A.task = task_out; A.mach = mach_out; A.job = job_out; A.best = best_out;
    if (so.T <= WAVE) hipLaunchKernelGGL(k_lookahead_select<true>, dim3(so.B), dim3(WAVE), 0, so.stream, A);
    else hipLaunchKernelGGL(k_lookahead_select<false>, dim3(so.B), dim3(WAVE), 0, so.stream, A);
    if (hipGetLastError() != hipSuccess) return mtfjsp_env_fail(scratch, MTFJSP_ERR_HIP, "mtfjsp_lookahead_select: launch failed");
    return MTFJSP_OK;
}
