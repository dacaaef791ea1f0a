// mtfjsp_env_dev.h — definitions of the environment state that more than one translation unit needs.  Device side (the step kernels
// of mtfjsp_env.hip; mtfjsp_encoder.hip, whose machine-actor heads kernel can run the grouped step of its 16 instances as its tail,
// k_headsx_envstep; the search baselines mtfjsp_pdr.hip, mtfjsp_lookahead.hip, mtfjsp_beam.hip, mtfjsp_group.hip, mtfjsp_plan.hip): kernel parameter
// block, per-task / per-machine records, scalar slots, uniform lane reads — the wave-wide selections on top of them are in
// mtfjsp_wave_select.h.  Host side (the five baseline units): a view of a handle and the checks their entry points share.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mtfjsp.h"
#include "mtfjsp_env_select.h"     // WAVE, SCAL_N, the group sizes and the launch selection

// scalar slots (SCAL_N doubles per instance)
#define S_MK_PREV 0
#define S_E1_PREV 1
#define S_TR_PREV 2
#define S_ID_PREV 3
#define S_TR_THIS 4
#define S_W3 5             // 5,6,7
#define S_R 8              // 8..11   RewardScaling.R
#define S_MEAN 12          // 12..15
#define S_S 16             // 16..19
#define S_STD 20           // 20..23
#define S_N 24             // RunningMeanStd.n
#define S_NSCHED 25        // number of scheduled tasks
#define S_TRLAST 26        // transport time of the previous step's job edge (the entry tt[mach(lastm-1), mach(lastm)] that the reverting merged edge needs)
#define S_LASTM 27         // node whose merged job+machine edge was created by the previous step (-1), as a double

struct __align__(8) Link { short mach, prev, pos, pad; };      // per task: machine (-1), route predecessor (-1), rank in route, route successor (pad)
// Dynamic state, round 6: 16-byte records so that a lane's share of the state is three wide loads (it was eleven 8-byte ones) and
// fewer bytes: the finish time is not stored (ft == st + dur, the very addition that made it: env:356), the transport matrix is
// read as ONE row of its transpose behind the action (the step only ever needs column m), per-job and per-machine words share records.
struct __align__(16) TaskSD { double st, dur; };               // per task: start, duration (0, 0 while unscheduled)
struct __align__(16) TaskPL { double pte; Link link; };        // per task: estimated / real processing energy (env:1995), route links
struct __align__(16) JobR { double jmax, jrow; };              // per job: max estimated finish / max real finish
struct __align__(8) MJRec { short head, tail, len, cnt; };     // element i: route head / tail / length of MACHINE i, scheduled ops of JOB i

struct EnvParams {
    int B, J, M, T, left_shift, obs_f32;
    unsigned inv_M;                    // ceil(2^32 / M)
    double w_mk, w_ec, w_tt, divisor, gamma;
    // instance constants
    const double *t, *p, *tt;          // [B,T,M] [B,T,M] [B,M,M]
    const double2 *cst;                // [B,T] {min_dur, min_pt}
    const double *ttT;                 // [B,M,M] transport times transposed: ttT[b][m][x] = tt[b][x][m]
    // dynamic state
    TaskSD *sd;                        // [B,T]
    TaskPL *pl;                        // [B,T]
    JobR *jr;                          // [B,J]
    MJRec *mj;                         // [B,MJ], MJ = max(J, M) (ops of a job are scheduled in order: cnt is the job's next op)
    int MJ;
    double *mfea;                      // [B,M,8] f64 master copy of machines_fea
    double *scal;                      // [B,SCAL_N]
    // inputs
    const int *task_idx, *mach_idx;    // [B]
    const double *w3;                  // [B,3] (reset)
    // reset of an EPISODE in one launch (mtfjsp_reset_episode): draw = 1: the reward weights are drawn here (k_draw_w3's Philox stream for
    // (draw_seed, draw_episode, instance): same bits) and written to w3_out; reset_returns = 1: the discounted returns R of the reward
    // scaler are zeroed as well (pt:123, run:283-284)
    int draw, reset_returns;
    unsigned long long draw_seed, draw_episode;
    double *w3_out;
    // outputs
    mtfjsp_obs_t obs;
    unsigned long long *stamps;        // diagnostic build only
    float *rec_r4, *rec_done;          // optional f32 trajectory record of this step ([4,B], [B])
    const short *pw_tab;               // leaves and merges of numpy's pairwise sum over T elements (pw_table; T > 128 only)
    int pw_nleaf;
};

__device__ __forceinline__ long trunc_l(double x) { return (long)x; }   // numpy astype(int): toward zero
__device__ __forceinline__ int rl_i(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ double rl_d(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
// lane moves that stay in the vector ALU (no LDS round trip): DPP controls (0xB1 / 0x4E: lane ^ 1 / ^ 2 inside a quad, 0x141: lane -> 7 - lane
// inside 8 lanes, 0x108: lane <- lane + 8 inside a row of 16, 0x138: lane <- lane - 1 across the wave; a lane without a source reads 0)
template <int CTRL> __device__ __forceinline__ int dpp_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ double dpp_d(double x) { return __hiloint2double(dpp_i<CTRL>(__double2hiint(x)), dpp_i<CTRL>(__double2loint(x))); }
// gfx950's row swaps: lanes 0..15 <- lanes 16..31 (and 32..47 <- 48..63) | lanes 0..31 <- lanes 32..63
__device__ __forceinline__ int up16_i(int x) { return (int)__builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false)[1]; }
__device__ __forceinline__ int up32_i(int x) { return (int)__builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false)[1]; }
__device__ __forceinline__ double up16_d(double x) { return __hiloint2double(up16_i(__double2hiint(x)), up16_i(__double2loint(x))); }
__device__ __forceinline__ double up32_d(double x) { return __hiloint2double(up32_i(__double2hiint(x)), up32_i(__double2loint(x))); }

// numpy float64 add.reduce over one leaf block (n <= 128) of a contiguous row: plain left to right below 8 elements, 8 accumulators
// from 8 on (numpy's pairwise_sum; the caller adds the reduction's initial 0)
__device__ __forceinline__ double pw_leaf(const double *a, int n)
{
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += a[i];
    return res;
}

// Philox4x32-10 (counter-based; Salmon et al. 2011)
__device__ __forceinline__ void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// host side: what the library's other translation units (mtfjsp_pdr.hip, mtfjsp_lookahead.hip, mtfjsp_beam.hip, mtfjsp_group.hip, mtfjsp_plan.hip, mtfjsp_replay.hip) see of a handle; defined in mtfjsp_env.hip
struct EnvHostView {
    int B, J, M, T, device_id;
    bool loaded;
    const double *t, *p;               // [B,T,M] device instance arrays
    hipStream_t stream;
    bool was_reset, obs_bound;
    const MJRec *mj;                   // [B,MJ]: .cnt of element j = scheduled operations of job j
    int MJ;
    const TaskSD *sd;                  // [B,T] per-task records: start, duration
    const TaskPL *pl;                  // [B,T] per-task records: energy, route links
    mtfjsp_obs_t obs;                  // the bound observation (valid with obs_bound)
    const double *scal;                // [B,SCAL_N] per-instance scalar state (slots above)
    const double *tt;                  // [B,M,M] device transport times (mtfjsp_critical_path: the tightness of a job arc)
    // mtfjsp_replay_plans (mtfjsp_replay.hip)
    int replayed;                      // 0, or since the last reset: 1 = replayed, 2 = replayed with the sd / pl records written
    int left_shift;
    size_t lds_max;                    // LDS bytes a workgroup may use on the handle's device
    const double2 *cst;                // [B,T] {min_dur, min_pt}
    const short *pw_tab;               // numpy's pairwise sum over T elements (pw_table)
    int pw_nleaf;
    // sd and pl hold a schedule: after a reset, or after a replay that wrote them
    bool has_schedule() const { return was_reset || replayed == 2; }
};
__attribute__((visibility("hidden"))) void mtfjsp_env_host_view(mtfjsp_handle_t h, EnvHostView *v);
// after mtfjsp_replay_plans: the handle is no longer reset (everything that needs a reset refuses with MTFJSP_ERR_STATE) until the next reset;
// how = 2: sd and pl hold the replayed schedules
__attribute__((visibility("hidden"))) void mtfjsp_env_set_replayed(mtfjsp_handle_t h, int how);
__attribute__((visibility("hidden"))) int mtfjsp_env_fail(mtfjsp_handle_t h, int code, const char *msg);   // sets mtfjsp_last_error, returns code
// the check behind every HIP call of an entry point `who`: e != hipSuccess sets "<who>: <msg>" and returns MTFJSP_ERR_HIP, else MTFJSP_OK
__attribute__((visibility("hidden"))) int mtfjsp_env_hip_check(mtfjsp_handle_t h, hipError_t e, const char *who, const char *msg);
static inline int mtfjsp_env_set_device(mtfjsp_handle_t h, int device_id, const char *who) { return mtfjsp_env_hip_check(h, hipSetDevice(device_id), who, "hipSetDevice failed"); }
static inline int mtfjsp_env_launched(mtfjsp_handle_t h, const char *who) { return mtfjsp_env_hip_check(h, hipGetLastError(), who, "launch failed"); }
// before the launch of a kernel `fn` with `lds` bytes of dynamic LDS: above the 48 KiB every kernel may have, the attribute that allows them
static inline int mtfjsp_env_dyn_lds(mtfjsp_handle_t h, const void *fn, size_t lds, const char *who)
{
    return lds <= 48 * 1024 ? MTFJSP_OK : mtfjsp_env_hip_check(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), who,
                                                               "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
}
// both views of a (scratch, source) pair of the look-ahead's shape — another handle of the same size on the same device, scratch batch =
// source batch * T — or MTFJSP_ERR_ARG on the scratch handle; noun: what the message calls the source ("source", "beam")
__attribute__((visibility("hidden"))) int mtfjsp_env_pair_views(const char *who, const char *noun, mtfjsp_handle_t scratch, mtfjsp_handle_t src, EnvHostView *sc,
                                                                EnvHostView *so);
// mtfjsp_fork's checks and launch.  src_index == nullptr: destination instance i takes source instance i / div (the look-ahead's
// implicit index: T copies per source instance); the public entry point always passes an index.
__attribute__((visibility("hidden"))) int mtfjsp_env_fork_launch(mtfjsp_handle_t dst, mtfjsp_handle_t src, const int32_t *src_index, int div, int flags,
                                                                 const char *who);
