// mtfjsp_pdr.hip — the priority dispatch rules of the reference's tester/pdrs.py ("pdrs:") planned on the device: for every
// instance of a handle, the task of each of the T steps and the machine it runs on, under one of 6 operation rules x 2 machine
// rules (the 12 pairs test_all.py:484-540 compares the policy with).  All 12 are static: pdrs:680-753 fixes both lists from t, p
// before the first env.step, so one launch plans whole episodes and the ordinary step kernel (left shift off, pdrs:669) replays them.
//
// One 64-lane wavefront (= one workgroup) plans one instance:
//   1. lanes over tasks: each lane walks its task's M entries of t (and p where a rule needs it) ONCE, in machine order — the
//      argmin machine (pdrs:46-66) and the mean of the positive entries (pdrs:170-178, Python's left-to-right sum) — and keeps
//      one byte and one double per task in LDS
//   2. lanes over jobs: refer[j] = np.sum of the job's row of task values (numpy's add.reduce order: pw_leaf)
//   3. T selections: wave-wide first-index argmin / argmax of refer, the owner lane emits the job's next task (pdrs:183-208)
//   4. the plan leaves LDS in coalesced stores
// Every float is binary64, evaluated in the reference's order without contraction (build with -ffp-contract=off, like the
// environment unit): the argmin decisions must come out the same bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_wave_select.h"

struct PdrArgs {
    int B, J, M, T;
    const double *t, *p;               // [B,T,M]
    const int *o_rule, *m_rule;        // [B]
    const int *mor_order;              // [B,M,J] or null
    unsigned long long seed;
    int *task_out, *mach_out;          // [B,T]
};

// LDS of one instance: v[T] f64 | refer[J] f64 | order[T] i32 | next[J] i32 | machine[T] u8
static size_t pdr_lds_bytes(int J, int T) { return (size_t)T * 13 + (size_t)J * 12; }

// REG: J <= 64 — lane j keeps refer[j] and the job's next operation in registers, and a selection is one reduction, one ballot
// and one LDS read by the owner lane.  Otherwise both live in LDS and every lane scans the jobs j = lane, lane + 64, ...
template <bool REG>
__global__ __launch_bounds__(64) void k_pdr_plan(PdrArgs A)
{
    extern __shared__ double pdr_lds[];
    const int b = blockIdx.x, lane = threadIdx.x, J = A.J, M = A.M, T = A.T;
    const int o = uni(A.o_rule[b]), mr = uni(A.m_rule[b]);
    if ((unsigned)o > 5u || (unsigned)mr > 1u) return;              // (the host has checked: nothing is written for a bad id)
    double *v = pdr_lds, *refer = v + T;
    int *order = (int *)(refer + J), *next = order + T;
    unsigned char *machine = (unsigned char *)(next + J);
    const bool v_pt = o == 3 || o == 5, most = o >= 4, need_p = mr == 1 || v_pt;

    // 1. per task: machine rule and task value, one pass over the task's row(s)
    const double *tb = A.t + (size_t)b * T * M, *pb = A.p + (size_t)b * T * M;
    for (int a = lane; a < T; a += WAVE) {
        const double *tr = tb + (size_t)a * M, *pr = pb + (size_t)a * M;
        double best = INFINITY, s = 0.0;
        int bm = 0, n = 0;
        for (int m = 0; m < M; m++) {
            const double tv = tr[m];
            const double e = need_p ? tv * fabs(pr[m]) : 0.0;       // pdrs:62, :228 np.multiply(t, np.abs(p)): the sign of t stays
            const double c = mr ? e : tv;                           // SEC : SPT
            const double k = c < 0.0 ? INFINITY : c;                // pdrs:50, :64
            if (k < best) { best = k; bm = m; }                     // np.argmin: the first minimum
            const double x = v_pt ? e : tv;
            if (x > 0.0) { s += x; n++; }                           // pdrs:173-175: sum(positive_elements), left to right
        }
        machine[a] = (unsigned char)bm;
        v[a] = n ? s / (double)n : 0.0;
    }
    __syncthreads();

    if (o == 0) {                                                   // FIFO (pdrs:123-125)
        for (int s = lane; s < T; s += WAVE) order[s] = s;
    } else if (o == 1) {                                            // MOR (pdrs:128-137): column by column, its J tasks shuffled
        if (A.mor_order) {
            const int *mo = A.mor_order + (size_t)b * T;
            for (int i = lane; i < T; i += WAVE) order[i] = mo[i] * M + i / J;
        } else {
            for (int c = lane; c < M; c += WAVE) {                  // one Fisher-Yates per column; Philox counters (seed; instance, column, block)
                int *col = order + c * J;
                for (int i = 0; i < J; i++) col[i] = i;
                uint32_t r[4];
                int have = 0, blk = 0;
                for (int i = J - 1; i > 0; i--) {
                    if (!have) {
                        r[0] = (uint32_t)b; r[1] = (uint32_t)c; r[2] = (uint32_t)blk++; r[3] = 0x70647231u;
                        philox4x32(r, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
                        have = 4;
                    }
                    const uint32_t u = have == 4 ? r[0] : have == 3 ? r[1] : have == 2 ? r[2] : r[3];
                    have--;
                    const int k = (int)(((uint64_t)u * (uint64_t)(i + 1)) >> 32);      // uniform in [0, i]
                    const int x = col[i]; col[i] = col[k]; col[k] = x;
                }
                for (int i = 0; i < J; i++) col[i] = col[i] * M + c;
            }
        }
    } else if (REG) {                                               // L/MWKR (pdrs:162-208, :226-286)
        const double fin = most ? -INFINITY : INFINITY;
        double rf = lane < J ? 0.0 + pw_leaf(v + lane * M, M) : fin;        // pdrs:181 np.sum(t_new, axis=1)
        int nx = 0;
        for (int s = 0; s < T; s++) {
            const double key = lane < J ? (most ? -rf : rf) : INFINITY;     // argmax(x) == argmin(-x), ties included
            const double mn = wave_ext<false>(key);
            const unsigned long long eq = __ballot(lane < J && key == mn);
            const int jj = eq ? __ffsll((long long)eq) - 1 : 0;             // first index; every value +inf: index 0
            if (lane == jj) {
                const int k = nx < M ? nx : M - 1;                          // (the reference raises when a finished job comes again)
                order[s] = lane * M + k;
                const double r = rf - v[lane * M + k];
                nx++;
                rf = (r == 0.0 || nx > M - 1) ? fin : r;                    // pdrs:202: both clauses are reference behaviour
            }
        }
    } else {
        const double fin = most ? -INFINITY : INFINITY;
        for (int j = lane; j < J; j += WAVE) { refer[j] = 0.0 + pw_leaf(v + j * M, M); next[j] = 0; }
        __syncthreads();
        for (int s = 0; s < T; s++) {
            double best = INFINITY;
            int bj = INT_MAX;
            for (int j = lane; j < J; j += WAVE) {
                const double key = most ? -refer[j] : refer[j];
                if (bj == INT_MAX || key < best) { best = key; bj = j; }
            }
            const double mn = wave_ext<false>(best);
            const int jj = wave_min(best == mn ? bj : INT_MAX);         // lanes >= J: (inf, INT_MAX)
            if (lane == 0) {
                const int nx = next[jj], k = nx < M ? nx : M - 1;
                order[s] = jj * M + k;
                const double r = refer[jj] - v[jj * M + k];
                next[jj] = nx + 1;
                refer[jj] = (r == 0.0 || nx + 1 > M - 1) ? fin : r;
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // 4. (task, machine) of step s (pdrs:751-754)
    for (int s = lane; s < T; s += WAVE) {
        const int a = order[s];
        A.task_out[(size_t)b * T + s] = a;
        A.mach_out[(size_t)b * T + s] = (unsigned)a < (unsigned)T ? machine[a] : 0;     // (a mor_order entry outside 0..J-1)
    }
}

extern "C" int mtfjsp_pdr_plan(mtfjsp_handle_t h, const int32_t *o_rule, const int32_t *m_rule, const int32_t *mor_order, uint64_t seed,
                               int32_t *task_out, int32_t *mach_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!o_rule || !m_rule || !task_out || !mach_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_pdr_plan: null argument");
    EnvHostView e;
    mtfjsp_env_host_view(h, &e);
    if (!e.loaded) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_pdr_plan: no instances loaded or generated");
    const size_t lds = pdr_lds_bytes(e.J, e.T);
    if (lds > 64 * 1024) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_pdr_plan: instance too large (13*T + 12*J bytes of LDS must fit 64 KiB)");
    if (int rc = mtfjsp_env_set_device(h, e.device_id, "mtfjsp_pdr_plan")) return rc;
    {   // the rule ids are device data, and a bad one must leave the outputs untouched: they are read back and checked before the launch
        std::vector<int32_t> r(2 * (size_t)e.B);
        if (hipMemcpyAsync(r.data(), o_rule, (size_t)e.B * 4, hipMemcpyDeviceToHost, e.stream) != hipSuccess ||
            hipMemcpyAsync(r.data() + e.B, m_rule, (size_t)e.B * 4, hipMemcpyDeviceToHost, e.stream) != hipSuccess ||
            hipStreamSynchronize(e.stream) != hipSuccess)
            return mtfjsp_env_fail(h, MTFJSP_ERR_HIP, "mtfjsp_pdr_plan: reading the rule ids failed");
        for (int b = 0; b < e.B; b++)
            if (r[b] < 0 || r[b] > 5 || r[e.B + b] < 0 || r[e.B + b] > 1) {
                char msg[160];
                snprintf(msg, sizeof msg, "mtfjsp_pdr_plan: rule id out of range at instance %d (o_rule %d not in 0..5 or m_rule %d not in 0..1)",
                         b, r[b], r[e.B + b]);
                return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, msg);
            }
    }
    PdrArgs A{e.B, e.J, e.M, e.T, e.t, e.p, o_rule, m_rule, mor_order, seed, task_out, mach_out};
    if (e.J <= WAVE) hipLaunchKernelGGL(k_pdr_plan<true>, dim3(e.B), dim3(WAVE), lds, e.stream, A);
    else hipLaunchKernelGGL(k_pdr_plan<false>, dim3(e.B), dim3(WAVE), lds, e.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_pdr_plan");
}
