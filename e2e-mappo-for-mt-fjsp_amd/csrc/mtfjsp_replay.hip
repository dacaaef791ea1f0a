// mtfjsp_replay.hip — plans evaluated in ONE launch (the replay every search on plans pays per round or generation: mtfjsp_reset, T x
// mtfjsp_step, mtfjsp_final_costs = T + 2 launches, each step reloading the whole dynamic state and writing rewards, RewardScaling and
// observations that a search never reads).
//   mtfjsp_replay_plans            k_replay_plans: one wavefront per copy, G copies per workgroup, a copy's schedule in LDS for the
//                                  whole episode; out come the four final costs and done, and with MTFJSP_REPLAY_STATE the sd / pl records
//   mtfjsp_replay_launch_info_for  G and the dynamic LDS bytes of that launch for a shape (no GPU needed)
// Per step only part A of the step kernel (env_step_wave, mtfjsp_env.hip, "A. scheduling", env:1476-1685) — the validity tests, EMPTY,
// FRONT, the gap search with its (pos << 16) | v key, APPEND, the position shift and the link, head, tail, length and count updates: the
// same operations in the same order — and the transport accumulation S_TR_THIS + new_tr (env_grp_tail_seq: trans_this).
// After the last step, for a copy that scheduled all T tasks, what T step launches leave in S_MK_PREV, S_E1_PREV, S_TR_PREV, S_ID_PREV:
//   makespan   the maximum over jobs of jmax.  The step kernel refreshes jmax of the ACTING job only, with the chain of env:1920-1999
//              (a scheduled operation whose finish is 0.0 counts as having no real finish: `ft != 0.0`).  The chain reads the job's own
//              operations (machine, start, finish) and min_dur, and a scheduled operation never changes again: the value it leaves at
//              a job's last accepted step — in a finished copy the step that schedules the job's last operation — is the value the chain
//              gives on the finished schedule.  So the chain is KEPT, and runs once per job after the last step (lane = job, the
//              operations left to right as the step kernel's uniform walk does).  It is not replaced by the maximum real finish.
//   energy     numpy's pairwise sum of pte = d * pk (one leaf block for T <= 128, the handle's pw_tab recursion above: the step kernel's
//              own code), then 0.0 + sum
//   transport  the accumulated value
//   idle       the terms in (machine, position) order, summed strictly left to right from +0.0
// cost4 = (mk, e1 / T, tr, idle) with the one binary64 division of k_final_costs; done = (nsched == T).  A copy that is not done gets
// four NaNs (the step path leaves estimates of a partial schedule there): k_group_reduce, k_walk_accept and k_front_rank all test
// `done != 0` before anything else of a copy, so such a copy is ineligible on either path.
// Nothing is contracted into FMA (the library is built with -ffp-contract=off); no observation, reward, scaler word, mask, mfea or jr is
// read or written; every global store is an ordinary vector store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_plan_dev.h"
#include "mtfjsp_wave_select.h"

#define REPLAY_GMAX 4                  // copies (waves) per workgroup, as the other search kernels
#define REPLAY_LDS_SOFT (64 * 1024)    // G shrinks (4 -> 2 -> 1) to stay below this: two workgroups per CU

// One copy's LDS region.  Doubles [Tp] each: st, ft, pte (per task) | d, pk, tr (per STEP: gathered from the plan before the first
// step; after the last step the three are free: idle terms, leaf sums).  tt [M,M].  Ints: head, tail, len [M], mstart [M + 1], cnt [J].
// Shorts [Tp] each: mach, prev, pos (per task) | the plan's task, machine (per step) | mu (per task: the planned machine while the
// operands are gathered, then the step that scheduled it) | pm (per step: the planned machine of the job predecessor, whose
// transport time tr holds).  62 bytes per task.
struct ReplayLds {
    int Tp;
    size_t o_tt, o_int, o_short, bytes;
    __host__ __device__ ReplayLds(int J, int M, int T)
    {
        Tp = (T + 3) & ~3;
        size_t off = (size_t)6 * Tp * sizeof(double);
        o_tt = off; off += (size_t)M * M * sizeof(double);
        o_int = off; off += (size_t)(4 * M + 1 + J) * sizeof(int);
        off = (off + 7) & ~(size_t)7;
        o_short = off; off += (size_t)7 * Tp * sizeof(short);
        bytes = (off + 15) & ~(size_t)15;
    }
};

// the launch: G = the largest of 4, 2, 1 whose regions stay below REPLAY_LDS_SOFT (and lds_max) and that the batch can fill at least
// half; one region alone may take up to lds_max.  false: one copy does not fit
static bool replay_select(int J, int M, int batch, size_t lds_max, int *G, size_t *lds)
{
    const ReplayLds L(J, M, J * M);
    if (L.bytes > lds_max) return false;
    const size_t soft = lds_max < REPLAY_LDS_SOFT ? lds_max : (size_t)REPLAY_LDS_SOFT;
    int g = REPLAY_GMAX;
    while (g > 1 && ((size_t)g * L.bytes > soft || g >= 2 * batch)) g >>= 1;
    *G = g; *lds = (size_t)g * L.bytes;
    return true;
}

struct ReplayArgs {
    int B, J, M, T, left_shift, G, G_log2;
    unsigned inv_M;                    // ceil(2^32 / M)
    const double *t, *p, *tt;          // [B,T,M] [B,T,M] [B,M,M]
    const double2 *cst;                // [B,T] {min_dur, min_pt}
    const short *pw_tab;               // the handle's pairwise-sum table (T > 128)
    int pw_nleaf;
    const int *task, *mach;            // [T,stride]
    long long stride;
    double *cost4;                     // [B,4]
    uint8_t *done;                     // [B]
    TaskSD *sd;                        // [B,T] or null (MTFJSP_REPLAY_STATE)
    TaskPL *pl;
};

// a wave's hand-off through its own LDS region: the LDS executes a wave's DS instructions in issue order (mtfjsp_env.hip: WSYNC)
#define RSYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

__global__ __launch_bounds__(REPLAY_GMAX * WAVE) void k_replay_plans(ReplayArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const ReplayLds L(A.J, A.M, A.T);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = uni(tid >> 6);
    const int G = A.G, T = A.T, M = A.M, J = A.J, Tp = L.Tp;
    const unsigned invM = A.inv_M;
#define DIVM(x) ((int)__umulhi((unsigned)(x), invM))
    const long b0 = (long)blockIdx.x * G;
    // ---- the workgroup's [T x G] tile of the plans, lanes across copies first: a row's G words are one contiguous run.  An entry out
    // of range becomes (-1, -1): the step rejects it (env_step_wave: `valid`)
    for (int e = tid; e < (T << A.G_log2); e += G * WAVE) {
        const int s = e >> A.G_log2, c = e & (G - 1);
        const long bc = b0 + c;
        if (bc < A.B) {
            const int a = A.task[(size_t)s * A.stride + bc], m = A.mach[(size_t)s * A.stride + bc];
            const bool ok = (unsigned)a < (unsigned)T && (unsigned)m < (unsigned)M;
            short *sh = reinterpret_cast<short *>(smem + (size_t)c * L.bytes + L.o_short);
            sh[3 * Tp + s] = (short)(ok ? a : -1);
            sh[4 * Tp + s] = (short)(ok ? m : -1);
        }
    }
    __syncthreads();
    const long b = b0 + wave;
    if (b >= A.B) return;                                              // (wave-uniform; no workgroup barrier below)
    unsigned char *R = smem + (size_t)wave * L.bytes;
    double *s_st = reinterpret_cast<double *>(R), *s_ft = s_st + Tp, *s_pte = s_ft + Tp, *o_d = s_pte + Tp, *o_pk = o_d + Tp, *o_tr = o_pk + Tp;
    double *s_tt = reinterpret_cast<double *>(R + L.o_tt);
    int *s_head = reinterpret_cast<int *>(R + L.o_int), *s_tail = s_head + M, *s_len = s_tail + M, *s_mstart = s_len + M, *s_cnt = s_mstart + M + 1;
    short *s_mach = reinterpret_cast<short *>(R + L.o_short), *s_prev = s_mach + Tp, *s_pos = s_prev + Tp, *p_task = s_pos + Tp, *p_mach = p_task + Tp;
    short *s_mu = p_mach + Tp, *p_pm = s_mu + Tp;
    const size_t bT = (size_t)b * T;

    // ---- an empty schedule (k_env_reset), the copy's transport times
    for (int v = lane; v < T; v += WAVE) { s_st[v] = 0.0; s_ft[v] = 0.0; s_pte[v] = 0.0; s_mach[v] = -1; s_prev[v] = -1; s_pos[v] = 0; s_mu[v] = -1; }
    for (int i = lane; i < M * M; i += WAVE) s_tt[i] = A.tt[(size_t)b * M * M + i];
    for (int i = lane; i < M; i += WAVE) { s_head[i] = -1; s_tail[i] = -1; s_len[i] = 0; }
    for (int i = lane; i < J; i += WAVE) s_cnt[i] = 0;
    RSYNC();
    // ---- the plan is known in full: every step's operands now, not one dependent load behind each action.  mu = the machine the plan
    // gives a task (a task named twice keeps either: the step checks the predecessor's real machine against pm)
    for (int s = lane; s < T; s += WAVE) { const int a = p_task[s]; if (a >= 0) s_mu[a] = p_mach[s]; }
    RSYNC();
    for (int s = lane; s < T; s += WAVE) {
        const int a = p_task[s], m = p_mach[s];
        double d = 0.0, pk = 0.0, tr = 0.0;
        int pm = -1;
        if (a >= 0) {
            d = A.t[(bT + a) * M + m];
            pk = A.p[(bT + a) * M + m];
            if (a != DIVM(a) * M) pm = s_mu[a - 1];
            if (pm >= 0) tr = s_tt[pm * M + m];
        }
        o_d[s] = d; o_pk[s] = pk; o_tr[s] = tr; p_pm[s] = (short)pm;
    }
    RSYNC();

    // ---- T steps: A. scheduling (env:1476-1685) as env_step_wave has it, s_ttc[x] = tt[x][m] read from the copy's own matrix
    int nsched = 0;
    double trans = 0.0;
    for (int s = 0; s < T; s++) {
        const int a = uni((int)p_task[s]), m = uni((int)p_mach[s]);
        if (a < 0) continue;                                           // index out of range: nothing changes
        const int ja = DIVM(a), op = a - ja * M;
        if (uni((int)s_mach[a]) >= 0) continue;                        // already scheduled (env:1504)
        const int mprev = op != 0 ? uni((int)s_mach[a - 1]) : 0;
        if (op != 0 && mprev < 0) continue;                            // job predecessor unscheduled (env:1520)
        const double d = o_d[s], pk = o_pk[s];
        const double x_tr = op == 0 ? 0.0 : (mprev == (int)p_pm[s] ? o_tr[s] : s_tt[mprev * M + m]);
        const double ttmm = s_tt[m * M + m];
        const double arr_k = op == 0 ? 0.0 : s_ft[a - 1] + x_tr;       // dg:46-66 over the single in-edge
        const int len = uni(s_len[m]), head = uni(s_head[m]), tail = uni(s_tail[m]);
        int Pk = -1, Nk = -1, ipos = 0;
        double st_k = 0.0;
        bool do_append = false;
        if (len == 0) { st_k = arr_k; ipos = 0; }                                                    // env:1684
        else if (!A.left_shift) do_append = true;                                                    // env:1680
        else {
            const double lb_ft = arr_k + d;
            const int jh = DIVM(head);
            const double arr_f = (head == jh * M) ? 0.0 : s_ft[head - 1] + s_tt[(int)s_mach[head - 1] * M + m];
            if (lb_ft <= arr_f) { st_k = arr_k; ipos = 0; Nk = head; }                               // env:1548
            else if (len == 1) do_append = true;                                                     // env:1577
            else {
                int key = 0x7fffffff;                                  // gap search over all consecutive (P,N) at once (env:1587-1604)
                for (int v = lane; v < T; v += WAVE) {
                    if (s_mach[v] == m && s_prev[v] >= 0) {
                        const int Pp = s_prev[v];
                        const int jv = DIVM(v);
                        const double jarr = (v == jv * M) ? 0.0 : s_ft[v - 1] + s_tt[(int)s_mach[v - 1] * M + m];
                        const double x = (DIVM(Pp) == jv) ? ttmm : 0.0;
                        const double nst = fmax(jarr, s_ft[Pp] + x);
                        const bool ok = !(lb_ft > nst) && !((nst - s_ft[Pp]) < d);
                        if (ok) { const int kk = ((int)s_pos[v] << 16) | v; key = kk < key ? kk : key; }
                    }
                }
                key = wave_min(key);
                if (key != 0x7fffffff) {
                    Nk = key & 0xffff; ipos = key >> 16; Pk = uni((int)s_prev[Nk]);
                    const double x = (DIVM(Pk) == ja) ? ttmm : 0.0;
                    st_k = fmax(arr_k, s_ft[Pk] + x);                          // env:1619
                } else do_append = true;                                       // env:1676
            }
        }
        if (do_append) {                                                       // env:1689-1775
            const double x = (DIVM(tail) == ja) ? ttmm : 0.0;
            st_k = fmax(arr_k, s_ft[tail] + x);
            ipos = len; Pk = tail;
        }
        const double ft_k = st_k + d;
        RSYNC();
        if (ipos < len)
            for (int v = lane; v < T; v += WAVE)
                if (s_mach[v] == m && s_pos[v] >= ipos) s_pos[v] = (short)(s_pos[v] + 1);
        RSYNC();
        if (lane == 0) {
            s_mach[a] = (short)m; s_prev[a] = (short)Pk; s_pos[a] = (short)ipos;
            s_st[a] = st_k; s_ft[a] = ft_k; s_pte[a] = d * pk;                    // env:356,2175
            s_mu[a] = (short)s;
            if (Nk >= 0) s_prev[Nk] = (short)a;
            if (ipos == 0) s_head[m] = a;
            if (ipos == len) s_tail[m] = a;
            s_len[m] = len + 1;
            s_cnt[ja] += 1;
        }
        nsched += 1;
        trans = trans + x_tr;                                                  // env:872-876: S_TR_THIS + new_tr, in step order
        RSYNC();
    }

    // ---- the records T step launches leave (machine, start, duration, energy, route links), partial schedules included
    if (A.sd) {
        for (int v = lane; v < T; v += WAVE) {
            const int mc = s_mach[v];
            const bool sch = mc >= 0;
            TaskSD x; x.st = s_st[v]; x.dur = sch ? o_d[s_mu[v]] : 0.0;
            TaskPL y; y.pte = sch ? s_pte[v] : A.cst[bT + v].y;
            y.link.mach = (short)mc; y.link.prev = s_prev[v]; y.link.pos = s_pos[v]; y.link.pad = sch ? 0 : -1;
            A.sd[bT + v] = x; A.pl[bT + v] = y;
        }
        RSYNC();
    }
    const bool done = nsched == T;
    if (!done) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (lane < 4) A.cost4[(size_t)b * 4 + lane] = nan;
        if (lane == 0) A.done[b] = 0;
        return;
    }
    // ---- makespan: per job the chain of env:1920-1999 on its finished operations, then np.amax (env:894)
    double mk = -INFINITY;
    for (int j = lane; j < J; j += WAVE) {
        double acc = 0.0, pft = 0.0, fm = -INFINITY;
        bool pq = false;
        for (int k = 0; k < M; k++) {
            const double ftv = s_ft[j * M + k], md = A.cst[bT + j * M + k].x;
            const bool q = ftv != 0.0;
            const double base = pq ? pft : acc;
            acc = base + md;
            fm = fmax(fm, q ? ftv : acc);
            pq = q; pft = ftv;
        }
        mk = fmax(mk, fm);
    }
    mk = wave_ext<true>(mk);
    // ---- energy: np.sum of pte (env:896) as env_step_wave forms it
    double e1;
    if (T <= 128) {                                                          // one leaf block: its 8 accumulators on 8 lanes, the ragged tail in order
        const int nb = T < 8 ? 0 : T - (T & 7);
        double r = 0.0;
        if (nb) {
            if (lane < 8) { r = s_pte[lane]; for (int i = 8 + lane; i < nb; i += 8) r += s_pte[i]; }
            r += __shfl_xor(r, 1); r += __shfl_xor(r, 2); r += __shfl_xor(r, 4);
        }
        e1 = rl_d(r, 0);
        for (int i = nb; i < T; i++) e1 += s_pte[i];
    } else {
        double *s_leaf = o_pk;
        const short *tab = A.pw_tab;
        const int nleaf = A.pw_nleaf;
        for (int l0 = 0; l0 < nleaf; l0 += 8) {
            const int lf = l0 + (lane >> 3), k = lane & 7;
            const bool on = lf < nleaf;
            const int off = on ? tab[2 * lf] : 0, n = on ? tab[2 * lf + 1] : 8;
            const int nb = n - (n & 7);
            const double *src = s_pte + off + k;
            double x[16];
#pragma unroll
            for (int i = 0; i < 16; i++) x[i] = 8 * i < nb ? src[8 * i] : 0.0;
            double r = x[0];
#pragma unroll
            for (int i = 1; i < 16; i++) if (8 * i < nb) r += x[i];
            r += __shfl_xor(r, 1); r += __shfl_xor(r, 2); r += __shfl_xor(r, 4);
            if (on && k == 0) {
                for (int i = nb; i < n; i++) r += s_pte[off + i];
                s_leaf[lf] = r;
            }
        }
        RSYNC();
        if (lane == 0) {
            const short *mg = tab + 2 * nleaf;
            for (int q = 0; q < nleaf - 1; q++) { const int i = mg[2 * q], j = mg[2 * q + 1]; s_leaf[i] = s_leaf[i] + s_leaf[j]; }
        }
        RSYNC();
        e1 = s_leaf[0];
    }
    e1 = 0.0 + e1;
    // ---- idle: the terms in (machine, position) order (dg:144-170), summed strictly left to right from +0.0
    {
        const int x = lane < M ? s_len[lane] : 0, incl = wave_scan_incl(x);
        if (lane < M) s_mstart[lane] = incl - x;
    }
    RSYNC();
    double *s_term = o_d;
    for (int v = lane; v < T; v += WAVE) {
        const int pr = s_prev[v];
        s_term[s_mstart[s_mach[v]] + s_pos[v]] = pr < 0 ? s_st[v] : s_st[v] - s_ft[pr];
    }
    RSYNC();
    double idle = 0.0;
    for (int i = 0; i < T; i++) idle = idle + s_term[i];
    if (lane == 0) {
        double *o = A.cost4 + (size_t)b * 4;
        o[0] = mk; o[1] = e1 / (double)T; o[2] = trans; o[3] = idle;
        A.done[b] = 1;
    }
#undef DIVM
}

extern "C" int mtfjsp_replay_launch_info_for(int32_t n_job, int32_t n_machine, int32_t batch, int64_t lds_max, int32_t *group_out, int64_t *lds_bytes_out)
{
    if (n_job < 1 || n_machine < 2 || n_machine > 64 || batch < 1 || (long)n_job * n_machine > 32767 || lds_max < 0) return MTFJSP_ERR_ARG;
    int G; size_t lds;
    if (!replay_select(n_job, n_machine, batch, (size_t)lds_max, &G, &lds)) return MTFJSP_ERR_ARG;
    if (group_out) *group_out = G;
    if (lds_bytes_out) *lds_bytes_out = (int64_t)lds;
    return MTFJSP_OK;
}

extern "C" int mtfjsp_replay_plans(mtfjsp_handle_t h, const int32_t *task, const int32_t *mach, int64_t stride, double *cost4_out, uint8_t *done_out,
                                   int32_t flags)
{
    const char *who = "mtfjsp_replay_plans";
    if (!h) return MTFJSP_ERR_ARG;
    if (!task || !mach || !cost4_out || !done_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_replay_plans: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.loaded) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_replay_plans: no instances loaded");
    if (stride < v.B || (flags & ~MTFJSP_REPLAY_STATE))
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_replay_plans: stride >= the handle's batch, flags 0 or MTFJSP_REPLAY_STATE");
    const unsigned __int128 n_src = ((unsigned __int128)(v.T - 1) * (unsigned __int128)stride + (unsigned __int128)v.B) * 4;
    const PlanSpan srcs[2] = {{task, n_src}, {mach, n_src}};
    const PlanSpan outs[2] = {{cost4_out, (unsigned __int128)v.B * 32}, {done_out, (unsigned __int128)v.B}};
    if (int rc = plan_check_overlap(h, who, 2, outs, 2, srcs)) return rc;
    int G; size_t lds;
    if (!replay_select(v.J, v.M, v.B, v.lds_max, &G, &lds))
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_replay_plans: n_job * n_machine is too large for one copy's schedule in a workgroup's LDS");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, who)) return rc;
    ReplayArgs A{};
    A.B = v.B; A.J = v.J; A.M = v.M; A.T = v.T; A.left_shift = v.left_shift; A.G = G; A.G_log2 = G == 4 ? 2 : (G == 2 ? 1 : 0);
    A.inv_M = (unsigned)((0x100000000ull + (unsigned)v.M - 1) / (unsigned)v.M);
    A.t = v.t; A.p = v.p; A.tt = v.tt; A.cst = v.cst; A.pw_tab = v.pw_tab; A.pw_nleaf = v.pw_nleaf;
    A.task = task; A.mach = mach; A.stride = stride; A.cost4 = cost4_out; A.done = done_out;
    const bool state = (flags & MTFJSP_REPLAY_STATE) != 0;
    A.sd = state ? const_cast<TaskSD *>(v.sd) : nullptr; A.pl = state ? const_cast<TaskPL *>(v.pl) : nullptr;
    if (int rc = mtfjsp_env_dyn_lds(h, (const void *)k_replay_plans, lds, who)) return rc;
    hipLaunchKernelGGL(k_replay_plans, dim3((unsigned)(((size_t)v.B + G - 1) / G)), dim3(G * WAVE), lds, v.stream, A);
    if (int rc = mtfjsp_env_launched(h, who)) return rc;
    mtfjsp_env_set_replayed(h, state ? 2 : 1);
    return MTFJSP_OK;
}
