// mtfjsp_plan.hip — neighbourhood moves on plans (local search over best-of-K replay: every group's incumbent plan becomes K
// neighbouring plans, copy c of group n = element n*K + c as in mtfjsp_group.hip; the ordinary step kernel replays them and
// mtfjsp_group_reduce keeps the best).
//   mtfjsp_plan_neighbours   k_plan_neighbours: a plan is the job string q[s] = task[s] / M and a machine mu[a] per task.  Copy 0 is
//                            the incumbent; copy c >= 1 draws ONE move — SWAP two positions of q, INSERT one position elsewhere,
//                            REASSIGN one task to another feasible machine — and is decoded again: task'[s] = q'[s]*M + (earlier
//                            occurrences of q'[s]), mach'[s] = mu'[task'[s]].  Any permutation of q is a plan: no repair.
//   mtfjsp_plan_neighbours_critical   the same kernel with two more kinds of move that a critical path directs (CRIT_SWAP: a machine arc
//                            of the path between two jobs is turned round; CRIT_REASSIGN: a task of the path changes machine); the
//                            instantiation the plain entry launches reads no path and has no LDS for one.
//   mtfjsp_critical_path     k_critical_path: one critical path per row out of a handle's finished (or partial) state — the task that
//                            ends last, then from every task its tight route predecessor, else its tight job predecessor.  One wave
//                            per row, lanes over tasks; the walk is pointer doubling in LDS, not one lane chasing T pointers.
// Integer arithmetic only (Philox words, (w * n) >> 32): the outputs must equal a host model element for element.
// Shape: the tile of mtfjsp_plan_dev.h, which also holds the move itself (draw, position map, REASSIGN's pick, operation ranks), the cell,
// the tile's way out and the host side of the launch; here are the incumbent's (and the path's) load and what a critical path directs.
// The K copies of a group read one source column: the caches serve it, and a wave reloads it only where the group changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_plan_dev.h"
#include "mtfjsp_wave_select.h"

#define PLAN_CRIT_SWAP 8
#define PLAN_CRIT_REASSIGN 16
#define PLAN_CRIT (PLAN_CRIT_SWAP | PLAN_CRIT_REASSIGN)

struct PlanArgs {
    int B, K, T, J, M;
    int tile, tile_log2, pitch;        // copies per workgroup, its log2, words per cell row (tile + 1: odd)
    unsigned inv_M;                    // ceil(2^32 / M): task / M = (task * inv_M) >> 32 for task < 2^15
    const double *t;                   // [B,T,M]
    const int *src_task, *src_mach;    // [T,src_stride]
    long long src_stride;
    const int *src_col;                // [B/K] or null
    uint32_t seed_lo, seed_hi, ctr_lo, first_lo, moves, n_moves;   // ctr_lo: the round
    int *task_out, *mach_out;          // [T,B]
    int8_t *kind_out;                  // [B] or null
    const int *path_task, *path_len;   // [B/K,T], [B/K]: read by the CRIT instantiations only
    const int8_t *path_arc;            // [B/K,T]
};

// bytes of LDS: the tile's cells, then per wave the incumbent's tasks (u16 [T]), the machine of every task (i16 [T]) and the
// operations of every job seen in earlier passes (i32 [J]); crit: per wave also the position of every task in the incumbent, the
// group's path and the path's eligible swap arcs (u16 [T] each)
static size_t plan_lds_bytes(int T, int J, int tile, bool crit = false)
{
    return (size_t)T * (tile + 1) * 4 + (size_t)PLAN_WAVES * ((size_t)T * 4 + (size_t)J * 4) + (crit ? (size_t)PLAN_WAVES * T * 6 : 0);
}

// SMALL: T <= 64 — one pass, the incumbent's job string stays in registers and the position map is a ds_bpermute
// CRIT: moves has PLAN_CRIT_SWAP or PLAN_CRIT_REASSIGN — a path row per group, staged in LDS where the group changes as the incumbent is
template <bool SMALL, bool CRIT>
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_neighbours(PlanArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = uni(tid >> 6);
    const int T = A.T, M = A.M, J = A.J, pitch = A.pitch, B = A.B;
    uint32_t *cell = reinterpret_cast<uint32_t *>(smem);                                   // [T][pitch]
    uint16_t *inc = reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)wave * T;
    int16_t *mu = reinterpret_cast<int16_t *>(reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)PLAN_WAVES * T) + (size_t)wave * T;
    int *cnt = reinterpret_cast<int *>(reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)2 * PLAN_WAVES * T) + (size_t)wave * J;
    uint16_t *pos = reinterpret_cast<uint16_t *>(reinterpret_cast<int *>(reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)2 * PLAN_WAVES * T) + (size_t)PLAN_WAVES * J) + (size_t)wave * T;   // CRIT only
    uint16_t *ptk = pos + (size_t)PLAN_WAVES * T, *elig = ptk + (size_t)PLAN_WAVES * T;
    int L = 0, nA = 0;                                                 // CRIT: the group's path length, its number of eligible swap arcs
    const long g0 = (long)blockIdx.x * A.tile;
    const int per = A.tile / PLAN_WAVES;
    int n_have = -1;
    bool bad = false;                                                  // the incumbent in LDS is not the source's: column or an entry out of range
    int q_r = 0, tk_r = 0;                                             // SMALL: lane s = position s of the incumbent (job, task)
    for (int i = 0; i < per; i++) {
        const int ct = wave * per + i;
        const long gl = g0 + ct;
        const int g = (int)(gl < B ? gl : B - 1);                     // (a copy past the batch rebuilds the last one; its column is never stored)
        const int n = g / A.K, c = g - n * A.K;
        // ---- the incumbent of group n: tasks into inc[], machines scattered into mu[] (-1 where no position names the task)
        if (n != n_have) {
            n_have = n;
            long col = A.src_col ? (long)A.src_col[n] : (long)n;
            const bool cbad = col < 0 || col >= A.src_stride;
            col = cbad ? 0 : col;
            for (int s = lane; s < T; s += WAVE) mu[s] = -1;
            if (CRIT)
                for (int s = lane; s < T; s += WAVE) pos[s] = 0;
            plan_wave_sync();
            unsigned long long badm = 0;
            for (int s0 = 0; s0 < T; s0 += WAVE) {
                const int s = s0 + lane, sc = s < T ? s : T - 1;
                const int tk = A.src_task[(size_t)sc * A.src_stride + col], mc = A.src_mach[(size_t)sc * A.src_stride + col];
                const bool ok = (unsigned)tk < (unsigned)T && (unsigned)mc < (unsigned)M;
                badm |= __ballot(!ok);
                const int tkc = ok ? tk : 0, mcc = ok ? mc : 0;
                if (s < T) { inc[s] = (uint16_t)tkc; mu[tkc] = (int16_t)mcc; }
                if (CRIT && s < T) pos[tkc] = (uint16_t)s;
                if (SMALL) { tk_r = tkc; q_r = (int)plan_mulhi((uint32_t)tkc, A.inv_M); }
            }
            bad = cbad || badm != 0;
            if (CRIT) {
                // ---- the path of group n: tasks into ptk[], then A = the machine arcs between two jobs, ascending, into elig[]
                L = uni(A.path_len[n]);
                const bool lbad = L < 0 || L > T;
                L = lbad ? 0 : L;
                unsigned long long pbad = 0;
                for (int k0 = 0; k0 < L; k0 += WAVE) {
                    const int k = k0 + lane;
                    const int tk = k < L ? A.path_task[(size_t)n * T + k] : 0;
                    const bool ok = (unsigned)tk < (unsigned)T;
                    pbad |= __ballot(!ok);
                    if (k < L) ptk[k] = (uint16_t)(ok ? tk : 0);
                }
                plan_wave_sync();
                nA = 0;
                for (int k0 = 0; k0 + 1 < L; k0 += WAVE) {
                    const int k = k0 + lane;
                    const bool in = k + 1 < L;
                    const int kc = in ? k : 0;                          // (L >= 2 inside this loop)
                    const bool e = in && A.path_arc[(size_t)n * T + kc] == 1 && plan_mulhi((uint32_t)ptk[kc], A.inv_M) != plan_mulhi((uint32_t)ptk[kc + 1], A.inv_M);
                    const unsigned long long eb = __ballot(e);
                    if (e) elig[nA + plan_below(eb)] = (uint16_t)k;
                    nA += __popcll(eb);
                }
                bad = bad || lbad || pbad != 0;
            }
            plan_wave_sync();
        }
        // ---- the draw (plan_draw: wave-uniform).  Copy 0 takes none.
        const PlanMove d = plan_draw(A.first_lo + (uint32_t)n, (uint32_t)c, A.ctr_lo, A.seed_lo, A.seed_hi, A.moves, A.n_moves, T);
        int x = d.x, y = d.y, move = c == 0 ? 0 : d.move;              // 0: identity
        int a = SMALL ? rl_i(tk_r, x) : (int)inc[x];                   // REASSIGN's task
        if (CRIT) {
            if (d.kind == PLAN_CRIT_SWAP) {                               // INSERT of the arc's later task before its earlier one: v = path[k], u = path[k + 1]
                move = 0;
                if (nA > 0) {
                    const int k = (int)elig[plan_mulhi(d.wx, (uint32_t)nA)];
                    x = uni((int)pos[ptk[k]]);
                    y = uni((int)pos[ptk[k + 1]]);
                    move = c == 0 ? 0 : PLAN_INSERT;
                }
            }
            if (d.kind == PLAN_CRIT_REASSIGN) {                           // REASSIGN of a task of the path
                move = 0;
                if (L > 0) {
                    a = uni((int)ptk[plan_mulhi(d.wx, (uint32_t)L)]);
                    move = c == 0 ? 0 : PLAN_REASSIGN;
                }
            }
        }
        const int old_m = mu[a];
        int new_m;
        const int nf = plan_other_machine(A.t, ((size_t)g * T + a) * M, M, old_m, d.wy, lane, &new_m);
        const bool reassign = move == PLAN_REASSIGN && nf > 0;
        if (reassign) {
            if (lane == 0) mu[a] = (int16_t)new_m;
            plan_wave_sync();
        }
        if (!SMALL) {
            for (int j = lane; j < J; j += WAVE) cnt[j] = 0;
            plan_wave_sync();
        }
        // ---- q' = q gathered through the move's position map, the operation ranks, the machines
        for (int s0 = 0; s0 < T; s0 += WAVE) {
            const int s = s0 + lane, src = plan_src(move, s, x, y, T);
            int qn;
            if (SMALL) qn = __builtin_amdgcn_ds_bpermute(src << 2, q_r);
            else qn = (int)plan_mulhi((uint32_t)inc[src], A.inv_M);
            const bool live = s < T;
            const int rank = plan_rank<!SMALL>(qn, live, J, lane, cnt);
            const bool okr = c == 0 || rank < M;                        // (fails only for an incumbent that is no plan: too many operations of one job)
            int tn = okr ? qn * M + rank : 0;
            if (c == 0) tn = SMALL ? tk_r : (int)inc[live ? s : T - 1];  // copy 0 is the incumbent word for word, not its decoding
            const int mn = mu[tn];
            const uint32_t word = (bad || !okr) ? PLAN_CELL_KILLED : plan_cell(tn, mn);
            if (live) cell[(size_t)s * pitch + ct] = word;
        }
        if (reassign) {
            plan_wave_sync();
            if (lane == 0) mu[a] = (int16_t)old_m;
            plan_wave_sync();
        }
        if (A.kind_out && lane == 0 && gl < B) A.kind_out[g] = (int8_t)(c == 0 ? -1 : d.kind);
    }
    __syncthreads();
    plan_tile_store(A, cell, T, pitch, B, g0, tid);
}

// both entry points: max_moves = 7 for the plain one, whose launches are the CRIT = false instantiations whatever else is passed
static int plan_launch(const char *who, mtfjsp_handle_t h, int32_t K, const int32_t *src_task, const int32_t *src_mach, int64_t src_stride,
                       const int32_t *src_col, uint64_t seed, uint64_t round, uint64_t first_instance, uint32_t moves, uint32_t max_moves,
                       int32_t *task_out, int32_t *mach_out, int8_t *kind_out, const int32_t *path_task, const int8_t *path_arc, const int32_t *path_len)
{
    if (!h) return MTFJSP_ERR_ARG;
    const std::string pre = std::string(who) + ": ";
    if (!src_task || !src_mach || !task_out || !mach_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, (pre + "null argument").c_str());
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.loaded) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, (pre + "no instances loaded").c_str());
    if (K < 1 || v.B % K || moves == 0 || moves > max_moves || src_stride < 1)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, (pre + "K >= 1 must divide the handle's batch, moves must be 1.." + std::to_string(max_moves) + ", src_stride >= 1").c_str());
    const bool crit = (moves & PLAN_CRIT) != 0;
    if (crit && (!path_task || !path_arc || !path_len)) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, (pre + "a critical-path move needs path_task, path_arc and path_len").c_str());
    const unsigned __int128 n_src = (unsigned __int128)v.T * (unsigned __int128)src_stride * 4, n_out = (unsigned __int128)v.T * v.B * 4;
    const unsigned __int128 N = (unsigned __int128)(v.B / K);
    const PlanSpan srcs[6] = {{src_task, n_src}, {src_mach, n_src}, {src_col, N * 4}, {path_task, N * v.T * 4}, {path_arc, N * v.T}, {path_len, N * 4}};
    const PlanSpan outs[3] = {{task_out, n_out}, {mach_out, n_out}, {kind_out, (unsigned __int128)v.B}};
    if (int rc = plan_check_overlap(h, who, 3, outs, 6, srcs)) return rc;
    int tile; size_t lds;
    if (int rc = plan_choose_tile(h, who, [&](int tl) { return plan_lds_bytes(v.T, v.J, tl, crit); }, &tile, &lds)) return rc;
    PlanArgs A{};
    A.K = K; A.src_task = src_task; A.src_mach = src_mach; A.src_stride = src_stride; A.src_col = src_col;
    A.path_task = path_task; A.path_arc = path_arc; A.path_len = path_len;
    const bool small = v.T <= WAVE;
    void (*fn)(PlanArgs) = crit ? (small ? k_plan_neighbours<true, true> : k_plan_neighbours<false, true>)
                                : (small ? k_plan_neighbours<true, false> : k_plan_neighbours<false, false>);
    return plan_launch_tiles(h, who, v, fn, A, tile, lds, seed, round, first_instance, moves, task_out, mach_out, kind_out);
}

extern "C" int mtfjsp_plan_neighbours(mtfjsp_handle_t h, int32_t K, const int32_t *src_task, const int32_t *src_mach, int64_t src_stride,
                                      const int32_t *src_col, uint64_t seed, uint64_t round, uint64_t first_instance, uint32_t moves,
                                      int32_t *task_out, int32_t *mach_out, int8_t *kind_out)
{
    return plan_launch("mtfjsp_plan_neighbours", h, K, src_task, src_mach, src_stride, src_col, seed, round, first_instance, moves, 7u, task_out, mach_out,
                       kind_out, nullptr, nullptr, nullptr);
}

extern "C" int mtfjsp_plan_neighbours_critical(mtfjsp_handle_t h, int32_t K, const int32_t *src_task, const int32_t *src_mach, int64_t src_stride,
                                               const int32_t *src_col, uint64_t seed, uint64_t round, uint64_t first_instance, uint32_t moves,
                                               int32_t *task_out, int32_t *mach_out, int8_t *kind_out, const int32_t *path_task, const int8_t *path_arc,
                                               const int32_t *path_len)
{
    return plan_launch("mtfjsp_plan_neighbours_critical", h, K, src_task, src_mach, src_stride, src_col, seed, round, first_instance, moves, 31u, task_out,
                       mach_out, kind_out, path_task, path_arc, path_len);
}

// ---------------------------------------------------------------- critical path
struct CritArgs {
    int B, n, T, M;
    unsigned inv_M;
    const TaskSD *sd;                  // [B,T]
    const TaskPL *pl;                  // [B,T]
    const double *tt;                  // [B,M,M]
    const int *col;                    // [n] or null
    int *path_task;                    // [n,T]
    int8_t *path_arc;                  // [n,T]
    int *path_len;                     // [n]
};

// per wave: two jump tables that take turns and the walk's positions (u16 [T + 1] each; index T = "no task", which points at itself), the
// arc kind of every task (i8 [T + 1]); rows padded to 4 elements
__host__ __device__ static inline int crit_pitch(int T) { return (T + 4) & ~3; }
static size_t crit_lds_bytes(int T) { return (size_t)PLAN_WAVES * 7 * crit_pitch(T); }

// One wave per row, lanes over tasks.  Every task's own records load coalesced (16 bytes a lane); its two predecessors' records are
// gathers that the caches serve, the wave has just loaded them.  nx[a] = the tight route predecessor, else the tight job predecessor,
// else T.  path_task[k] = nx^k(first): the tables nx^(2^b) are built one from the other by squaring, and position k applies table b
// where bit b of k is set — powers of one map commute, so two tables in LDS are enough and no lane follows more than log2 T pointers.
// The only floating-point operations are ft = st + dur and ft + transport time, the sums the step kernel formed (no multiply next to
// them: nothing to contract).
__global__ __launch_bounds__(PLAN_THREADS) void k_critical_path(CritArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = uni(tid >> 6);
    const int T = A.T, M = A.M, Tp = crit_pitch(T);
    uint16_t *ja = reinterpret_cast<uint16_t *>(smem + (size_t)wave * 7 * Tp), *jb = ja + Tp, *cur = jb + Tp;
    int8_t *ak = reinterpret_cast<int8_t *>(cur + Tp);
    const long row = (long)blockIdx.x * PLAN_WAVES + wave;
    if (row >= A.n) return;                                            // (wave-uniform; the kernel has no workgroup barrier)
    int *pt = A.path_task + (size_t)row * T;
    int8_t *pa = A.path_arc + (size_t)row * T;
    const long b = A.col ? (long)A.col[row] : row;
    WaveBest<true> best;
    if (b >= 0 && b < A.B) {
        const size_t bT = (size_t)b * T;
        const double *tt = A.tt + (size_t)b * M * M;
        for (int s0 = 0; s0 < T; s0 += WAVE) {
            const int a = s0 + lane;
            const bool live = a < T;
            const int ac = live ? a : T - 1;
            const TaskSD x = A.sd[bT + ac];
            const Link l = A.pl[bT + ac].link;
            const int m = l.mach, mp = l.prev;
            const bool sch = live && (unsigned)m < (unsigned)M;
            const int ja_ = (int)plan_mulhi((uint32_t)ac, A.inv_M), op = ac - ja_ * M;
            int nx = T, kind = -1;
            if (sch && (unsigned)mp < (unsigned)T) {
                const TaskSD y = A.sd[bT + mp];
                const double xm = (int)plan_mulhi((uint32_t)mp, A.inv_M) == ja_ ? tt[m * M + m] : 0.0;
                if (x.st == (y.st + y.dur) + xm) { nx = mp; kind = 1; }
            }
            if (sch && kind < 0 && op != 0) {
                const int mj = A.pl[bT + ac - 1].link.mach;
                if ((unsigned)mj < (unsigned)M) {
                    const TaskSD y = A.sd[bT + ac - 1];
                    if (x.st == (y.st + y.dur) + tt[mj * M + m]) { nx = ac - 1; kind = 0; }
                }
            }
            best.pass(sch, x.st + x.dur, s0);
            if (live) { ja[a] = (uint16_t)nx; ak[a] = (int8_t)kind; }
        }
    }
    if (lane == 0) { ja[T] = (uint16_t)T; ak[T] = -1; }
    const int first = best.i < 0 ? T : best.i;
    for (int k = lane; k < T; k += WAVE) cur[k] = (uint16_t)first;
    plan_wave_sync();
    if (first != T) {
        uint16_t *src = ja, *dst = jb;
        for (int bit = 0; (1 << bit) < T; bit++) {
            for (int k = lane; k < T; k += WAVE)
                if ((k >> bit) & 1) cur[k] = src[cur[k]];
            if ((2 << bit) < T) {
                for (int e = lane; e <= T; e += WAVE) dst[e] = src[src[e]];
                plan_wave_sync();
            }
            uint16_t *const t_ = src; src = dst; dst = t_;
        }
    }
    int len = 0;
    for (int s0 = 0; s0 < T; s0 += WAVE) {
        const int k = s0 + lane;
        const int c = k < T ? (int)cur[k] : T;
        len += __popcll(__ballot(c != T));
        if (k < T) { pt[k] = c != T ? c : -1; pa[k] = ak[c]; }
    }
    if (lane == 0) A.path_len[row] = len;
}

extern "C" int mtfjsp_critical_path(mtfjsp_handle_t h, int32_t n, const int32_t *col, int32_t *path_task, int8_t *path_arc, int32_t *path_len)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!path_task || !path_arc || !path_len) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_critical_path: null output");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (n < 1 || (!col && n != v.B)) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_critical_path: n >= 1, and n = the handle's batch without col");
    if (!v.has_schedule()) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_critical_path: the handle holds no schedule (never reset, or plans replayed without MTFJSP_REPLAY_STATE)");
    const size_t lds = crit_lds_bytes(v.T);
    if (lds > PLAN_LDS_HARD) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_critical_path: n_job * n_machine is too large for four paths in LDS");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_critical_path")) return rc;
    CritArgs A{};
    A.B = v.B; A.n = n; A.T = v.T; A.M = v.M;
    A.inv_M = (unsigned)((0x100000000ull + (unsigned)v.M - 1) / (unsigned)v.M);
    A.sd = v.sd; A.pl = v.pl; A.tt = v.tt; A.col = col;
    A.path_task = path_task; A.path_arc = path_arc; A.path_len = path_len;
    if (int rc = mtfjsp_env_dyn_lds(h, (const void *)k_critical_path, lds, "mtfjsp_critical_path")) return rc;
    hipLaunchKernelGGL(k_critical_path, dim3((unsigned)(((size_t)n + PLAN_WAVES - 1) / PLAN_WAVES)), dim3(PLAN_THREADS), lds, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_critical_path");
}

