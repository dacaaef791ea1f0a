// mtfjsp_plan.hip — neighbourhood moves on plans (local search over best-of-K replay: every group's incumbent plan becomes K
// neighbouring plans, copy c of group n = element n*K + c as in mtfjsp_group.hip; the ordinary step kernel replays them and
// mtfjsp_group_reduce keeps the best).
//   mtfjsp_plan_neighbours   k_plan_neighbours: a plan is the job string q[s] = task[s] / M and a machine mu[a] per task.  Copy 0 is
//                            the incumbent; copy c >= 1 draws ONE move — SWAP two positions of q, INSERT one position elsewhere,
//                            REASSIGN one task to another feasible machine — and is decoded again: task'[s] = q'[s]*M + (earlier
//                            occurrences of q'[s]), mach'[s] = mu'[task'[s]].  Any permutation of q is a plan: no repair.
// Integer arithmetic only (Philox words, (w * n) >> 32): the outputs must equal a host model element for element.
// Shape: a workgroup of 4 waves builds a TILE of consecutive copies (64, 32 or 16 by T: the tile lives in LDS), every wave a quarter
// of them one after the other, lanes over positions.  The tile's cells (task | machine << 16) have an odd row pitch: a wave writes
// one copy's column (lane = position) and reads one row (lane = copy) without a bank conflict, and every output row leaves as one
// contiguous run of TILE words — with lane = position the 4-byte stores of a copy would lie N*K*4 bytes apart.  The K copies of a
// group read one source column: the caches serve it, and a wave reloads it only where the group changes.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"

#define PLAN_WAVES 4
#define PLAN_THREADS (PLAN_WAVES * WAVE)
#define PLAN_LDS_SOFT (64 * 1024)      // the tile shrinks (64 -> 32 -> 16 copies) to stay below this: two workgroups per CU
#define PLAN_LDS_HARD (160 * 1024)     // what a workgroup can have at all: the smallest tile may use it
#define PLAN_TAG_MOVE 0x6d6f7665u      // "move"
#define PLAN_SWAP 1
#define PLAN_INSERT 2
#define PLAN_REASSIGN 4

struct PlanArgs {
    int B, K, T, J, M;
    int tile, tile_log2, pitch;        // copies per workgroup, its log2, words per cell row (tile + 1: odd)
    unsigned inv_M;                    // ceil(2^32 / M): task / M = (task * inv_M) >> 32 for task < 2^15
    const double *t;                   // [B,T,M]
    const int *src_task, *src_mach;    // [T,src_stride]
    long long src_stride;
    const int *src_col;                // [B/K] or null
    uint32_t seed_lo, seed_hi, round_lo, first_lo, moves, n_moves;
    int *task_out, *mach_out;          // [T,B]
    int8_t *kind_out;                  // [B] or null
};

// LDS of one wave is written by some lanes and read by others: the hardware keeps a wave's LDS operations in order, this keeps hipcc from moving them
__device__ __forceinline__ void plan_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t plan_mulhi(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * (uint64_t)n) >> 32); }
__device__ __forceinline__ int plan_below(unsigned long long b)          // set bits of b in the lanes below this one
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// bytes of LDS: the tile's cells, then per wave the incumbent's tasks (u16 [T]), the machine of every task (i16 [T]) and the
// operations of every job seen in earlier passes (i32 [J])
static size_t plan_lds_bytes(int T, int J, int tile) { return (size_t)T * (tile + 1) * 4 + (size_t)PLAN_WAVES * ((size_t)T * 4 + (size_t)J * 4); }

// SMALL: T <= 64 — one pass, the incumbent's job string stays in registers and the position map is a ds_bpermute
template <bool SMALL>
__global__ __launch_bounds__(PLAN_THREADS) void k_plan_neighbours(PlanArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = uni(tid >> 6);
    const int T = A.T, M = A.M, J = A.J, pitch = A.pitch, B = A.B;
    uint32_t *cell = reinterpret_cast<uint32_t *>(smem);                                   // [T][pitch]
    uint16_t *inc = reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)wave * T;
    int16_t *mu = reinterpret_cast<int16_t *>(reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)PLAN_WAVES * T) + (size_t)wave * T;
    int *cnt = reinterpret_cast<int *>(reinterpret_cast<uint16_t *>(cell + (size_t)T * pitch) + (size_t)2 * PLAN_WAVES * T) + (size_t)wave * J;
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
            plan_wave_sync();
            unsigned long long badm = 0;
            for (int s0 = 0; s0 < T; s0 += WAVE) {
                const int s = s0 + lane, sc = s < T ? s : T - 1;
                const int tk = A.src_task[(size_t)sc * A.src_stride + col], mc = A.src_mach[(size_t)sc * A.src_stride + col];
                const bool ok = (unsigned)tk < (unsigned)T && (unsigned)mc < (unsigned)M;
                badm |= __ballot(!ok);
                const int tkc = ok ? tk : 0, mcc = ok ? mc : 0;
                if (s < T) { inc[s] = (uint16_t)tkc; mu[tkc] = (int16_t)mcc; }
                if (SMALL) { tk_r = tkc; q_r = (int)plan_mulhi((uint32_t)tkc, A.inv_M); }
            }
            bad = cbad || badm != 0;
            plan_wave_sync();
        }
        // ---- the draw (wave-uniform).  Copy 0 takes none.
        uint32_t w[4] = {A.first_lo + (uint32_t)n, (uint32_t)c, A.round_lo, PLAN_TAG_MOVE};
        philox4x32(w, A.seed_lo, A.seed_hi);
        uint32_t mv = A.moves;
        for (int k = (int)plan_mulhi(w[0], A.n_moves); k > 0; k--) mv &= mv - 1;
        const int kind = (int)(mv & (0u - mv));
        const int x = uni((int)plan_mulhi(w[1], (uint32_t)T));
        int y = T >= 2 ? (int)plan_mulhi(w[2], (uint32_t)(T - 1)) : 0;
        y += (T >= 2 && y >= x) ? 1 : 0;
        const int move = (c == 0 || (T < 2 && kind != PLAN_REASSIGN)) ? 0 : kind;   // 0: identity
        // ---- REASSIGN's candidates: the feasible machines of task a other than its own, ascending = lane order (M <= 64)
        const int a = SMALL ? rl_i(tk_r, x) : (int)inc[x];
        const int old_m = mu[a];
        const double tv = A.t[((size_t)g * T + a) * M + (lane < M ? lane : M - 1)];
        const bool feas = lane < M && tv >= 0 && lane != old_m;
        const unsigned long long fb = __ballot(feas);
        const int nf = __popcll(fb);
        const int pick = (int)plan_mulhi(w[2], (uint32_t)nf);
        const unsigned long long sel = __ballot(feas && plan_below(fb) == pick);
        const bool reassign = move == PLAN_REASSIGN && nf > 0;
        if (reassign) {
            if (lane == 0) mu[a] = (int16_t)__builtin_ctzll(sel);
            plan_wave_sync();
        }
        if (!SMALL) {
            for (int j = lane; j < J; j += WAVE) cnt[j] = 0;
            plan_wave_sync();
        }
        // ---- q' = q gathered through the move's position map, the operation ranks, the machines
        for (int s0 = 0; s0 < T; s0 += WAVE) {
            const int s = s0 + lane;
            int src = s;
            if (move == PLAN_SWAP) src = s == x ? y : (s == y ? x : s);
            if (move == PLAN_INSERT) {                                  // q.pop(x), q.insert(y, it)
                if (s == y) src = x;
                else if (x < y && s >= x && s < y) src = s + 1;
                else if (y < x && s > y && s <= x) src = s - 1;
            }
            src = src < T ? src : T - 1;
            int qn;
            if (SMALL) qn = __builtin_amdgcn_ds_bpermute(src << 2, q_r);
            else qn = (int)plan_mulhi((uint32_t)inc[src], A.inv_M);
            const bool live = s < T;
            int rank = 0;
            bool last = false;                                          // the pass's last position of its job
            for (int j = 0; j < J; j++) {                               // one wave-uniform ballot per job
                const unsigned long long b = __ballot(live && qn == j);
                if (qn == j) { rank = plan_below(b); last = (b >> lane) == 1ull; }
            }
            if (!SMALL) {
                rank += cnt[qn];
                plan_wave_sync();
                if (live && last) cnt[qn] = rank + 1;
                plan_wave_sync();
            }
            const bool okr = c == 0 || rank < M;                        // (fails only for an incumbent that is no plan: too many operations of one job)
            int tn = okr ? qn * M + rank : 0;
            if (c == 0) tn = SMALL ? tk_r : (int)inc[live ? s : T - 1];  // copy 0 is the incumbent word for word, not its decoding
            const int mn = mu[tn];
            const uint32_t word = (bad || !okr) ? 0xFFFFFFFFu : ((uint32_t)tn | ((uint32_t)(uint16_t)mn << 16));
            if (live) cell[(size_t)s * pitch + ct] = word;
        }
        if (reassign) {
            plan_wave_sync();
            if (lane == 0) mu[a] = (int16_t)old_m;
            plan_wave_sync();
        }
        if (A.kind_out && lane == 0 && gl < B) A.kind_out[g] = (int8_t)(c == 0 ? -1 : kind);
    }
    __syncthreads();
    // ---- the tile leaves row by row: lane = copy, one contiguous run per row and array
    const int total = T << A.tile_log2;
    for (int e = tid; e < total; e += PLAN_THREADS) {
        const int s = e >> A.tile_log2, ct = e & (A.tile - 1);
        const long gl = g0 + ct;
        const uint32_t word = cell[(size_t)s * pitch + ct];
        if (gl < B) {
            A.task_out[(size_t)s * B + gl] = (int)(int16_t)(word & 0xFFFFu);
            A.mach_out[(size_t)s * B + gl] = (int)(int16_t)(word >> 16);
        }
    }
}

static bool plan_overlap(const void *a, unsigned __int128 na, const void *b, unsigned __int128 nb)
{
    if (!a || !b) return false;
    const unsigned __int128 x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

extern "C" int mtfjsp_plan_neighbours(mtfjsp_handle_t h, int32_t K, const int32_t *src_task, const int32_t *src_mach, int64_t src_stride,
                                      const int32_t *src_col, uint64_t seed, uint64_t round, uint64_t first_instance, uint32_t moves,
                                      int32_t *task_out, int32_t *mach_out, int8_t *kind_out)
{
    if (!h) return MTFJSP_ERR_ARG;
    if (!src_task || !src_mach || !task_out || !mach_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_neighbours: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.loaded) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_plan_neighbours: no instances loaded");
    if (K < 1 || v.B % K || moves == 0 || moves > 7 || src_stride < 1)
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_neighbours: K >= 1 must divide the handle's batch, moves must be 1..7, src_stride >= 1");
    const unsigned __int128 n_src = (unsigned __int128)v.T * (unsigned __int128)src_stride * 4, n_out = (unsigned __int128)v.T * v.B * 4;
    const void *srcs[3] = {src_task, src_mach, src_col};
    const unsigned __int128 n_srcs[3] = {n_src, n_src, (unsigned __int128)(v.B / K) * 4};
    const void *outs[3] = {task_out, mach_out, kind_out};
    const unsigned __int128 n_outs[3] = {n_out, n_out, (unsigned __int128)v.B};
    for (int o = 0; o < 3; o++) {
        for (int s = 0; s < 3; s++)
            if (plan_overlap(outs[o], n_outs[o], srcs[s], n_srcs[s]))
                return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_neighbours: an output array overlaps a source array");
        for (int p = 0; p < o; p++)
            if (plan_overlap(outs[o], n_outs[o], outs[p], n_outs[p]))
                return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_neighbours: the output arrays overlap");
    }
    int tile = 64;
    while (tile > 16 && plan_lds_bytes(v.T, v.J, tile) > PLAN_LDS_SOFT) tile >>= 1;
    const size_t lds = plan_lds_bytes(v.T, v.J, tile);
    if (lds > PLAN_LDS_HARD) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_neighbours: n_job * n_machine is too large for a tile of 16 plans in LDS");
    if (int rc = mtfjsp_env_set_device(h, v.device_id, "mtfjsp_plan_neighbours")) return rc;
    PlanArgs A{};
    A.B = v.B; A.K = K; A.T = v.T; A.J = v.J; A.M = v.M;
    A.tile = tile; A.tile_log2 = tile == 64 ? 6 : (tile == 32 ? 5 : 4); A.pitch = tile + 1;
    A.inv_M = (unsigned)((0x100000000ull + (unsigned)v.M - 1) / (unsigned)v.M);
    A.t = v.t; A.src_task = src_task; A.src_mach = src_mach; A.src_stride = src_stride; A.src_col = src_col;
    A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32); A.round_lo = (uint32_t)round; A.first_lo = (uint32_t)first_instance;
    A.moves = moves; A.n_moves = (uint32_t)__builtin_popcount(moves);
    A.task_out = task_out; A.mach_out = mach_out; A.kind_out = kind_out;
    const void *fn = v.T <= WAVE ? (const void *)k_plan_neighbours<true> : (const void *)k_plan_neighbours<false>;
    if (lds > 48 * 1024)
        if (int rc = mtfjsp_env_hip_check(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "mtfjsp_plan_neighbours",
                                          "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"))
            return rc;
    const dim3 grid((unsigned)(((size_t)v.B + tile - 1) / tile));
    if (v.T <= WAVE) hipLaunchKernelGGL(k_plan_neighbours<true>, grid, dim3(PLAN_THREADS), lds, v.stream, A);
    else hipLaunchKernelGGL(k_plan_neighbours<false>, grid, dim3(PLAN_THREADS), lds, v.stream, A);
    return mtfjsp_env_launched(h, "mtfjsp_plan_neighbours");
}
