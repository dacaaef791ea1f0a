// mtfjsp_plan_dev.h — what the kernels on plans share (mtfjsp_plan.hip: neighbourhood moves, critical path; mtfjsp_evolve.hip: offspring
// of a population): the workgroup shape and wave-level helpers; THE MOVE, stated once — the rule include/mtfjsp.h describes and
// tests/plan_moves_ref.py models; THE TILE of plans in LDS and its way out; the host side of a launch by tiles.
// The loads of a source column stay with their kernels (k_plan_neighbours' incumbent, evo_load): the first keeps the job string in registers
// for SMALL and the position map for CRIT, the second checks for duplicates — one body would need mode flags.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "mtfjsp_env_dev.h"

#define PLAN_WAVES 4
#define PLAN_THREADS (PLAN_WAVES * WAVE)
#define PLAN_LDS_SOFT (64 * 1024)      // the tile shrinks (64 -> 32 -> 16 copies) to stay below this: two workgroups per CU
#define PLAN_LDS_HARD (160 * 1024)     // what a workgroup can have at all: the smallest tile may use it
#define PLAN_TAG_MOVE 0x6d6f7665u      // "move"
#define PLAN_SWAP 1
#define PLAN_INSERT 2
#define PLAN_REASSIGN 4
#define PLAN_CELL_KILLED 0xFFFFFFFFu   // a cell of a column that cannot be formed: -1 in both outputs

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

// ---------------------------------------------------------------- the move
// kind: the drawn bit of `moves`; move: what is applied — the kind, or 0 (identity) where T < 2 leaves SWAP and INSERT nothing to do;
// x, y: two different positions (y = x only for T < 2); wx, wy: the words they came from — REASSIGN picks its machine with wy, the moves
// a critical path directs pick their arc or task with wx
struct PlanMove { int kind, move, x, y; uint32_t wx, wy; };
// the draw (wave-uniform) of copy `copy` of instance word `inst` under the counter word `ctr` (a round, a generation)
__device__ __forceinline__ PlanMove plan_draw(uint32_t inst, uint32_t copy, uint32_t ctr, uint32_t seed_lo, uint32_t seed_hi, uint32_t moves, uint32_t n_moves, int T)
{
    uint32_t w[4] = {inst, copy, ctr, PLAN_TAG_MOVE};
    philox4x32(w, seed_lo, seed_hi);
    uint32_t mv = moves;
    for (int k = (int)plan_mulhi(w[0], n_moves); k > 0; k--) mv &= mv - 1;
    PlanMove d;
    d.kind = (int)(mv & (0u - mv));
    d.x = uni((int)plan_mulhi(w[1], (uint32_t)T));
    d.y = T >= 2 ? (int)plan_mulhi(w[2], (uint32_t)(T - 1)) : 0;
    d.y += (T >= 2 && d.y >= d.x) ? 1 : 0;
    d.move = (T < 2 && d.kind != PLAN_REASSIGN) ? 0 : d.kind;
    d.wx = w[1]; d.wy = w[2];
    return d;
}
// the position map: position s of the moved job string is position plan_src of the string before (clamped for the lanes past T)
__device__ __forceinline__ int plan_src(int move, int s, int x, int y, int T)
{
    int src = s;
    if (move == PLAN_SWAP) src = s == x ? y : (s == y ? x : s);
    if (move == PLAN_INSERT) {                                          // q.pop(x), q.insert(y, it)
        if (s == y) src = x;
        else if (x < y && s >= x && s < y) src = s + 1;
        else if (y < x && s > y && s <= x) src = s - 1;
    }
    return src < T ? src : T - 1;
}
// REASSIGN's candidates: the feasible machines of a task (its M times from t[row]) other than old_m, ascending = lane order (M <= 64)
// -> their number; *chosen = the one the word picks, -1 where there is none
__device__ __forceinline__ int plan_other_machine(const double *t, size_t row, int M, int old_m, uint32_t word, int lane, int *chosen)
{
    const double tv = t[row + (lane < M ? lane : M - 1)];
    const bool feas = lane < M && tv >= 0 && lane != old_m;
    const unsigned long long fb = __ballot(feas);
    const int nf = __popcll(fb);
    const unsigned long long sel = __ballot(feas && plan_below(fb) == (int)plan_mulhi(word, (uint32_t)nf));
    *chosen = nf > 0 ? (int)__builtin_ctzll(sel) : -1;
    return nf;
}
// the rank of a position's job q among the earlier live positions of q: one wave-uniform ballot per job for the pass of 64 positions.
// CARRY (more passes than one, T > 64): cnt[j] (LDS of the wave, zero before the first pass) holds the operations of job j seen in
// earlier passes; without it cnt is not touched
template <bool CARRY>
__device__ __forceinline__ int plan_rank(int q, bool live, int J, int lane, int *cnt)
{
    int rank = 0;
    bool last = false;                                                  // the pass's last position of its job
    for (int j = 0; j < J; j++) {
        const unsigned long long b = __ballot(live && q == j);
        if (q == j) { rank = plan_below(b); last = (b >> lane) == 1ull; }
    }
    if (CARRY) {
        rank += cnt[q];
        plan_wave_sync();
        if (live && last) cnt[q] = rank + 1;
        plan_wave_sync();
    }
    return rank;
}

// ---------------------------------------------------------------- the tile
// A workgroup of 4 waves builds a TILE of consecutive copies (64, 32 or 16 by T: the tile lives in LDS), every wave a quarter of them one
// after the other, lanes over positions.  The tile's cells have an odd row pitch: a wave writes one copy's column (lane = position) and
// reads one row (lane = copy) without a bank conflict, and every output row leaves as one contiguous run of TILE words — with lane =
// position the 4-byte stores of a copy would lie B*4 bytes apart.  A cell: task in the low half, machine in the high half — both in
// range, or the column is one that gets PLAN_CELL_KILLED in every row (an entry out of range would spill into the other half)
__device__ __forceinline__ uint32_t plan_cell(int task, int mach) { return (uint32_t)task | ((uint32_t)(uint16_t)mach << 16); }
// the tile leaves row by row (after the workgroup's barrier): lane = copy, one contiguous run per row and array; A: the kernel's arguments
template <class Args>
__device__ __forceinline__ void plan_tile_store(const Args &A, const uint32_t *cell, int T, int pitch, int B, long g0, int tid)
{
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

// ---------------------------------------------------------------- the host side of a launch by tiles
struct PlanSpan { const void *p; unsigned __int128 bytes; };            // an argument array; a null one overlaps nothing
static inline bool plan_overlap(const PlanSpan &a, const PlanSpan &b)
{
    const unsigned __int128 x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}
// every output against every source and against the outputs before it -> 0 or MTFJSP_ERR_ARG
static inline int plan_check_overlap(mtfjsp_handle_t h, const char *who, int n_out, const PlanSpan *outs, int n_src, const PlanSpan *srcs)
{
    for (int o = 0; o < n_out; o++) {
        for (int s = 0; s < n_src; s++)
            if (plan_overlap(outs[o], srcs[s])) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, (std::string(who) + ": an output array overlaps a source array").c_str());
        for (int p = 0; p < o; p++)
            if (plan_overlap(outs[o], outs[p])) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, (std::string(who) + ": the output arrays overlap").c_str());
    }
    return 0;
}
// the tile: the largest of 64, 32, 16 whose bytes(tile) of LDS stay below PLAN_LDS_SOFT, else 16 -> 0 or MTFJSP_ERR_ARG (16 does not fit at all)
template <class Bytes>
static inline int plan_choose_tile(mtfjsp_handle_t h, const char *who, Bytes bytes, int *tile, size_t *lds)
{
    *tile = 64;
    while (*tile > 16 && bytes(*tile) > PLAN_LDS_SOFT) *tile >>= 1;
    *lds = bytes(*tile);
    if (*lds > PLAN_LDS_HARD) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, (std::string(who) + ": n_job * n_machine is too large for a tile of 16 plans in LDS").c_str());
    return 0;
}
// A (the kernel's own fields set by the caller) gets the fields PlanArgs and EvoArgs share, fn its dynamic LDS above 48 KiB, and the
// launch goes out: one workgroup per tile of the handle's batch
template <class Args>
static inline int plan_launch_tiles(mtfjsp_handle_t h, const char *who, const EnvHostView &v, void (*fn)(Args), Args A, int tile, size_t lds, uint64_t seed,
                                    uint64_t counter, uint64_t first_instance, uint32_t moves, int32_t *task_out, int32_t *mach_out, int8_t *kind_out)
{
    if (int rc = mtfjsp_env_set_device(h, v.device_id, who)) return rc;
    A.B = v.B; A.T = v.T; A.J = v.J; A.M = v.M;
    A.tile = tile; A.tile_log2 = tile == 64 ? 6 : (tile == 32 ? 5 : 4); A.pitch = tile + 1;
    A.inv_M = (unsigned)((0x100000000ull + (unsigned)v.M - 1) / (unsigned)v.M); A.t = v.t;
    A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32); A.ctr_lo = (uint32_t)counter; A.first_lo = (uint32_t)first_instance;
    A.moves = moves; A.n_moves = (uint32_t)__builtin_popcount(moves); A.task_out = task_out; A.mach_out = mach_out; A.kind_out = kind_out;
    if (int rc = mtfjsp_env_dyn_lds(h, (const void *)fn, lds, who)) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)(((size_t)v.B + tile - 1) / tile)), dim3(PLAN_THREADS), lds, v.stream, A);
    return mtfjsp_env_launched(h, who);
}
