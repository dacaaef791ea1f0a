// mtfjsp_evolve.hip — recombination of plans (evolutionary search over best-of-K replay: a population of P plans per instance, member c
// of group n = element n*P + c as in mtfjsp_group.hip, becomes its offspring in one launch; the ordinary step kernel replays them and
// mtfjsp_group_reduce writes the objectives and the best member the next generation selects by).
//   mtfjsp_plan_offspring   k_plan_offspring: child 0 is the elite (the reduction's best member, word for word); every other child draws
//                           two parents by binary tournaments on src_obj, with probability cross_thr / 2^32 crosses them — the job string
//                           by precedence-preserving order crossover (the jobs of a random set S keep parent A's positions, the other
//                           positions take parent B's remaining entries in B's order), the machine of every task from A or B by a coin —
//                           with probability mut_thr / 2^32 takes one move of mtfjsp_plan_neighbours, and is decoded as that kernel decodes.
// Integer arithmetic and comparisons only (Philox words, (w * n) >> 32, binary64 <): the outputs must equal a host model element for
// element.
// Shape: k_plan_neighbours' — the tile, the move, the decoding's ranks, the tile's way out and the host side of the launch are
// mtfjsp_plan_dev.h's, used by both.  What is here: a child has parents of its own, so a wave keeps two of them in LDS (tasks by position,
// machine by task) and reloads one only where it changes; the set S and the machine coins are the Philox words themselves, one block
// per lane, kept as bit maps; the crossover's fill is a stream compaction (ballot + mbcnt ranks of B's entries outside S into a list,
// position s outside S reads list[rank(s)]).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtfjsp.h"

#include "mtfjsp_env_dev.h"
#include "mtfjsp_plan_dev.h"

#define EVO_TAG_PARE 0x70617265u       // "pare"
#define EVO_TAG_CROS 0x63726f73u       // "cros"
#define EVO_TAG_JSET 0x6a736574u       // "jset"
#define EVO_TAG_MACH 0x6d616368u       // "mach"

struct EvoArgs {
    int B, P, T, J, M;
    int tile, tile_log2, pitch;        // children per workgroup, its log2, words per cell row (tile + 1: odd)
    int sw, mw;                        // words of the bit maps: the job set S (J bits), the machine coins (T bits)
    unsigned inv_M;                    // ceil(2^32 / M): task / M = (task * inv_M) >> 32 for task < 2^15
    const double *t;                   // [B,T,M]
    const int *src_task, *src_mach;    // [T,B]
    const double *src_obj;             // [B]
    const int *src_best;               // [B/P] or null
    uint32_t seed_lo, seed_hi, ctr_lo, first_lo, moves, n_moves;   // ctr_lo: the generation
    unsigned long long cross_thr, mut_thr;
    int *task_out, *mach_out;          // [T,B]
    int *parent_out;                   // [B,2] or null
    int8_t *kind_out;                  // [B] or null
};

// bytes of LDS of one wave: both parents' tasks by position (u16 [T]) and machine by task (i16 [T]), the child's job string and the list
// of B's entries outside S (u16 [T] each), the operations of every job seen in earlier passes (i32 [J]), the two bit maps
static size_t evo_wave_bytes(int T, int J) { return (size_t)T * 12 + (size_t)J * 4 + (size_t)((J + 31) / 32 + (T + 31) / 32) * 4; }
static size_t evo_lds_bytes(int T, int J, int tile) { return (size_t)T * (tile + 1) * 4 + (size_t)PLAN_WAVES * evo_wave_bytes(T, J); }

// one column of the population into a wave's LDS: tasks by position, machines scattered by task (-1 where no position names the task)
// -> the column is no parent: an entry out of range (it is stored as task 0 / machine 0: every later access stays inside the arrays), or
// not every task exactly once
__device__ __forceinline__ bool evo_load(const EvoArgs &A, long col, uint16_t *tk_, int16_t *mu_, int lane)
{
    const int T = A.T;
    for (int s = lane; s < T; s += WAVE) mu_[s] = -1;
    plan_wave_sync();
    unsigned long long badm = 0;
    for (int s0 = 0; s0 < T; s0 += WAVE) {
        const int s = s0 + lane, sc = s < T ? s : T - 1;
        const int tk = A.src_task[(size_t)sc * A.B + col], mc = A.src_mach[(size_t)sc * A.B + col];
        const bool ok = (unsigned)tk < (unsigned)T && (unsigned)mc < (unsigned)A.M;
        badm |= __ballot(!ok);
        const int tkc = ok ? tk : 0, mcc = ok ? mc : 0;
        if (s < T) { tk_[s] = (uint16_t)tkc; mu_[tkc] = (int16_t)mcc; }
    }
    plan_wave_sync();
    for (int s0 = 0; s0 < T; s0 += WAVE) badm |= __ballot(s0 + lane < T && mu_[s0 + lane < T ? s0 + lane : 0] < 0);   // a task twice leaves another without a machine
    return badm != 0;
}

// the better of members i and j of a group: the smaller objective, a NaN loses to any number, equal ones or two NaNs go to the lower index
__device__ __forceinline__ int evo_better(const double *obj, int i, int j)
{
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const double ol = obj[lo], oh = obj[hi];
    return (oh < ol || (ol != ol && oh == oh)) ? hi : lo;
}

__device__ __forceinline__ uint32_t evo_word(const uint32_t w[4], int k) { return k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : w[3])); }

__global__ __launch_bounds__(PLAN_THREADS) void k_plan_offspring(EvoArgs A)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = uni(tid >> 6);
    const int T = A.T, M = A.M, J = A.J, pitch = A.pitch, B = A.B, P = A.P;
    uint32_t *cell = reinterpret_cast<uint32_t *>(smem);                                   // [T][pitch]
    unsigned char *mine = reinterpret_cast<unsigned char *>(cell + (size_t)T * pitch) + (size_t)wave * ((size_t)T * 12 + (size_t)(J + A.sw + A.mw) * 4);
    uint16_t *tkA = reinterpret_cast<uint16_t *>(mine), *tkB = tkA + 2 * (size_t)T, *qn = tkA + 4 * (size_t)T, *list = tkA + 5 * (size_t)T;
    int16_t *muA = reinterpret_cast<int16_t *>(tkA + T), *muB = reinterpret_cast<int16_t *>(tkB + T);
    int *cnt = reinterpret_cast<int *>(tkA + 6 * (size_t)T);
    uint32_t *sb = reinterpret_cast<uint32_t *>(cnt + J), *mb = sb + A.sw;
    const long g0 = (long)blockIdx.x * A.tile;
    const int per = A.tile / PLAN_WAVES;
    long haveA = -1, haveB = -1;                                       // the columns in tkA / muA and tkB / muB
    bool badA = false, badB = false;
    for (int i = 0; i < per; i++) {
        const int ct = wave * per + i;
        const long gl = g0 + ct;
        const int g = (int)(gl < B ? gl : B - 1);                     // (a child past the batch rebuilds the last one; its column is never stored)
        const int n = g / P, c = g - n * P;
        const long base = (long)n * P;
        const uint32_t inst = A.first_lo + (uint32_t)n;
        plan_wave_sync();
        bool kill;                                                     // the child cannot be formed: -1 in every row
        int kind_o = -1, pa = -1, pb = -1;
        if (A.src_best && c == 0) {
            // ---- the elite: the reduction's best member as it is
            long col = (long)A.src_best[n];
            col = (col < base || col >= base + P) ? base : col;
            unsigned long long badm = 0;
            for (int s0 = 0; s0 < T; s0 += WAVE) {
                const int s = s0 + lane, sc = s < T ? s : T - 1;
                const int tk = A.src_task[(size_t)sc * B + col], mc = A.src_mach[(size_t)sc * B + col];
                badm |= __ballot(!((unsigned)tk < (unsigned)T && (unsigned)mc < (unsigned)M));
                if (s < T) cell[(size_t)s * pitch + ct] = plan_cell(tk, mc);   // (an entry out of range: the column is killed below)
            }
            kill = badm != 0;
        } else {
            // ---- the draws (wave-uniform): two tournaments, the crossover and mutation events
            uint32_t w[4] = {inst, (uint32_t)c, A.ctr_lo, EVO_TAG_PARE};
            philox4x32(w, A.seed_lo, A.seed_hi);
            const double *obj = A.src_obj + base;
            const int ma = uni(evo_better(obj, (int)plan_mulhi(w[0], (uint32_t)P), (int)plan_mulhi(w[1], (uint32_t)P)));
            const int mbm = uni(evo_better(obj, (int)plan_mulhi(w[2], (uint32_t)P), (int)plan_mulhi(w[3], (uint32_t)P)));
            uint32_t v[4] = {inst, (uint32_t)c, A.ctr_lo, EVO_TAG_CROS};
            philox4x32(v, A.seed_lo, A.seed_hi);
            const bool cross = (unsigned long long)v[0] < A.cross_thr, mut = (unsigned long long)v[1] < A.mut_thr;
            const long colA = base + ma, colB = base + mbm;
            pa = (int)colA;
            pb = cross ? (int)colB : -1;
            if (colA != haveA) { badA = evo_load(A, colA, tkA, muA, lane); haveA = colA; }
            if (cross && colB != haveB) { badB = evo_load(A, colB, tkB, muB, lane); haveB = colB; }
            const bool bad = badA || (cross && badB);
            // ---- S and the machine coins: bit j % 32 of word (j / 32) % 4 of block j / 128 = bit j of the map.  No crossover: all of A
            for (int l = lane; l < A.sw; l += WAVE) {
                uint32_t u[4] = {inst, (uint32_t)c, A.ctr_lo, EVO_TAG_JSET + (uint32_t)(l >> 2)};
                philox4x32(u, A.seed_lo, A.seed_hi);
                sb[l] = cross ? evo_word(u, l & 3) : 0xFFFFFFFFu;
            }
            for (int l = lane; l < A.mw; l += WAVE) {
                uint32_t u[4] = {inst, (uint32_t)c, A.ctr_lo, EVO_TAG_MACH + (uint32_t)(l >> 2)};
                philox4x32(u, A.seed_lo, A.seed_hi);
                mb[l] = cross ? evo_word(u, l & 3) : 0xFFFFFFFFu;
            }
            for (int j = lane; j < J; j += WAVE) cnt[j] = 0;
            plan_wave_sync();
            // ---- q': B's entries outside S, in B's order, into list[]; then A's entries inside S stay, the holes take list[] in order
            int nL = 0, nH = 0;
            if (cross) {
                for (int s0 = 0; s0 < T; s0 += WAVE) {
                    const int s = s0 + lane;
                    const int jb = (int)plan_mulhi((uint32_t)tkB[s < T ? s : 0], A.inv_M);
                    const bool out = s < T && !((sb[jb >> 5] >> (jb & 31)) & 1u);
                    const unsigned long long eb = __ballot(out);
                    if (out) list[nL + plan_below(eb)] = (uint16_t)jb;
                    nL += __popcll(eb);
                }
                plan_wave_sync();
            }
            for (int s0 = 0; s0 < T; s0 += WAVE) {
                const int s = s0 + lane;
                const int ja = (int)plan_mulhi((uint32_t)tkA[s < T ? s : 0], A.inv_M);
                const bool hole = s < T && !((sb[ja >> 5] >> (ja & 31)) & 1u);
                const unsigned long long hb = __ballot(hole);
                const int r = nH + plan_below(hb);
                const int fill = (int)list[r < nL ? r : 0];            // (parents that are plans: as many holes as entries of the list)
                if (s < T) qn[s] = (uint16_t)(hole ? (r < nL ? fill : 0) : ja);
                nH += __popcll(hb);
            }
            plan_wave_sync();
            // ---- the mutation: one move of k_plan_neighbours (plan_draw) on q', mu'
            int move = 0, kind = 0, x = 0, y = 0, a = 0, am = -1;
            bool reassign = false;
            if (mut) {
                const PlanMove d = plan_draw(inst, (uint32_t)c, A.ctr_lo, A.seed_lo, A.seed_hi, A.moves, A.n_moves, T);
                kind = d.kind; move = d.move; x = d.x; y = d.y;
                if (move == PLAN_REASSIGN) {                           // a = the task at position x of q' decoded; F = its other feasible machines, ascending = lane order
                    const int jx = uni((int)qn[x]);
                    int rk = 0;
                    for (int s0 = 0; s0 < x; s0 += WAVE) {
                        const int s = s0 + lane;
                        rk += __popcll(__ballot(s < x && (int)qn[s < x ? s : 0] == jx));
                    }
                    a = rk < M ? jx * M + rk : 0;                      // (rk >= M only for parents that are no plans: the child is -1 anyway)
                    const int old_m = ((mb[a >> 5] >> (a & 31)) & 1u) ? (int)muA[a] : (int)muB[a];
                    reassign = plan_other_machine(A.t, ((size_t)g * T + a) * M, M, old_m, d.wy, lane, &am) > 0;
                }
            }
            kind_o = mut ? kind : 0;
            // ---- q' gathered through the move's position map, the operation ranks, the machines
            for (int s0 = 0; s0 < T; s0 += WAVE) {
                const int s = s0 + lane;
                const int qv = (int)qn[plan_src(move, s, x, y, T)];
                const bool live = s < T;
                const int rank = plan_rank<true>(qv, live, J, lane, cnt);
                const bool okr = rank < M;                              // (fails only for parents that are no plans, whose child is -1 anyway)
                const int tn = okr ? qv * M + rank : 0;
                const int mn = (reassign && tn == a) ? am : (((mb[tn >> 5] >> (tn & 31)) & 1u) ? (int)muA[tn] : (int)muB[tn]);
                if (live) cell[(size_t)s * pitch + ct] = plan_cell(tn, mn);
            }
            kill = bad;
        }
        if (kill)
            for (int s = lane; s < T; s += WAVE) cell[(size_t)s * pitch + ct] = PLAN_CELL_KILLED;
        if (lane == 0 && gl < B) {
            if (A.kind_out) A.kind_out[g] = (int8_t)kind_o;
            if (A.parent_out) { A.parent_out[2 * (size_t)g] = pa; A.parent_out[2 * (size_t)g + 1] = pb; }
        }
    }
    __syncthreads();
    plan_tile_store(A, cell, T, pitch, B, g0, tid);
}

extern "C" int mtfjsp_plan_offspring(mtfjsp_handle_t h, int32_t P, const int32_t *src_task, const int32_t *src_mach, const double *src_obj,
                                     const int32_t *src_best, uint64_t seed, uint64_t generation, uint64_t first_instance, uint64_t cross_thr,
                                     uint64_t mut_thr, uint32_t moves, int32_t *task_out, int32_t *mach_out, int32_t *parent_out, int8_t *kind_out)
{
    const char *who = "mtfjsp_plan_offspring";
    if (!h) return MTFJSP_ERR_ARG;
    if (!src_task || !src_mach || !src_obj || !task_out || !mach_out) return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_offspring: null argument");
    EnvHostView v;
    mtfjsp_env_host_view(h, &v);
    if (!v.loaded) return mtfjsp_env_fail(h, MTFJSP_ERR_STATE, "mtfjsp_plan_offspring: no instances loaded");
    if (P < 1 || v.B % P || moves == 0 || moves > 7 || cross_thr > (1ull << 32) || mut_thr > (1ull << 32))
        return mtfjsp_env_fail(h, MTFJSP_ERR_ARG, "mtfjsp_plan_offspring: P >= 1 must divide the handle's batch, moves must be 1..7, the thresholds at most 2^32");
    const unsigned __int128 n_plan = (unsigned __int128)v.T * v.B * 4;
    const PlanSpan srcs[4] = {{src_task, n_plan}, {src_mach, n_plan}, {src_obj, (unsigned __int128)v.B * 8}, {src_best, (unsigned __int128)(v.B / P) * 4}};
    const PlanSpan outs[4] = {{task_out, n_plan}, {mach_out, n_plan}, {parent_out, (unsigned __int128)v.B * 8}, {kind_out, (unsigned __int128)v.B}};
    if (int rc = plan_check_overlap(h, who, 4, outs, 4, srcs)) return rc;
    int tile; size_t lds;
    if (int rc = plan_choose_tile(h, who, [&](int tl) { return evo_lds_bytes(v.T, v.J, tl); }, &tile, &lds)) return rc;
    EvoArgs A{};
    A.P = P; A.sw = (v.J + 31) / 32; A.mw = (v.T + 31) / 32;
    A.src_task = src_task; A.src_mach = src_mach; A.src_obj = src_obj; A.src_best = src_best;
    A.cross_thr = cross_thr; A.mut_thr = mut_thr; A.parent_out = parent_out;
    return plan_launch_tiles(h, who, v, k_plan_offspring, A, tile, lds, seed, generation, first_instance, moves, task_out, mach_out, kind_out);
}
