// mtfjsp_copy_costs.h — a copy's costs: the rule that the kernels selecting over a group of copies follow (k_group_reduce, k_walk_accept,
// k_front_rank), and what of it they can share as code.  Copy c has four final costs (mtfjsp_final_costs: makespan, processing energy / T,
// transport time, idle time) and a done flag.
//   THE POINT    (mk, ec, tt) = (c0, c1 + c3, c2), objective ob = (w_mk * mk + w_ec * ec) + w_tt * tt: ONE addition for the energy, then numpy's
//                `w[0] * mk + w[1] * ec + w[2] * tt` left to right, never contracted — evaluate.episode_results' Objective, and the order
//                tests/group_reduce_ref.py, walk_ref.py and nsga_ref.py model bit for bit
//   ELIGIBLE     the copy exists (c < K), is done and none of mk, ec, tt is a NaN; an ineligible copy carries NaN for mk and ob: every
//                comparison with it is false, so it neither dominates nor is picked.  THE RECORD: (mk, ec, tt, ob), 32 bytes of LDS
//   THE MINIMUM  thread tid of THREADS owns copies tid, tid + THREADS, ... in registers; pass i of wave w over the minimum — copies w*64 +
//                THREADS*i + lane — is exactly its i-th owned copy, so the minimum reads no LDS (WaveBest, mtfjsp_wave_select.h)
// Shared as code: the weights, and the dominance rule for k_front_rank.  The point, the load and the minimum stay written out in the three
// kernels, and the dominance test in k_group_reduce: as inlined functions they change the kernels' code, and k_group_reduce measured up to
// 40 % slower, k_walk_accept needed a register more or lost the order of its loads (profiles/HISTORY.md).  A change of the rule is a change in
// all three.
#pragma once
#include <hip/hip_runtime.h>

struct CopyWeights { double mk, ec, tt; };
static inline CopyWeights copy_weights(const double *w3cfg_host) { return CopyWeights{w3cfg_host[0], w3cfg_host[1], w3cfg_host[2]}; }

// DOMINANCE: copy q with the record o dominates copy c iff it is nowhere worse and somewhere better, or equal throughout with q < c (a NaN mk: false)
__device__ __forceinline__ bool copy_dominates(const double4 &o, int q, double mk, double ec, double tt, int c)
{
    const bool le = o.x <= mk && o.y <= ec && o.z <= tt;
    const bool lt = o.x < mk || o.y < ec || o.z < tt;
    return le && (lt || q < c);
}
