// mtfjsp_plan_dev.h — what the kernels on plans share (mtfjsp_plan.hip: neighbourhood moves, critical path; mtfjsp_evolve.hip: offspring
// of a population): the workgroup shape, the LDS budget of a tile of plans, the move stream's tag and kinds, and the wave-level helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtfjsp_env_dev.h"

#define PLAN_WAVES 4
#define PLAN_THREADS (PLAN_WAVES * WAVE)
#define PLAN_LDS_SOFT (64 * 1024)      // the tile shrinks (64 -> 32 -> 16 copies) to stay below this: two workgroups per CU
#define PLAN_LDS_HARD (160 * 1024)     // what a workgroup can have at all: the smallest tile may use it
#define PLAN_TAG_MOVE 0x6d6f7665u      // "move"
#define PLAN_SWAP 1
#define PLAN_INSERT 2
#define PLAN_REASSIGN 4

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

static inline bool plan_overlap(const void *a, unsigned __int128 na, const void *b, unsigned __int128 nb)
{
    if (!a || !b) return false;
    const unsigned __int128 x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
