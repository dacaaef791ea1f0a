// mtfjsp_wave_select.h — the wave-wide selections of the library, once: the step kernels' reductions (mtfjsp_env.hip) and the "first
// index of the extremum" of the search baselines (mtfjsp_pdr.hip, mtfjsp_lookahead.hip, mtfjsp_beam.hip, mtfjsp_group.hip).  Values
// are compared and never computed with, and a reported value is read back from the lane that was picked — fmax / fmin return one of
// their operands, but of -0.0 and +0.0, which are equal, not necessarily the picked one's — so every selection equals a host model's bit
// for bit, ties, NaNs and signed zeros included.
#pragma once
#include <math.h>
#include "mtfjsp_env_dev.h"

// Reductions on the cross-lane data path (DPP: no LDS round trip per step): after four row shifts lane 15 of every row of 16 holds
// its row's result, row_bcast:15 / :31 carry it on; the wave's result is in LANE 63 only.  Lanes without a source keep their own
// value (max / min are idempotent).  All 64 lanes must be active.
template <int CTRL> __device__ __forceinline__ int dpp_keep(int x) { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, false); }
template <bool MAX, int CTRL> __device__ __forceinline__ double wave_ext_step(double x)
{
    const int lo = dpp_keep<CTRL>(__double2loint(x)), hi = dpp_keep<CTRL>(__double2hiint(x));
    return MAX ? fmax(x, __hiloint2double(hi, lo)) : fmin(x, __hiloint2double(hi, lo));
}
template <int CTRL> __device__ __forceinline__ int wave_min_step(int x)
{
    const int y = dpp_keep<CTRL>(x);
    return y < x ? y : x;
}
template <bool MAX> __device__ __forceinline__ double wave_ext_lane63(double x)
{
    x = wave_ext_step<MAX, 0x111>(x); x = wave_ext_step<MAX, 0x112>(x); x = wave_ext_step<MAX, 0x114>(x); x = wave_ext_step<MAX, 0x118>(x);
    x = wave_ext_step<MAX, 0x142>(x); x = wave_ext_step<MAX, 0x143>(x);
    return x;
}
__device__ __forceinline__ int wave_min_lane63(int x)
{
    x = wave_min_step<0x111>(x); x = wave_min_step<0x112>(x); x = wave_min_step<0x114>(x); x = wave_min_step<0x118>(x);
    x = wave_min_step<0x142>(x); x = wave_min_step<0x143>(x);
    return x;
}
// the same, read back to every lane
template <bool MAX> __device__ __forceinline__ double wave_ext(double x) { return rl_d(wave_ext_lane63<MAX>(x), 63); }
__device__ __forceinline__ int wave_min(int x) { return rl_i(wave_min_lane63(x), 63); }

// inclusive prefix sum over the wave's lanes (zero fill; row_bcast adds the previous rows' totals)
__device__ __forceinline__ int wave_scan_incl(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);      // rows 1, 3 += lane 15 of the row before
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);      // rows 2, 3 += lane 31
    return x;
}

// The first index of the extremum over any number of candidates, 64 at a time in ascending index.  One pass: lane l offers
// candidate first + l with value x if ok (a lane that is not ok contributes -/+inf and is never picked: neither is a NaN, which
// equals nothing); the pass's winner is its lowest lane that holds the wave extremum, and it replaces what is held only with a
// strictly better value — so the lowest index of the extremum is kept.  v is the picked candidate's own x, not the wave extremum e (which
// equals it, but may be the other zero).  i < 0: nothing picked yet (v is then meaningless).  Every lane holds the same (v, i).
template <bool MAX>
struct WaveBest {
    double v = 0.0;
    int i = -1;
    __device__ __forceinline__ bool better(double a, double b) const { return MAX ? a > b : a < b; }
    __device__ __forceinline__ void pass(bool ok, double x, int first)
    {
        const double e = wave_ext<MAX>(ok ? x : (MAX ? -INFINITY : INFINITY));
        const unsigned long long eq = __ballot(ok && x == e);
        if (eq && (i < 0 || better(e, v))) {
            const int l = __ffsll((long long)eq) - 1;
            v = rl_d(x, l); i = first + l;
        }
    }
    // one wave's result into a combination of several: (strictly better value, else equal value and lower index); a wave that
    // picked nothing (j < 0) is skipped.  Whatever the number of waves and their order, the lowest index of the extremum, with the value
    // that came with that index.
    __device__ __forceinline__ void merge(double x, int j)
    {
        if (j >= 0 && (i < 0 || better(x, v) || (x == v && j < i))) { v = x; i = j; }
    }
};
// the combination of NW waves' partial results (value, index), e.g. as lane 0 of each wave left them in LDS
template <bool MAX, int NW>
__device__ __forceinline__ WaveBest<MAX> wave_best_combine(const double *part_v, const int *part_i)
{
    WaveBest<MAX> g;
#pragma unroll
    for (int q = 0; q < NW; q++) g.merge(part_v[q], part_i[q]);
    return g;
}
