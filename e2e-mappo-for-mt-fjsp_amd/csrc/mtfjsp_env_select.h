// mtfjsp_env_select.h — which of the seven environment step kernels serves a handle, stated ONCE (mtfjsp_step launches from this plan,
// mtfjsp_step_params decides by it, mtfjsp_step_kernel_name[_for] report it), with the host size arithmetic the rule needs.  Plain C++17,
// no HIP header: a host-only program can include it.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#ifdef __HIP__
#define ENV_HD __host__ __device__
#else
#define ENV_HD
#endif

#define WAVE 64
#define SCAL_N 28          // doubles of per-instance scalar state (slots: mtfjsp_env_dev.h)
// Instances (= waves) per workgroup of the grouped register kernels (mtfjsp_env_grp.h); the scalar part uses 4 lanes per instance.  Two
// builds (measured, tools/env_variants.py): 16 instances and 4 waves per SIMD (no spills) while all waves of the batch are resident at
// once (<= EG_SMALL_MAX_B instances: 14.4 us at 4096 against 16.1 us for k_env_reg); 4 instances and 8 waves per SIMD for chip-filling
// batches, where occupancy and short barrier waits matter more than the amortisation (262 144 instances: 335 us = 0.78 of the copy rate
// against 442 us = 0.59).  The two-slot kernels hold twice the state per wave: half the batch.
#define EG_SMALL 16
#define EG_LARGE 4
#define EG_SMALL_MAX_B 8192
#define ENV_LDS_GMAX 8                         // instances (= waves) per workgroup of k_env_step_grp at most

enum EnvKernel { ENV_K_GRP16X2 = 0, ENV_K_GRP4X2, ENV_K_GRP16, ENV_K_GRP4, ENV_K_REG, ENV_K_STEP_GRP, ENV_K_STEP, ENV_K_COUNT };   // grouped register kernels first
static const char *const ENV_KERNEL_NAME[ENV_K_COUNT] = {"k_env_grp16x2", "k_env_grp4x2", "k_env_grp16", "k_env_grp4", "k_env_reg", "k_env_step_grp", "k_env_step"};

// one task slot per lane: the shapes of k_env_reg, k_env_grp16 / k_env_grp4 and of the step as the tail of a heads launch
static inline bool env_one_slot(int J, int M, int T) { return T <= 64 && M * M <= 64 && J <= 64; }

static inline size_t env_step_lds_bytes(int J, int M, int T, bool f32)                  // k_env_step: one instance per workgroup
{
    const int Tp = (T + 7) & ~7;
    size_t off = (size_t)(4 * T + Tp + M * M + 3 * M + 2 * J + SCAL_N + 8) * sizeof(double);
    off = (off + 15) & ~(size_t)15;
    off += (size_t)M * 12 * (f32 ? 4 : 8);
    off = (off + 15) & ~(size_t)15;
    off += (size_t)(3 * T + J + 4 * M + 1 + 4) * sizeof(int);
    return off;
}

struct EnvStepLds {                            // k_env_step_grp: layout of one instance's LDS region
    int T, Tp, M, J, nleaf;
    // f64 part, offsets in doubles: start | finish | processing energy per task, idle terms in rank order, column m of the transport
    // times, the acting job's min durations / estimated starts / finishes, per-job maxima, scalars, the acting machine's feature
    // row, leaf sums of the pairwise energy sum.  (Round 3: 18.0 KB per J20M20 instance instead of 26.7 — durations and the other
    // transport columns are read from memory by the few lanes that need one, route links are 16-bit — so that 8 instances fit a CU
    // and 2048 of them run in ONE round of workgroups: 2 x 29 us of dependent chain -> 1 x.)
    int d_ft, d_pte, d_term, d_ttc, d_mind, d_jste, d_jfte, d_jmax, d_jrow, d_sc, d_mfr, d_leaf, d_end;
    size_t o_stage, o_link, o_int, o_un, o_in, bytes;          // bytes from the region's start
    ENV_HD EnvStepLds(int J_, int M_, int T_, bool f32, int nleaf_) : T(T_), Tp((T_ + 7) & ~7), M(M_), J(J_), nleaf(nleaf_)
    {
        d_ft = T; d_pte = 2 * T; d_term = 3 * T; d_ttc = d_term + Tp; d_mind = d_ttc + M; d_jste = d_mind + M; d_jfte = d_jste + M;
        d_jmax = d_jfte + M; d_jrow = d_jmax + J; d_sc = d_jrow + J; d_mfr = d_sc + SCAL_N; d_leaf = d_mfr + 8; d_end = d_leaf + nleaf;
        size_t off = (size_t)d_end * sizeof(double);
        off = (off + 15) & ~(size_t)15;
        o_stage = off; off += (size_t)M * 12 * (f32 ? 4 : 8);
        off = (off + 15) & ~(size_t)15;
        o_link = off; off += (size_t)3 * T * sizeof(short);     // machine | route predecessor | rank per task
        off = (off + 15) & ~(size_t)15;
        o_int = off; off += (size_t)(J + 4 * M + 1 + 4) * sizeof(int);
        off = (off + 15) & ~(size_t)15;
        o_un = off; off += 16 * sizeof(double);
        o_in = off; off += 8 * sizeof(int);
        bytes = (off + 15) & ~(size_t)15;
    }
};
// numpy's pairwise recursion (n > 128: halves, the left one rounded down to a multiple of 8) as a table the step kernel walks:
// [2l], [2l+1] = offset, length of leaf l (in order); then nleaf - 1 merges (i, j): leaf-sum slot i += slot j, in post-order, so
// that the total ends in slot 0.  Depends on T only; built once per handle.
static inline int pw_table(int off, int n, int depth, std::vector<short> &leaves, std::vector<short> &merges)
{
    if (n <= 128 || depth == 0) { const int idx = (int)leaves.size() / 2; leaves.push_back((short)off); leaves.push_back((short)n); return idx; }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const int l = pw_table(off, n2, depth - 1, leaves, merges), r = pw_table(off + n2, n - n2, depth - 1, leaves, merges);
    merges.push_back((short)l); merges.push_back((short)r);
    return l;
}
static inline int pw_nleaf(int T) { std::vector<short> l, m; pw_table(0, T, 6, l, m); return (int)l.size() / 2; }   // (a handle keeps its count)

struct EnvStepPlan {
    EnvKernel kernel;
    int G, grid, block;                        // G: instances per workgroup
    size_t lds, lds_inst;                      // dynamic LDS bytes of the launch | one instance's region of k_env_step_grp (0 on the register path)
    bool overridden;                           // a diagnostic switch is set (whether or not it changed the choice)
};
// The rule.  force / force_lds_env / step_g: the values of MTFJSP_ENV_KERNEL (lds | lds1 | reg1 | grp16 | grp4), MTFJSP_ENV_LDS and
// MTFJSP_ENV_STEP_G, or nullptr — read by the caller, per call.  lds_max: LDS a workgroup may use on the handle's device;
// grp_lds_ok: that device lets k_env_step_grp have it; nleaf: pw_nleaf(J * M).
static inline EnvStepPlan env_step_plan(int J, int M, int B, bool f32, size_t lds_max, bool grp_lds_ok, int nleaf, const char *force,
                                        const char *force_lds_env, const char *step_g)
{
    const int T = J * M;
    const auto is = [force](const char *s) { return force && !strcmp(force, s); };
    const bool force_lds = force_lds_env || is("lds") || is("lds1"), force_reg1 = is("reg1");
    const bool reg_ok = env_one_slot(J, M, T) && !force_lds;
    const bool reg2_ok = !reg_ok && T <= 128 && M * M <= 128 && M <= 16 && J <= 64 && !force_lds && !force_reg1;   // two task slots per lane
    EnvStepPlan pl{ENV_K_REG, 1, B, WAVE, 0, 0, force || force_lds_env || step_g};
    if (reg2_ok || (reg_ok && !force_reg1)) {                             // register kernels, groups of instances per workgroup
        const bool small = is("grp16") ? true : is("grp4") ? false : B <= (reg2_ok ? EG_SMALL_MAX_B / 2 : EG_SMALL_MAX_B);
        pl.kernel = reg2_ok ? (small ? ENV_K_GRP16X2 : ENV_K_GRP4X2) : (small ? ENV_K_GRP16 : ENV_K_GRP4);
        pl.G = small ? EG_SMALL : EG_LARGE;
    } else if (!reg_ok) {
        // LDS kernel: groups of G instances per workgroup where at least two regions fit (MTFJSP_ENV_STEP_G overrides; 1 = k_env_step)
        pl.lds_inst = EnvStepLds(J, M, T, f32, nleaf).bytes;
        const int gmax = !grp_lds_ok ? 1 : lds_max < 512 ? 0 : (int)((lds_max - 512) / pl.lds_inst);
        int G = gmax >= 8 ? 8 : gmax >= 4 ? 4 : gmax >= 2 ? 2 : 1;
        if (step_g) { G = atoi(step_g); G = G < 1 ? 1 : G > ENV_LDS_GMAX ? ENV_LDS_GMAX : G; G = G > gmax ? (gmax < 1 ? 1 : gmax) : G; }
        if (is("lds1")) G = 1;
        pl.kernel = G > 1 ? ENV_K_STEP_GRP : ENV_K_STEP; pl.G = G;
        pl.lds = G > 1 ? (size_t)G * pl.lds_inst : env_step_lds_bytes(J, M, T, f32);
    }                                                                     // else: k_env_reg, one instance per workgroup (the A/B reference of the grouped form)
    pl.grid = (B + pl.G - 1) / pl.G; pl.block = pl.G * WAVE;
    return pl;
}
