// gsf_lever.hip -- antenna lever arm: the joint Gauss-Newton fit of (s, t, l, rotation increment) per track and the pose-wise move of a
// fix between antenna and camera (gsf_lever_fit_dev / gsf_lever_apply_dev; definitions in include/gsf.h, every rule in gsf_lever_core.hpp).
//
//   lever_fit_kernel     one wave per track, LEVER_WAVES waves to a block.  The wave classifies its rows once (first usable row, counts: ballots),
//                        then runs lev_fit_track(): per round one pass over the rows -- lane k takes rows first + k, first + k + 64, ... --
//                        accumulates the 49 distinct sums behind N and g in registers, reduces them with the DPP sums of wave_sum(), and
//                        every lane runs the 10 x 10 scaled Cholesky on the wave-uniform totals with compile-time indices.  A last pass
//                        gives rms_after.  No LDS, no atomics; the rows of later rounds come from L2.  Lane 0 writes every output byte.
//   lever_apply_kernel   one thread per pose, laid out like apply_sim3_kernel: out = gps + sign R (M(q) l).
// Compiled under -ffp-contract=on like gsf_local.hip: which operations fuse is a property of the source, so a track alone and the same
// track inside a batch are the same instructions on the same numbers.
#include "gsf_wave_common.hpp"      // DPP-routed wave_sum()
#include "gsf_lever_core.hpp"

using namespace gsf;

namespace {

struct LeverFitArgs {
    const double* pos; const double* quat; const double* gps; const uint8_t* valid; const int64_t* offsets;
    const double* R; const double* t; const double* s; const double* l0; const int32_t* run_status;
    double* R_out; double* t_out; double* s_out; double* l_out; double* l_cov; int32_t* n_rows; int32_t* n_bad_quat;
    double* rms_before; double* rms_after; double* last_step; int32_t* flags;
    LevRule rule; int64_t B;
};

struct WavePass {
    const LeverFitArgs& a; int64_t i0, i1, first; int lane;
    __device__ __forceinline__ int kind(int64_t i, Quat& qn) const { return lev_row_kind(a.valid[i], a.pos + i * 3, a.quat + i * 4, a.gps + i * 3, qn); }
    __device__ __forceinline__ void scan(int64_t& first_out, int32_t& n, int32_t& n_bad)
    {
        first = -1; n = 0; n_bad = 0;
        for (int64_t base = i0; base < i1; base += 64) {
            const int64_t i = base + lane;
            Quat qn;
            const int k = i < i1 ? kind(i, qn) : 2;
            const u64 m = __ballot(k == 0);
            if (first < 0 && m != 0ull) first = base + (__ffsll((long long)m) - 1);
            n += __popcll(m); n_bad += __popcll(__ballot(k == 1));
        }
        first_out = first;
    }
    __device__ __forceinline__ void shift(double* pf, double* gf) const
    {
#pragma unroll
        for (int c = 0; c < 3; ++c) { pf[c] = a.pos[first * 3 + c]; gf[c] = a.gps[first * 3 + c]; }
    }
    __device__ __forceinline__ void sums(const LevState& x, const double* pf, const double* gf, LevSums& S) const
    {
        lev_sums_zero(S);
        for (int64_t i = first + lane; i < i1; i += 64) {
            Quat qn;
            if (kind(i, qn) == 0) lev_add_row(S, x, pf, gf, a.pos + i * 3, a.gps + i * 3, qn);
        }
#pragma unroll
        for (int k = 0; k < LEV_NSUM; ++k) S.a[k] = wave_sum(S.a[k]);
    }
};

constexpr int LEVER_WAVES = 4;

__global__ __launch_bounds__(64 * LEVER_WAVES) void lever_fit_kernel(const LeverFitArgs a)
{
    const int64_t b = (int64_t)blockIdx.x * LEVER_WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;                                                   // (wave-uniform)
    const int lane = threadIdx.x & 63;
    WavePass pass{ a, a.offsets[b], a.offsets[b + 1], -1, lane };
    double R0[9], t0[3], l0[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) R0[c] = a.R[b * 9 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) { t0[c] = a.t[b * 3 + c]; l0[c] = a.l0[b * 3 + c]; }
    LevOut o;
    lev_fit_track(pass, a.rule, R0, t0, a.s[b], l0, a.run_status ? a.run_status[b] : 0, o);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) { a.R_out[b * 9 + c] = o.R[c]; a.l_cov[b * 9 + c] = o.lcov[c]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) { a.t_out[b * 3 + c] = o.t[c]; a.l_out[b * 3 + c] = o.l[c]; }
        a.s_out[b] = o.s; a.n_rows[b] = o.n_rows; a.n_bad_quat[b] = o.n_bad_quat;
        a.rms_before[b] = o.rms_before; a.rms_after[b] = o.rms_after; a.last_step[b] = o.last_step; a.flags[b] = o.flags;
    }
}

__global__ __launch_bounds__(256) void lever_apply_kernel(const double* __restrict__ quat, const double* __restrict__ xyz,
                                                          const int64_t* __restrict__ offsets, const double* __restrict__ R,
                                                          const double* __restrict__ l, double sign, double* __restrict__ xyz_out,
                                                          int32_t* __restrict__ pose_flags)
{
    const int64_t b = blockIdx.x;
    const int64_t i0 = offsets[b], i1 = offsets[b + 1];
    if (i1 <= i0) return;
    double Rb[9], lb[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Rb[c] = R[b * 9 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) lb[c] = l[b * 3 + c];
    for (int64_t i = i0 + blockIdx.y * blockDim.x + threadIdx.x; i < i1; i += (int64_t)blockDim.x * gridDim.y) {
        const double q[4] = { quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3] };
        const double g[3] = { xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2] };
        double o[3];
        const int32_t f = lev_apply_row(Rb, lb, sign, q, g, o);
        xyz_out[i * 3] = o[0]; xyz_out[i * 3 + 1] = o[1]; xyz_out[i * 3 + 2] = o[2];
        pose_flags[i] = f;
    }
}

}  // namespace

namespace gsf {

int launch_lever_fit(gsf_ctx* ctx, const double* pos, const double* quat, const double* gps, const uint8_t* valid, const int64_t* offsets, int64_t B,
                     const double* R, const double* t, const double* s, const double* l0, const int32_t* run_status, const gsf_lever_config* cfg,
                     double* R_out, double* t_out, double* s_out, double* l_out, double* l_cov, int32_t* n_rows, int32_t* n_bad_quat,
                     double* rms_before, double* rms_after, double* last_step, int32_t* flags)
{
    GSF_HIP(hipSetDevice(ctx->device));
    LevRule rule;
    rule.sigma_fix = cfg->sigma_fix; rule.sigma_rot = cfg->sigma_rot; rule.ratio_max = cfg->ratio_max; rule.pivot_min = cfg->pivot_min;
    rule.weak_ratio = cfg->weak_ratio; rule.conv_tol = cfg->conv_tol;
    for (int c = 0; c < 3; ++c) rule.sigma_prior[c] = cfg->sigma_prior[c];
    rule.min_rows = cfg->min_rows; rule.iters = cfg->iters; rule.fit_scale = cfg->fit_scale; rule.fit_rotation = cfg->fit_rotation;
    const LeverFitArgs a{ pos, quat, gps, valid, offsets, R, t, s, l0, run_status, R_out, t_out, s_out, l_out, l_cov, n_rows, n_bad_quat,
                          rms_before, rms_after, last_step, flags, rule, B };
    hipLaunchKernelGGL(lever_fit_kernel, dim3((unsigned)((B + LEVER_WAVES - 1) / LEVER_WAVES)), dim3(64 * LEVER_WAVES), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

int launch_lever_apply(gsf_ctx* ctx, const double* quat, const double* xyz, const int64_t* offsets, int64_t B, const double* R, const double* l,
                       double sign, double* xyz_out, int32_t* pose_flags)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const unsigned gy = B >= 2048 ? 1u : (B >= 256 ? 4u : 64u);               // few tracks: several blocks per track (launch_apply_sim3's rule)
    hipLaunchKernelGGL(lever_apply_kernel, dim3((unsigned)B, gy), dim3(256), 0, ctx->stream, quat, xyz, offsets, R, l, sign, xyz_out, pose_flags);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace gsf
