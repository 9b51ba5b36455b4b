// gsf_local.hip -- local Sim3 alignment: Sim3 knots on a time grid along each track and the pose-wise blend of neighbouring knots
// (gsf_sim3_local_fit_dev / gsf_sim3_local_apply_dev; definitions in include/gsf.h, every index and flag rule in gsf_local_core.hpp).
//
//   local_track_kernel   one wave per track: are the stamps non-decreasing, K_b, track_status.
//   local_fit_kernel     one wave per (track, knot): the wave finds its window in the sorted stamps by binary search, finds the window's
//                        first usable row (the shift), accumulates the 17 shifted raw moments of the usable rows -- lane l takes rows
//                        lo + l, lo + l + 64, ... -- reduces them with the DPP sums of wave_sum() and runs the closed form on the
//                        wave-uniform totals; a second pass over the same rows (L1 / L2 hits) gives the RMS residual under the knot.
//                        No LDS, no atomics.  Slots k >= n_knots[b] of a track are NaN-filled, so every byte of the knot arrays is
//                        written by every call.
//   local_index_kernel   one lane per track: nearest valid knot to the left / right of every knot, into the kernel workspace (the
//                        apply entry takes knots from anywhere, so it builds the tables itself from the flags it is handed).
//   local_apply_kernel   one thread per pose, laid out like apply_sim3_kernel; the two knots of a pose are 2 x 104 B shared by its
//                        neighbours in the wave: plain loads.
// Compiled under -ffp-contract=on like gsf_sim3.hip: T(p) is written as apply_sim3_kernel writes it and is then the same instructions,
// which is what makes knots equal to the global transform return gsf_apply_sim3_batch_dev's bytes.
#include "gsf_wave_common.hpp"      // DPP-routed wave_sum()
#include "gsf_local_core.hpp"

using namespace gsf;

namespace {

__global__ __launch_bounds__(64) void local_track_kernel(const double* __restrict__ ts, const int64_t* __restrict__ offsets, double spacing,
                                                         int32_t Kmax, int32_t* __restrict__ n_knots, int32_t* __restrict__ track_status)
{
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t i0 = offsets[b], i1 = offsets[b + 1];
    if (i1 <= i0) { if (lane == 0) { n_knots[b] = 0; track_status[b] = LOC_EMPTY; } return; }
    bool bad = false;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const double t = ts[i];
        bad = bad || loc_stamp_bad(t, i + 1 < i1, i + 1 < i1 ? ts[i + 1] : t);
    }
    const bool unsorted = __ballot(bad) != 0ull;
    if (lane != 0) return;
    const int32_t K = loc_knot_count(ts[i0], ts[i1 - 1], spacing);
    const int32_t st = loc_track_status(i1 - i0, unsorted, K, Kmax);
    n_knots[b] = st ? 0 : K;
    track_status[b] = st;
}

struct LocalFitArgs {
    const double* ts; const double* pos; const double* gps; const uint8_t* valid; const int64_t* offsets;
    const double* R; const double* t; const double* s;
    double* knot_R; double* knot_t; double* knot_s; int32_t* knot_n; double* knot_rms; int32_t* knot_flags;
    const int32_t* n_knots;
    double spacing, half_window; LocFitRule rule; int32_t Kmax;
};

constexpr int FIT_WAVES = 4;

__global__ __launch_bounds__(64 * FIT_WAVES) void local_fit_kernel(const LocalFitArgs a)
{
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t k = (int32_t)blockIdx.y * FIT_WAVES + (threadIdx.x >> 6);
    if (k >= a.Kmax) return;
    const int64_t slot = b * (int64_t)a.Kmax + k;
    const double nan = __builtin_nan("");
    if (k >= a.n_knots[b]) {                                                // beyond the track's grid (a flagged track: every slot)
        if (lane < 9) a.knot_R[slot * 9 + lane] = nan;
        else if (lane < 12) a.knot_t[slot * 3 + (lane - 9)] = nan;
        else if (lane == 12) a.knot_s[slot] = nan;
        else if (lane == 13) a.knot_rms[slot] = nan;
        else if (lane == 14) a.knot_n[slot] = 0;
        else if (lane == 15) a.knot_flags[slot] = 0;
        return;
    }
    const int64_t i0 = a.offsets[b], i1 = a.offsets[b + 1];
    const double tau = loc_tau(a.ts[i0], a.spacing, k);
    int64_t lo, hi;
    loc_window(a.ts, i0, i1, tau, a.half_window, lo, hi);                   // wave-uniform
    // ---- the shift: the window's first usable row
    int64_t first = -1;
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t i = base + lane;
        const bool ok = i < hi && loc_usable(a.valid[i], a.gps[i * 3], a.gps[i * 3 + 1], a.gps[i * 3 + 2]);
        const u64 m = __ballot(ok);
        if (m != 0ull) { first = base + (__ffsll((long long)m) - 1); break; }
    }
    LocMoments m;
    loc_moments_zero(m);
    if (first >= 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { m.as[c] = a.pos[first * 3 + c]; m.bs[c] = a.gps[first * 3 + c]; }
        for (int64_t i = first + lane; i < hi; i += 64)                     // windows of more than 64 rows: strided
            if (loc_usable(a.valid[i], a.gps[i * 3], a.gps[i * 3 + 1], a.gps[i * 3 + 2])) loc_add_row(m, a.pos + i * 3, a.gps + i * 3);
    }
    m.n = wave_sum(m.n); m.Saa = wave_sum(m.Saa);
#pragma unroll
    for (int c = 0; c < 3; ++c) { m.Sa[c] = wave_sum(m.Sa[c]); m.Sb[c] = wave_sum(m.Sb[c]); }
#pragma unroll
    for (int c = 0; c < 9; ++c) m.Sab[c] = wave_sum(m.Sab[c]);
    // ---- the closed form, on wave-uniform inputs in every lane
    double Rg[9], Rk[9], tk[3], sk = nan;
#pragma unroll
    for (int c = 0; c < 9; ++c) { Rg[c] = a.R[b * 9 + c]; Rk[c] = nan; }
    tk[0] = tk[1] = tk[2] = nan;
    const int32_t flags = loc_knot_fit(m, a.rule, Rg, a.s[b], Rk, tk, sk);
    double rms = nan;
    if (loc_knot_valid(flags)) {                                            // RMS of T_k(p_i) - fix_i over the window's usable rows
        double e = 0.0;
        for (int64_t i = first + lane; i < hi; i += 64)
            if (loc_usable(a.valid[i], a.gps[i * 3], a.gps[i * 3 + 1], a.gps[i * 3 + 2])) {
                const Vec3 q = loc_map(Rk, tk, sk, Vec3{ a.pos[i * 3], a.pos[i * 3 + 1], a.pos[i * 3 + 2] });
                const double d0 = q.x - a.gps[i * 3], d1 = q.y - a.gps[i * 3 + 1], d2 = q.z - a.gps[i * 3 + 2];
                e += d0 * d0 + d1 * d1 + d2 * d2;
            }
        rms = sqrt(wave_sum(e) / m.n);
    } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) Rk[c] = nan;
        tk[0] = tk[1] = tk[2] = nan; sk = nan;
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) a.knot_R[slot * 9 + c] = Rk[c];
        a.knot_t[slot * 3] = tk[0]; a.knot_t[slot * 3 + 1] = tk[1]; a.knot_t[slot * 3 + 2] = tk[2];
        a.knot_s[slot] = sk; a.knot_rms[slot] = rms; a.knot_n[slot] = (int32_t)m.n; a.knot_flags[slot] = flags;
    }
}

__device__ __forceinline__ int32_t knots_of(const int32_t* n_knots, const int32_t* track_status, int64_t b, int32_t Kmax)
{
    const int32_t K = n_knots[b];
    return track_status[b] != 0 ? 0 : (K < 0 ? 0 : (K > Kmax ? Kmax : K));
}

__global__ __launch_bounds__(64) void local_index_kernel(const int32_t* __restrict__ knot_flags, const int32_t* __restrict__ n_knots,
                                                         const int32_t* __restrict__ track_status, int64_t B, int32_t Kmax,
                                                         int32_t* __restrict__ nl, int32_t* __restrict__ nr)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    loc_index_track(knot_flags + b * Kmax, knots_of(n_knots, track_status, b, Kmax), nl + b * Kmax, nr + b * Kmax);
}

struct LocalApplyArgs {
    const double* ts; const double* pos; const double* quat; const int64_t* offsets;
    const double* R; const double* t; const double* s;
    const double* knot_R; const double* knot_t; const double* knot_s;
    const int32_t* n_knots; const int32_t* track_status; const int32_t* nl; const int32_t* nr;
    double* pos_out; double* quat_out; double* scale_at; int32_t* pose_flags;
    double spacing; int32_t Kmax;
};

__global__ __launch_bounds__(256) void local_apply_kernel(const LocalApplyArgs a)
{
    const int64_t b = blockIdx.x;
    const int64_t i0 = a.offsets[b], i1 = a.offsets[b + 1];
    if (i1 <= i0) return;
    const double nan = __builtin_nan("");
    const bool flagged = a.track_status[b] != 0;
    const int32_t K = knots_of(a.n_knots, a.track_status, b, a.Kmax);
    LocKnot g;
#pragma unroll
    for (int c = 0; c < 9; ++c) g.R[c] = a.R[b * 9 + c];
    g.t[0] = a.t[b * 3]; g.t[1] = a.t[b * 3 + 1]; g.t[2] = a.t[b * 3 + 2]; g.s = a.s[b];
    const double t0 = a.ts[i0];
    const int64_t kb = b * (int64_t)a.Kmax;
    for (int64_t i = i0 + blockIdx.y * blockDim.x + threadIdx.x; i < i1; i += (int64_t)blockDim.x * gridDim.y) {
        LocPose o;
        if (flagged) {                                                     // no grid is defined: NaN rows
            o.p = Vec3{ nan, nan, nan }; o.q = Quat{ nan, nan, nan, nan }; o.scale = nan; o.flags = LP_TRACK;
        } else {
            const double t = a.ts[i];
            const int32_t k = loc_cell(t, t0, a.spacing, K);
            int32_t L, Rr;
            loc_neighbours(a.nl + kb, a.nr + kb, k, K, L, Rr);
            const int32_t kind = loc_pose_kind(L, Rr);
            const bool both = (kind & (LP_HELD | LP_GLOBAL)) == 0;
            const int64_t ka = kb + (L >= 0 ? L : (Rr >= 0 ? Rr : 0)), kc = kb + (both ? Rr : 0);   // (slot 0 of the track: loaded, not used)
            LocKnot A, Bk;
#pragma unroll
            for (int c = 0; c < 9; ++c) { A.R[c] = a.knot_R[ka * 9 + c]; Bk.R[c] = a.knot_R[kc * 9 + c]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) { A.t[c] = a.knot_t[ka * 3 + c]; Bk.t[c] = a.knot_t[kc * 3 + c]; }
            A.s = a.knot_s[ka]; Bk.s = a.knot_s[kc];
            if (kind & LP_GLOBAL) A = g;
            const double w = both ? loc_weight(t, t0, a.spacing, L, Rr) : 0.0;
            o = loc_blend(Vec3{ a.pos[i * 3], a.pos[i * 3 + 1], a.pos[i * 3 + 2] },
                          Quat{ a.quat[i * 4], a.quat[i * 4 + 1], a.quat[i * 4 + 2], a.quat[i * 4 + 3] }, w, kind, A, Bk);
        }
        a.pos_out[i * 3] = o.p.x; a.pos_out[i * 3 + 1] = o.p.y; a.pos_out[i * 3 + 2] = o.p.z;
        a.quat_out[i * 4] = o.q.x; a.quat_out[i * 4 + 1] = o.q.y; a.quat_out[i * 4 + 2] = o.q.z; a.quat_out[i * 4 + 3] = o.q.w;
        a.scale_at[i] = o.scale;
        a.pose_flags[i] = o.flags;
    }
}

}  // namespace

namespace gsf {

int launch_local_fit(gsf_ctx* ctx, const double* ts, const double* pos, const double* gps, const uint8_t* valid, const int64_t* offsets,
                     int64_t B, const double* R, const double* t, const double* s, const gsf_local_config* cfg, int32_t Kmax, double* knot_R,
                     double* knot_t, double* knot_s, int32_t* knot_n, double* knot_rms, int32_t* knot_flags, int32_t* n_knots,
                     int32_t* track_status)
{
    GSF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(local_track_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, ts, offsets, cfg->spacing, Kmax, n_knots, track_status);
    GSF_HIP(hipGetLastError());
    const LocalFitArgs a{ ts, pos, gps, valid, offsets, R, t, s, knot_R, knot_t, knot_s, knot_n, knot_rms, knot_flags, n_knots,
                          cfg->spacing, cfg->half_window, LocFitRule{ cfg->mode, cfg->min_rows, cfg->rot_open, cfg->ratio_max }, Kmax };
    hipLaunchKernelGGL(local_fit_kernel, dim3((unsigned)B, (unsigned)((Kmax + FIT_WAVES - 1) / FIT_WAVES)), dim3(64 * FIT_WAVES), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

int launch_local_apply(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets, int64_t B, const double* R,
                       const double* t, const double* s, double spacing, int32_t Kmax, const double* knot_R, const double* knot_t,
                       const double* knot_s, const int32_t* knot_flags, const int32_t* n_knots, const int32_t* track_status, double* pos_out,
                       double* quat_out, double* scale_at, int32_t* pose_flags)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const size_t table = (size_t)B * (size_t)Kmax;
    const int rc = ensure_workspace(ctx, GSF_WS_KERNEL, 2 * table * sizeof(int32_t));     // nl | nr, one word per (track, knot) each
    if (rc != GSF_OK) return rc;
    int32_t* nl = workspace<int32_t>(ctx, GSF_WS_KERNEL);
    int32_t* nr = nl + table;
    hipLaunchKernelGGL(local_index_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, knot_flags, n_knots, track_status, B, Kmax, nl, nr);
    GSF_HIP(hipGetLastError());
    const LocalApplyArgs a{ ts, pos, quat, offsets, R, t, s, knot_R, knot_t, knot_s, n_knots, track_status, nl, nr,
                            pos_out, quat_out, scale_at, pose_flags, spacing, Kmax };
    const unsigned gy = B >= 2048 ? 1u : (B >= 256 ? 4u : 64u);               // few tracks: several blocks per track (launch_apply_sim3's rule)
    hipLaunchKernelGGL(local_apply_kernel, dim3((unsigned)B, gy), dim3(256), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace gsf
