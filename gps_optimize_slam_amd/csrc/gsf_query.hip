// gsf_query.hip -- the fused track at any stamp (gsf_pose_query_dev) and sensor points carried into its frame (gsf_georef_points_dev).
//
// M is the number of POINTS of a drive, not of poses: the kernel is a stream over q_t / x / the output rows, and the poses it interpolates
// between are a small table beside it.  Definitions: include/gsf.h ("pose queries"); traffic per query and measurements: DESIGN.md 7e.
//
// Two launches, stream-ordered, no workspace, no atomics:
//  1. query_track_state_kernel, one block per track: one pass over the track's stamps (sorted? NaN?), run_status, ext_q -> track_state[b].
//  2. query_kernel<POINTS>, flat over the queries, 256 threads.  A lane finds its track by a search in q_offsets and classifies its query
//     against the track's first and last stamp.  Then one of two routes, chosen per wave:
//     - window: all bracketed queries of the wave belong to one track and the brackets of their smallest and largest stamp lie within 64
//       consecutive poses (time-ordered sensor data: a wave of returns spans one or two poses).  The wave fetches those poses once, one pose
//       per lane, into its own 4 KB of LDS (64 stamps | 64 x 3 | 64 x 4 doubles) and every lane searches and interpolates out of LDS.
//     - general: every lane searches the track's stamps in global memory and reads its two poses from there.
//     Both call query_count_le / query_at of gsf_query_core.hpp -- one instance per address space -- on the same values.
//     The searches whose key is the same in every lane (the wave's first and last query in q_offsets, its smallest and largest stamp in the
//     track) spread their probes over the 64 lanes: ceil(log64 n) dependent loads instead of log2 n.
//  The 24- / 32-byte rows of x, out_xyz, out_pos and out_quat are read and written row by row, one lane each: on the MI355X that is as fast
//  as moving them as 16-byte pieces through the wave's LDS slice (the scheme of apply_sim3_slab_kernel; measured).
#include "gsf_internal.hpp"
#include "gsf_query_core.hpp"

namespace {

using namespace gsf;

typedef unsigned long long u64;
typedef __attribute__((address_space(3))) const double* lds_cdp;

struct QueryArgs {
    const double* ts; const double* pos; const double* quat; const int64_t* offsets; const uint8_t* pose_flags;
    const double* q_t; const int64_t* q_offsets; const double* x; const double* ext_q; const double* ext_t; const double* scale;
    const int32_t* track_state;
    double* out_a;                 // out_pos[M][3] (poses) or out_xyz[M][3] (points)
    double* out_quat;              // poses only
    uint8_t* q_flags; int32_t* q_index; uint8_t* q_pose_flags;
    int64_t B, M; double max_gap;
};

__global__ __launch_bounds__(256) void query_track_state_kernel(const double* __restrict__ ts, const int64_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ run_status, const double* __restrict__ ext_q,
                                                                int32_t* __restrict__ track_state)
{
    const int64_t b = blockIdx.x;
    if (run_status && run_status[b] != 0) {                              // (block-uniform) the track's rows are not read
        if (threadIdx.x == 0) track_state[b] = QT_SKIPPED;
        return;
    }
    const int64_t base = offsets[b], n = offsets[b + 1] - base;
    const double* __restrict__ t = ts + base;
    int bad = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double cur = t[i];
        bad |= (i == 0) ? (cur != cur) : query_stamp_breaks(t[i - 1], cur);
    }
    const int any_bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        int32_t st = (n <= 0) ? QT_EMPTY : (any_bad ? QT_UNSORTED : 0);
        if (ext_q) {
            Quat e;
            if (!quat_unit(Quat{ ext_q[b * 4], ext_q[b * 4 + 1], ext_q[b * 4 + 2], ext_q[b * 4 + 3] }, e)) st |= QT_BAD_EXTRINSIC;
        }
        track_state[b] = st;
    }
}

// query_count_le for a key that is the same in every lane, all 64 lanes active: lane l probes the (l + 1)-th of 64 evenly spaced elements.
// The array ascends, so the lanes whose probe is <= v form a prefix, and its length narrows [lo, hi) to less than one step.
template <class T, class V>
__device__ __forceinline__ int64_t wave_count_le(const T* __restrict__ a, const int64_t n, const V v, const int lane)
{
    int64_t lo = 0, hi = n;                                              // a[k] <= v for k < lo, a[k] > v for k >= hi
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t p = lo + (int64_t)(lane + 1) * step - 1;
        const int c = __popcll(__ballot(p < hi && a[p] <= v));
        lo += (int64_t)c * step;                                         // probe c - 1 is <= v; probe c, where it exists, is not
        hi = lo + step - 1 < hi ? lo + step - 1 : hi;
    }
    const int64_t p = lo + lane;
    return lo + __popcll(__ballot(p < hi && a[p] <= v));
}

// ---- 64 rows of C doubles, one lane each, of a contiguous slab of global memory that starts at g; rows <= 64 rows exist.  The idle
// lanes of the last wave store nothing and load its last row.
template <int C>
__device__ __forceinline__ void wave_rows_store(const int lane, const int rows, double* g, const double (&v)[C])
{
    if (lane < rows) {
#pragma unroll
        for (int c = 0; c < C; ++c) g[lane * C + c] = v[c];
    }
}
template <int C>
__device__ __forceinline__ void wave_rows_load(const int lane, const int rows, const double* g, double (&v)[C])
{
    const int r = lane < rows ? lane : rows - 1;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = g[r * C + c];
}

template <bool POINTS>
__global__ __launch_bounds__(256) void query_kernel(const QueryArgs a)
{
    __shared__ double lds_all[4][512];                                   // per wave: 64 stamps | 64 x 3 | 64 x 4 doubles = 4 KB
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* const slice = lds_all[wv];
    const int64_t m0 = (int64_t)blockIdx.x * 256 + wv * 64;
    if (m0 >= a.M) return;                                               // (wave-uniform; the kernel has no block-wide barrier)
    const int rows = (int)(a.M - m0 < 64 ? a.M - m0 : 64);
    const int64_t m = m0 + (lane < rows ? lane : rows - 1);              // idle lanes of the last wave repeat its last query and store nothing
    const double tau = a.q_t[m];

    double xin[3] = { 0.0, 0.0, 0.0 };
    if (POINTS) wave_rows_load<3>(lane, rows, a.x + m0 * 3, xin);

    // ---- the query's track and its class
    const int64_t b_lo = wave_count_le(a.q_offsets, a.B + 1, m0, lane) - 1, b_hi = wave_count_le(a.q_offsets, a.B + 1, m0 + rows - 1, lane) - 1;
    const int64_t b = (b_lo == b_hi) ? b_lo : query_count_le(a.q_offsets, a.B + 1, m) - 1;      // (wave-uniform) a wave inside one track
    const bool known = b >= 0 && b < a.B;                                // q_offsets that do not cover [0, M): such a query has no track
    const int64_t bc = known ? b : 0;
    const int32_t state = known ? a.track_state[bc] : -1;
    const int64_t base = a.offsets[bc], n = a.offsets[bc + 1] - base;
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    double t_first = 0.0, t_last = 0.0;
    if (state == 0) { t_first = tsb[0]; t_last = tsb[n - 1]; }           // state 0: n >= 1, stamps sorted and free of NaN
    const int cls = query_classify(state, tau, t_first, t_last);
    const bool inr = cls == 0;

    // ---- the route of this wave
    bool window = false; int64_t w0 = 0; int W = 0;
    const u64 inr_m = __ballot(inr);
    const int64_t b_first = __shfl(b, 0);
    if (inr_m != 0ull && __ballot(b != b_first) == 0ull) {
        double lo = inr ? tau : __builtin_inf(), hi = inr ? tau : -__builtin_inf();
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off)); hi = fmax(hi, __shfl_xor(hi, off)); }
        const int64_t i_lo = wave_count_le(tsb, n, lo, lane) - 1, i_hi = wave_count_le(tsb, n, hi, lane) - 1;
        const int64_t w1 = i_hi + 1 < n ? i_hi + 1 : n - 1;
        if (w1 - i_lo < 64) { window = true; w0 = i_lo; W = (int)(w1 - i_lo) + 1; }
    }

    QueryPose pose = query_nan_pose(cls);
    int64_t idx = -1;
    if (window) {
        double* wt = slice; double* wp = slice + 64; double* wq = slice + 256;
        const int64_t r = w0 + (lane < W ? lane : W - 1);
        wt[lane] = tsb[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) wp[lane * 3 + c] = posb[r * 3 + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) wq[lane * 4 + c] = quatb[r * 4 + c];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (inr) {
            const int64_t il = query_count_le((lds_cdp)wt, (int64_t)W, tau) - 1;
            pose = query_at((lds_cdp)wt, (lds_cdp)wp, (lds_cdp)wq, il, tau, a.max_gap);
            idx = w0 + il;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // the window is read before the slice stages output rows
    } else if (inr) {
        idx = query_count_le(tsb, n, tau) - 1;
        pose = query_at(tsb, posb, quatb, idx, tau, a.max_gap);
    }

    int flags = pose.flags;
    int pf = 0;
    if (a.q_pose_flags && a.pose_flags && idx >= 0) {
        pf = a.pose_flags[base + idx];
        if (!(flags & Q_EXACT)) pf |= a.pose_flags[base + idx + 1];
    }

    if (POINTS) {
        const double nan = __builtin_nan("");
        Vec3 o{ nan, nan, nan };
        if (idx >= 0 && !(flags & Q_GAP)) {
            QueryExtrinsic ext{ Quat{ 0.0, 0.0, 0.0, 1.0 }, Vec3{ 0.0, 0.0, 0.0 }, 1.0 };
            if (a.ext_q) quat_unit(Quat{ a.ext_q[bc * 4], a.ext_q[bc * 4 + 1], a.ext_q[bc * 4 + 2], a.ext_q[bc * 4 + 3] }, ext.e);
            if (a.ext_t) ext.t = Vec3{ a.ext_t[bc * 3], a.ext_t[bc * 3 + 1], a.ext_t[bc * 3 + 2] };
            if (a.scale) ext.s = a.scale[bc];
            if (!georef_point(pose, ext, Vec3{ xin[0], xin[1], xin[2] }, o)) flags |= Q_BAD_QUAT;
        }
        const double ov[3] = { o.x, o.y, o.z };
        wave_rows_store<3>(lane, rows, a.out_a + m0 * 3, ov);
    } else {
        const double pv[3] = { pose.p.x, pose.p.y, pose.p.z };
        const double qv[4] = { pose.q.x, pose.q.y, pose.q.z, pose.q.w };
        wave_rows_store<3>(lane, rows, a.out_a + m0 * 3, pv);
        wave_rows_store<4>(lane, rows, a.out_quat + m0 * 4, qv);
    }
    if (lane < rows) {
        a.q_flags[m] = (uint8_t)flags;
        if (a.q_index) a.q_index[m] = (int32_t)idx;
        if (a.q_pose_flags) a.q_pose_flags[m] = (uint8_t)pf;
    }
}

int launch_query(gsf_ctx* ctx, bool points, const double* run_ext_q, const int32_t* run_status, const QueryArgs& a, int32_t* track_state)
{
    GSF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(query_track_state_kernel, dim3((unsigned)a.B), dim3(256), 0, ctx->stream, a.ts, a.offsets, run_status, run_ext_q, track_state);
    GSF_HIP(hipGetLastError());
    const unsigned grid = (unsigned)((a.M + 255) / 256);
    if (points) hipLaunchKernelGGL(query_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(query_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace

extern "C" int gsf_pose_query_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets,
                                  const int32_t* run_status, const uint8_t* pose_flags, int64_t B, const double* q_t, const int64_t* q_offsets,
                                  int64_t M, double max_gap, double* out_pos, double* out_quat, uint8_t* q_flags, int32_t* q_index,
                                  uint8_t* q_pose_flags, int32_t* track_state)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_REQUIRE(B >= 0 && M >= 0, "negative B / M");
    if (B == 0 || M == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && offsets && q_t && q_offsets && out_pos && out_quat && q_flags && track_state, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff && (M + 255) / 256 <= (int64_t)0x7fffffff, "B / M too large for one launch");
    const QueryArgs a{ ts, pos, quat, offsets, pose_flags, q_t, q_offsets, nullptr, nullptr, nullptr, nullptr, track_state,
                       out_pos, out_quat, q_flags, q_index, q_pose_flags, B, M, max_gap };
    return launch_query(ctx, false, nullptr, run_status, a, track_state);
}

extern "C" int gsf_georef_points_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets,
                                     const int32_t* run_status, const uint8_t* pose_flags, int64_t B, const double* q_t, const int64_t* q_offsets,
                                     int64_t M, double max_gap, const double* x, const double* ext_q, const double* ext_t, const double* scale,
                                     double* out_xyz, uint8_t* q_flags, int32_t* q_index, uint8_t* q_pose_flags, int32_t* track_state)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_REQUIRE(B >= 0 && M >= 0, "negative B / M");
    if (B == 0 || M == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && offsets && q_t && q_offsets && x && out_xyz && q_flags && track_state, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff && (M + 255) / 256 <= (int64_t)0x7fffffff, "B / M too large for one launch");
    const QueryArgs a{ ts, pos, quat, offsets, pose_flags, q_t, q_offsets, x, ext_q, ext_t, scale, track_state,
                       out_xyz, nullptr, q_flags, q_index, q_pose_flags, B, M, max_gap };
    return launch_query(ctx, true, ext_q, run_status, a, track_state);
}
