// gsf_stream.hip -- streaming fusion (include/gsf.h, "streaming fusion"): open a stream, append poses to live tracks, gather ring rows.
//
// Mapping: ONE LANE PER TRACK.  An append is B short sequential chains (1 to ~100 poses each), not one long chain per track: the
// wave-per-track kernels' scans pay off over 64-pose chunks and would idle here, while 64 different outage histories per wave is what
// EkfTraj::step was written for (branch-free per-pose body, everything around an outage behind one wave vote).  The state is field-major
// (gsf_stream_core.hpp), so a wave loads and stores each of its 28 fields as one contiguous row; the segment runs from registers; the rows of a
// segment go to the ring and to the call's outputs.  The per-track body is stream_append_track() of gsf_stream_core.hpp, the code the CPU tier
// compiles with g++.
#include "gsf_internal.hpp"
#include "gsf_stream_core.hpp"

using namespace gsf;

namespace {

__global__ __launch_bounds__(64) void stream_open_kernel(int64_t B, int64_t cap, const double* __restrict__ init_pos, const double* __restrict__ init_quat,
                                                         const uint8_t* __restrict__ track_mask, double* __restrict__ sf, int64_t* __restrict__ si)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (track_mask && track_mask[b] == 0) return;
    stream_open_track(sf, si, B, b, cap, init_pos, init_quat);
}

__global__ __launch_bounds__(64) void stream_append_kernel(EkfConfig cfg, int64_t B, int64_t cap, double* __restrict__ sf, int64_t* __restrict__ si,
                                                           double* __restrict__ ring_t, double* __restrict__ ring_pos, double* __restrict__ ring_quat,
                                                           StreamSeg g, const int64_t* __restrict__ seg_offsets, int64_t* __restrict__ n_total,
                                                           int64_t* __restrict__ n_final, int64_t* __restrict__ revised_from, int32_t* __restrict__ status)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t lo = seg_offsets[b], m = seg_offsets[b + 1] - lo;
    const StreamReport r = stream_append_track(cfg, sf, si, B, b, cap, ring_t, ring_pos, ring_quat, g, lo, m);
    if (n_total) n_total[b] = r.n_total;
    if (n_final) n_final[b] = r.n_final;
    if (revised_from) revised_from[b] = r.revised_from;
    if (status) status[b] = r.status;
}

// a plain copy: block b moves track b's rows lo[b] .. of the ring into rows out_offsets[b] .. of the ragged outputs
__global__ __launch_bounds__(64) void stream_gather_kernel(int64_t B, int64_t cap, const int64_t* __restrict__ si, const double* __restrict__ ring_t,
                                                           const double* __restrict__ ring_pos, const double* __restrict__ ring_quat,
                                                           const int64_t* __restrict__ lo, const int64_t* __restrict__ out_offsets,
                                                           double* __restrict__ ts_out, double* __restrict__ pos_out, double* __restrict__ quat_out)
{
    const int64_t b = blockIdx.x;
    const int64_t o = out_offsets[b], cnt = out_offsets[b + 1] - o, first = lo[b];
    const bool ok = si[SI_VERSION * B + b] == STREAM_LAYOUT_VERSION && si[SI_CAP * B + b] == cap;
    const int64_t n = ok ? si[SI_NTOTAL * B + b] : 0;                    // (a state of another layout holds no rows)
    for (int64_t r = threadIdx.x; r < cnt; r += blockDim.x) {
        double t; Vec3 p; Quat q;
        stream_gather_row(ring_t + b * cap, ring_pos + b * cap * 3, ring_quat + b * cap * 4, cap, n, first + r, t, p, q);
        const int64_t w = o + r;
        if (ts_out) ts_out[w] = t;
        if (pos_out) { pos_out[w * 3] = p.x; pos_out[w * 3 + 1] = p.y; pos_out[w * 3 + 2] = p.z; }
        if (quat_out) { quat_out[w * 4] = q.x; quat_out[w * 4 + 1] = q.y; quat_out[w * 4 + 2] = q.z; quat_out[w * 4 + 3] = q.w; }
    }
}

}  // namespace

extern "C" int gsf_stream_open_dev(gsf_ctx* ctx, int64_t B, int64_t cap, const double* init_pos, const double* init_quat, const uint8_t* track_mask,
                                   double* state_f64, int64_t* state_i64)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_REQUIRE(B >= 0 && cap >= 1, "negative B or cap < 1");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(init_pos && init_quat && state_f64 && state_i64, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff * 64 && cap <= ((int64_t)1 << 40), "B or cap too large");
    GSF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stream_open_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, B, cap, init_pos, init_quat, track_mask, state_f64,
                       state_i64);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

extern "C" int gsf_stream_append_dev(gsf_ctx* ctx, const gsf_ekf_config* cfg, int64_t B, int64_t cap, double* state_f64, int64_t* state_i64,
                                     double* ring_t, double* ring_pos, double* ring_quat, const double* ts, const double* pos, const double* quat,
                                     const double* gps, const uint8_t* valid, const int64_t* seg_offsets, double* pos_out, double* quat_out,
                                     double* cov_out, int64_t* n_total, int64_t* n_final, int64_t* revised_from, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg, "ctx/cfg is NULL");
    GSF_REQUIRE(B >= 0 && cap >= 1, "negative B or cap < 1");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(state_f64 && state_i64 && ring_t && ring_pos && ring_quat && seg_offsets, "NULL state, ring or seg_offsets");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff * 64 && cap <= ((int64_t)1 << 40), "B or cap too large");
    for (int i = 0; i < 7; ++i) GSF_REQUIRE(cfg->initial_cov_diag[i] == cfg->initial_cov_diag[i], "NaN in config");
    GSF_HIP(hipSetDevice(ctx->device));
    const StreamSeg g{ ts, pos, quat, gps, valid, pos_out, quat_out, cov_out };   // (the segment arrays are read only by tracks with rows)
    hipLaunchKernelGGL(stream_append_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, to_core(cfg), B, cap, state_f64, state_i64, ring_t,
                       ring_pos, ring_quat, g, seg_offsets, n_total, n_final, revised_from, status);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

extern "C" int gsf_stream_gather_dev(gsf_ctx* ctx, int64_t B, int64_t cap, const int64_t* state_i64, const double* ring_t, const double* ring_pos,
                                     const double* ring_quat, const int64_t* lo, const int64_t* out_offsets, double* ts_out, double* pos_out,
                                     double* quat_out)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_REQUIRE(B >= 0 && cap >= 1, "negative B or cap < 1");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(state_i64 && ring_t && ring_pos && ring_quat && lo && out_offsets, "NULL array");
    GSF_REQUIRE(B <= 0x7fffffff && cap <= ((int64_t)1 << 40), "B or cap too large");
    GSF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, B, cap, state_i64, ring_t, ring_pos, ring_quat, lo, out_offsets,
                       ts_out, pos_out, quat_out);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}
