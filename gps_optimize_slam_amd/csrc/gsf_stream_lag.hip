// gsf_stream_lag.hip -- fixed-lag RTS smoothing of a stream (include/gsf.h, gsf_stream_append_lag_dev): two launches on the context's stream.
//
// FORWARD: gsf_stream.hip's mapping and body -- one lane per track, stream_append_track() -- under the parking policy LagPark
// (gsf_stream_lag_core.hpp), which also stores each pose's forward quantities into ring_lag.  It leaves every track's plan for the second
// launch, { n_total before the call, poses taken (-1: refused or bad state) }, in the context's GSF_WS_STREAM workspace: the state no
// longer tells a refused track from one that took its segment.
// BACK-PASS: one wave per track, lane = row, rows [max(0, n0 - lag), n0 + m) in chunks of 64.  A chunk's lanes walk rows c0 .. c0 + 63 + lag,
// and a walk is one dependent chain per step, so what a step reads must not be a global load: the chunk first STAGES what the walks need
// of those <= 64 + lag rows in LDS -- per row the three gains A (formed once per row instead of once per lane and step: the division leaves
// the walk), g, u and the tag bits, field-major so that neighbouring lanes read neighbouring doubles (9 x 576 x 8 B + 576 B = 42 048 B) -- and
// every lane then runs lag_smooth_row() on its own row out of LDS.  A row's value is lag_smooth_row's, a function of the parked rows and
// (i, we) in one fixed order: independent of how the track was cut into calls, and of which chunk or lane computed it.
#include "gsf_internal.hpp"
#include "gsf_stream_lag_core.hpp"

using namespace gsf;

namespace {

constexpr int LAG_ROWS = 64 + STREAM_LAG_MAX;                             // rows a chunk stages at most

__global__ __launch_bounds__(64) void stream_append_lag_kernel(EkfConfig cfg, int64_t B, int64_t cap, int64_t lag, double* __restrict__ sf,
                                                               int64_t* __restrict__ si, double* __restrict__ ring_t, double* __restrict__ ring_pos,
                                                               double* __restrict__ ring_quat, double* __restrict__ ring_lag, StreamSeg g,
                                                               const int64_t* __restrict__ seg_offsets, int64_t* __restrict__ n_total,
                                                               int64_t* __restrict__ n_final, int64_t* __restrict__ revised_from,
                                                               int32_t* __restrict__ status, int64_t* __restrict__ plan)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t lo = seg_offsets[b], m = seg_offsets[b + 1] - lo;
    const LagPark park{ ring_lag + b * cap * STREAM_LAG_F64, lag };
    const StreamReport r = stream_append_track(cfg, sf, si, B, b, cap, ring_t, ring_pos, ring_quat, g, lo, m, park);
    if (n_total) n_total[b] = r.n_total;
    if (n_final) n_final[b] = r.n_final;
    if (revised_from) revised_from[b] = r.revised_from;
    if (status) status[b] = r.status;
    const bool taken = (r.status & (STREAM_FULL | STREAM_BAD_STATE)) == 0;
    const int64_t mm = m < 0 ? 0 : m;
    plan[b * 2] = taken ? r.n_total - mm : r.n_total;                    // (a bad state reports 0 poses: no row is final)
    plan[b * 2 + 1] = taken ? mm : -1;
}

struct LdsRows {                        // lag_smooth_row's Rows over the staged chunk; row k sits at k - c0
    const double* sA; const double* sG; const double* sU; const uint8_t* sT; int64_t c0;
    __device__ __forceinline__ double A(int64_t k, int c) const { return sA[c * LAG_ROWS + (int)(k - c0)]; }
    __device__ __forceinline__ double g(int64_t k, int c) const { return sG[c * LAG_ROWS + (int)(k - c0)]; }
    __device__ __forceinline__ double u(int64_t k, int c) const { return sU[c * LAG_ROWS + (int)(k - c0)]; }
    __device__ __forceinline__ int tags(int64_t k) const { return sT[(int)(k - c0)]; }
};

__global__ __launch_bounds__(64) void stream_lag_backpass_kernel(int64_t cap, int64_t lag, const double* __restrict__ ring_lag,
                                                                 double* __restrict__ ring_spos, double* __restrict__ ring_svar,
                                                                 const int64_t* __restrict__ seg_offsets, const int64_t* __restrict__ plan, LagOut o,
                                                                 int64_t* __restrict__ smooth_from, int64_t* __restrict__ n_smooth_final)
{
    __shared__ double sA[3 * LAG_ROWS], sG[3 * LAG_ROWS], sU[3 * LAG_ROWS];
    __shared__ uint8_t sT[LAG_ROWS];
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t lo = seg_offsets[b], mseg = seg_offsets[b + 1] - lo;
    const int64_t n0 = plan[b * 2], m = plan[b * 2 + 1];
    const int64_t n = n0 + (m < 0 ? 0 : m), from = lag_final_count(n0, lag), fin = m < 0 ? from : lag_final_count(n, lag);
    if (lane == 0) {
        if (smooth_from) smooth_from[b] = from;
        if (n_smooth_final) n_smooth_final[b] = fin;
    }
    // the segment's rows that did not become final (all of them for a refused track): NaN, flags 0
    for (int64_t r = lo + (fin - from) + lane; r < lo + mseg; r += 64) lag_nan_rows(o, r, r + 1);
    if (m <= 0) return;                                                  // (wave-uniform)
    const double* rl = ring_lag + b * cap * STREAM_LAG_F64;
    double* rs = ring_spos + b * cap * 3;
    double* rv = ring_svar + b * cap * 3;
    const int64_t s_from = from % cap;                                   // rows [from, n) are at most cap: a slot is s_from + (k - from), wrapped once
    for (int64_t c0 = from; c0 < n; c0 += 64) {
        const int64_t top = (c0 + 64 + lag < n ? c0 + 64 + lag : n);      // rows [c0, top) are staged: top - c0 <= LAG_ROWS
        for (int64_t k = c0 + lane; k < top; k += 64) {
            int64_t s = s_from + (k - from); s -= s >= cap ? cap : 0;
            int64_t sn = s + 1; sn -= sn >= cap ? cap : 0;
            const bool linked = k + 1 < n;
            const double* row = rl + s * STREAM_LAG_F64;
            const double* nx = rl + (linked ? sn : s) * STREAM_LAG_F64;
            const double Ppn[3] = { smooth_untag(nx[LG_PP]), nx[LG_PP + 1], nx[LG_PP + 2] };
            const LagTerms t = lag_terms(row, Ppn, linked);
            const int r = (int)(k - c0);
#pragma unroll
            for (int c = 0; c < 3; ++c) { sA[c * LAG_ROWS + r] = t.A[c]; sG[c * LAG_ROWS + r] = t.g[c]; sU[c * LAG_ROWS + r] = t.u[c]; }
            sT[r] = (uint8_t)t.tags;
        }
        __syncthreads();
        const int64_t i = c0 + lane;
        if (i < n) {
            const LagSmoothed sm = lag_smooth_row(LdsRows{ sA, sG, sU, sT, c0 }, i, lag, n);
            int64_t s = s_from + (i - from); s -= s >= cap ? cap : 0;
            double xs[3], Ps[3]; uint8_t fl;
            lag_finish_row(rl + s * STREAM_LAG_F64, sm, xs, Ps, fl);
#pragma unroll
            for (int c = 0; c < 3; ++c) { rs[s * 3 + c] = xs[c]; rv[s * 3 + c] = Ps[c]; }
            if (i < fin) {
                const int64_t w = lo + (i - from);
                if (o.spos) { o.spos[w * 3] = xs[0]; o.spos[w * 3 + 1] = xs[1]; o.spos[w * 3 + 2] = xs[2]; }
                if (o.svar) { o.svar[w * 3] = Ps[0]; o.svar[w * 3 + 1] = Ps[1]; o.svar[w * 3 + 2] = Ps[2]; }
                if (o.sflags) o.sflags[w] = fl;
            }
        }
        __syncthreads();                                                 // the next chunk's staging overwrites what these walks read
    }
}

}  // namespace

extern "C" int gsf_stream_append_lag_dev(gsf_ctx* ctx, const gsf_ekf_config* cfg, int64_t B, int64_t cap, int64_t lag, double* state_f64,
                                         int64_t* state_i64, double* ring_t, double* ring_pos, double* ring_quat, double* ring_lag, double* ring_spos,
                                         double* ring_svar, const double* ts, const double* pos, const double* quat, const double* gps,
                                         const uint8_t* valid, const int64_t* seg_offsets, double* pos_out, double* quat_out, double* cov_out,
                                         int64_t* n_total, int64_t* n_final, int64_t* revised_from, int32_t* status, double* spos_out,
                                         double* svar_out, uint8_t* sflags_out, int64_t* smooth_from, int64_t* n_smooth_final)
{
    GSF_REQUIRE(ctx && cfg, "ctx/cfg is NULL");
    GSF_REQUIRE(B >= 0 && cap >= 1, "negative B or cap < 1");
    GSF_REQUIRE(lag >= 1 && lag <= GSF_STREAM_LAG_MAX, "lag outside 1 .. GSF_STREAM_LAG_MAX");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(state_f64 && state_i64 && ring_t && ring_pos && ring_quat && seg_offsets, "NULL state, ring or seg_offsets");
    GSF_REQUIRE(ring_lag && ring_spos && ring_svar, "NULL ring_lag, ring_spos or ring_svar");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff && cap <= ((int64_t)1 << 40), "B or cap too large");
    for (int i = 0; i < 7; ++i) GSF_REQUIRE(cfg->initial_cov_diag[i] == cfg->initial_cov_diag[i], "NaN in config");
    GSF_HIP(hipSetDevice(ctx->device));
    { const int rc = ensure_workspace(ctx, GSF_WS_STREAM, (size_t)B * 2 * sizeof(int64_t)); if (rc) return rc; }
    int64_t* plan = workspace<int64_t>(ctx, GSF_WS_STREAM);
    const StreamSeg g{ ts, pos, quat, gps, valid, pos_out, quat_out, cov_out };
    hipLaunchKernelGGL(stream_append_lag_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, to_core(cfg), B, cap, lag, state_f64,
                       state_i64, ring_t, ring_pos, ring_quat, ring_lag, g, seg_offsets, n_total, n_final, revised_from, status, plan);
    GSF_HIP(hipGetLastError());
    const LagOut o{ spos_out, svar_out, sflags_out };
    hipLaunchKernelGGL(stream_lag_backpass_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, cap, lag, ring_lag, ring_spos, ring_svar, seg_offsets,
                       plan, o, smooth_from, n_smooth_final);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}
