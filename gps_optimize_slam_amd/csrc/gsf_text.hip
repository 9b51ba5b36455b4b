// gsf_text.hip -- step 7 of main_process_gui (ref :1085-1104) on the device: every byte of the TUM files np.savetxt writes, for B ragged
// tracks at once (gsf_tum_text_dev).  The digits come from gsf_text.hpp (integer arithmetic on the bit pattern, the same code the
// g++ harness checks against Python's '%.{p}f').
//
// Two calls.  The SIZE call runs tum_size_kernel (one wave per track: the length routine over its rows, the track's state) and
// tum_scan_kernel (one block: the lengths -> text_offsets[B+1], in place).  The WRITE call runs tum_write_kernel: one wave per track again,
// 64 rows per trip; every lane recomputes its row's length with the SAME routine, a wave-wide prefix sum places the row, the lane writes it.
// So no per-row workspace exists: the placement costs one 6-step shuffle scan per trip of 64 rows, and the write pass reads the rows once more
// (64 B per row and pass).  Bytes outside [text_offsets[b], text_offsets[b+1]) are never written, even for inconsistent input.
#include "gsf_internal.hpp"
#include "gsf_text.hpp"

using namespace gsf;

namespace {

constexpr int TEXT_BLOCK = 256, TEXT_WAVES = TEXT_BLOCK / 64;

// rows [i0, i1) of track b, clamped into [0, P) so that no read leaves the arrays whatever the offsets hold
__device__ __forceinline__ void track_rows(const int64_t* offsets, int64_t b, int64_t P, int64_t& i0, int64_t& i1)
{
    i0 = offsets[b]; i1 = offsets[b + 1];
    i1 = i1 < 0 ? 0 : (i1 > P ? P : i1);
    i0 = i0 < 0 ? 0 : (i0 > i1 ? i1 : i0);
}

__global__ __launch_bounds__(TEXT_BLOCK) void tum_size_kernel(int format, const double* __restrict__ ts, const double* __restrict__ xyz,
                                                              const double* __restrict__ quat, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ run_status, int64_t B, int64_t P,
                                                              int64_t* __restrict__ text_offsets, int32_t* __restrict__ track_state)
{
    const int64_t b = (int64_t)blockIdx.x * TEXT_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    if (run_status && run_status[b] != 0) {                       // the reference raised before step 7: no file
        if (lane == 0) { text_offsets[b + 1] = 0; track_state[b] = 1; }
        return;
    }
    int64_t i0, i1;
    track_rows(offsets, b, P, i0, i1);
    int64_t len = 0;
    int big = 0;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        double v[TUM_COLS];
        FixedField f[TUM_COLS];
        bool oor = false;
        tum_row_values(ts, xyz, quat, i, v);
        len += tum_row_len(format, v, f, oor);
        big |= oor ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { len += __shfl_xor(len, o, 64); big |= __shfl_xor(big, o, 64); }
    if (lane == 0) {
        text_offsets[b + 1] = big ? 0 : tum_header_len(format) + len;
        track_state[b] = big ? 2 : 0;                             // 2: a finite |x| >= 2^63 -- the host writes this track
    }
}

// text_offsets[1..B] = inclusive prefix sums of the lengths stored there, text_offsets[0] = 0; one block, a contiguous run per thread
__global__ __launch_bounds__(1024) void tum_scan_kernel(int64_t B, int64_t* __restrict__ text_offsets)
{
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (B + 1023) / 1024;
    const int64_t j0 = 1 + t * per, j1 = (j0 + per < B + 1) ? j0 + per : B + 1;
    int64_t s = 0;
    for (int64_t j = j0; j < j1; ++j) s += text_offsets[j];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                          // Hillis-Steele over the 1024 partial sums
        const int64_t add = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t j = j0; j < j1; ++j) { run += text_offsets[j]; text_offsets[j] = run; }
    if (t == 0) text_offsets[0] = 0;
}

__global__ __launch_bounds__(TEXT_BLOCK) void tum_write_kernel(int format, const double* __restrict__ ts, const double* __restrict__ xyz,
                                                               const double* __restrict__ quat, const int64_t* __restrict__ offsets, int64_t B,
                                                               int64_t P, const int64_t* __restrict__ text_offsets,
                                                               const int32_t* __restrict__ track_state, uint8_t* __restrict__ text)
{
    const int64_t b = (int64_t)blockIdx.x * TEXT_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B || track_state[b] != 0) return;
    const int64_t t0 = text_offsets[b], t1 = text_offsets[b + 1];
    const int hl = tum_header_len(format);
    if (t1 - t0 < hl) return;                                     // not what the size call produced: write nothing
    const char* h = tum_header(format);
    if (lane < hl) text[t0 + lane] = (uint8_t)h[lane];
    int64_t i0, i1;
    track_rows(offsets, b, P, i0, i1);
    int64_t pos = t0 + hl;
    for (int64_t base = i0; base < i1; base += 64) {
        const int64_t i = base + lane;
        FixedField f[TUM_COLS];
        int len = 0;
        if (i < i1) {
            double v[TUM_COLS];
            bool oor = false;
            tum_row_values(ts, xyz, quat, i, v);
            len = tum_row_len(format, v, f, oor);
            if (oor) len = 0;                                     // (a state-0 track holds none: the size call saw the same rows)
        }
        int incl = len;                                           // wave-wide inclusive prefix sum of the row lengths
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const int64_t at = pos + incl - len;
        if (len && at + len <= t1) tum_row_write(format, f, text + at);
        pos += __shfl(incl, 63, 64);
    }
}

}  // namespace

extern "C" {

int gsf_tum_text_dev(gsf_ctx* ctx, int32_t format, const double* ts, const double* xyz, const double* quat, const int64_t* offsets,
                     const int32_t* run_status, int64_t B, int64_t P, int64_t* text_offsets, int32_t* track_state, uint8_t* text)
{
    GSF_REQUIRE(ctx && offsets && text_offsets && track_state, "NULL argument");
    GSF_REQUIRE(format == GSF_TUM_UTM || format == GSF_TUM_WGS84, "format must be GSF_TUM_UTM or GSF_TUM_WGS84");
    GSF_REQUIRE(B >= 0 && B <= ((int64_t)0x7fffffff) * TEXT_WAVES && P >= 0, "bad B / P");
    GSF_REQUIRE(P == 0 || (ts && xyz && quat), "NULL rows");
    GSF_HIP(hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)((B + TEXT_WAVES - 1) / TEXT_WAVES);
    if (!text) {
        GSF_HIP(hipMemsetAsync(text_offsets, 0, sizeof(int64_t), ctx->stream));
        if (B == 0) return GSF_OK;
        hipLaunchKernelGGL(tum_size_kernel, dim3(grid), dim3(TEXT_BLOCK), 0, ctx->stream, (int)format, ts, xyz, quat, offsets, run_status, B, P,
                           text_offsets, track_state);
        GSF_HIP(hipGetLastError());
        hipLaunchKernelGGL(tum_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, B, text_offsets);
        GSF_HIP(hipGetLastError());
        return GSF_OK;
    }
    if (B == 0) return GSF_OK;
    hipLaunchKernelGGL(tum_write_kernel, dim3(grid), dim3(TEXT_BLOCK), 0, ctx->stream, (int)format, ts, xyz, quat, offsets, B, P, text_offsets,
                       track_state, text);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // extern "C"
