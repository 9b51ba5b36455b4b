// gsf_ekf_wave.hip -- K4 (and the fused K2+K3+K4 pipeline) with ONE WAVEFRONT PER TRAJECTORY.
//
// apply_ekf_correction (EKFGPSSLAM.py:831-935) is a serial recursion over the poses of one track, but every
// piece of it is an associative scan once the covariance is known to stay diagonal:
//   * orientation      q_i = q_{i-1} * dq_i                 -> prefix PRODUCT of quaternions
//   * variances        P_i = r(P+qdt)/((P+qdt)+r) or P+qdt   -> prefix composition of 2x2 Moebius maps
//   * positions        p_i = (1-k_i)(p_{i-1}+u_i) + k_i z_i  -> prefix composition of affine maps
//   * outage structure (start / recovery / sharp-turn gate)  -> 64-bit ballots + bit scans
//   * per-outage RTS   x_s[k] = x_f[k] + (P_f[k]/P_p[r]) (x_f[r]-x_p[r])   (the product of the gains A_j telescopes)
// so a wave takes 64 consecutive poses per iteration (lane = pose), runs log2(64) = 6 shuffle stages per scan (4 or 5 for a last
// chunk of at most 16 / 32 poses: the cross-row stages cannot reach its lanes) and carries ~30 scalars to the next 64 poses.  All loads/stores of a chunk are contiguous (the natural
// trajectory-major layout of stacked TUM files), B trajectories give B independent waves, and a 271-pose track costs
// 5 iterations instead of 270 dependent steps: this is the low-latency / small-batch path (configs C1, C2); the
// lane-per-trajectory kernel of gsf_ekf.hip is the streaming path for huge batches.
//
// Arithmetic differs from the serial form only in rounding order (quaternion renormalisation once per chunk instead of
// every step, Moebius instead of Joseph variance update, local coordinates per chunk): observed |dp| ~1e-9 m against
// the 1e-6 m gate; the tests compare against the dense-7x7 CPU oracle.
#include "gsf_wave_common.hpp"

using namespace gsf;

namespace {

// AXMODE 1: x and y share (P0, Q, R), z does not (checked by the launcher; the default CONFIG) -- see wave_serial_chunks.
// This file holds the SMALL-batch builds (inlined cold blocks, direct loads and stores; scheduled with iterative-ilp for the lone wave);
// the big-batch builds of the same template live in gsf_ekf_wave_big.hip (slab loads / stores through LDS, scheduled with max-ilp:
// iterative-ilp crashes clang's register allocator on them, and max-ilp is the faster of the two at many waves per SIMD anyway).
template <bool PIPELINE, bool SMALLBATCH, int AXMODE>
__global__ __launch_bounds__(64, 1) void ekf_wave_kernel(WaveArgs a, EkfConfig cfg)
{
    static_assert(SMALLBATCH, "big-batch instantiations belong to gsf_ekf_wave_big.hip");
    wave_serial_body<PIPELINE, false, SMALLBATCH, 1, AXMODE>(a, cfg, (int64_t)blockIdx.x, (int)threadIdx.x);
}
// The builds for tracks whose last chunk ends below lane 16 | 32 (TAILNS 4 | 5): every chunk before the last is a full one, known at
// compile time, and the last one runs its scans without the cross-row stages that cannot reach its lanes (wave_serial_chunks,
// GSF_SCAN_STAGES_N; same bits as the kernel above) -- and the build for tracks of a multiple of 64 poses (WAVE_TAIL_FULL: full chunks
// only).  The launcher picks the build from N.  They are OVERLOADS of the kernel above
// -- the build travels in the argument's type -- and not a fourth template argument, so that a profile, bench.py and the tools keep
// finding the kernel of a workload under the one name ekf_wave_kernel<PIPELINE, SMALLBATCH, AXMODE>.
template <int TAILNS> struct WaveArgsTail { WaveArgs a; };
#define GSF_WAVE_TAIL_KERNEL(T_)                                                                                                      \
    template <bool PIPELINE, bool SMALLBATCH, int AXMODE>                                                                             \
    __global__ __launch_bounds__(64, 1) void ekf_wave_kernel(WaveArgsTail<T_> w, EkfConfig cfg)                                       \
    {                                                                                                                                 \
        static_assert(SMALLBATCH, "big-batch instantiations belong to gsf_ekf_wave_big.hip");                                         \
        wave_serial_body<PIPELINE, false, SMALLBATCH, 1, AXMODE, T_>(w.a, cfg, (int64_t)blockIdx.x, (int)threadIdx.x);                \
    }
GSF_WAVE_TAIL_KERNEL(4)
GSF_WAVE_TAIL_KERNEL(5)
GSF_WAVE_TAIL_KERNEL(WAVE_TAIL_FULL)
#undef GSF_WAVE_TAIL_KERNEL


// Two waves per trajectory for SMALL batches of the fused pipeline (one wave per SIMD, every wave in the same phase at the same
// time): while wave 0 is busy with the fit -- a memory burst followed by a latency-bound 3x3 Jacobi chain that leave the SIMD
// mostly idle -- wave 1 computes the variances of EVERY chunk (they depend on stamps and availability only, not on the fit) into
// LDS; after one block barrier wave 0 runs the chunk loop without its two Moebius scans (-28 % instructions per chunk).
// Same functions, same operands, same order as the one-wave kernel: bit-identical results.
#ifndef GSF_DUO_ROLE_SHIFT
#define GSF_DUO_ROLE_SHIFT 2        // measured best of 0..3 at 1 000 tracks (22.6 vs 23.1-23.2 us; 23.6 us without the helper)
#endif
template <bool PIPELINE, int AXMODE, int TAILNS>
__device__ __forceinline__ void wave_duo_body(const WaveArgs& a, const EkfConfig& cfg, const int pv_stride)
{
    extern __shared__ double gsf_pv[];
    const int lane = threadIdx.x & 63;
    const int64_t b = blockIdx.x;
    // which wave of the block helps alternates with the block index: when two blocks share a pair of SIMDs, each SIMD then holds
    // one main and one helper wave (complementary phases) instead of two of a kind
    const bool helper = ((threadIdx.x >> 6) ^ ((blockIdx.x >> GSF_DUO_ROLE_SHIFT) & 1u)) != 0u;
    if (a.N <= 0) { if (!helper && lane == 0 && a.status) a.status[b] = 0; return; }   // empty tracks: both waves leave before any barrier
    if (helper) {
        wave_variance_helper<TAILNS>(a, cfg, b, lane, gsf_pv, pv_stride);
        __syncthreads();
        return;
    }
    wave_serial_body<PIPELINE, true, true, 1, AXMODE, TAILNS>(a, cfg, b, lane, gsf_pv, pv_stride);
}
template <bool PIPELINE, int AXMODE>
__global__ __launch_bounds__(128) void ekf_wave_duo_kernel(WaveArgs a, EkfConfig cfg, int pv_stride) { wave_duo_body<PIPELINE, AXMODE, 6>(a, cfg, pv_stride); }
// (the builds with the last chunk's scans sized, as overloads under the same name: see ekf_wave_kernel)
template <bool PIPELINE, int AXMODE>
__global__ __launch_bounds__(128) void ekf_wave_duo_kernel(WaveArgsTail<4> w, EkfConfig cfg, int pv_stride) { wave_duo_body<PIPELINE, AXMODE, 4>(w.a, cfg, pv_stride); }
template <bool PIPELINE, int AXMODE>
__global__ __launch_bounds__(128) void ekf_wave_duo_kernel(WaveArgsTail<5> w, EkfConfig cfg, int pv_stride) { wave_duo_body<PIPELINE, AXMODE, 5>(w.a, cfg, pv_stride); }
template <bool PIPELINE, int AXMODE>
__global__ __launch_bounds__(128) void ekf_wave_duo_kernel(WaveArgsTail<WAVE_TAIL_FULL> w, EkfConfig cfg, int pv_stride) { wave_duo_body<PIPELINE, AXMODE, WAVE_TAIL_FULL>(w.a, cfg, pv_stride); }

// the kernel argument of the build whose last chunk's scans run T stages: the build travels in its type (see WaveArgsTail)
template <int T> auto tail_args(const WaveArgs& a) { if constexpr (T == 6) return a; else return WaveArgsTail<T>{ a }; }

}  // namespace

namespace gsf {

// trajectory-major launches (called from gsf_ekf.hip's C entry points): the arguments and the config once, the build from wave_route()
int launch_ekf_wave(gsf_ctx* ctx, bool pipeline, const double* ts, const double* pos, const double* quat, const double* gps,
                    const uint8_t* valid, const double* init_pos, const double* init_quat, const gsf_ekf_config* cfg, int64_t B,
                    int64_t N, double* R, double* t, double* s, double* pos_out, double* quat_out, int32_t* status,
                    const int64_t* offsets)
{
    GSF_REQUIRE(B <= 0x7fffffff, "B too large for one launch");
    const WaveArgs a{ ts, pos, quat, gps, valid, init_pos, init_quat, R, t, s, pos_out, quat_out, status, B, N, offsets, pipeline ? ctx->fit_rows : FitRows{ 0, 0, 0.0, 0.0 } };
    const EkfConfig k = to_core(cfg);
    const WaveRoute r = wave_route({ ctx->block_kernel, ctx->duo_kernel, ctx->early_variances, ctx->tail_scan_stages, pipeline, wave_xy_layout(k), offsets != nullptr, B, N });
    switch (r.family) {
    case WAVE_BLOCK: return launch_ekf_block(ctx, r, a, k);
    case WAVE_EARLY: return launch_ekf_wave_early(ctx, r, a, k);
    case WAVE_BIG: return launch_ekf_wave_big(ctx, r, a, k);
    case WAVE_DUO:
        wave_lift<1, 0>(r.xy, [&](auto x) { wave_lift<4, 5, WAVE_TAIL_FULL, 6>(r.tail, [&](auto tl) {
            hipLaunchKernelGGL((ekf_wave_duo_kernel<true, decltype(x)::value>), dim3((unsigned)B), dim3(128), (size_t)r.pv_stride * 9 * sizeof(double), ctx->stream,
                               tail_args<decltype(tl)::value>(a), k, r.pv_stride); }); });
        break;
    case WAVE_ONE:
        wave_lift<1, 0>(r.pipeline, [&](auto p) { wave_lift<1, 0>(r.xy, [&](auto x) { wave_lift<4, 5, WAVE_TAIL_FULL, 6>(r.tail, [&](auto tl) {
            hipLaunchKernelGGL((ekf_wave_kernel<decltype(p)::value != 0, true, decltype(x)::value>), dim3((unsigned)B), dim3(64), 0, ctx->stream,
                               tail_args<decltype(tl)::value>(a), k); }); }); });
        break;
    }
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

const char* wave_small_build_info() { return GSF_TU_BUILD_INFO("gsf_ekf_wave.hip"); }

}  // namespace gsf
