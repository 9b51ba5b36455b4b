// gsf_ekf_wave_big.hip -- the wave-per-trajectory kernels (gsf_ekf_wave.hip, gsf_wave_common.hpp) built for BIG batches: more than two
// waves per SIMD (B > 2 048 trajectories; C3, the C5 shard).  Same template, same arithmetic, same bits as the small-batch builds; what
// differs is how a chunk's rows travel: with several waves per SIMD the launch sits on the memory system under its mixed read + write
// stream (the C3 timing probes), so the strided 8-byte loads / stores of a lane's own row are replaced by whole
// 16-byte pieces of the chunk's contiguous slabs, lane after lane, transposed through a few KB of LDS (the !SMALLBATCH
// paths of gsf_wave_common.hpp).  A separate translation unit because the two regimes want different instruction schedulers
// (Makefile): iterative-ilp for the lone wave of the small batches, max-ilp here.
#define GSF_ROWS_ROUND 4                                                  // rounds of the row-choice pass: six chunks in flight spill 17 registers at 168 per lane
#include "gsf_wave_common.hpp"

using namespace gsf;

namespace {

#ifndef GSF_BIG_OCC
#define GSF_BIG_OCC 3                                                     // three waves per SIMD: 168 registers (max-ilp left alone takes 216 and halves the occupancy)
#endif
template <bool PIPELINE, int AXMODE>
__global__ __launch_bounds__(64, GSF_BIG_OCC) void ekf_wave_big_kernel(WaveArgs a, EkfConfig cfg)
{
    wave_serial_body<PIPELINE, false, false, 1, AXMODE>(a, cfg, (int64_t)blockIdx.x, (int)threadIdx.x);
}

}  // namespace

namespace gsf {

int launch_ekf_wave_big(gsf_ctx* ctx, const WaveRoute& r, const WaveArgs& a, const EkfConfig& k)
{
    wave_lift<1, 0>(r.pipeline, [&](auto p) { wave_lift<1, 0>(r.xy, [&](auto x) {
        hipLaunchKernelGGL((ekf_wave_big_kernel<decltype(p)::value != 0, decltype(x)::value>), dim3((unsigned)a.B), dim3(64), 0, ctx->stream, a, k); }); });
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

const char* wave_big_build_info() { return GSF_TU_BUILD_INFO("gsf_ekf_wave_big.hip"); }

}  // namespace gsf
