// gsf_weighted.hip -- per-fix GNSS noise: the kernel that carries per-fix variances onto SLAM stamps (gsf_fix_var_at_poses_dev).  The
// filter and smoother that take them, gsf_ekf_smooth_weighted_dev and gsf_ekf_smooth_reweighted_dev, are ekf_smooth_kernel<SMOOTH_WEIGHTED>
// and <SMOOTH_REWEIGHTED> of gsf_smooth.hip, launched from there: the kernel lives in that unit.
#include "gsf_wave_common.hpp"
#include "gsf_weighted_core.hpp"

namespace {

// ---- per-fix variances onto SLAM stamps: one thread per pose
struct FixVarArgs {
    const double* ts; const int64_t* slam_offsets; const double* gps_t; const int64_t* gps_offsets; const uint8_t* gps_keep;
    const double* fix_var; const uint8_t* valid; double* pose_var; int64_t B, P;
};

__global__ __launch_bounds__(256) void fix_var_at_poses_kernel(const FixVarArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const double inf = __builtin_huge_val();
    Vec3 v{ inf, inf, inf };
    if (!a.valid || a.valid[i] != 0) {
        // the pose's track: the last b with slam_offsets[b] <= i (an empty track shares its offset with the next one and is passed over)
        int64_t b = query_count_le(a.slam_offsets, a.B + 1, i) - 1;
        b = b < 0 ? 0 : (b > a.B - 1 ? a.B - 1 : b);
        const int64_t g0 = a.gps_offsets[b], n = a.gps_offsets[b + 1] - g0;
        v = fix_var_bracket(a.gps_t + g0, a.gps_keep ? a.gps_keep + g0 : (const uint8_t*)nullptr, a.fix_var + g0 * 3, n, a.ts[i]);
    }
    a.pose_var[i * 3] = v.x; a.pose_var[i * 3 + 1] = v.y; a.pose_var[i * 3 + 2] = v.z;
}

}  // namespace

namespace gsf {

int launch_fix_var_at_poses(gsf_ctx* ctx, const double* ts, const int64_t* slam_offsets, const double* gps_t, const int64_t* gps_offsets,
                            const uint8_t* gps_keep, const double* fix_var, const uint8_t* valid, int64_t B, int64_t P, double* pose_var)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const FixVarArgs a{ ts, slam_offsets, gps_t, gps_offsets, gps_keep, fix_var, valid, pose_var, B, P };
    hipLaunchKernelGGL(fix_var_at_poses_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace gsf
