// TEST-ONLY host harness: compiles the GSF_HD helpers of gsf_query_core.hpp (what gsf_query.hip calls per lane) with g++, so that
// tests/test_pose_query_host.py can compare them with the long-double restatement in the CPU-only tier.  Never shipped, never loaded by
// the package.
#include <cstdint>
#include "../gps_optimize_slam_amd/csrc/gsf_query_core.hpp"

using namespace gsf;

extern "C" {

int64_t hq_count_le(const double* t, int64_t n, double tau) { return query_count_le(t, n, tau); }
int64_t hq_count_le_i64(const int64_t* a, int64_t n, int64_t v) { return query_count_le(a, n, v); }
int hq_track_unsorted(const double* t, int64_t n) { return query_track_unsorted(t, n) ? 1 : 0; }

// One track, used the way the kernel's general route uses the helpers: classify -> search -> query_at [-> georef_point].
// x == NULL: poses (out_a = positions, out_q = quaternions); else points (out_a = xyz, out_q unused; ext_q must be normalisable).
void hq_query(const double* t, const double* pos, const double* quat, int64_t n, int32_t state, const double* tau, int64_t m, double max_gap,
              const double* x, const double* ext_q, const double* ext_t, double scale, double* out_a, double* out_q, uint8_t* flags, int32_t* index)
{
    for (int64_t k = 0; k < m; ++k) {
        const int cls = query_classify(state, tau[k], (state == 0) ? t[0] : 0.0, (state == 0) ? t[n - 1] : 0.0);
        QueryPose pose = query_nan_pose(cls);
        int64_t idx = -1;
        if (cls == 0) {
            idx = query_count_le(t, n, tau[k]) - 1;
            pose = query_at(t, pos, quat, idx, tau[k], max_gap);
        }
        int fl = pose.flags;
        if (x) {
            const double nan = __builtin_nan("");
            Vec3 o{ nan, nan, nan };
            if (idx >= 0 && !(fl & Q_GAP)) {
                QueryExtrinsic ext{ Quat{ 0.0, 0.0, 0.0, 1.0 }, Vec3{ 0.0, 0.0, 0.0 }, scale };
                if (ext_q) quat_unit(Quat{ ext_q[0], ext_q[1], ext_q[2], ext_q[3] }, ext.e);
                if (ext_t) ext.t = Vec3{ ext_t[0], ext_t[1], ext_t[2] };
                if (!georef_point(pose, ext, Vec3{ x[k * 3], x[k * 3 + 1], x[k * 3 + 2] }, o)) fl |= Q_BAD_QUAT;
            }
            out_a[k * 3] = o.x; out_a[k * 3 + 1] = o.y; out_a[k * 3 + 2] = o.z;
        } else {
            out_a[k * 3] = pose.p.x; out_a[k * 3 + 1] = pose.p.y; out_a[k * 3 + 2] = pose.p.z;
            out_q[k * 4] = pose.q.x; out_q[k * 4 + 1] = pose.q.y; out_q[k * 4 + 2] = pose.q.z; out_q[k * 4 + 3] = pose.q.w;
        }
        flags[k] = (uint8_t)fl;
        index[k] = (int32_t)idx;
    }
}
}
