// gsf_query_core.hpp -- the fused track at any stamp, and sensor points carried into its frame: the pieces of gsf_query.hip that are plain
// host/device C++ (definitions: include/gsf.h, "pose queries").
//
// What this header holds:
//  * the bracket search on a sorted stamp array, templated on the POINTER TYPE: the kernel instantiates it once for global memory and once
//    for the wave's staged copy in LDS, so neither instance goes through a generic pointer (a generic pointer makes every access a flat
//    instruction: HISTORY, time_align_kernel),
//  * the classification of a query against its track,
//  * query_interp: the weight, the position and quaternion_nlerp (ref :94-105, quat_nlerp of gsf_math.hpp as it stands),
//  * georef_point: a sensor point through its extrinsics and the interpolated pose.
// Both routes of the kernel call query_at on the same values, so a query's result does not depend on the route that served it;
// tests/host_harness_query.cpp compiles the same functions with g++ and compares them with a long-double restatement.
#pragma once
#include "gsf_math.hpp"

namespace gsf {

enum : int32_t {                   // per-track state bits (include/gsf.h)
    QT_EMPTY = 1, QT_UNSORTED = 2, QT_SKIPPED = 4, QT_BAD_EXTRINSIC = 8
};
enum : int32_t {                   // per-query flag bits (include/gsf.h)
    Q_EXACT = 1, Q_BEFORE = 2, Q_AFTER = 4, Q_GAP = 8, Q_NAN = 16, Q_TRACK = 32, Q_BAD_QUAT = 64
};

// #{k < n : a[k] <= v} for ascending a: np.searchsorted(a, v, side='right').  Among equal values it counts all of them.
template <class P, class V>
GSF_HD int64_t query_count_le(P a, int64_t n, V v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a stamp that breaks the order after `prev` (a NaN on either side counts)
GSF_HD bool query_stamp_breaks(double prev, double cur) { return !(cur >= prev); }

// GSF_QT_UNSORTED of one track, sequentially (the kernel takes the same pair test lane-parallel)
template <class P>
GSF_HD bool query_track_unsorted(P t, int64_t n)
{
    if (n <= 0) return false;
    if (t[0] != t[0]) return true;
    for (int64_t i = 1; i < n; ++i) if (query_stamp_breaks(t[i - 1], t[i])) return true;
    return false;
}

// a query against its track's state and end stamps: 0 = it has a bracket
GSF_HD int query_classify(int32_t track_state, double tau, double t_first, double t_last)
{
    if (track_state != 0) return Q_TRACK;
    if (tau != tau) return Q_NAN;
    if (tau < t_first) return Q_BEFORE;
    if (tau > t_last) return Q_AFTER;
    return 0;
}

struct QueryPose { Vec3 p; Quat q; int flags; };

GSF_HD QueryPose query_nan_pose(int flags)
{
    const double nan = __builtin_nan("");
    return QueryPose{ Vec3{ nan, nan, nan }, Quat{ nan, nan, nan, nan }, flags };
}

// between pose i (stamp ti) and pose j (stamp tj > ti), ti < tau <= tj: two subtractions, one IEEE division, one fma per axis, nlerp
GSF_HD QueryPose query_interp(double tau, double ti, double tj, const Vec3& pi, const Vec3& pj, const Quat& qi, const Quat& qj)
{
    const double w = (tau - ti) / (tj - ti);
    QueryPose o;
    o.p = Vec3{ fma(w, pj.x - pi.x, pi.x), fma(w, pj.y - pi.y, pi.y), fma(w, pj.z - pi.z, pi.z) };
    o.q = quat_nlerp(qi, qj, w);
    o.flags = 0;
    return o;
}

// The pose at tau from rows i, i + 1 of (t, pos, quat); i = query_count_le(t, n, tau) - 1 >= 0 and tau <= t[n - 1].  An exact hit copies
// row i and reads nothing of row i + 1; a bracket wider than max_gap (> 0) gives NaN.  TP / RP: plain pointers or LDS pointers.
template <class TP, class RP>
GSF_HD QueryPose query_at(TP t, RP pos, RP quat, int64_t i, double tau, double max_gap)
{
    const double ti = t[i];
    const Vec3 pi{ pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] };
    const Quat qi{ quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3] };
    if (ti == tau) return QueryPose{ pi, qi, Q_EXACT };
    const int64_t j = i + 1;
    const double tj = t[j];
    if (max_gap > 0.0 && tj - ti > max_gap) return query_nan_pose(Q_GAP);
    const Vec3 pj{ pos[j * 3], pos[j * 3 + 1], pos[j * 3 + 2] };
    const Quat qj{ quat[j * 4], quat[j * 4 + 1], quat[j * 4 + 2], quat[j * 4 + 3] };
    return query_interp(tau, ti, tj, pi, pj, qi, qj);
}

// sensor -> body of one track: e = unit(ext_q), ext_t, scale
struct QueryExtrinsic { Quat e; Vec3 t; double s; };

// out = p(tau) + R(unit(q(tau))) * (scale * (R(e) x + ext_t)); false (out untouched): q(tau) cannot be normalised
GSF_HD bool georef_point(const QueryPose& pose, const QueryExtrinsic& ext, const Vec3& x, Vec3& out)
{
    const Vec3 r = quat_rotate(ext.e, x);
    const Vec3 y{ ext.s * (r.x + ext.t.x), ext.s * (r.y + ext.t.y), ext.s * (r.z + ext.t.z) };
    Quat qh;
    if (!quat_unit(pose.q, qh)) return false;
    const Vec3 w = quat_rotate(qh, y);
    out = Vec3{ pose.p.x + w.x, pose.p.y + w.y, pose.p.z + w.z };
    return true;
}

}  // namespace gsf
