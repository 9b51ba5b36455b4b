// gsf_traj_eval_core.hpp -- trajectory evaluation against 6-DoF truth (gsf_traj_eval_dev): the pieces of gsf_traj_eval.hip that are plain
// host/device C++ (definitions: include/gsf.h, "trajectory evaluation").
//
// What this header holds:
//  * te_associate: one estimate pose against the truth stamps of its track (nearest stamp, or the interpolation rule of gsf_pose_query_dev
//    through the helpers of gsf_query_core.hpp as they are), both quaternions normalised once,
//  * te_truth_pose: the truth pose of a pose that te_associate matched, formed again from match_index by the same calls (the same bits),
//  * te_align_pose / te_ape: p' = s R p + t, q' = q_R (x) q (transform_trajectory, ref :461-468) and the two absolute errors,
//  * te_angle: the angle of a quaternion as 2 atan2(|v|, |w|),
//  * te_last_frame / te_pair_error: the pair search and the pair error of the relative-error scenarios (KITTI's calcSequenceErrors),
//  * te_select_kth: an exact order statistic of non-negative doubles by counting on their bit patterns.
// tests/host_harness_traj_eval.cpp compiles the same functions with g++ and tests/test_traj_eval_host.py compares them with a 50-digit
// restatement (tests/traj_eval_ref.py), whose bounds count the rounded operations of the longest path through the code below.
#pragma once
#include "gsf_math.hpp"
#include "gsf_query_core.hpp"

namespace gsf {

enum : int32_t { TE_NEAREST = 0, TE_INTERP = 1 };                                        // assoc_mode
enum : int32_t { TE_ALIGN_NONE = 0, TE_ALIGN_SE3 = 1, TE_ALIGN_SIM3 = 2 };                // align_mode
enum : int32_t { TE_FRAMES = 0, TE_METRES = 1, TE_SECONDS = 2 };                          // rpe_kind
enum : int32_t { TE_MATCHED = 1, TE_NO_TRUTH = 2, TE_NAN = 4, TE_BAD_QUAT = 8, TE_TRACK = 16 };   // pose_flags
enum : int32_t { TE_TRACK_SKIPPED = 1, TE_TRACK_EMPTY = 2, TE_TRACK_UNSORTED = 4, TE_TRACK_FEW = 8, TE_TRACK_DEGENERATE = 16 };
constexpr int32_t TE_TRACK_UNREAD = TE_TRACK_SKIPPED | TE_TRACK_EMPTY | TE_TRACK_UNSORTED;   // decided before anything is searched

// #{k < n : a[k] < v} for ascending a: np.searchsorted(a, v, side='left')
template <class P, class V>
GSF_HD int64_t te_count_lt(P a, int64_t n, V v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

GSF_HD bool te_finite3(const Vec3& p) { return fabs(p.x) < INFINITY && fabs(p.y) < INFINITY && fabs(p.z) < INFINITY; }

struct TeMatch { int32_t flags; int64_t index; Vec3 g; Quat qg; Quat qe; };   // truth position, unit truth quaternion, unit estimate quaternion

// The truth pose that match_index names: NEAREST -- row `index`; INTERP -- query_at on the bracket `index` (an exact stamp copies the row).
// false: the bracket is wider than max_diff (INTERP only; te_associate has then reported TE_NO_TRUTH).
template <class TP, class RP>
GSF_HD bool te_truth_row(int32_t assoc_mode, double max_diff, double tau, TP rt, RP rpos, RP rquat, int64_t index, Vec3& g, Quat& q)
{
    if (assoc_mode == TE_INTERP) {
        const QueryPose o = query_at(rt, rpos, rquat, index, tau, max_diff);
        g = o.p; q = o.q;
        return !(o.flags & Q_GAP);
    }
    g = Vec3{ rpos[index * 3], rpos[index * 3 + 1], rpos[index * 3 + 2] };
    q = Quat{ rquat[index * 4], rquat[index * 4 + 1], rquat[index * 4 + 2], rquat[index * 4 + 3] };
    return true;
}

// One estimate pose (stamp tau, position p, quaternion q) against the G >= 1 sorted, NaN-free truth stamps rt of its track.  The checks come
// in this order and the first that fails names the flag: estimate position, estimate quaternion, the search, truth position, truth quaternion.
template <class TP, class RP>
GSF_HD TeMatch te_associate(int32_t assoc_mode, double max_diff, double tau, const Vec3& p, const Quat& q, TP rt, RP rpos, RP rquat, int64_t G)
{
    const double nan = __builtin_nan("");
    TeMatch m{ 0, -1, Vec3{ nan, nan, nan }, Quat{ nan, nan, nan, nan }, Quat{ nan, nan, nan, nan } };
    if (!te_finite3(p)) { m.flags = TE_NAN; return m; }
    if (!quat_unit(q, m.qe)) { m.flags = TE_BAD_QUAT; return m; }
    int64_t j;
    if (assoc_mode == TE_INTERP) {
        if (tau < rt[0] || tau > rt[G - 1]) { m.flags = TE_NO_TRUTH; return m; }     // no extrapolation
        j = query_count_le(rt, G, tau) - 1;
    } else {
        // c truth stamps are <= tau.  The candidates are the first stamp after tau (row c: among equal stamps it is the first) and the
        // last stamp at or before it, taken at the FIRST row that holds that stamp; on a tie of the two distances the earlier row.
        const int64_t c = query_count_le(rt, G, tau);
        double dl = INFINITY, dr = INFINITY;
        int64_t jl = -1;
        if (c > 0) { const double tl = rt[c - 1]; jl = te_count_lt(rt, G, tl); dl = tau - tl; }
        if (c < G) dr = rt[c] - tau;
        const bool left = dl <= dr;
        j = left ? jl : c;
        if (!((left ? dl : dr) <= max_diff)) { m.flags = TE_NO_TRUTH; return m; }
    }
    Vec3 g; Quat qg;
    if (!te_truth_row(assoc_mode, max_diff, tau, rt, rpos, rquat, j, g, qg)) { m.flags = TE_NO_TRUTH; return m; }
    if (!te_finite3(g)) { m.flags = TE_NAN; return m; }
    Quat qu;
    if (!quat_unit(qg, qu)) { m.flags = TE_BAD_QUAT; return m; }
    m.flags = TE_MATCHED; m.index = j; m.g = g; m.qg = qu;
    return m;
}

// the truth pose and the unit estimate quaternion of a MATCHED pose again, from match_index: the calls of te_associate on the same values
template <class TP, class RP>
GSF_HD void te_truth_pose(int32_t assoc_mode, double max_diff, double tau, const Quat& q, TP rt, RP rpos, RP rquat, int64_t index,
                          Vec3& g, Quat& qg, Quat& qe)
{
    quat_unit(q, qe);
    Quat raw;
    te_truth_row(assoc_mode, max_diff, tau, rt, rpos, rquat, index, g, raw);
    quat_unit(raw, qg);
}

// the angle of the rotation a quaternion stands for, in [0, pi]: 2 atan2(|v|, |w|).  acos(|w|) has the derivative 1 / |v|: at an angle of
// 1e-12 rad w rounds to 1 and every digit is lost; atan2 takes the small number |v| as it is.
GSF_HD double te_angle(const Quat& q)
{
    const double v = sqrt(fma(q.z, q.z, fma(q.y, q.y, q.x * q.x)));
    return 2.0 * atan2(v, fabs(q.w));
}

struct TeAlign { double R[9]; double t[3]; double s; Quat qR; };

GSF_HD TeAlign te_align_identity()
{
    return TeAlign{ { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 }, { 0.0, 0.0, 0.0 }, 1.0, Quat{ 0.0, 0.0, 0.0, 1.0 } };
}

// p' = s (R p) + t: a three-term fma chain per axis, then one fma
GSF_HD Vec3 te_align_point(const TeAlign& a, const Vec3& p)
{
    const double rx = fma(a.R[2], p.z, fma(a.R[1], p.y, a.R[0] * p.x));
    const double ry = fma(a.R[5], p.z, fma(a.R[4], p.y, a.R[3] * p.x));
    const double rz = fma(a.R[8], p.z, fma(a.R[7], p.y, a.R[6] * p.x));
    return Vec3{ fma(a.s, rx, a.t[0]), fma(a.s, ry, a.t[1]), fma(a.s, rz, a.t[2]) };
}

GSF_HD double te_norm3(double x, double y, double z) { return sqrt(fma(z, z, fma(y, y, x * x))); }

// the absolute errors of one matched pose: pa / qa = the aligned estimate
GSF_HD void te_ape(const TeAlign& a, const Vec3& p, const Quat& qe, const Vec3& g, const Quat& qg, Vec3& pa, Quat& qa, double& ape_t, double& ape_r)
{
    pa = te_align_point(a, p);
    qa = quat_mul(a.qR, qe);
    ape_t = te_norm3(pa.x - g.x, pa.y - g.y, pa.z - g.z);
    ape_r = te_angle(quat_mul(quat_conj(qg), qa));
}

// ---- relative errors over the matched poses m = 0 .. M-1 of a track.  A row of the matched table: 16 doubles.
enum : int { TE_ROW = 16, TE_ROW_G = 0, TE_ROW_QG = 3, TE_ROW_P = 7, TE_ROW_Q = 10, TE_ROW_TS = 14, TE_ROW_D = 15 };

template <class RP>
struct TeColumn {                                          // one column of the table as an array over m
    RP rows; int col;
    GSF_HD double operator[](int64_t m) const { return rows[m * TE_ROW + col]; }
};

// the last frame of first frame f, or -1 (no pair): f < l < M always
template <class RP>
GSF_HD int64_t te_last_frame(int32_t kind, double value, RP rows, int64_t M, int64_t f)
{
    int64_t l = -1;
    if (kind == TE_FRAMES) {
        if (!(value >= 1.0 && value < 9.2e18)) return -1;
        const int64_t step = (int64_t)value;
        l = (step < M - f) ? f + step : -1;
    } else if (kind == TE_METRES) {                        // the smallest l > f with d[l] > d[f] + value
        const TeColumn<RP> d{ rows + (f + 1) * TE_ROW, TE_ROW_D };
        const double target = rows[f * TE_ROW + TE_ROW_D] + value;
        if (target != target) return -1;
        l = f + 1 + query_count_le(d, M - f - 1, target);
    } else if (kind == TE_SECONDS) {                       // the smallest l > f with ts[l] >= ts[f] + value
        const TeColumn<RP> t{ rows + (f + 1) * TE_ROW, TE_ROW_TS };
        const double target = rows[f * TE_ROW + TE_ROW_TS] + value;
        if (target != target) return -1;
        l = f + 1 + te_count_lt(t, M - f - 1, target);
    }
    return (l > f && l < M) ? l : -1;
}

template <class RP> GSF_HD Vec3 te_row_vec(RP row, int c) { return Vec3{ row[c], row[c + 1], row[c + 2] }; }
template <class RP> GSF_HD Quat te_row_quat(RP row, int c) { return Quat{ row[c], row[c + 1], row[c + 2], row[c + 3] }; }

// E = (g_f^-1 g_l)^-1 (e_f^-1 e_l): et = |E.t|, er = the angle of E.R.  E.t = R_A^T (t_B - t_A) with A, B the two relative poses, and
// a rotation keeps the length, so et is taken as |t_B - t_A|.
template <class RP>
GSF_HD void te_pair_error(RP rf, RP rl, double& et, double& er)
{
    const Quat gf = te_row_quat(rf, TE_ROW_QG), gl = te_row_quat(rl, TE_ROW_QG), ef = te_row_quat(rf, TE_ROW_Q), el = te_row_quat(rl, TE_ROW_Q);
    const Vec3 pgf = te_row_vec(rf, TE_ROW_G), pgl = te_row_vec(rl, TE_ROW_G), pef = te_row_vec(rf, TE_ROW_P), pel = te_row_vec(rl, TE_ROW_P);
    const Vec3 ta = quat_rotate(quat_conj(gf), Vec3{ pgl.x - pgf.x, pgl.y - pgf.y, pgl.z - pgf.z });
    const Vec3 tb = quat_rotate(quat_conj(ef), Vec3{ pel.x - pef.x, pel.y - pef.y, pel.z - pef.z });
    const Quat qa = quat_mul(quat_conj(gf), gl), qb = quat_mul(quat_conj(ef), el);
    et = te_norm3(tb.x - ta.x, tb.y - ta.y, tb.z - ta.z);
    er = te_angle(quat_mul(quat_conj(qa), qb));
}

// ---- exact order statistics.  Non-negative doubles order as their bit patterns do as unsigned integers, so the k-th smallest (k from 0)
// is found bit by bit from the top: of the values that share the prefix found so far, count those whose next bit is 0.  `count(prefix_mask,
// prefix, bit)` returns that count; 64 rounds, no sort, no length limit.
template <class COUNT>
GSF_HD uint64_t te_select_kth(int64_t k, COUNT count)
{
    uint64_t prefix = 0, mask = 0;
    for (int b = 63; b >= 0; --b) {
        const uint64_t bit = (uint64_t)1 << b;
        const int64_t zeros = count(mask, prefix, bit);
        if (k >= zeros) { k -= zeros; prefix |= bit; }
        mask |= bit;
    }
    return prefix;
}

}  // namespace gsf
