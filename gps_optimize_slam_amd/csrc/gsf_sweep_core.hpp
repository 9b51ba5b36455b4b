// gsf_sweep_core.hpp -- EKF noise sweep (gsf_ekf_noise_sweep_dev): the pieces of gsf_noise_sweep.hip that are plain host/device C++.
//
// Given the gains, a position axis of the reference's filter is an affine recurrence (all covariances are diagonal, H = [I3 0]):
//     without a usable fix   p[i] = p[i-1] + d[i]                                  (ref :702-715)
//     with one               p[i] = (1 - w g) (p[i-1] + d[i]) + w g z[i]          (ref :722-731; w: the one-step blend of :752-768)
// so a chunk of 64 poses is a prefix composition of pairs (a, b): x -> a x + b, and what the sweep keeps of a pose is twelve terms of its
// innovation y = z - (p[i-1] + d[i]), S = Pp + R.  This header holds the pair, its composition, the twelve terms and the
// figures derived from a row of sums (nll, mean NIS, the pick); the kernel evaluates them per lane, scans / sums across lanes and carries a
// candidate's last pose from one chunk to the next; tests/host_harness_sweep.cpp compiles them with g++ and compares them with per-pose loops.
#pragma once
#include "gsf_math.hpp"

namespace gsf {

constexpr int SWEEP_NSTAT = 12;        // doubles of a stats row (include/gsf.h)
constexpr int SWEEP_MAX_K = 4096;      // candidates of one call
constexpr int SWEEP_MAX_GROUP = 64;    // candidates of one wave (one lane holds the carry of one candidate)

enum : int32_t { NS_NONE = 1, NS_TIE = 2 };   // ns_status bits (include/gsf.h)

struct Affine { double a, b; };        // x -> a x + b

// the pose's own map: (1, d) without an update, (1 - w g, (1 - w g) d + w g z) with one
GSF_HD Affine sweep_affine(const bool avail, const double wg, const double d, const double z)
{
    const double om = 1.0 - wg;
    const double bu = om * d + wg * z;
    return Affine{ avail ? om : 1.0, avail ? bu : d };
}
// later o earlier
GSF_HD Affine affine_compose(const Affine& later, const Affine& earlier)
{
    const double b = later.a * earlier.b + later.b;
    return Affine{ later.a * earlier.a, b };
}
GSF_HD double affine_apply(const Affine& m, const double x)
{
    const double r = m.a * x + m.b;
    return r;
}

// Normalised innovation nu = y / sqrt(S) of one pose per axis, zero where the pose is not a counted update.
GSF_HD void sweep_pose_nu(const double* y, const double* S, const bool counted, double* nu)
{
    for (int c = 0; c < 3; ++c) {
        const double n = y[c] * fast_rsqrt(S[c]);
        nu[c] = counted ? n : 0.0;
    }
}
// The twelve terms of one pose (zero where the pose is not a counted update).  y, S: innovation and its variance per axis; nu / nu_prev:
// sweep_pose_nu of this pose and of the pose before it; counted / counted_prev: whether this pose / the pose before it belongs to U.
GSF_HD void sweep_pose_terms(const double* y, const double* S, const double* nu, const double* nu_prev, const bool counted,
                             const bool counted_prev, double* term)
{
    double lag = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double y2 = y[c] * y[c];
        const double nis = y2 * fast_rcp(S[c]);
        term[1 + c] = counted ? nis : 0.0;
        term[4 + c] = counted ? log(S[c]) : 0.0;
        term[7 + c] = counted ? y2 : 0.0;
        const double pr = nu[c] * nu_prev[c];
        lag = lag + pr;
    }
    const bool both = counted && counted_prev;
    term[0] = counted ? 1.0 : 0.0;
    term[10] = both ? lag : 0.0;
    term[11] = both ? 1.0 : 0.0;
}

// ---- figures of a row of sums (the Python binding computes the same ones for every row; the pick kernel needs them to choose)
GSF_HD bool sweep_row_finite(const double* row)
{
    bool ok = true;
    for (int j = 0; j < SWEEP_NSTAT; ++j) ok = ok && (fabs(row[j]) <= 1.7976931348623157e308);   // false for NaN and infinities
    return ok;
}
// nll = (3 n ln 2pi + sum log S + sum NIS) / 2
GSF_HD double sweep_nll(const double* row)
{
    const double ln2pi = 1.8378770664093453;
    const double c = 3.0 * row[0];
    const double k = c * ln2pi;
    const double ls = (row[4] + row[5]) + row[6];
    const double ns = (row[1] + row[2]) + row[3];
    return 0.5 * ((k + ls) + ns);
}
GSF_HD double sweep_mean_nis(const double* row) { return ((row[1] + row[2]) + row[3]) / row[0]; }
// criterion 0: nll, criterion 1: |mean NIS - 3|; +inf for a row that may not be picked (not finite, or the score is not)
GSF_HD double sweep_score(const double* row, const int criterion)
{
    const double inf = __builtin_huge_val();
    if (!sweep_row_finite(row)) return inf;
    const double s = criterion == 0 ? sweep_nll(row) : fabs(sweep_mean_nis(row) - 3.0);
    return (fabs(s) <= 1.7976931348623157e308) ? s : inf;
}
// "the first k with the smallest score": (s1, k1) goes before (s0, k0)
GSF_HD bool sweep_pick_before(const double s1, const int k1, const double s0, const int k0)
{
    return s1 < s0 || (s1 == s0 && k1 < k0);
}

}  // namespace gsf
