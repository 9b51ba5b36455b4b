// gsf_weighted_core.hpp -- per-fix measurement noise (gsf_ekf_smooth_weighted_dev, gsf_fix_var_at_poses_dev): the rules of ekf_smooth_kernel<SMOOTH_WEIGHTED> (gsf_smooth.hip) and gsf_weighted.hip
// that are plain host/device C++ (definitions: include/gsf.h, "per-fix GNSS noise").
//
//  * which variance is usable, what a row's three variances make of the row (usable / bad / "no information"), and the row's availability:
//    the smoother's avail[i] AND three usable variances.  A row that fails only on its variances is a pose without a fix in every respect
//    and carries POSE_BAD_SIGMA -- unless all three are +inf, the caller's way of saying that there is nothing to weigh;
//  * the normalised innovation squared of a used row;
//  * the bracket rule that carries per-fix variances onto SLAM stamps: among the KEPT fixes of a log the last one at or before the stamp
//    and the first one at or after it, the larger variance of the two per axis.  The bracket is found by the binary search of
//    gsf_query_core.hpp and a walk over removed fixes; both stay inside [0, n) whatever the stamps hold.
// The kernels call them per lane / per thread; tests/host_harness_weighted.cpp compiles them with g++ and compares them with the
// restatement of tests/weighted_ref.py bit for bit.
#pragma once
#include "gsf_smooth_core.hpp"
#include "gsf_query_core.hpp"

namespace gsf {

enum : int32_t { POSE_BAD_SIGMA = 32 };   // per-pose flag bit (include/gsf.h), beside gsf_cov_core.hpp's and POSE_SPAN_START

// the stated range of a per-fix variance: gsf_ekf_config's range of meas_noise_diag, both ends included
constexpr double WVAR_MIN = 1e-8, WVAR_MAX = 1e8;

// finite and inside the range (false for NaN, for both infinities, for 0 and for negative values)
GSF_HD bool wvar_usable(const double v) { return v >= WVAR_MIN && v <= WVAR_MAX; }

enum : int { WROW_USABLE = 0, WROW_BAD = 1, WROW_NO_INFO = 2 };
// what the three variances of a row say: all usable; all +inf ("no information": no fix, no flag); anything else is a bad row
GSF_HD int wvar_row(const double v0, const double v1, const double v2)
{
    const double inf = __builtin_huge_val();
    if (wvar_usable(v0) && wvar_usable(v1) && wvar_usable(v2)) return WROW_USABLE;
    if (v0 == inf && v1 == inf && v2 == inf) return WROW_NO_INFO;
    return WROW_BAD;
}

struct WeightedAvail { bool avail, bad; };
// base: the smoother's avail[i] (i >= 1, mask byte set, fix free of NaN; ref :867-869).  Where base is false the variances decide nothing
// (the kernel passes whatever the row holds): any bytes there change no output and set no bit.
GSF_HD WeightedAvail weighted_avail(const bool base, const double v0, const double v1, const double v2)
{
    const int k = wvar_row(v0, v1, v2);
    return WeightedAvail{ base && k == WROW_USABLE, base && k == WROW_BAD };
}

// one axis' share of the normalised innovation squared: y^2 / (Pp + r), y the innovation before any blend
GSF_HD double weighted_nis_term(const double y, const double Pp, const double r)
{
    const double y2 = y * y;
    const double S = Pp + r;
    return y2 * fast_rcp(S);
}

// #{k < n : a[k] < v} for ascending a: np.searchsorted(a, v, side='left') (query_count_le is side='right')
template <class P, class V>
GSF_HD int64_t query_count_lt(P a, int64_t n, V v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the larger of two variances; a NaN on either side gives NaN (the filter then flags the row)
GSF_HD double wvar_max(const double a, const double b)
{
    if (a != a || b != b) return __builtin_nan("");
    return a > b ? a : b;
}

// The variance of a pose at stamp tau from ONE log: t[n] ascending stamps, keep[n] (NULL: all kept), var[n][3].  lo = the last kept fix
// with stamp <= tau, hi = the first kept fix with stamp >= tau; either missing: +inf x3.  With repeated stamps at tau, lo is the last and
// hi the first of them.  Every index stays in [0, n): the searches return 0..n and the walks stop at the ends, whatever t holds (a NaN
// tau compares false everywhere: no lo, +inf).
template <class TP, class KP, class VP>
GSF_HD Vec3 fix_var_bracket(TP t, KP keep, VP var, const int64_t n, const double tau)
{
    const double inf = __builtin_huge_val();
    const Vec3 none{ inf, inf, inf };
    if (n <= 0) return none;
    int64_t lo = query_count_le(t, n, tau) - 1;                          // last stamp <= tau, or -1
    while (lo >= 0 && keep && keep[lo] == 0) --lo;                       // ... that is kept
    if (lo < 0) return none;
    int64_t hi = query_count_lt(t, n, tau);                              // first stamp >= tau, or n
    while (hi < n && keep && keep[hi] == 0) ++hi;
    if (hi >= n) return none;
    return Vec3{ wvar_max(var[lo * 3], var[hi * 3]), wvar_max(var[lo * 3 + 1], var[hi * 3 + 1]), wvar_max(var[lo * 3 + 2], var[hi * 3 + 2]) };
}

}  // namespace gsf
