// gsf_smooth_core.hpp -- whole-track RTS smoothing (gsf_ekf_smooth_ragged_dev): the pieces of gsf_smooth.hip that are plain host/device C++.
//
// All covariances are diagonal, so the backward pass of rts_smoother_segment (ref :777-803) over a span is, per axis and in
// correction coordinates e = xs - xf, d = Ps - Pf, a pair of affine recurrences that run from the span's last pose down to its first:
//     e[k] = A[k] (e[k+1] + g[k+1]),   d[k] = A[k]^2 (d[k+1] + (Pf[k+1] - Pp[k+1])),   A[k] = Pf[k] / Pp[k+1],   Pp[k+1] = Pf[k] + Q dt[k+1]
// with g = xf - xp the correction the filter applied (0 without an update), and A[k] = 0 on a span's last pose.  This header holds
//  * the gain A (0 where Pp[k+1] == 0: the reference's pinv lands there) and the two maps of a row,
//  * the two tag bits the forward pass parks with a row -- "a fix was applied here", "a span starts here" -- in the sign bits of two
//    values that are never negative (a variance, a sum of dt), so that the backward pass reads 56 B per row and nothing else of the filter,
//  * which rows a later fix of their own span reaches (GSF_POSE_SMOOTHED), as bit operations on the 64-bit lane masks of a chunk in
//    SCAN ORDER: scan lane j holds row c0 + 63 - j, so that "the row after" is the lane before and a suffix scan over the rows is the
//    prefix scan of the wave kernels.
// The kernel calls them per lane; tests/host_harness_smooth.cpp compiles them with g++ and drives them over whole tracks.
#pragma once
#include "gsf_cov_core.hpp"
#include "gsf_sweep_core.hpp"

namespace gsf {

enum : int32_t { POSE_SPAN_START = 16 };   // per-pose flag bit (include/gsf.h), beside gsf_cov_core.hpp's

// ---- the tag in the sign bit of a value that is >= 0 (-0.0 carries it as well: bit operations only)
GSF_HD double smooth_tag(const double v, const bool bit)
{
    unsigned long long u; __builtin_memcpy(&u, &v, 8);
    u = (u & 0x7fffffffffffffffull) | (bit ? 0x8000000000000000ull : 0ull);
    double r; __builtin_memcpy(&r, &u, 8);
    return r;
}
GSF_HD bool smooth_tag_of(const double v)
{
    unsigned long long u; __builtin_memcpy(&u, &v, 8);
    return (u >> 63) != 0ull;
}
GSF_HD double smooth_untag(const double v) { return smooth_tag(v, false); }

// predicted variance of the row after k (ref :712-714) and the smoother gain A[k] = Pf[k] / Pp[k+1] (:789, F = I); 0 <= A <= 1
GSF_HD double smooth_pred(const double Pf_k, const double q, const double dt_next)
{
    const double Pp = Pf_k + q * dt_next;
    return Pp;
}
GSF_HD double smooth_gain(const double Pf_k, const double Pp_next, const bool linked)
{
    const bool ok = linked && (Pp_next > 0.0);                            // (false for NaN as well)
    const double A = Pf_k * fast_rcp(ok ? Pp_next : 1.0);
    return ok ? A : 0.0;
}
// the maps of row k: e[k] = A e[k+1] + A g[k+1];  d[k] = A^2 d[k+1] + A^2 u[k+1], u = Pf - Pp of the row after (0 without an update)
GSF_HD Affine smooth_map_e(const double A, const double g_next)
{
    const double b = A * g_next;
    return Affine{ A, b };
}
GSF_HD Affine smooth_map_d(const double A, const double Pf_next, const double Pp_next, const bool fix_next)
{
    const double A2 = A * A;
    const double u = Pf_next - Pp_next;
    const double b = A2 * (fix_next ? u : 0.0);
    return Affine{ A2, b };
}

// Is the row in scan lane j reached by a later fix of its own span?  fix / start: the chunk's "a fix was applied" / "a span starts" rows
// as lane masks in scan order (lanes that hold no row: 0); carry: the answer "reached, or itself a fix, and not a span start" of the
// first row of the chunk above (false above the track's last row).  The rows after j are the lanes below j: the nearest of them that
// carries either bit decides -- a fix that starts no span reaches down, a span start stops (its own fix belongs to the span above).
GSF_HD bool smooth_row_reached(const cov_mask fix, const cov_mask start, const int j, const bool carry)
{
    const cov_mask lower = cov_bits(0, j - 1);
    const cov_mask f = fix & lower, s = start & lower;
    if (f == 0ull) return s == 0ull && carry;
    if (s == 0ull) return true;
    return __builtin_clzll(f) < __builtin_clzll(s);                       // the nearest fix lies below the nearest span start
}
// the carry for the chunk below, from its top scan lane (63 = the chunk's first row)
GSF_HD bool smooth_reach_carry(const cov_mask fix, const cov_mask start, const bool reached63)
{
    const bool st = (start >> 63) != 0ull, fx = (fix >> 63) != 0ull;
    return !st && (fx || reached63);
}

}  // namespace gsf
