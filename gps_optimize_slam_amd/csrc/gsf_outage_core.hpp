// gsf_outage_core.hpp -- GNSS outage study (gsf_outage_study_dev): the pieces of gsf_outage_study.hip that are plain host/device C++.
//
// A scenario withholds the fixes of a window W of poses.  Nothing before the outage [a, b) that W creates changes (GNSS never
// touches the state quaternion, every covariance is diagonal), so the unmodified run's filtered state at the anchor c = max(a - 1, 0) is the
// modified run's as well, and inside the outage no pose takes an update:
//     p_dr[k] = p_f[c] + (D[k] - D[c]),   Pdr[k] = Pf[c] + Q (T[k] - T[c])        D, T: prefix sums of d[i] and dt[i] over the track
// rts_smoother_segment (ref :777-803) over [a..b] with F = I and no update inside telescopes (see cov_smooth, gsf_cov_core.hpp) to
//     p_fu[k] = p_dr[k] + (Pdr[k] / Pp[b]) g y,   g = Pp[b] / S,  S = Pp[b] + R,  y = z[b] - p-[b]
// This header holds: the window -> [a, b) walk over a flag array, the flag word, the recovery's terms and the closed form.  The kernel finds
// a and b with ballots over the same flag bytes, evaluates the rest per lane and sums across lanes; tests/host_harness_outage.cpp compiles
// this header with g++ and compares it with per-pose loops and with the backward recurrence.
#pragma once
#include "gsf_math.hpp"

namespace gsf {

constexpr int OUTAGE_NSTAT = 13;       // doubles of a stats row (include/gsf.h)
constexpr int OUTAGE_MAX_K = 4096;     // scenarios of one call
constexpr int OUTAGE_ROW = 11;         // doubles of a base-pass row: p_f - init_pos [3], Pf [3], D [3], T, sum |d|

enum : int32_t {                       // os_flags bits (include/gsf.h)
    OS_EMPTY = 1, OS_NO_RECOVERY = 2, OS_SMOOTHED = 4, OS_SHARP_TURN = 8, OS_MERGED = 16, OS_FROM_START = 32, OS_UNSORTED = 64, OS_SKIPPED = 128
};
enum : uint8_t { OSF_AVAIL = 1, OSF_PAIR = 2 };   // base-pass byte of a pose: avail[i]; the pair (i - 1, i) exceeds the yaw-rate threshold

// W = [w0, w1) is usable: a window of NaN or without length holds no pose
GSF_HD bool outage_window_ok(const double s, const double L) { return s == s && L == L && L > 0.0; }

// The outage [a, b) that withholding W = [w0, w1), w0 < w1 <= n, creates: the maximal run of poses without a usable fix around W.
// flags[i] & OSF_AVAIL = avail[i] of the unmodified run.  b = n: no recovery.
GSF_HD void outage_span(const uint8_t* flags, const int64_t n, const int64_t w0, const int64_t w1, int64_t& a, int64_t& b)
{
    a = w0;
    while (a > 0 && !(flags[a - 1] & OSF_AVAIL)) --a;
    b = w1;
    while (b < n && !(flags[b] & OSF_AVAIL)) ++b;
}
// the sharp-turn decision at the recovery (ref :882-889, :826): >= 2 poses and a pair strictly inside (a, b) above the threshold, or a
// negative threshold
GSF_HD bool outage_sharp(const int64_t a, const int64_t b, const bool pair_inside, const bool neg_thr) { return (b - a >= 2) && (pair_inside || neg_thr); }
GSF_HD bool outage_sharp(const uint8_t* flags, const int64_t a, const int64_t b, const bool neg_thr)
{
    bool any = false;
    for (int64_t j = a + 1; j < b; ++j) any = any || (flags[j] & OSF_PAIR) != 0;
    return outage_sharp(a, b, any, neg_thr);
}
GSF_HD int32_t outage_flag_word(const int64_t n, const int64_t w0, const int64_t w1, const int64_t a, const int64_t b, const bool sharp)
{
    int32_t f = 0;
    if (b >= n) f |= OS_NO_RECOVERY; else f |= sharp ? OS_SHARP_TURN : OS_SMOOTHED;
    if (a < w0 || b > w1) f |= OS_MERGED;
    if (a == 0) f |= OS_FROM_START;
    return f;
}

// one axis of the dead-reckoned state of pose k from the rows of the anchor c and of k (positions relative to init_pos)
GSF_HD double outage_dr_pos(const double x_c, const double D_c, const double D_k) { return x_c + (D_k - D_c); }
GSF_HD double outage_dr_var(const double Pf_c, const double Q, const double T_c, const double T_k) { return Pf_c + Q * (T_k - T_c); }
// one axis of the recovery: innovation y, its variance S and the smoother's push g y
struct OutageAxis { double y, S, gy; };
GSF_HD OutageAxis outage_recovery(const double z_b, const double pm_b, const double Pp_b, const double R)
{
    OutageAxis r;
    r.y = z_b - pm_b;
    r.S = Pp_b + R;
    const double g = Pp_b * fast_rcp(r.S);
    r.gy = g * r.y;
    return r;
}
// the telescoped rts_smoother_segment for one axis of pose k, a <= k < b
GSF_HD double outage_smooth(const double p_dr, const double Pdr, const double Pp_b, const double gy)
{
    const double w = Pdr * fast_rcp(Pp_b);
    return p_dr + w * gy;
}

}  // namespace gsf
