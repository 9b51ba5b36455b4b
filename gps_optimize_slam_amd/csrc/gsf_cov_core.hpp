// gsf_cov_core.hpp -- per-pose covariance of the fused track: the pieces of gsf_ekf_cov.hip that are plain host/device C++.
//
// All covariances of the reference are diagonal (P0, Q, R from np.diag, H = [I3 0], the Joseph form keeps the diagonal; see the header
// comment of gsf_ekf_core.hpp), so 7 doubles per pose are the whole matrix.  What this header holds:
//  * the smoothed variance of rts_smoother_segment (ref :777-803) in closed form,
//  * the outage structure of one 64-pose chunk -- outage starts, recoveries, pairs inside an outage -- as bit operations on the
//    64-bit "GNSS available" mask of the chunk, with the state carried in from the chunk before (ref :848, :859-862, :875-894, :926-932).
// The kernel calls them wave-uniformly; tests/host_harness_cov.cpp compiles them with g++ and compares them with a per-pose restatement.
#pragma once
#include "gsf_math.hpp"

namespace gsf {

typedef unsigned long long cov_mask;

enum : int32_t {                   // per-pose flag bits (include/gsf.h)
    POSE_GNSS_USED = 1, POSE_IN_OUTAGE = 2, POSE_SMOOTHED = 4, POSE_SHARP_TURN = 8
};

// bits lo..hi (inclusive) of a 64-bit mask; empty if lo > hi
GSF_HD cov_mask cov_bits(int lo, int hi)
{
    if (lo > hi) return 0ull;
    const cov_mask upto_hi = (hi >= 63) ? ~0ull : ((1ull << (hi + 1)) - 1ull);
    const cov_mask below_lo = (lo <= 0) ? 0ull : ((1ull << lo) - 1ull);
    return upto_hi & ~below_lo;
}

// Smoothed variance of pose k of a segment [a..b] handed to rts_smoother_segment (a = outage start, b = the recovery), a <= k < b.
// Ps[b] = Pf[b]; Ps[k] = Pf[k] + A^2 (Ps[k+1] - Pp[k+1]), A = Pf[k] / Pp[k+1] (:786-801, F = I).  No pose a..b-1 was updated, so
// Pf[k] = Pp[k] there, the product of the A telescopes to Pf[k] / Pp[b], and the backward recurrence collapses to
//     Ps[k] = Pf[k] + (Pf[k] / Pp[b])^2 (Pf[b] - Pp[b]).
// An axis without an update at b (the quaternion axes) has Pf[b] == Pp[b] and comes back unchanged, bit for bit.
GSF_HD double cov_smooth(double Pf_k, double Pp_b, double Pf_b)
{
    const double g = Pf_k * fast_rcp(Pp_b);
    return Pf_k + (g * g) * (Pf_b - Pp_b);
}

// Outage structure of one chunk.  act: lanes that hold a pose; av: "GNSS available" of those poses (pose 0 of the track: the raw mask
// byte, :848; every other pose: mask byte set and a fix free of NaN, :867-869); first_chunk: lane 0 is pose 0 of the track;
// prev_avail: the flag of the pose before lane 0 (ignored in the first chunk).
struct OutageMasks {
    cov_mask start;                // an outage begins at this pose (:875-877; pose 0: :861-862)
    cov_mask rec;                  // GNSS recovers at this pose (:879)
    cov_mask pair;                 // this pose and the one before it both lie inside an outage: a pair of is_sharp_turn_in_segment (:814-816)
};
GSF_HD OutageMasks outage_masks(cov_mask act, cov_mask av, bool first_chunk, bool prev_avail)
{
    const cov_mask step = first_chunk ? (act & ~1ull) : act;             // pose 0 takes no filter step
    const cov_mask a = act & av;
    const cov_mask ap = (a << 1) | ((first_chunk || prev_avail) ? 1ull : 0ull);   // the flag of the pose before (pose 0: "available")
    OutageMasks m;
    m.start = act & ~av & ap;
    m.rec = step & av & ~ap;
    m.pair = step & ~av & ~ap;
    return m;
}

// The outage that the recovery at lane r of the chunk closes.  start: OutageMasks::start; sharp_pairs: lanes of OutageMasks::pair whose
// pair exceeds the yaw-rate threshold; c0: index of lane 0's pose; ostart / seg_sharp: the open outage carried in (used if no outage
// starts before r in this chunk); neg_thr: the threshold is negative, so the maximum rate of :813 -- 0 where no pair was evaluated -- exceeds it.
struct OutageSeg {
    int start_lane;                // first lane of the outage, -1: it began in an earlier chunk, at pose `first`
    int64_t first;                 // index of its first pose (a)
    bool sharp;                    // judged a sharp turn: >= 2 poses and a pair above the threshold, or a negative threshold (:882-889, :826)
};
GSF_HD OutageSeg outage_closed_at(cov_mask start, cov_mask sharp_pairs, int r, int64_t c0, int64_t ostart, bool seg_sharp, bool neg_thr = false)
{
    OutageSeg o;
    const cov_mask sm = start & cov_bits(0, r - 1);
    bool seg;
    if (sm != 0ull) {
        o.start_lane = 63 - __builtin_clzll(sm);
        o.first = c0 + o.start_lane;
        seg = (sharp_pairs & cov_bits(o.start_lane + 1, r - 1)) != 0ull;
    } else {
        o.start_lane = -1;
        o.first = ostart;
        seg = seg_sharp || (sharp_pairs & cov_bits(0, r - 1)) != 0ull;
    }
    o.sharp = (c0 + r - o.first >= 2) && (seg || neg_thr);
    return o;
}

// State handed to the next chunk; L = last lane that holds a pose.
struct OutageCarry {
    bool prev_avail;               // flag of the chunk's last pose; false: the chunk ends inside an outage ...
    int64_t ostart;                // ... that began at this pose ...
    bool seg_sharp;                // ... and has had a pair above the threshold so far
};
GSF_HD OutageCarry outage_carry(const OutageCarry& in, cov_mask av, cov_mask start, cov_mask sharp_pairs, int L, int64_t c0)
{
    OutageCarry o = in;
    const bool open = ((av >> L) & 1ull) == 0ull;
    if (open) {
        const cov_mask sm = start & cov_bits(0, L);
        if (sm != 0ull) {
            const int s = 63 - __builtin_clzll(sm);
            o.ostart = c0 + s;
            o.seg_sharp = (sharp_pairs & cov_bits(s + 1, L)) != 0ull;
        } else {
            o.seg_sharp = in.seg_sharp || (sharp_pairs & cov_bits(0, L)) != 0ull;
        }
    }
    o.prev_avail = !open;
    return o;
}

}  // namespace gsf
