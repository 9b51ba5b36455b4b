// gsf_rows_rule.hpp -- the Sim3 row choice of main_process_gui (ref :973-998) as DECISIONS on lane masks: the wave-uniform part of the
// early-variance build's row rule (gsf_ekf_wave_early.hip, step 2b), pure host code (no HIP include; compiled with g++ into
// tests/host_rows_rule_harness.cpp and checked on the CPU against oracle.pick_sim3_rows by tests/test_rows_rule_host.py).
// A track of at most R chunks of 64 rows.  The caller forms three lane masks per chunk with per-lane compares --
//   m[k]    row 64 k + l is a row of the track and valid,
//   graw[k] the stamp of row 64 k + l exceeds the stamp of row 64 k + l - 1 by more than max_gap (bit 0 of chunk 0: anything),
//   le[k]   the stamp of row 64 k + l is <= segment_start_time + max_dur, segment_start_time = the stamp of rows_first_valid()'s row --
// and hands over a way to fetch single stamps (the one or two either side of a hole).  rows_rule_choose() walks the candidates of the
// first gap as fit_moments_reference_rows (gsf_wave_common.hpp) does and then DECIDES what that pass finds out by summing again: the two
// fall-backs (:984, :993-995) and the ValueError cases (:975, :997) are functions of popcounts.  What comes out is the final set of rows as
// one mask per chunk, in the terms of that pass: valid AND in front of row_end AND (state 0 only) inside the duration limit.
#pragma once
#include <stdint.h>
#include "gsf_math.hpp"

namespace gsf {
typedef unsigned long long rows_u64;

GSF_HD rows_u64 rows_first(const int n) { return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull)); }   // lanes 0..n-1
GSF_HD int rows_top(const rows_u64 m) { return 63 - __builtin_clzll(m); }                                  // highest set lane (m != 0)

template <int R> struct RowsChoice {
    rows_u64 mo[R];        // the rows the fit sums, chunk by chunk
    int row_end;           // the rows considered are in front of this one (the row in front of the first gap; N when there is none)
    int nT;                // how many rows mo holds
    int nF;                // valid rows of the first segment (V[:k], :981-982)
    int32_t rows_flag;     // 0 (the timed subset), SIM3_FLAG_ROWS_SEGMENT, SIM3_FLAG_ROWS_ALL or SIM3_FLAG_FEW_ROWS
    int dep_end;           // the choice is a function of the validity of rows 0 .. dep_end - 1 alone (the gap's row is the last one looked at,
                           // unless every valid row is taken)
};

// chunk and lane of the first valid row: the GNSS-side shift and segment_start_time (:988); false when no row is valid
template <int R> GSF_HD bool rows_first_valid(const rows_u64* m, int& k0, int& l0)
{
    k0 = -1; l0 = 0;
#pragma unroll
    for (int k = R - 1; k >= 0; --k) if (m[k] != 0ull) { k0 = k; l0 = __builtin_ctzll(m[k]); }
    return k0 >= 0;
}

// N: rows of the track (<= 64 R).  stamp_at(i): the stamp of row i, asked for only either side of a hole in the valid rows.
template <int R, class StampAt>
GSF_HD void rows_rule_choose(const rows_u64* m, const rows_u64* graw, const rows_u64* le, const int N, const int min_samples, const double max_gap,
                             StampAt stamp_at, RowsChoice<R>& out)
{
    // ---- the first gap (np.diff of the VALID rows' stamps, :979-980).  Candidates: a valid row right behind a valid row whose stamp is
    // more than max_gap later (g), and the first row of a run of valid rows (s), whose predecessor among the valid rows sits across a hole.
    rows_u64 g[R], s[R], g_any = 0ull; int nst = 0, nvalid = 0; bool top = false;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const rows_u64 mp = (m[k] << 1) | (top ? 1ull : 0ull);            // row i - 1 is valid
        g[k] = graw[k] & m[k] & mp; s[k] = m[k] & ~mp;
        g_any |= g[k]; nst += __builtin_popcountll(s[k]); nvalid += __builtin_popcountll(m[k]); top = (m[k] >> 63) != 0ull;
    }
    bool gap_found = false; int row_end = N, nF = nvalid, gap_row = -1;
    if (g_any != 0ull || nst > 1) {                                       // (the usual track: one run of valid rows and no step above max_gap -- no candidate)
        int e = -1, cnt = 0;                                              // last valid row so far, number of valid rows up to and including it
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (gap_found || m[k] == 0ull) continue;
            rows_u64 cand = g[k] | s[k];
            while (cand != 0ull && !gap_found) {
                const int l = __builtin_ctzll(cand); cand &= cand - 1ull;
                const rows_u64 lower = m[k] & rows_first(l);             // valid rows of this chunk in front of the candidate
                const int ep = lower != 0ull ? 64 * k + rows_top(lower) : e;                                   // the valid row in front of it ...
                const int before = lower != 0ull ? cnt + __builtin_popcountll(lower) - 1 : cnt - 1;            // ... and how many valid rows precede THAT one
                if (ep < 0) continue;                                     // the first valid row of the track
                bool gap = ((g[k] >> l) & 1ull) != 0ull;
                if (!gap) gap = stamp_at(64 * k + l) - stamp_at(ep) > max_gap;                                 // across a hole
                if (gap) { gap_found = true; row_end = ep; nF = before; gap_row = 64 * k + l; }                // V[:k] leaves row ep out as well (:981-982)
            }
            e = 64 * k + rows_top(m[k]); cnt += __builtin_popcountll(m[k]);
        }
    }
    // ---- which rows are summed (:983-997)
    rows_u64 seg[R], tim[R];                                              // the first segment, and its rows inside the duration limit
    int nT = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        seg[k] = gap_found ? (m[k] & rows_first(row_end - 64 * k)) : m[k];
        tim[k] = seg[k] & le[k];
        nT += __builtin_popcountll(tim[k]);
    }
    int32_t flag = 0; bool all = false, timed = true;
    if (nF < min_samples) {                                               // :983
        if (!gap_found) flag = SIM3_FLAG_FEW_ROWS;                        // V itself is that short: ValueError (:975); the sums are not used
        else { all = true; timed = false; row_end = N; nT = nvalid; flag = nT < min_samples ? SIM3_FLAG_FEW_ROWS : SIM3_FLAG_ROWS_ALL; }   // :984 (:975)
    } else if (nT < min_samples) { timed = false; nT = nF; flag = SIM3_FLAG_ROWS_SEGMENT; }                    // :993-995: the whole first segment
#pragma unroll
    for (int k = 0; k < R; ++k) out.mo[k] = all ? m[k] : (timed ? tim[k] : seg[k]);
    out.row_end = row_end; out.nT = nT; out.nF = nF; out.rows_flag = flag;
    out.dep_end = (gap_found && !all) ? gap_row + 1 : N;
}
}  // namespace gsf
