// gsf_gate_core.hpp -- innovation gate (gsf_innovation_gate_dev): the pieces of gsf_gate.hip that are plain host/device C++.
//
// The gate rejects a GNSS fix whose normalised innovation squared (NIS) exceeds a threshold; a rejected fix is a pose without a fix in
// every respect, so a rejection changes the state, the variance and the outage structure of every later pose: the decisions are
// sequential.  The kernel scans a chunk of 64 poses under a SPECULATED rejection mask and repairs it: of the lanes that are over the gate
// under the current mask, the LOWEST one has seen only settled decisions before it, so its own decision is final -- a rejection, or a
// forced accept when max_run rejected fixes immediately precede it.  This header holds that step (gate_settle), the run count it needs
// (gate_run_before), the counts of a settled chunk (gate_chunk_counts) and the NIS itself, all as bit operations on 64-bit lane masks
// with the state carried in from the chunk before.  The kernel calls them wave-uniformly; tests/host_harness_gate.cpp compiles them with
// g++ and compares them with a per-pose loop.  The outage bookkeeping of a rejection (merging with a natural outage, a run across a
// chunk boundary) is gsf_cov_core.hpp's, fed with the availability mask minus the rejected lanes.
#pragma once
#include "gsf_cov_core.hpp"

namespace gsf {

constexpr int GATE_NSTAT = 8;          // doubles of a stats row (include/gsf.h)
constexpr int GATE_MAX_K = 64;         // gates of one call

enum : int32_t {                       // gate_status bits (include/gsf.h)
    GATE_SKIPPED = 1, GATE_EMPTY = 2, GATE_UNSORTED = 4, GATE_ANY_REJECTED = 8, GATE_ANY_FORCED = 16
};

// NIS of one pose: (y0^2 / S0 + y1^2 / S1) + y2^2 / S2
GSF_HD double gate_nis(const double* y, const double* S)
{
    const double a = y[0] * y[0], b = y[1] * y[1], c = y[2] * y[2];
    const double n0 = a * fast_rcp(S[0]), n1 = b * fast_rcp(S[1]), n2 = c * fast_rcp(S[2]);
    const double n01 = n0 + n1;
    return n01 + n2;
}

GSF_HD int gate_popc(cov_mask m) { return __builtin_popcountll(m); }

// The run of rejected fixes immediately before lane j.  fix: lanes whose pose has a usable fix (before any rejection); rej: the rejected
// ones among them (settled below j); run_in: the run the chunk before ended with.  Poses without a fix neither count nor reset the run.
GSF_HD int gate_run_before(cov_mask fix, cov_mask rej, int j, int run_in)
{
    const cov_mask below = cov_bits(0, j - 1);
    const cov_mask applied = fix & ~rej & below;
    if (applied != 0ull) {
        const int a = 63 - __builtin_clzll(applied);                     // the last applied fix before j
        return gate_popc(rej & cov_bits(a + 1, j - 1));
    }
    return run_in + gate_popc(rej & below);
}

// State of the repair loop of one chunk.  Lanes below `from` are settled.
struct GateRepair {
    cov_mask rej;                      // rejected lanes so far
    cov_mask forced;                   // lanes applied by the forced-accept rule
    int from;
};
// One step.  over: the lanes that are tested, applied under g.rej and over the gate in the scan made under g.rej.  Settles the lowest
// such lane at or above g.from: a forced accept changes nothing a later lane has seen, so the step goes on to the next lane of `over`;
// a rejection invalidates every later lane of the scan, so the step ends.  Returns true when it added a rejection (scan again), false
// when `over` is exhausted (the chunk is settled).
GSF_HD bool gate_settle(GateRepair& g, cov_mask over, cov_mask fix, int run_in, int max_run)
{
    over &= ~cov_bits(0, g.from - 1) & fix & ~g.rej;
    while (over != 0ull) {
        const int j = __builtin_ctzll(over);
        g.from = j + 1;
        if (max_run > 0 && gate_run_before(fix, g.rej, j, run_in) >= max_run) {
            g.forced |= 1ull << j;
            over &= over - 1ull;
            continue;
        }
        g.rej |= 1ull << j;
        return true;
    }
    g.from = 64;
    return false;
}

// Exact counts of a track, carried from chunk to chunk.
struct GateCounts {
    int64_t n_avail, n_tested, n_rejected, n_forced, longest, first;     // first: index of the first rejected pose, -1: none
    int run;                                                             // rejected fixes at the end of the track so far
};
GSF_HD GateCounts gate_counts_init() { return GateCounts{ 0, 0, 0, 0, 0, -1, 0 }; }
// tested: lanes whose stamp lies beyond the arming time (any lanes; only those of `fix` count); c0: index of lane 0's pose
GSF_HD void gate_chunk_counts(GateCounts& c, cov_mask fix, cov_mask tested, cov_mask rej, cov_mask forced, int64_t c0)
{
    c.n_avail += gate_popc(fix);
    c.n_tested += gate_popc(fix & tested);
    c.n_rejected += gate_popc(rej);
    c.n_forced += gate_popc(forced);
    if (c.first < 0 && rej != 0ull) c.first = c0 + __builtin_ctzll(rej);
    if (rej == 0ull) {                                                   // every fix of the chunk was applied
        if (fix != 0ull) c.run = 0;
        return;
    }
    for (cov_mask m = fix; m != 0ull; m &= m - 1ull) {
        const int l = __builtin_ctzll(m);
        if ((rej >> l) & 1ull) { ++c.run; if (c.run > c.longest) c.longest = c.run; }
        else c.run = 0;
    }
}

}  // namespace gsf
