// TEST-ONLY host harness: compiles the GSF_HD helpers of gsf_cov_core.hpp (what gsf_ekf_cov.hip calls wave-uniformly) with g++, so that
// tests/test_cov_host.py can compare them with its per-pose restatement in the CPU-only tier.  Never shipped, never loaded by the package.
#include <cstdint>
#include "../gps_optimize_slam_amd/csrc/gsf_cov_core.hpp"

using namespace gsf;

extern "C" {

void hc_cov_smooth(const double* Pf_k, const double* Pp_b, const double* Pf_b, int64_t n, double* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = cov_smooth(Pf_k[i], Pp_b[i], Pf_b[i]);
}

uint64_t hc_bits(int lo, int hi) { return cov_bits(lo, hi); }

// One chunk, used the way the kernel uses the helpers: masks -> every recovery in lane order -> carry.  act must be lanes 0..L.
// sharp_raw: per-lane "the pair (lane-1, lane) exceeds the threshold", looked at only where the pair lies inside an outage.
// Returns the number of recoveries; rec_*[k] describe the k-th one.  prev_avail / ostart / seg_sharp: carried state, in and out.
int hc_chunk(uint64_t act, uint64_t av, int first_chunk, int64_t c0, uint64_t sharp_raw, int32_t* prev_avail, int64_t* ostart, int32_t* seg_sharp,
             uint64_t* masks, int32_t* rec_lane, int32_t* rec_start_lane, int64_t* rec_first, int32_t* rec_sharp)
{
    const OutageCarry in{ *prev_avail != 0, *ostart, *seg_sharp != 0 };
    const OutageMasks om = outage_masks(act, av, first_chunk != 0, in.prev_avail);
    const cov_mask f = sharp_raw & om.pair;
    masks[0] = om.start; masks[1] = om.rec; masks[2] = om.pair;
    int n = 0;
    for (cov_mask rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
        const int r = __builtin_ctzll(rm);
        const OutageSeg sg = outage_closed_at(om.start, f, r, c0, in.ostart, in.seg_sharp);
        rec_lane[n] = r; rec_start_lane[n] = sg.start_lane; rec_first[n] = sg.first; rec_sharp[n] = sg.sharp ? 1 : 0;
        ++n;
    }
    const int L = 63 - __builtin_clzll(act);
    const OutageCarry out = outage_carry(in, av & act, om.start, f, L, c0);
    *prev_avail = out.prev_avail ? 1 : 0; *ostart = out.ostart; *seg_sharp = out.seg_sharp ? 1 : 0;
    return n;
}
}
