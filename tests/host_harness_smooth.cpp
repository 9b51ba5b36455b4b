// TEST-ONLY host harness: compiles the GSF_HD helpers of gsf_smooth_core.hpp (what pass 2 of gsf_smooth.hip calls per lane) with g++ and
// drives them the way the kernel does -- 64 rows per chunk from the track's last chunk down, scan lane j = row c0 + 63 - j, the tag bits
// through the parked values, the carries of the chunk above -- so that tests/test_smooth_host.py can compare whole tracks with its per-pose
// restatement in the CPU-only tier.  The wave's prefix scan is a plain loop over the scan lanes here.  Never shipped, never loaded by the
// package.
#include <cstdint>
#include "../gps_optimize_slam_amd/csrc/gsf_smooth_core.hpp"

using namespace gsf;

extern "C" {

// tag round trip: out[i] = the untagged value, bit[i] = the tag read back
void hs_tags(const double* v, const uint8_t* bit, int64_t n, double* tagged, double* out, uint8_t* back)
{
    for (int64_t i = 0; i < n; ++i) { tagged[i] = smooth_tag(v[i], bit[i] != 0); out[i] = smooth_untag(tagged[i]); back[i] = smooth_tag_of(tagged[i]) ? 1 : 0; }
}

double hs_gain(double Pf_k, double Pp_next, int linked) { return smooth_gain(Pf_k, Pp_next, linked != 0); }

// The backward pass of one track.  ts[N]; Pf[N][3] the filtered variances; g[N][3] the applied corrections; fix[N] / start[N] the two tag
// bits; Q[3].  Out: e[N][3], d[N][3] (0 where no later fix of the row's span reaches it), reached[N].
void hs_backward(int64_t N, const double* ts, const double* Pf, const double* g, const uint8_t* fix, const uint8_t* start, const double* Q,
                 double* e, double* d, uint8_t* reached)
{
    if (N <= 0) return;
    double c_e[3] = { 0, 0, 0 }, c_d[3] = { 0, 0, 0 }, c_g[3] = { 0, 0, 0 }, c_Pf[3] = { 0, 0, 0 }, c_t = 0.0;
    bool c_fix = false, c_start = true, c_reach = false;
    for (int64_t c0 = ((N - 1) >> 6) << 6; c0 >= 0; c0 -= 64) {
        // what pass 1 parked, through the tags, in scan order (lanes without a row: zeros, no bits)
        double lPf[64][3], lg[64][3], lt[64];
        cov_mask fix_m = 0ull, start_m = 0ull;
        for (int j = 0; j < 64; ++j) {
            const int64_t k = c0 + 63 - j;
            const bool act = k < N;
            const int64_t kl = act ? k : N - 1;
            const double p0 = smooth_tag(Pf[kl * 3], fix[kl] != 0), s6 = smooth_tag(1.0 + (double)kl, start[kl] != 0);
            if (act && smooth_tag_of(p0)) fix_m |= 1ull << j;
            if (act && smooth_tag_of(s6)) start_m |= 1ull << j;
            lt[j] = ts[kl];
            for (int c = 0; c < 3; ++c) { lPf[j][c] = act ? (c == 0 ? smooth_untag(p0) : Pf[kl * 3 + c]) : 0.0; lg[j][c] = act ? g[kl * 3 + c] : 0.0; }
        }
        const cov_mask fixn_m = (fix_m << 1) | (c_fix ? 1ull : 0ull), startn_m = (start_m << 1) | (c_start ? 1ull : 0ull);
        Affine pe[3] = { { 1, 0 }, { 1, 0 }, { 1, 0 } }, pd[3] = { { 1, 0 }, { 1, 0 }, { 1, 0 } };      // prefix compositions over the scan lanes
        cov_mask reach_m = 0ull;
        double le[64][3], ld[64][3];
        for (int j = 0; j < 64; ++j) {
            const int64_t k = c0 + 63 - j;
            const bool act = k < N;
            const bool fix_n = (fixn_m >> j) & 1ull, start_n = (startn_m >> j) & 1ull;
            const bool linked = act && k != N - 1 && !start_n;
            const double t_n = j ? lt[j - 1] : c_t;
            const double dt_n = fmax(1e-6, t_n - lt[j]);
            for (int c = 0; c < 3; ++c) {
                const double Pf_n = j ? lPf[j - 1][c] : c_Pf[c], g_n = j ? lg[j - 1][c] : c_g[c];
                const double Pp_n = smooth_pred(lPf[j][c], Q[c], dt_n);
                const double A = smooth_gain(lPf[j][c], Pp_n, linked);
                pe[c] = affine_compose(smooth_map_e(A, g_n), pe[c]);
                pd[c] = affine_compose(smooth_map_d(A, Pf_n, Pp_n, fix_n), pd[c]);
                le[j][c] = affine_apply(pe[c], c_e[c]); ld[j][c] = affine_apply(pd[c], c_d[c]);
            }
            const bool r = act && smooth_row_reached(fix_m, start_m, j, c_reach);
            if (r) reach_m |= 1ull << j;
            if (act) {
                reached[k] = r ? 1 : 0;
                for (int c = 0; c < 3; ++c) { e[k * 3 + c] = r ? le[j][c] : 0.0; d[k * 3 + c] = r ? ld[j][c] : 0.0; }
            }
        }
        const bool r63 = (reach_m >> 63) != 0ull;
        c_reach = smooth_reach_carry(fix_m, start_m, r63);
        c_fix = (fix_m >> 63) != 0ull; c_start = (start_m >> 63) != 0ull;
        for (int c = 0; c < 3; ++c) { c_e[c] = r63 ? le[63][c] : 0.0; c_d[c] = r63 ? ld[63][c] : 0.0; c_g[c] = lg[63][c]; c_Pf[c] = lPf[63][c]; }
        c_t = lt[63];
    }
}
}
