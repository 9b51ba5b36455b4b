// TEST-ONLY stand-alone program: compiles the GSF_HD helpers of gsf_sweep_core.hpp (what gsf_noise_sweep.hip evaluates per lane) with g++
// and checks them against plain per-pose loops -- the affine composition the kernel scans across lanes, a chunk's twelve sums, and the
// carry from one 64-pose chunk to the next for tracks of 63, 64 and 65 poses (and 129: two boundaries).  tests/test_noise_sweep_host.py
// builds and runs it, once more under -fsanitize=address,undefined.  Exit status 0 and a line "OK ..." when everything agrees.
// Never shipped, never loaded by the package.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_sweep_core.hpp"

using namespace gsf;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni()                                                       // [0, 1)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
static double rel(double a, double b) { const double d = std::fabs(a - b), m = std::fmax(std::fabs(a), std::fabs(b)); return m > 0.0 ? d / std::fmax(m, 1e-300) : 0.0; }

struct Track {
    int n;
    std::vector<char> avail, counted;
    std::vector<double> wg, S;           // [n][3]: w g and S per axis
    std::vector<double> d, z;            // [n][3]
};
static Track make_track(int n)
{
    Track t; t.n = n;
    t.avail.assign(n, 0); t.counted.assign(n, 0);
    t.wg.assign(3 * n, 0.0); t.S.assign(3 * n, 1.0); t.d.assign(3 * n, 0.0); t.z.assign(3 * n, 0.0);
    for (int i = 1; i < n; ++i) {
        t.avail[i] = uni() < 0.8;
        t.counted[i] = t.avail[i] && i > 4;
        for (int c = 0; c < 3; ++c) {
            t.wg[3 * i + c] = (uni() < 0.1 ? 0.2 : 1.0) * (0.05 + 0.9 * uni());
            t.S[3 * i + c] = std::pow(10.0, -3.0 + 6.0 * uni());
            t.d[3 * i + c] = uni() - 0.3;
            t.z[3 * i + c] = 0.7 * i + 3.0 * (uni() - 0.5);
        }
    }
    return t;
}

// the per-pose loop: positions and the twelve sums of a whole track, written without the header
static void serial(const Track& t, double* x_end, double* sums)
{
    double x[3] = { 0.0, 0.0, 0.0 }, nu_prev[3] = { 0.0, 0.0, 0.0 };
    bool counted_prev = false;
    for (int j = 0; j < 12; ++j) sums[j] = 0.0;
    for (int i = 1; i < t.n; ++i) {
        double nu[3] = { 0.0, 0.0, 0.0 };
        for (int c = 0; c < 3; ++c) {
            const double pm = x[c] + t.d[3 * i + c];
            if (t.avail[i]) {
                const double y = t.z[3 * i + c] - pm, S = t.S[3 * i + c];
                x[c] = pm + t.wg[3 * i + c] * y;
                if (t.counted[i]) {
                    sums[1 + c] += y * y / S; sums[4 + c] += std::log(S); sums[7 + c] += y * y;
                    nu[c] = y / std::sqrt(S);
                    if (counted_prev) sums[10] += nu[c] * nu_prev[c];
                }
            } else x[c] = pm;
        }
        if (t.counted[i]) { sums[0] += 1.0; if (counted_prev) sums[11] += 1.0; }
        for (int c = 0; c < 3; ++c) nu_prev[c] = nu[c];
        counted_prev = t.counted[i];
    }
    for (int c = 0; c < 3; ++c) x_end[c] = x[c];
}

// the kernel's way: chunks of 64 poses, a six-stage inclusive scan of the pose maps (the lanes' DPP stages as array shifts), the carry
// applied afterwards, the terms of every pose summed per chunk, the carry handed on
static void chunked(const Track& t, double* x_end, double* sums)
{
    double cx[3] = { 0.0, 0.0, 0.0 }, cnu[3] = { 0.0, 0.0, 0.0 };
    bool c_counted = false;
    for (int j = 0; j < 12; ++j) sums[j] = 0.0;
    for (int c0 = 0; c0 < t.n; c0 += 64) {
        const int L = t.n - c0 < 64 ? t.n - c0 - 1 : 63;
        Affine m[3][64];
        double x[3][64], y[64][3], S[64][3], nu[64][3];
        for (int c = 0; c < 3; ++c) {
            for (int l = 0; l < 64; ++l) {
                const int i = c0 + l;
                const bool stepping = i < t.n && i != 0;
                m[c][l] = stepping ? sweep_affine(t.avail[i] != 0, t.wg[3 * i + c], t.d[3 * i + c], t.z[3 * i + c]) : Affine{ 1.0, 0.0 };
            }
            for (int off = 1; off < 64; off <<= 1) {
                Affine nx[64];
                for (int l = 0; l < 64; ++l) nx[l] = l >= off ? affine_compose(m[c][l], m[c][l - off]) : affine_compose(m[c][l], Affine{ 1.0, 0.0 });
                for (int l = 0; l < 64; ++l) m[c][l] = nx[l];
            }
            for (int l = 0; l < 64; ++l) x[c][l] = affine_apply(m[c][l], cx[c]);
        }
        for (int l = 0; l <= L; ++l) {
            const int i = c0 + l;
            for (int c = 0; c < 3; ++c) {
                const double pm = (l == 0 ? cx[c] : x[c][l - 1]) + t.d[3 * i + c];
                y[l][c] = t.z[3 * i + c] - pm; S[l][c] = t.S[3 * i + c];
            }
            sweep_pose_nu(y[l], S[l], t.counted[i] != 0, nu[l]);
        }
        for (int l = 0; l <= L; ++l) {
            const int i = c0 + l;
            double term[SWEEP_NSTAT];
            const bool cprev = l == 0 ? c_counted : t.counted[i - 1] != 0;
            sweep_pose_terms(y[l], S[l], nu[l], l == 0 ? cnu : nu[l - 1], t.counted[i] != 0, cprev, term);
            for (int j = 0; j < SWEEP_NSTAT; ++j) sums[j] += term[j];
        }
        for (int c = 0; c < 3; ++c) { cx[c] = x[c][L]; cnu[c] = nu[L][c]; }
        c_counted = t.counted[c0 + L] != 0;
    }
    for (int c = 0; c < 3; ++c) x_end[c] = cx[c];
}

int main()
{
    double worst_x = 0.0, worst_s = 0.0;
    int bad = 0;
    const int lengths[] = { 1, 2, 3, 63, 64, 65, 129 };
    for (int rep = 0; rep < 50; ++rep) {
        for (int n : lengths) {
            const Track t = make_track(n);
            double xs[3], xc[3], ss[12], sc[12];
            serial(t, xs, ss); chunked(t, xc, sc);
            for (int c = 0; c < 3; ++c) { const double e = std::fabs(xs[c] - xc[c]); worst_x = std::fmax(worst_x, e); if (!(e < 1e-9)) ++bad; }
            for (int j = 0; j < 12; ++j) {
                const bool count = j == 0 || j == 11;
                const double e = count ? std::fabs(ss[j] - sc[j]) : std::fabs(ss[j] - sc[j]) / std::fmax(1.0, std::fabs(ss[j]));
                if (!count) worst_s = std::fmax(worst_s, e);
                if (count ? e != 0.0 : !(e < 1e-11)) { ++bad; std::printf("n=%d sum %d: %.17g vs %.17g\n", n, j, ss[j], sc[j]); }
            }
        }
    }
    // the figures of a row and the pick order
    const double row[12] = { 10, 9.0, 11.0, 10.5, -3.0, -2.0, 4.0, 1, 1, 1, 0.5, 9 };
    const double nll = 0.5 * (30.0 * std::log(2.0 * M_PI) + (-1.0) + 30.5);
    if (!(rel(sweep_nll(row), nll) < 1e-14) || !(rel(sweep_mean_nis(row), 3.05) < 1e-15)) { ++bad; std::printf("nll / mean_nis\n"); }
    double nanrow[12]; for (int j = 0; j < 12; ++j) nanrow[j] = row[j];
    nanrow[5] = std::nan("");
    if (sweep_row_finite(nanrow) || !sweep_row_finite(row) || sweep_score(nanrow, 0) != HUGE_VAL || sweep_score(nanrow, 1) != HUGE_VAL) { ++bad; std::printf("finite\n"); }
    if (!sweep_pick_before(1.0, 5, 2.0, 1) || sweep_pick_before(2.0, 0, 1.0, 5) || !sweep_pick_before(1.0, 2, 1.0, 3) || sweep_pick_before(1.0, 3, 1.0, 2)) { ++bad; std::printf("pick order\n"); }
    if (bad) { std::printf("FAILED: %d\n", bad); return 1; }
    std::printf("OK worst position %.3e m, worst sum %.3e relative\n", worst_x, worst_s);
    return 0;
}
