// host_harness_lever.cpp -- gsf_lever_core.hpp (antenna lever arm) compiled with g++ and driven as gsf_lever.hip drives it, with a plain loop
// over the rows where the kernel has lanes and DPP sums.  Reads a case file (argv[1], written by tests/test_lever_host.py), prints what the
// header decides and computes with hexadecimal floats, and the test compares the lines with the NumPy restatement of tests/lever_ref.py.
//
// File:  B  sigma_fix sigma_prior[3] sigma_rot ratio_max pivot_min weak_ratio conv_tol  min_rows iters fit_scale fit_rotation
//        per track:  n run_status  R[9] t[3] s l0[3]  l_fed[3] sign_fed,  n rows (pos[3] quat[4] gps[3] valid)
// Lines: F b flags n_rows n_bad_quat first  R[9] t[3] s l[3] l_cov[9] rms_before rms_after last_step     the fit (lev_fit_track)
//        A b i flag out[3]                                                                                 the apply under (R, l_fed, sign_fed)
//        Z b i flag out[3]                                                                                 the apply under l = 0
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gps_optimize_slam_amd/csrc/gsf_lever_core.hpp"

using namespace gsf;

static double rd(FILE* f)
{
    char tok[64];
    if (fscanf(f, "%63s", tok) != 1) { fprintf(stderr, "short file\n"); exit(2); }
    return strtod(tok, nullptr);                                            // (hexadecimal floats, nan, inf)
}
static long ri(FILE* f) { long v; if (fscanf(f, "%ld", &v) != 1) { fprintf(stderr, "short file\n"); exit(2); } return v; }

struct HostPass {
    const std::vector<double>&pos, &quat, &gps; const std::vector<uint8_t>& valid; long n; int64_t first;
    int kind(long i, Quat& qn) const { return lev_row_kind(valid[i], &pos[3 * i], &quat[4 * i], &gps[3 * i], qn); }
    void scan(int64_t& first_out, int32_t& nr, int32_t& nb)
    {
        first = -1; nr = 0; nb = 0;
        for (long i = 0; i < n; ++i) {
            Quat qn;
            const int k = kind(i, qn);
            if (k == 0) { if (first < 0) first = i; ++nr; }
            if (k == 1) ++nb;
        }
        first_out = first;
    }
    void shift(double* pf, double* gf) const { for (int c = 0; c < 3; ++c) { pf[c] = pos[3 * first + c]; gf[c] = gps[3 * first + c]; } }
    void sums(const LevState& x, const double* pf, const double* gf, LevSums& S) const
    {
        lev_sums_zero(S);
        for (long i = first; i < n; ++i) {
            Quat qn;
            if (kind(i, qn) == 0) lev_add_row(S, x, pf, gf, &pos[3 * i], &gps[3 * i], qn);
        }
    }
};

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const long B = ri(f);
    LevRule rule;
    rule.sigma_fix = rd(f);
    for (int c = 0; c < 3; ++c) rule.sigma_prior[c] = rd(f);
    rule.sigma_rot = rd(f); rule.ratio_max = rd(f); rule.pivot_min = rd(f); rule.weak_ratio = rd(f); rule.conv_tol = rd(f);
    rule.min_rows = (int32_t)ri(f); rule.iters = (int32_t)ri(f); rule.fit_scale = (int32_t)ri(f); rule.fit_rotation = (int32_t)ri(f);
    for (long b = 0; b < B; ++b) {
        const long n = ri(f); const int32_t run_status = (int32_t)ri(f);
        double R[9], t[3], s, l0[3], lfed[3], sign;
        for (int c = 0; c < 9; ++c) R[c] = rd(f);
        for (int c = 0; c < 3; ++c) t[c] = rd(f);
        s = rd(f);
        for (int c = 0; c < 3; ++c) l0[c] = rd(f);
        for (int c = 0; c < 3; ++c) lfed[c] = rd(f);
        sign = rd(f);
        std::vector<double> pos(3 * n + 1), quat(4 * n + 1), gps(3 * n + 1);
        std::vector<uint8_t> valid(n + 1);
        for (long i = 0; i < n; ++i) {
            for (int c = 0; c < 3; ++c) pos[3 * i + c] = rd(f);
            for (int c = 0; c < 4; ++c) quat[4 * i + c] = rd(f);
            for (int c = 0; c < 3; ++c) gps[3 * i + c] = rd(f);
            valid[i] = (uint8_t)ri(f);
        }
        HostPass pass{ pos, quat, gps, valid, n, -1 };
        LevOut o;
        lev_fit_track(pass, rule, R, t, s, l0, run_status, o);
        printf("F %ld %d %d %d %lld", b, o.flags, o.n_rows, o.n_bad_quat, (long long)pass.first);
        for (int c = 0; c < 9; ++c) printf(" %a", o.R[c]);
        for (int c = 0; c < 3; ++c) printf(" %a", o.t[c]);
        printf(" %a", o.s);
        for (int c = 0; c < 3; ++c) printf(" %a", o.l[c]);
        for (int c = 0; c < 9; ++c) printf(" %a", o.lcov[c]);
        printf(" %a %a %a\n", o.rms_before, o.rms_after, o.last_step);
        const double zero[3] = { 0.0, 0.0, 0.0 };
        for (long i = 0; i < n; ++i) {
            double out[3];
            int32_t fl = lev_apply_row(R, lfed, sign, &quat[4 * i], &gps[3 * i], out);
            printf("A %ld %ld %d %a %a %a\n", b, i, fl, out[0], out[1], out[2]);
            fl = lev_apply_row(R, zero, -sign, &quat[4 * i], &gps[3 * i], out);
            printf("Z %ld %ld %d %a %a %a\n", b, i, fl, out[0], out[1], out[2]);
        }
    }
    fclose(f);
    printf("OK\n");
    return 0;
}
