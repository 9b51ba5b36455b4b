// host_harness_poly.cpp -- gsf_poly_core.hpp (the pre-filter's polynomial fit) compiled for the host, driven by tests/test_prefilter_fit_host.py.
//
// stdin:  P, then per problem:  form degree ms n nq | t[n] | y[n] | idx[ms] | tq[nq]      (doubles as C99 hex floats or decimals)
//         form 0: fit_subset_t<3,16,false> (scratch form)   1: fit_subset_regs<3,8>   2: fit_subset_regs<3,16>   3: fit_subset_t<8,64,true> (wide)
// The problem's first stamp t[0] is the origin of window-local time, as in the kernels: the fit gets t0 = t[0] and poly_predict gets tq - t0.
// stdout: "OK P", then per problem one line: 8 coefficients (zeros beyond the form's MAXD), the intercept, nq predictions -- hex floats.
// A problem outside its form's limits (degree, ms) or with an index outside [0, n) ends the program with status 2: nothing is dereferenced.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_poly_core.hpp"

using namespace gsf;

static bool read_d(double& v) { char buf[128]; if (scanf("%127s", buf) != 1) return false; char* e; v = strtod(buf, &e); return e != buf && *e == 0; }
static bool read_i(long& v) { return scanf("%ld", &v) == 1; }

template <int MAXD>
static void emit(const PolyModelT<MAXD>& m, int degree, const std::vector<double>& tq, double t0)
{
    for (int k = 0; k < 8; ++k) printf("%a ", k < MAXD ? m.coef[k] : 0.0);
    printf("%a", m.intercept);
    for (double q : tq) printf(" %a", poly_predict(m, degree, q - t0));
    printf("\n");
}

int main()
{
    long P;
    if (!read_i(P) || P < 0 || P > 100000) return 2;
    printf("OK %ld\n", P);
    for (long p = 0; p < P; ++p) {
        long form, degree, ms, n, nq;
        if (!read_i(form) || !read_i(degree) || !read_i(ms) || !read_i(n) || !read_i(nq)) return 2;
        const long maxd = form == 3 ? RPW_MAX_DEGREE : RP_MAX_DEGREE, maxs = form == 3 ? RPW_MAX_SAMPLES : (form == 1 ? 8 : RP_MAX_SAMPLES);
        if (form < 0 || form > 3 || degree < 1 || degree > maxd || ms < 1 || ms > maxs || n < 1 || n > 1000000 || nq < 0 || nq > 1000000) return 2;
        std::vector<double> t(n), y(n), tq(nq);
        std::vector<int32_t> idx(ms);
        for (auto& v : t) if (!read_d(v)) return 2;
        for (auto& v : y) if (!read_d(v)) return 2;
        for (auto& v : idx) { long i; if (!read_i(i) || i < 0 || i >= n) return 2; v = (int32_t)i; }
        for (auto& v : tq) if (!read_d(v)) return 2;
        const double t0 = t[0];
        const int d = (int)degree, m = (int)ms;
        if (form == 0) emit(fit_subset_t<RP_MAX_DEGREE, RP_MAX_SAMPLES, false>(t.data(), y.data(), idx.data(), m, d, 1, t0), d, tq, t0);
        else if (form == 1) emit(fit_subset_regs<RP_MAX_DEGREE, 8>(t.data(), y.data(), idx.data(), m, d, 1, t0), d, tq, t0);
        else if (form == 2) emit(fit_subset_regs<RP_MAX_DEGREE, RP_MAX_SAMPLES>(t.data(), y.data(), idx.data(), m, d, 1, t0), d, tq, t0);
        else emit(fit_subset_t<RPW_MAX_DEGREE, RPW_MAX_SAMPLES, true>(t.data(), y.data(), idx.data(), m, d, 1, t0), d, tq, t0);
    }
    return 0;
}
