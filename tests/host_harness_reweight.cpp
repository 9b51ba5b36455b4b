// TEST-ONLY host harness: compiles the GSF_HD rules of gsf_reweight_core.hpp (what ekf_smooth_kernel<SMOOTH_REWEIGHTED> of gsf_smooth.hip
// calls per lane) with g++ as a STAND-ALONE PROGRAM, so that tests/test_reweight_host.py can run it plain and under
// -fsanitize=address,undefined and compare what it writes with tests/reweight_ref.py bit for bit.  Never shipped, never loaded by the package.
//
//   host_harness_reweight weights IN OUT   IN: int64 n; double rows[n][3] = { loss (0 / 1), c2, u2 }            OUT: double w[n]
//   host_harness_reweight vars IN OUT      IN: int64 n; double rows[n][2] = { v, w }                            OUT: double r_eff[n]
//   host_harness_reweight rows IN OUT      IN: int64 n; double rows[n][14] = { loss, c2, zr[3], xr[3], e[3], v[3] }
//                                          OUT: double out[n][5] = { res0, res1, res2, u2, w }
//   host_harness_reweight fixed IN OUT     IN: int64 n; double rows[n][2] = { w_new, w_used }                   OUT: int32 same[n]
//   host_harness_reweight args IN OUT      IN: int64 n; double rows[n][3] = { loss, c2, rounds }                OUT: int32 ok[n]
// Every array lives in a heap block of exactly its size.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_reweight_core.hpp"

using namespace gsf;

static bool get_rows(FILE* f, std::vector<double>& v, int64_t& n, int width)
{
    if (fread(&n, 8, 1, f) != 1 || n < 0) return false;
    v.resize((size_t)n * (size_t)width);
    return v.empty() || fread(v.data(), 8, v.size(), f) == v.size();
}

template <class T>
static int put(FILE* f, const std::vector<T>& o) { return (o.empty() || fwrite(o.data(), sizeof(T), o.size(), f) == o.size()) ? 0 : 3; }

static int run(const char* mode, FILE* in, FILE* out)
{
    std::vector<double> r;
    int64_t n = 0;
    if (!strcmp(mode, "weights")) {
        if (!get_rows(in, r, n, 3)) return 2;
        std::vector<double> o((size_t)n);
        for (int64_t i = 0; i < n; ++i) o[(size_t)i] = reweight_weight((int32_t)r[(size_t)i * 3], r[(size_t)i * 3 + 2], r[(size_t)i * 3 + 1]);
        return put(out, o);
    }
    if (!strcmp(mode, "vars")) {
        if (!get_rows(in, r, n, 2)) return 2;
        std::vector<double> o((size_t)n);
        for (int64_t i = 0; i < n; ++i) o[(size_t)i] = reweight_var(r[(size_t)i * 2], r[(size_t)i * 2 + 1]);
        return put(out, o);
    }
    if (!strcmp(mode, "rows")) {
        if (!get_rows(in, r, n, 14)) return 2;
        std::vector<double> o((size_t)n * 5);
        for (int64_t i = 0; i < n; ++i) {
            const double* q = &r[(size_t)i * 14];
            double* p = &o[(size_t)i * 5];
            for (int c = 0; c < 3; ++c) p[c] = reweight_residual(q[2 + c], q[5 + c], q[8 + c]);
            p[3] = reweight_u2(p[0], p[1], p[2], q[11], q[12], q[13]);
            p[4] = reweight_weight((int32_t)q[0], p[3], q[1]);
        }
        return put(out, o);
    }
    if (!strcmp(mode, "fixed")) {
        if (!get_rows(in, r, n, 2)) return 2;
        std::vector<int32_t> o((size_t)n);
        for (int64_t i = 0; i < n; ++i) o[(size_t)i] = reweight_same_bits(r[(size_t)i * 2], r[(size_t)i * 2 + 1]);
        return put(out, o);
    }
    if (!strcmp(mode, "args")) {
        if (!get_rows(in, r, n, 3)) return 2;
        std::vector<int32_t> o((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const double l = r[(size_t)i * 3], k = r[(size_t)i * 3 + 2];                                   // (both small integers in the test)
            o[(size_t)i] = reweight_args_ok((int32_t)l, r[(size_t)i * 3 + 1], (int32_t)k);
        }
        return put(out, o);
    }
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s weights|vars|rows|fixed|args IN OUT\n", argv[0]); return 1; }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 1; }
    const int rc = run(argv[1], in, out);
    fclose(in);
    return fclose(out) == 0 ? rc : 3;
}
