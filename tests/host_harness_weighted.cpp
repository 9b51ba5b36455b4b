// TEST-ONLY host harness: compiles the GSF_HD rules of gsf_weighted_core.hpp (what gsf_smooth.hip and gsf_weighted.hip call per lane / per thread) with g++ as
// a STAND-ALONE PROGRAM, so that tests/test_weighted_host.py can run it plain and under -fsanitize=address,undefined and compare what it
// writes with tests/weighted_ref.py bit for bit.  Never shipped, never loaded by the package.
//
//   host_harness_weighted rows IN OUT      IN: int64 n; double rows[n][4] = { base (0 / 1), v0, v1, v2 }
//                                          OUT: int32 out[n][6] = { usable(v0), usable(v1), usable(v2), row kind, avail, bad }
//   host_harness_weighted bracket IN OUT   IN: int64 P, B, T, has_keep, has_valid; double ts[P]; int64 slam_offsets[B+1]; double gps_t[T];
//                                              int64 gps_offsets[B+1]; uint8 keep[T] (if has_keep); double fix_var[T][3]; uint8 valid[P] (if)
//                                          OUT: double pose_var[P][3]
// Every array lives in a heap block of exactly its size, and every log is copied into blocks of its own, so that the sanitizer sees any
// read outside [gps_offsets[b], gps_offsets[b+1]).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_weighted_core.hpp"

using namespace gsf;

template <class T>
static bool get(FILE* f, std::vector<T>& v, int64_t n)
{
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

static int run_rows(FILE* in, FILE* out)
{
    int64_t n = 0;
    if (fread(&n, 8, 1, in) != 1 || n < 0) return 2;
    std::vector<double> rows;
    if (!get(in, rows, n * 4)) return 2;
    std::vector<int32_t> o((size_t)n * 6);
    for (int64_t i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * 4];
        const WeightedAvail wa = weighted_avail(r[0] != 0.0, r[1], r[2], r[3]);
        int32_t* q = &o[(size_t)i * 6];
        q[0] = wvar_usable(r[1]); q[1] = wvar_usable(r[2]); q[2] = wvar_usable(r[3]);
        q[3] = wvar_row(r[1], r[2], r[3]); q[4] = wa.avail; q[5] = wa.bad;
    }
    return (n == 0 || fwrite(o.data(), 4, o.size(), out) == o.size()) ? 0 : 3;
}

static int run_bracket(FILE* in, FILE* out)
{
    int64_t h[5];
    if (fread(h, 8, 5, in) != 5) return 2;
    const int64_t P = h[0], B = h[1], T = h[2];
    const bool has_keep = h[3] != 0, has_valid = h[4] != 0;
    if (P < 0 || B < 1 || T < 0) return 2;
    std::vector<double> ts, gps_t, fix_var;
    std::vector<int64_t> so, go;
    std::vector<uint8_t> keep, valid;
    if (!get(in, ts, P) || !get(in, so, B + 1) || !get(in, gps_t, T) || !get(in, go, B + 1)) return 2;
    if (has_keep && !get(in, keep, T)) return 2;
    if (!get(in, fix_var, T * 3)) return 2;
    if (has_valid && !get(in, valid, P)) return 2;
    std::vector<double> pv((size_t)P * 3);
    const double inf = __builtin_huge_val();
    for (int64_t i = 0; i < P; ++i) {                                    // what one thread of fix_var_at_poses_kernel does
        Vec3 v{ inf, inf, inf };
        if (!has_valid || valid[(size_t)i] != 0) {
            int64_t b = query_count_le(so.data(), B + 1, i) - 1;
            b = b < 0 ? 0 : (b > B - 1 ? B - 1 : b);
            const int64_t g0 = go[(size_t)b], n = go[(size_t)b + 1] - g0;
            // the log in blocks of its own
            std::vector<double> lt(gps_t.begin() + g0, gps_t.begin() + g0 + n), lv(fix_var.begin() + g0 * 3, fix_var.begin() + (g0 + n) * 3);
            std::vector<uint8_t> lk;
            if (has_keep) lk.assign(keep.begin() + g0, keep.begin() + g0 + n);
            v = fix_var_bracket((const double*)lt.data(), has_keep ? (const uint8_t*)lk.data() : (const uint8_t*)nullptr, (const double*)lv.data(), n,
                                ts[(size_t)i]);
        }
        pv[(size_t)i * 3] = v.x; pv[(size_t)i * 3 + 1] = v.y; pv[(size_t)i * 3 + 2] = v.z;
    }
    return (P == 0 || fwrite(pv.data(), 8, pv.size(), out) == pv.size()) ? 0 : 3;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s rows|bracket IN OUT\n", argv[0]); return 1; }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 1; }
    const int rc = !strcmp(argv[1], "rows") ? run_rows(in, out) : !strcmp(argv[1], "bracket") ? run_bracket(in, out) : 1;
    fclose(in);
    return fclose(out) == 0 ? rc : 3;
}
