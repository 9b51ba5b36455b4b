// Test-only host build of gps_optimize_slam_amd/csrc/gsf_rows_rule.hpp (the Sim3 row choice as decisions on lane masks), compiled with
// g++ by tests/test_rows_rule_host.py.  The lane masks are formed here as the kernel's lanes form them (gsf_ekf_wave_early.hip, step 2b):
// lane l of chunk k holds row min(64 k + l, N - 1), the stamp in front of lane 0 is lane 63 of the chunk before.
// With -DROWS_RULE_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): random and edge tracks against a plain
// restatement of the rule on index lists; exit status 0 when every case agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_rows_rule.hpp"

namespace {
constexpr int R = 6;

// info: rows_flag, nT, row_end, nF, dep_end, first valid row (-1: none), stamps fetched one by one
void choose(const double* ts, const uint8_t* valid, const int N, const int ms, const double max_gap, const double max_dur, uint8_t* rows, int32_t* info)
{
    gsf::rows_u64 m[R], graw[R], le[R];
    double pt[R][64];
    for (int k = 0; k < R; ++k) {
        m[k] = 0ull;
        for (int l = 0; l < 64; ++l) {
            const int i = 64 * k + l;
            pt[k][l] = 64 * k < N ? ts[i < N ? i : N - 1] : 0.0;            // (chunks past the end of the track hold zeros)
            if (i < N && valid[i]) m[k] |= 1ull << l;
        }
    }
    int k0, l0;
    const bool any = gsf::rows_first_valid<R>(m, k0, l0);
    const double tlim = any ? pt[k0][l0] + max_dur : 0.0;
    double tb = 0.0;
    for (int k = 0; k < R; ++k) {
        graw[k] = le[k] = 0ull;
        for (int l = 0; l < 64; ++l) {
            const double tp = l > 0 ? pt[k][l - 1] : tb;
            if (pt[k][l] - tp > max_gap) graw[k] |= 1ull << l;
            if (pt[k][l] <= tlim) le[k] |= 1ull << l;
        }
        tb = pt[k][63];
    }
    int fetched = 0;
    gsf::RowsChoice<R> c;
    gsf::rows_rule_choose<R>(m, graw, le, N, ms, max_gap, [&](int i) { ++fetched; if (i < 0 || i >= N) abort(); return ts[i]; }, c);
    for (int i = 0; i < N; ++i) rows[i] = (uint8_t)((c.mo[i / 64] >> (i % 64)) & 1ull);
    for (int k = (N + 63) / 64; k < R; ++k) if (c.mo[k] != 0ull) abort();   // nothing past the end of the track
    info[0] = c.rows_flag; info[1] = c.nT; info[2] = c.row_end; info[3] = c.nF; info[4] = c.dep_end; info[5] = any ? 64 * k0 + l0 : -1; info[6] = fetched;
}
}  // namespace

extern "C" {
int rr_chunks() { return R; }
void rr_flags(int32_t* f) { f[0] = gsf::SIM3_FLAG_FEW_ROWS; f[1] = gsf::SIM3_FLAG_ROWS_ALL; f[2] = gsf::SIM3_FLAG_ROWS_SEGMENT; }
// n tracks, track c = rows off[c] .. off[c + 1] of ts / valid / rows; info holds eight int32 per track
void rr_choose(const double* ts, const uint8_t* valid, const int64_t* off, const int64_t n, const int ms, const double max_gap, const double max_dur,
               uint8_t* rows, int32_t* info)
{
    for (int64_t c = 0; c < n; ++c) choose(ts + off[c], valid + off[c], (int)(off[c + 1] - off[c]), ms, max_gap, max_dur, rows + off[c], info + 8 * c);
}
}

#ifdef ROWS_RULE_MAIN
namespace {
// the rule on index lists (main_process_gui :973-998): rows chosen, or flag FEW_ROWS
int32_t plain(const std::vector<double>& ts, const std::vector<uint8_t>& valid, const int ms, const double max_gap, const double max_dur, std::vector<uint8_t>& rows)
{
    const int N = (int)ts.size();
    rows.assign(N, 0);
    std::vector<int> V;
    for (int i = 0; i < N; ++i) if (valid[i]) V.push_back(i);
    if ((int)V.size() < ms) return gsf::SIM3_FLAG_FEW_ROWS;
    int end = (int)V.size();
    for (int k = 0; k + 1 < (int)V.size(); ++k) if (ts[V[k + 1]] - ts[V[k]] > max_gap) { end = k; break; }
    if (end < ms) { for (int i : V) rows[i] = 1; return gsf::SIM3_FLAG_ROWS_ALL; }
    const double tlim = ts[V[0]] + max_dur;
    int nt = 0;
    for (int k = 0; k < end; ++k) if (ts[V[k]] <= tlim) ++nt;
    if (nt < ms) { for (int k = 0; k < end; ++k) rows[V[k]] = 1; return gsf::SIM3_FLAG_ROWS_SEGMENT; }
    for (int k = 0; k < end; ++k) if (ts[V[k]] <= tlim) rows[V[k]] = 1;
    return 0;
}
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
}  // namespace

int main()
{
    int bad = 0, cases = 0;
    for (int it = 0; it < 4000; ++it) {
        const int N = 65 + (int)(rnd() % 320), ms = 1 + (int)(rnd() % 8);
        std::vector<double> ts(N); std::vector<uint8_t> valid(N, 1), rows(N), want;
        double t = 1000.0;
        const int gaps = (int)(rnd() % 3), holes = (int)(rnd() % 4);
        for (int i = 0; i < N; ++i) { t += (rnd() % 16 == 0) ? 0.0 : 0.1; ts[i] = t; }
        for (int g = 0; g < gaps; ++g) { const int at = 1 + (int)(rnd() % (N - 1)); for (int i = at; i < N; ++i) ts[i] += 5.0 + (rnd() % 2) * 0.5; }
        for (int h = 0; h < holes; ++h) { const int at = (int)(rnd() % N), len = 1 + (int)(rnd() % 70); for (int i = at; i < N && i < at + len; ++i) valid[i] = 0; }
        if (it % 7 == 0) for (int i = 0; i < N; ++i) if (rnd() % 3) valid[i] = 0;
        const double max_dur = (it % 3 == 0) ? 6.0 + (rnd() % 20) : 180.0;
        int32_t info[8] = { 0 };
        choose(ts.data(), valid.data(), N, ms, 5.0, max_dur, rows.data(), info);
        const int32_t flag = plain(ts, valid, ms, 5.0, max_dur, want);
        ++cases;
        bool same = flag == info[0];
        if (same && flag != gsf::SIM3_FLAG_FEW_ROWS) { int n = 0; for (int i = 0; i < N; ++i) { same = same && rows[i] == want[i]; n += want[i]; } same = same && n == info[1]; }
        if (!same) { if (bad < 5) fprintf(stderr, "case %d (N = %d, min_samples = %d): flag %d, expected %d\n", it, N, ms, info[0], flag); ++bad; }
    }
    printf("%d cases, %d differ\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
