// TEST-ONLY stand-alone program: compiles the GSF_HD helpers of gsf_gate_core.hpp (what gsf_gate.hip evaluates wave-uniformly per chunk)
// with g++ and drives the speculate-and-repair loop over lane arrays exactly as the kernel does -- scan the chunk under the current
// rejection mask, ballot the lanes over the gate, gate_settle(), scan again -- against a plain per-pose loop that takes every decision
// when its pose is reached.  The NIS of a pose is PLANTED as a function of what the gated run did before it (the number of poses since
// the last applied fix scales it), so a rejection really does change what later lanes see and a scan under a stale mask is wrong.
//  * all 2^10 availability patterns of a 10-pose track x 12 planted NIS rows x max_run in {0, 1, 2} x arming at pose 0 / 3, in chunks of
//    64, 4 and 3 lanes (the narrow chunks put every carry -- the run count, the outage state, the gap -- across a boundary);
//  * the rejected set, the forced accepts, n_avail / n_tested / n_rejected / n_forced, the longest run, the first rejected pose and the
//    outage a recovery closes (gsf_cov_core.hpp fed with the availability minus the rejections) must be EXACT.
// tests/test_innovation_gate_host.py builds and runs it, once more under -fsanitize=address,undefined.  Exit status 0 and a line "OK ..."
// when everything agrees.  Never shipped, never loaded by the package.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_gate_core.hpp"

using namespace gsf;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni()                                                       // [0, 1)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

struct Run {
    std::vector<char> rej, forced;
    std::vector<int> ostart;            // per pose: first pose of the outage a recovery at this pose closes, -1: no recovery here
    long n_avail, n_tested, n_rej, n_forced, longest, first;
};

// NIS of pose i when `gap` poses have passed since the last applied fix (pose 0 counts as one)
static double planted_nis(const std::vector<double>& base, int i, int gap) { return base[i] * (double)gap; }

// ---- the definition: one pose after the other
static Run per_pose(int n, const std::vector<char>& raw0, const std::vector<char>& fix, const std::vector<double>& base, double gate,
                    int arm, int max_run)
{
    Run r; r.rej.assign(n, 0); r.forced.assign(n, 0); r.ostart.assign(n, -1);
    r.n_avail = r.n_tested = r.n_rej = r.n_forced = r.longest = 0; r.first = -1;
    int gap = 0, run = 0;
    bool in_outage = !raw0[0]; int start = 0;
    for (int i = 1; i < n; ++i) {
        ++gap;
        bool av = fix[i];
        if (av) {
            ++r.n_avail;
            const bool tested = i >= arm;
            if (tested) ++r.n_tested;
            if (tested && planted_nis(base, i, gap) > gate) {
                if (max_run > 0 && run >= max_run) { r.forced[i] = 1; ++r.n_forced; }
                else { r.rej[i] = 1; av = false; ++r.n_rej; ++run; if (run > r.longest) r.longest = run; if (r.first < 0) r.first = i; }
            }
            if (av) { run = 0; gap = 0; }
        }
        if (!av && !in_outage) { in_outage = true; start = i; }
        else if (av && in_outage) { r.ostart[i] = start; in_outage = false; }
    }
    return r;
}

// ---- the kernel's way: chunks of W lanes, the repair loop, carries from the settled pass
static Run chunked(int n, int W, const std::vector<char>& raw0, const std::vector<char>& fix, const std::vector<double>& base, double gate,
                   int arm, int max_run, long& passes)
{
    Run r; r.rej.assign(n, 0); r.forced.assign(n, 0); r.ostart.assign(n, -1);
    GateCounts cnt = gate_counts_init();
    OutageCarry oc{ true, 0, false };
    int c_gap = 0;                                                        // poses since the last applied fix, at the chunk's start
    for (int c0 = 0; c0 < n; c0 += W) {
        const int L = (n - c0 < W) ? (n - c0 - 1) : W - 1;
        const cov_mask act = cov_bits(0, L);
        cov_mask fix_m = 0ull, tested_m = 0ull;
        for (int l = 0; l <= L; ++l) {
            if (c0 + l >= 1 && fix[c0 + l]) fix_m |= 1ull << l;
            if (c0 + l >= arm) tested_m |= 1ull << l;
        }
        tested_m &= fix_m;
        GateRepair g{ 0ull, 0ull, 0 };
        cov_mask av_m = 0ull; OutageMasks om{ 0ull, 0ull, 0ull };
        std::vector<int> gap_after(64, 0);
        for (;;) {
            ++passes;
            // "scan": every lane's NIS under the CURRENT mask
            cov_mask over = 0ull;
            int gap = c_gap;
            for (int l = 0; l <= L; ++l) {
                if (c0 + l == 0) { gap_after[l] = gap; continue; }
                ++gap;
                const bool applied = ((fix_m & ~g.rej) >> l) & 1ull;
                if (((fix_m >> l) & 1ull) && planted_nis(base, c0 + l, gap) > gate) over |= 1ull << l;
                if (applied) gap = 0;
                gap_after[l] = gap;
            }
            av_m = ((fix_m & ~g.rej) | ((c0 == 0 && raw0[0]) ? 1ull : 0ull)) & act;
            om = outage_masks(act, av_m, c0 == 0, oc.prev_avail);
            if (!gate_settle(g, over & tested_m, fix_m, cnt.run, max_run)) break;
        }
        for (cov_mask rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
            const int rl = __builtin_ctzll(rm);
            r.ostart[c0 + rl] = (int)outage_closed_at(om.start, 0ull, rl, c0, oc.ostart, oc.seg_sharp).first;
        }
        for (int l = 0; l <= L; ++l) { r.rej[c0 + l] = (g.rej >> l) & 1ull; r.forced[c0 + l] = (g.forced >> l) & 1ull; }
        gate_chunk_counts(cnt, fix_m, tested_m, g.rej, g.forced, c0);
        oc = outage_carry(oc, av_m, om.start, 0ull, L, c0);
        c_gap = gap_after[L];
    }
    r.n_avail = cnt.n_avail; r.n_tested = cnt.n_tested; r.n_rej = cnt.n_rejected; r.n_forced = cnt.n_forced;
    r.longest = cnt.longest; r.first = cnt.first;
    return r;
}

int main()
{
    const int n = 10;
    long cases = 0, rejections = 0, forced = 0, passes = 0, merged = 0;
    // gate_nis is the plain expression
    {
        const double y[3] = { 3.0, -4.0, 0.5 }, S[3] = { 2.0, 8.0, 0.25 };
        const double want = (9.0 / 2.0 + 16.0 / 8.0) + 0.25 / 0.25;
        if (std::fabs(gate_nis(y, S) - want) > 1e-15 * want) { std::printf("FAIL gate_nis\n"); return 1; }
    }
    for (int pat = 0; pat < (1 << n); ++pat) {
        std::vector<char> fix(n), raw0(n);
        for (int i = 0; i < n; ++i) { fix[i] = (pat >> i) & 1; raw0[i] = fix[i]; }
        for (int row = 0; row < 12; ++row) {
            std::vector<double> base(n);
            for (int i = 0; i < n; ++i) {                                 // low / borderline (over the gate after a gap) / high, NaN now and then
                const double u = uni();
                base[i] = u < 0.35 ? 0.2 : (u < 0.65 ? 0.6 : (u < 0.97 ? 5.0 : std::nan("")));
            }
            if (row == 0) for (int i = 0; i < n; ++i) base[i] = 5.0;     // every fix over the gate
            if (row == 1) for (int i = 0; i < n; ++i) base[i] = 0.6;     // every fix over it only after a gap of two
            for (int max_run = 0; max_run <= 2; ++max_run)
                for (int arm = 0; arm <= 3; arm += 3) {
                    const double gate = 1.0;
                    const Run want = per_pose(n, raw0, fix, base, gate, arm, max_run);
                    for (int W : { 64, 4, 3 }) {
                        const Run got = chunked(n, W, raw0, fix, base, gate, arm, max_run, passes);
                        ++cases;
                        bool ok = got.n_avail == want.n_avail && got.n_tested == want.n_tested && got.n_rej == want.n_rej
                            && got.n_forced == want.n_forced && got.longest == want.longest && got.first == want.first;
                        for (int i = 0; i < n; ++i) ok = ok && got.rej[i] == want.rej[i] && got.forced[i] == want.forced[i] && got.ostart[i] == want.ostart[i];
                        if (!ok) {
                            std::printf("FAIL pattern %d row %d max_run %d arm %d W %d: rejected %ld/%ld forced %ld/%ld longest %ld/%ld first %ld/%ld\n",
                                        pat, row, max_run, arm, W, got.n_rej, want.n_rej, got.n_forced, want.n_forced, got.longest, want.longest,
                                        got.first, want.first);
                            return 1;
                        }
                    }
                    rejections += want.n_rej; forced += want.n_forced;
                    for (int i = 1; i < n; ++i)                           // a recovery that closes an outage made of rejected AND natural poses
                        if (want.ostart[i] >= 0) {
                            bool anyr = false, anyn = false;
                            for (int j = want.ostart[i]; j < i; ++j) { anyr = anyr || want.rej[j]; anyn = anyn || !fix[j]; }
                            merged += (anyr && anyn);
                        }
                }
        }
    }
    if (rejections == 0 || forced == 0 || merged == 0) { std::printf("FAIL the sweep met no rejection / forced accept / merged outage\n"); return 1; }
    std::printf("OK %ld cases, %ld rejections, %ld forced accepts, %ld merged outages, %ld passes\n", cases, rejections, forced, merged, passes);
    return 0;
}
