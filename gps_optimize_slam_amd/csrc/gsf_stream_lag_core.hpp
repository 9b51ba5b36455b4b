// gsf_stream_lag_core.hpp -- fixed-lag RTS smoothing of a stream (include/gsf.h, gsf_stream_append_lag_dev): everything that is not a launch.
//
// The forward side is stream_append_track() of gsf_stream_core.hpp under the parking policy LagPark: beside the ring it keeps, per pose, the
// forward quantities the smoother of gsf_smooth_core.hpp runs on -- { xf[3], Pf[3], g[3], Pp[3] } with g = xf - xp, STREAM_LAG_F64 doubles in
// ring_lag's slot i % cap -- and two tag bits in the sign bits of two values that are never negative (smooth_tag): "a fix was applied
// here" in Pf[0], "a span starts here" (row 0, every sharp-turn recovery) in Pp[0].  xf is the filter's position as the step left it, before
// any later outage back-pass revises the ring's row; xp / Pp come through EkfTraj's optional Out::predicted().
//
// The back-pass of row i with window end we = min(i + lag, last row of i's span, n - 1) is rts_smoother_segment on rows [i .. we] in
// correction coordinates, per axis, IN THIS ORDER:
//     e = d = 0;  for k = we - 1 down to i:   e = A[k] * (e + g[k+1]);   d = (A[k] * A[k]) * (d + u[k+1])
//     A[k] = smooth_gain(Pf[k], Pp[k+1])  (0 where Pp[k+1] is not > 0),   u[k] = Pf[k] - Pp[k] on a row with a fix, else 0
//     xs = xf[i] + e,  Ps = Pf[i] + d   on a row that a fix in (i, we] reaches; every other row keeps xf, Pf exactly.
// A row's result is a function of (i, we) and the parked rows alone, each of which the forward side wrote once: how a track was cut into
// calls cannot change a bit of it.  lag_smooth_row() is that function over a `Rows` that serves A, g, u and the tags of a row; the kernel
// (gsf_stream_lag.hip) serves them from LDS, lag_backpass_track() below -- the kernel's per-track work written sequentially, which
// tests/host_harness_stream_lag.cpp compiles with g++ -- from the ring.
#pragma once
#include "gsf_stream_core.hpp"
#include "gsf_smooth_core.hpp"

namespace gsf {

constexpr int STREAM_LAG_F64 = 12;      // GSF_STREAM_LAG_F64
constexpr int STREAM_LAG_MAX = 512;     // GSF_STREAM_LAG_MAX
enum { LG_XF = 0, LG_PF = 3, LG_G = 6, LG_PP = 9 };
enum : int { LAG_FIX = 1, LAG_START = 2 };                                // a row's tags as the back-pass passes them around

// the lag's own capacity rule: the rows a call's back-pass reads and writes, min(lag, n_total) + m of them, must have a slot each
GSF_HD bool stream_lag_refused(int64_t lag, int64_t n_total, int64_t m, int64_t cap) { return (lag < n_total ? lag : n_total) + m > cap; }

// RingOut that also takes the step's prediction
struct LagRingOut : RingOut {
    double xp[3], Pp[3];
    GSF_HD void predicted(int64_t, const Vec3& pp, const double* P)
    {
        xp[0] = pp.x; xp[1] = pp.y; xp[2] = pp.z;
        Pp[0] = P[0]; Pp[1] = P[1]; Pp[2] = P[2];
    }
};

struct LagPark {
    using Out = LagRingOut;
    static constexpr bool parks = true;
    double* rl;                        // this track's ring_lag: [cap][STREAM_LAG_F64]
    int64_t lag;
    GSF_HD bool refused(int64_t n0, int64_t m, int64_t cap) const { return stream_lag_refused(lag, n0, m, cap); }
    // pose i right after its init / step: f holds xf, Pf and the outage state the step left, out the step's prediction
    GSF_HD void row(const EkfConfig& cfg, const EkfTraj<LagRingOut>& f, const LagRingOut& out, int64_t i, bool was_outage) const
    {
        double* w = rl + out.slot(i) * STREAM_LAG_F64;
        const double xf[3] = { f.p.x, f.p.y, f.p.z };
        if (i == 0) {                                                    // EkfTraj::init: the initial pose under P0, no fix applied, a span starts
#pragma unroll
            for (int c = 0; c < 3; ++c) { w[LG_XF + c] = xf[c]; w[LG_PF + c] = smooth_tag(f.P[c], false); w[LG_G + c] = 0.0; w[LG_PP + c] = smooth_tag(f.P[c], c == 0); }
            return;
        }
        const bool fix = f.prev_avail;                                   // == the step's `avail`
        // a recovery the step judged a sharp turn (gsf_ekf_core.hpp: neither ostart nor seg_sharp moves in a recovery step)
        const bool start = was_outage && fix && (i - f.ostart >= 2) && (f.seg_sharp || cfg.yaw_thr_rad < 0.0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            w[LG_XF + c] = xf[c];
            w[LG_PF + c] = smooth_tag(f.P[c], fix && c == 0);
            w[LG_G + c] = fix ? xf[c] - out.xp[c] : 0.0;
            w[LG_PP + c] = smooth_tag(out.Pp[c], start && c == 0);
        }
    }
};

// what the back-pass needs of a parked row k, given the row after it (Pp_next: untagged; linked = there is a row after in the track)
struct LagTerms { double A[3], g[3], u[3]; int tags; };
GSF_HD LagTerms lag_terms(const double* row, const double* Pp_next, bool linked)
{
    LagTerms t;
    const bool fix = smooth_tag_of(row[LG_PF]), start = smooth_tag_of(row[LG_PP]);
    t.tags = (fix ? LAG_FIX : 0) | (start ? LAG_START : 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double Pf = smooth_untag(row[LG_PF + c]), Pp = smooth_untag(row[LG_PP + c]);
        t.A[c] = smooth_gain(Pf, linked ? Pp_next[c] : 0.0, linked);
        t.g[c] = row[LG_G + c];
        const double u = Pf - Pp;
        t.u[c] = fix ? u : 0.0;
    }
    return t;
}

struct LagSmoothed { double e[3], d[3]; bool reached; int64_t we; };

// Rows: double A(k, c), g(k, c), u(k, c); int tags(k) for i <= k <= min(i + lag, n - 1)
template <class Rows>
GSF_HD LagSmoothed lag_smooth_row(const Rows& r, int64_t i, int64_t lag, int64_t n)
{
    LagSmoothed s;
    const int64_t hi = i + lag < n - 1 ? i + lag : n - 1;
    int64_t we = i;
    bool reached = false;
    while (we < hi) {                                                    // the window ends in front of the next span start
        const int tg = r.tags(we + 1);
        if (tg & LAG_START) break;
        reached = reached || (tg & LAG_FIX) != 0;
        ++we;
    }
    double e[3] = { 0.0, 0.0, 0.0 }, d[3] = { 0.0, 0.0, 0.0 };
    for (int64_t k = we - 1; k >= i; --k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double A = r.A(k, c);
            const double se = e[c] + r.g(k + 1, c);
            e[c] = A * se;
            const double sd = d[c] + r.u(k + 1, c);
            d[c] = (A * A) * sd;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { s.e[c] = e[c]; s.d[c] = d[c]; }
    s.reached = reached; s.we = we;
    return s;
}

// the smoothed row from its parked one: rows no fix reaches keep the filter's bytes
GSF_HD void lag_finish_row(const double* row, const LagSmoothed& s, double* xs, double* Ps, uint8_t& flags)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double xf = row[LG_XF + c], Pf = smooth_untag(row[LG_PF + c]);
        const double x = xf + s.e[c], P = Pf + s.d[c];
        xs[c] = s.reached ? x : xf;
        Ps[c] = s.reached ? P : Pf;
    }
    flags = (uint8_t)((s.reached ? POSE_SMOOTHED : 0) | (smooth_tag_of(row[LG_PP]) ? POSE_SPAN_START : 0));
}

GSF_HD int64_t lag_final_count(int64_t n, int64_t lag) { return n > lag ? n - lag : 0; }

// the rows served straight from a track's ring_lag (the sequential form)
struct LagRingRows {
    const double* rl; int64_t cap, n;
    GSF_HD const double* row(int64_t k) const { return rl + (k % cap) * STREAM_LAG_F64; }
    GSF_HD LagTerms terms(int64_t k) const
    {
        const bool linked = k + 1 < n;
        double Ppn[3] = { 0.0, 0.0, 0.0 };
        if (linked) { const double* nx = row(k + 1); Ppn[0] = smooth_untag(nx[LG_PP]); Ppn[1] = nx[LG_PP + 1]; Ppn[2] = nx[LG_PP + 2]; }
        return lag_terms(row(k), Ppn, linked);
    }
    GSF_HD double A(int64_t k, int c) const { return terms(k).A[c]; }
    GSF_HD double g(int64_t k, int c) const { return terms(k).g[c]; }
    GSF_HD double u(int64_t k, int c) const { return terms(k).u[c]; }
    GSF_HD int tags(int64_t k) const { return terms(k).tags; }
};

struct LagOut { double* spos; double* svar; uint8_t* sflags; };          // the call's ragged outputs, each may be NULL

GSF_HD void lag_nan_rows(const LagOut& o, int64_t from, int64_t to)
{
    for (int64_t r = from; r < to; ++r) {
        if (o.spos) { o.spos[r * 3] = NAN; o.spos[r * 3 + 1] = NAN; o.spos[r * 3 + 2] = NAN; }
        if (o.svar) { o.svar[r * 3] = NAN; o.svar[r * 3 + 1] = NAN; o.svar[r * 3 + 2] = NAN; }
        if (o.sflags) o.sflags[r] = 0;
    }
}

// One track's back-pass after an append that took it from n0 to n0 + m poses (m < 0: the append refused the track, or its state was bad:
// nothing but NaN rows): rows [max(0, n0 - lag), n0 + m) of ring_spos / ring_svar, the newly final ones also to rows lo .. of the outputs.
GSF_HD void lag_backpass_track(const double* rl, double* rs, double* rv, int64_t cap, int64_t lag, int64_t n0, int64_t m, const LagOut& o,
                               int64_t lo, int64_t mseg, int64_t& smooth_from, int64_t& n_smooth_final)
{
    if (m < 0) { lag_nan_rows(o, lo, lo + mseg); smooth_from = n_smooth_final = lag_final_count(n0, lag); return; }
    const int64_t n = n0 + m, from = lag_final_count(n0, lag), fin = lag_final_count(n, lag);
    smooth_from = from; n_smooth_final = fin;
    lag_nan_rows(o, lo + (fin - from), lo + mseg);
    if (m == 0) return;
    const LagRingRows rows{ rl, cap, n };
    for (int64_t i = from; i < n; ++i) {
        const LagSmoothed s = lag_smooth_row(rows, i, lag, n);
        double xs[3], Ps[3]; uint8_t fl;
        lag_finish_row(rows.row(i), s, xs, Ps, fl);
        const int64_t sl = i % cap;
#pragma unroll
        for (int c = 0; c < 3; ++c) { rs[sl * 3 + c] = xs[c]; rv[sl * 3 + c] = Ps[c]; }
        if (i < fin) {
            const int64_t w = lo + (i - from);
            if (o.spos) { o.spos[w * 3] = xs[0]; o.spos[w * 3 + 1] = xs[1]; o.spos[w * 3 + 2] = xs[2]; }
            if (o.svar) { o.svar[w * 3] = Ps[0]; o.svar[w * 3 + 1] = Ps[1]; o.svar[w * 3 + 2] = Ps[2]; }
            if (o.sflags) o.sflags[w] = fl;
        }
    }
}

}  // namespace gsf
