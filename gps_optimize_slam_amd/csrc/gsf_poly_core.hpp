// gsf_poly_core.hpp -- the least-squares polynomial fit of the GPS pre-filter (gsf_gpsfilter.hip): the pieces that are plain host/device C++.
//
// One RANSAC trial of filter_gps_outliers_ransac (EKFGPSSLAM.py:136-247) is LinearRegression(fit_intercept=True) on PolynomialFeatures(d)(t)
// of min_samples rows, then |y - prediction| <= threshold over every row of the window.  This header holds that fit in its three forms
// (fit_subset_t: per-thread arrays with run-time bounds; fit_subset_regs: the same operations with compile-time bounds, arrays in
// registers; the re-orthogonalising instance of fit_subset_t for the wide kernel), the prediction, and scikit-learn's dynamic trial count.
// The kernels call them per lane; tests/host_harness_poly.cpp compiles them with g++ and tests/test_prefilter_fit_host.py holds them to
// the 50-digit yardstick of tests/prefilter_fit_ref.py.
//
// DOMAIN ("Domain of the pre-filter's fit"; include/gsf.h states the same contract):
//   * WINDOW-LOCAL TIME.  Every stamp is taken relative to t0 -- the first row of the problem (fed-sample entries) or of the window (chain
//     kernel) -- where it is loaded: the fit sees t - t0 and poly_predict is given t - t0.  With raw Unix stamps (1.3e9 s) the term coef t^2
//     cancels against the intercept to ~30 m at the default degree 2, and the part of the centred t^2 column that is orthogonal to t lies
//     below its own rounding; in local time the same arithmetic stays within a few ulps of the target.
//   * RANK RULE.  A column counts as dependent when its norm after the Gram-Schmidt sweep is at most POLY_RANK_TOL x ms x (its norm before
//     centring and the sweep): repeated stamps leave fewer distinct stamps than degree + 1, the data are then exactly rank deficient and what
//     is left of the column is rounding.  A dependent column gets coefficient 0 and takes no part in the later columns' sweeps, so a sample
//     with m distinct stamps gets the least-squares polynomial of degree m - 1.
#pragma once
#include <math.h>
#include <stdint.h>
#include "gsf_math.hpp"

namespace gsf {

constexpr int RP_MAX_SAMPLES = 16;
constexpr int RP_MAX_DEGREE = 3;
constexpr int RPW_MAX_DEGREE = 8, RPW_MAX_SAMPLES = 64;
// the rank test: |column after the sweep| <= POLY_RANK_TOL * ms * |column as loaded|.  The order of the rcond LinearRegression's lstsq uses
// (max(rows, columns) x 2^-52); the factor 4 keeps the sweep's own rounding (a few 2^-53 of the loaded column per swept column) below it.
constexpr double POLY_RANK_TOL = 4.0 * 2.220446049250313e-16;

template <int MAXD> struct PolyModelT { double coef[MAXD], intercept; };
typedef PolyModelT<RP_MAX_DEGREE> PolyModel;

// t: the stamp in the time the model was fitted in (window-local: stamp - t0)
template <int MAXD>
GSF_HD double poly_predict(const PolyModelT<MAXD>& m, int degree, double t)
{
    // (compile-time bounds: a loop to the run-time degree indexes m.coef dynamically, which put every model of the chain kernel into scratch
    // memory -- each prediction then started with dependent trips to it.  The terms k < degree are formed exactly as that loop formed them.)
    double acc = 0.0, tk = t;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) { acc = (k < degree) ? (acc + m.coef[k] * tk) : acc; tk *= t; }
    return acc + m.intercept;
}

// LinearRegression(fit_intercept=True) on PolynomialFeatures(degree)(t - t0): centre the columns (t - t0)^k and y by their subset means,
// solve the least squares by modified Gram-Schmidt (the constant column is identically zero after centring: coefficient 0),
// intercept = mean(y) - sum coef_k mean((t - t0)^k).
// MAXD / MAXS size the per-thread arrays (3 / 16 for the kernels of the hot path, 8 / 64 for the wide kernel); REORTH: a second
// Gram-Schmidt sweep per column ("twice is enough"), for the higher degrees whose centred power columns are nearly dependent.
template <int MAXD, int MAXS, bool REORTH>
GSF_HD PolyModelT<MAXD> fit_subset_t(const double* __restrict__ t, const double* __restrict__ y, const int32_t* __restrict__ idx,
                                     int ms, int degree, int ystride, double t0)
{
    double c[MAXD][MAXS], yy[MAXS], mean[MAXD], raw2[MAXD], ymean = 0.0;
    for (int k = 0; k < MAXD; ++k) { mean[k] = 0.0; raw2[k] = 0.0; }
    for (int i = 0; i < ms; ++i) {
        const double ti = t[idx[i]] - t0;
        double tk = ti;
        for (int k = 0; k < degree; ++k) { c[k][i] = tk; mean[k] += tk; raw2[k] += tk * tk; tk *= ti; }
        yy[i] = y[(int64_t)idx[i] * ystride]; ymean += yy[i];
    }
    const double rn = 1.0 / (double)ms;
    const double tol2 = (POLY_RANK_TOL * (double)ms) * (POLY_RANK_TOL * (double)ms);
    ymean *= rn;
    for (int k = 0; k < degree; ++k) mean[k] *= rn;
    for (int i = 0; i < ms; ++i) { yy[i] -= ymean; for (int k = 0; k < degree; ++k) c[k][i] -= mean[k]; }
    // MGS: c_k = sum_{j<=k} R[j][k] q_j, q_j stored in place of c_j;  z_j = q_j . y
    double Rm[MAXD][MAXD], z[MAXD];
    for (int k = 0; k < MAXD; ++k) { z[k] = 0.0; for (int j = 0; j < MAXD; ++j) Rm[k][j] = 0.0; }
    for (int k = 0; k < degree; ++k) {
        for (int j = 0; j < k; ++j) {
            double d = 0.0;
            for (int i = 0; i < ms; ++i) d += c[j][i] * c[k][i];
            Rm[j][k] = d;
            for (int i = 0; i < ms; ++i) c[k][i] -= d * c[j][i];
        }
        if (REORTH) {
            for (int j = 0; j < k; ++j) {
                double d = 0.0;
                for (int i = 0; i < ms; ++i) d += c[j][i] * c[k][i];
                Rm[j][k] += d;
                for (int i = 0; i < ms; ++i) c[k][i] -= d * c[j][i];
            }
        }
        double nn = 0.0;
        for (int i = 0; i < ms; ++i) nn += c[k][i] * c[k][i];
        const bool indep = nn > tol2 * raw2[k];                           // the rank rule of the header comment, on the squares (all-zero column: dependent)
        nn = sqrt(nn);
        Rm[k][k] = indep ? nn : 0.0;
        const double inv = indep ? 1.0 / nn : 0.0;                        // a dependent column gets coefficient 0 and leaves the basis (q_k = 0)
        double d = 0.0;
        for (int i = 0; i < ms; ++i) { c[k][i] *= inv; d += c[k][i] * yy[i]; }
        z[k] = d;
    }
    PolyModelT<MAXD> m;
    for (int k = degree - 1; k >= 0; --k) {                               // back substitution R coef = z
        double v = z[k];
        for (int j = k + 1; j < degree; ++j) v -= Rm[k][j] * m.coef[j];
        m.coef[k] = Rm[k][k] > 0.0 ? v / Rm[k][k] : 0.0;
    }
    for (int k = degree; k < MAXD; ++k) m.coef[k] = 0.0;
    double off = 0.0;
    for (int k = 0; k < degree; ++k) off += mean[k] * m.coef[k];
    m.intercept = ymean - off;
    return m;
}
// The same fit with every array in REGISTERS: fit_subset_t's c[MAXD][MAXS] / yy[MAXS] are indexed by run-time loop bounds (ms, degree), which
// puts them in scratch memory -- 656 bytes per lane in the chain kernel, and the two fits of a window-axis problem (the batch's models, the
// winner's model again) were 51 % of its time (23 k + 27 k of 98 k cycles, in-kernel clocks).  Here every loop
// has a compile-time bound and is unrolled; rows >= ms and columns >= degree hold zeros, which the sums take in as exact no-ops (x + 0 * 0 = x),
// so the operations that matter happen in fit_subset_t's order: the same bits.
template <int MAXD, int MAXS>
GSF_HD PolyModelT<MAXD> fit_subset_regs(const double* __restrict__ t, const double* __restrict__ y, const int32_t* __restrict__ idx,
                                        const int ms, const int degree, const int ystride, const double t0)
{
    double c[MAXD][MAXS], yy[MAXS], mean[MAXD], raw2[MAXD], ymean = 0.0;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) { mean[k] = 0.0; raw2[k] = 0.0; }
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
        const bool on = i < ms;
        const int32_t ix = idx[on ? i : 0];
        const double ti = t[ix] - t0, yv = y[(int64_t)ix * ystride];
        double tk = ti;
#pragma unroll
        for (int k = 0; k < MAXD; ++k) {
            const bool use = on && k < degree;
            c[k][i] = use ? tk : 0.0;
            mean[k] += use ? tk : 0.0;
            raw2[k] += use ? tk * tk : 0.0;
            tk *= ti;
        }
        yy[i] = on ? yv : 0.0; ymean += on ? yv : 0.0;
    }
    const double rn = 1.0 / (double)ms;
    const double tol2 = (POLY_RANK_TOL * (double)ms) * (POLY_RANK_TOL * (double)ms);
    ymean *= rn;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) mean[k] *= rn;
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
        const bool on = i < ms;
        yy[i] = on ? yy[i] - ymean : 0.0;
#pragma unroll
        for (int k = 0; k < MAXD; ++k) c[k][i] = (on && k < degree) ? c[k][i] - mean[k] : 0.0;
    }
    double Rm[MAXD][MAXD], z[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        z[k] = 0.0;
#pragma unroll
        for (int j = 0; j < MAXD; ++j) Rm[k][j] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        if (k < degree) {                                                 // (uniform over the wave: degree is a launch parameter)
#pragma unroll
            for (int j = 0; j < k; ++j) {
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < MAXS; ++i) d += c[j][i] * c[k][i];
                Rm[j][k] = d;
#pragma unroll
                for (int i = 0; i < MAXS; ++i) c[k][i] -= d * c[j][i];
            }
            double nn = 0.0;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) nn += c[k][i] * c[k][i];
            const bool indep = nn > tol2 * raw2[k];
            nn = sqrt(nn);
            Rm[k][k] = indep ? nn : 0.0;
            const double inv = indep ? 1.0 / nn : 0.0;
            double d = 0.0;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) { c[k][i] *= inv; d += c[k][i] * yy[i]; }
            z[k] = d;
        }
    }
    PolyModelT<MAXD> m;
#pragma unroll
    for (int k = MAXD - 1; k >= 0; --k) {
        double v = z[k];
#pragma unroll
        for (int j = k + 1; j < MAXD; ++j) if (j < degree) v -= Rm[k][j] * m.coef[j];
        m.coef[k] = (k < degree && Rm[k][k] > 0.0) ? v / Rm[k][k] : 0.0;
    }
    double off = 0.0;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) if (k < degree) off += mean[k] * m.coef[k];
    m.intercept = ymean - off;
    return m;
}
// REGS: the register form -- for the chain kernel, one wave per SIMD with registers to spare; the thread-per-trial kernels of the fed-sample
// route run several waves per SIMD and keep the compact scratch form (90 instead of 216 registers) unless GSF_POLY_FIT_REGS says otherwise
#ifndef GSF_POLY_FIT_REGS
#define GSF_POLY_FIT_REGS 0
#endif
template <bool REGS = (GSF_POLY_FIT_REGS != 0)>
GSF_HD PolyModel fit_subset(const double* __restrict__ t, const double* __restrict__ y, const int32_t* __restrict__ idx,
                            int ms, int degree, int ystride, double t0)
{
    if (!REGS) return fit_subset_t<RP_MAX_DEGREE, RP_MAX_SAMPLES, false>(t, y, idx, ms, degree, ystride, t0);
    if (ms <= 8) return fit_subset_regs<RP_MAX_DEGREE, 8>(t, y, idx, ms, degree, ystride, t0);
    return fit_subset_regs<RP_MAX_DEGREE, RP_MAX_SAMPLES>(t, y, idx, ms, degree, ystride, t0);
}

// sklearn.linear_model._ransac._dynamic_max_trials
GSF_HD double dynamic_max_trials(int n_inliers, int n_samples, int min_samples, double probability)
{
    const double EPS = 2.220446049250313e-16;                             // np.spacing(1)
    const double ratio = (double)n_inliers / (double)n_samples;
    const double nom = fmax(EPS, 1.0 - probability);
    const double denom = fmax(EPS, 1.0 - pow(ratio, (double)min_samples));
    if (nom == 1.0) return 0.0;
    if (denom == 1.0) return INFINITY;
    return fabs(ceil(log(nom) / log(denom)));
}

}  // namespace gsf
