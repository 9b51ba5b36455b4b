// gsf_lever_core.hpp -- antenna lever arm (gsf_lever_fit_dev / gsf_lever_apply_dev): every rule of the fit and of the de-levering of a fix,
// as plain host/device C++ without a HIP type.
//
// A GNSS fix measures the antenna, not the camera:  gps_i = s R pos_i + t + R M(q_i) l + noise,  l = the antenna offset in the sensor
// frame (metres), M(q) = the rotation matrix of the normalised SLAM quaternion.  The fit is a joint Gauss-Newton over ten unknowns
// x = (s, c[3], l[3], dtheta[3]) on the usable rows of a track, shifted by its first usable row f:
//   v_i = pos_i - pos_f,  u_i = R^T (gps_i - gps_f),  t = R (c - s pos_f) + gps_f       (no UTM-sized number enters a sum)
//   w_i = s v_i + c + M_i l,  r_i = u_i - w_i,  J_i = [ v_i | I | M_i | -[w_i]x ]
//   N = sum J^T J + priors,  g = sum J^T r + priors;  N d = g by Cholesky on the diagonally scaled matrix;
//   s += d_s, c += d_c, l += d_l, phi += d_theta, R <- R exp([d_theta]x)
// The driver lev_fit_track() is ONE body for the kernel and the host: what differs is the pass over the rows (a template argument --
// gsf_lever.hip: lane-strided rows and DPP sums; tests/host_harness_lever.cpp: a loop).  tests/lever_ref.py restates it row by row.
//
// The 49 distinct sums of a round (I^T I and M^T M are n I; the rest of N and g), LevSums::a[.]:
//   0 n | 1 v.v | 2-4 v | 5-7 M^T v | 8-10 w x v | 11-19 M | 20-22 w | 23-31 m_j . (e_k x w) | 32-37 w w^T (xx xy xz yy yz zz)
//   38 v.r | 39-41 r | 42-44 M^T r | 45-47 w x r | 48 r.r
#pragma once
#include "gsf_math.hpp"

namespace gsf {

enum : int32_t {                       // flags of a fit (include/gsf.h)
    LEVER_FEW = 1, LEVER_VAR0 = 2, LEVER_SINGULAR = 4, LEVER_SCALE = 8, LEVER_WEAK_X = 16, LEVER_WEAK_Y = 32, LEVER_WEAK_Z = 64,
    LEVER_NOT_CONVERGED = 128, LEVER_TRACK = 256,
    LEVER_KEPT = LEVER_FEW | LEVER_VAR0 | LEVER_SINGULAR | LEVER_SCALE | LEVER_TRACK      // the track keeps its starting values
};
enum : int32_t { LVP_BAD_QUAT = 1 };   // pose_flags bits of the apply entry
constexpr int LEV_NSUM = 49;
constexpr int LEV_MAX_ITERS = 8;

struct LevRule {                       // gsf_lever_config, field by field
    double sigma_fix, sigma_prior[3], sigma_rot, ratio_max, pivot_min, weak_ratio, conv_tol;
    int32_t min_rows, iters, fit_scale, fit_rotation;
};
struct LevState { double R[9], s, c[3], l[3], phi[3]; };
struct LevSums { double a[LEV_NSUM]; };
struct LevOut { double R[9], t[3], s, l[3], lcov[9], rms_before, rms_after, last_step; int32_t n_rows, n_bad_quat, flags; };

// ---- rows.  A quaternion is normalisable under the reference's rule |q| > 1e-9 (ExtendedKalmanFilter.normalize_quaternion), a NaN / inf
// norm fails it.  lev_row_kind: 0 = usable, 1 = a row whose ONLY defect is its quaternion (counted in n_bad_quat), 2 = not a row of the fit
GSF_HD bool lev_finite3(double a, double b, double c) { return (fabs(a) < INFINITY) && (fabs(b) < INFINITY) && (fabs(c) < INFINITY); }
GSF_HD bool lev_quat_unit(const Quat& q, Quat& o)
{
    const double n2 = quat_norm2(q);
    const bool ok = (n2 > 1e-18) && (n2 <= 1e280);
    const double r = fast_rsqrt(ok ? n2 : 1.0);
    o.x = q.x * r; o.y = q.y * r; o.z = q.z * r; o.w = q.w * r;
    return ok;
}
GSF_HD int lev_row_kind(uint8_t valid, const double* pos, const double* quat, const double* gps, Quat& qn)
{
    const bool q_ok = lev_quat_unit(Quat{ quat[0], quat[1], quat[2], quat[3] }, qn);
    if (!(valid != 0 && lev_finite3(gps[0], gps[1], gps[2]) && lev_finite3(pos[0], pos[1], pos[2]))) return 2;
    return q_ok ? 0 : 1;
}

// ---- one row into the sums of a round, under the state x and the shift (pf, gf)
GSF_HD void lev_sums_zero(LevSums& S)
{
#pragma unroll
    for (int k = 0; k < LEV_NSUM; ++k) S.a[k] = 0.0;
}
GSF_HD void lev_add_row(LevSums& S, const LevState& x, const double* pf, const double* gf, const double* pos, const double* gps, const Quat& qn)
{
    const double v0 = pos[0] - pf[0], v1 = pos[1] - pf[1], v2 = pos[2] - pf[2];
    const double d0 = gps[0] - gf[0], d1 = gps[1] - gf[1], d2 = gps[2] - gf[2];
    const double u0 = x.R[0] * d0 + x.R[3] * d1 + x.R[6] * d2, u1 = x.R[1] * d0 + x.R[4] * d1 + x.R[7] * d2, u2 = x.R[2] * d0 + x.R[5] * d1 + x.R[8] * d2;
    const Mat3 M = quat_matrix(qn);
    const double w0 = x.s * v0 + x.c[0] + (M.m00 * x.l[0] + M.m01 * x.l[1] + M.m02 * x.l[2]);
    const double w1 = x.s * v1 + x.c[1] + (M.m10 * x.l[0] + M.m11 * x.l[1] + M.m12 * x.l[2]);
    const double w2 = x.s * v2 + x.c[2] + (M.m20 * x.l[0] + M.m21 * x.l[1] + M.m22 * x.l[2]);
    const double r0 = u0 - w0, r1 = u1 - w1, r2 = u2 - w2;
    double* a = S.a;
    a[0] += 1.0;
    a[1] += v0 * v0 + v1 * v1 + v2 * v2;
    a[2] += v0; a[3] += v1; a[4] += v2;
    a[5] += M.m00 * v0 + M.m10 * v1 + M.m20 * v2; a[6] += M.m01 * v0 + M.m11 * v1 + M.m21 * v2; a[7] += M.m02 * v0 + M.m12 * v1 + M.m22 * v2;
    a[8] += w1 * v2 - w2 * v1; a[9] += w2 * v0 - w0 * v2; a[10] += w0 * v1 - w1 * v0;
    a[11] += M.m00; a[12] += M.m01; a[13] += M.m02; a[14] += M.m10; a[15] += M.m11; a[16] += M.m12; a[17] += M.m20; a[18] += M.m21; a[19] += M.m22;
    a[20] += w0; a[21] += w1; a[22] += w2;
    // m_j . (e_k x w), m_j = column j of M:  e_0 x w = (0, -w2, w1),  e_1 x w = (w2, 0, -w0),  e_2 x w = (-w1, w0, 0)
    a[23] += M.m20 * w1 - M.m10 * w2; a[24] += M.m00 * w2 - M.m20 * w0; a[25] += M.m10 * w0 - M.m00 * w1;
    a[26] += M.m21 * w1 - M.m11 * w2; a[27] += M.m01 * w2 - M.m21 * w0; a[28] += M.m11 * w0 - M.m01 * w1;
    a[29] += M.m22 * w1 - M.m12 * w2; a[30] += M.m02 * w2 - M.m22 * w0; a[31] += M.m12 * w0 - M.m02 * w1;
    a[32] += w0 * w0; a[33] += w0 * w1; a[34] += w0 * w2; a[35] += w1 * w1; a[36] += w1 * w2; a[37] += w2 * w2;
    a[38] += v0 * r0 + v1 * r1 + v2 * r2;
    a[39] += r0; a[40] += r1; a[41] += r2;
    a[42] += M.m00 * r0 + M.m10 * r1 + M.m20 * r2; a[43] += M.m01 * r0 + M.m11 * r1 + M.m21 * r2; a[44] += M.m02 * r0 + M.m12 * r1 + M.m22 * r2;
    a[45] += w1 * r2 - w2 * r1; a[46] += w2 * r0 - w0 * r2; a[47] += w0 * r1 - w1 * r0;
    a[48] += r0 * r0 + r1 * r1 + r2 * r2;
}

// ---- priors: weight (sigma_fix / sigma)^2, an infinite sigma means weight 0 (a NaN sigma: NaN, which ends in LEVER_SINGULAR)
GSF_HD double lev_weight(double sigma_fix, double sigma) { const double q = sigma_fix / sigma; return q * q; }

// ---- the normal equations of a round from its sums: N (10 x 10, row-major, both triangles), g (10).  Unknowns: 0 s, 1-3 c, 4-6 l, 7-9 theta
GSF_HD void lev_build(const LevSums& S, const LevState& x, const LevRule& rule, const double* l0, double* N, double* g)
{
    const double* a = S.a;
#pragma unroll
    for (int k = 0; k < 100; ++k) N[k] = 0.0;
    const double n = a[0];
    N[0] = a[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) { N[1 + k] = a[2 + k]; N[4 + k] = a[5 + k]; N[7 + k] = a[8 + k]; }
    const double W0 = a[20], W1 = a[21], W2 = a[22];
    const double ew[9] = { 0.0, W2, -W1, -W2, 0.0, W0, W1, -W0, 0.0 };          // ew[a * 3 + k] = (e_k x W)_a
    const double ww[9] = { a[32], a[33], a[34], a[33], a[35], a[36], a[34], a[36], a[37] };
    const double trw = a[32] + a[35] + a[37];
    const double wr = lev_weight(rule.sigma_fix, rule.sigma_rot);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double wl = lev_weight(rule.sigma_fix, rule.sigma_prior[r]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            N[(1 + r) * 10 + 1 + k] = (r == k) ? n : 0.0;
            N[(1 + r) * 10 + 4 + k] = a[11 + r * 3 + k];
            N[(1 + r) * 10 + 7 + k] = ew[r * 3 + k];
            N[(4 + r) * 10 + 4 + k] = (r == k) ? n + wl : 0.0;
            N[(4 + r) * 10 + 7 + k] = a[23 + r * 3 + k];
            N[(7 + r) * 10 + 7 + k] = (r == k) ? (trw - ww[r * 3 + k]) + wr : -ww[r * 3 + k];
        }
        g[1 + r] = a[39 + r];
        g[4 + r] = a[42 + r] + wl * (l0[r] - x.l[r]);
        g[7 + r] = a[45 + r] - wr * x.phi[r];
    }
    g[0] = a[38];
#pragma unroll
    for (int r = 0; r < 10; ++r)
#pragma unroll
        for (int k = 0; k < r; ++k) N[r * 10 + k] = N[k * 10 + r];
    // a pinned unknown: its row and column are the identity's, its g entry 0
    if (!rule.fit_scale) {
#pragma unroll
        for (int k = 0; k < 10; ++k) { N[k] = 0.0; N[k * 10] = 0.0; }
        N[0] = 1.0; g[0] = 0.0;
    }
    if (!rule.fit_rotation) {
#pragma unroll
        for (int r = 7; r < 10; ++r) {
#pragma unroll
            for (int k = 0; k < 10; ++k) { N[r * 10 + k] = 0.0; N[k * 10 + r] = 0.0; }
        }
#pragma unroll
        for (int r = 7; r < 10; ++r) { N[r * 10 + r] = 1.0; g[r] = 0.0; }
    }
}

// ---- N d = g by Cholesky on D N D, D = diag(N)^(-1/2); the l block of N^-1 by three more right-hand sides.  A pivot (the value under the
// square root) that is not > pivot_min, or not finite, makes the system singular; every comparison is written so that a NaN fails it.
template <int START>
GSF_HD void lev_chol_solve(const double* L, const double* b, double* x)
{
    double y[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i < START) { y[i] = 0.0; continue; }
        double acc = b[i];
#pragma unroll
        for (int k = START; k < i; ++k) acc -= L[i * 10 + k] * y[k];
        y[i] = acc / L[i * 10 + i];
    }
#pragma unroll
    for (int i = 9; i >= 0; --i) {
        double acc = y[i];
#pragma unroll
        for (int k = i + 1; k < 10; ++k) acc -= L[k * 10 + i] * x[k];
        x[i] = acc / L[i * 10 + i];
    }
}
GSF_HD bool lev_solve(const double* N, const double* g, double pivot_min, double* d, double* Ninv_ll)
{
    double D[10], L[100];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 10; ++j) D[j] = 1.0 / sqrt(N[j * 10 + j]);
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        double p = N[j * 10 + j] * D[j] * D[j];
#pragma unroll
        for (int k = 0; k < j; ++k) p -= L[j * 10 + k] * L[j * 10 + k];
        ok = ok && (p > pivot_min) && (p < INFINITY);
        const double ljj = sqrt(p);
        L[j * 10 + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 10; ++i) {
            double acc = N[i * 10 + j] * D[i] * D[j];
#pragma unroll
            for (int k = 0; k < j; ++k) acc -= L[i * 10 + k] * L[j * 10 + k];
            L[i * 10 + j] = acc / ljj;
        }
    }
    double b[10], x[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) b[j] = g[j] * D[j];
    lev_chol_solve<0>(L, b, x);
#pragma unroll
    for (int j = 0; j < 10; ++j) { d[j] = x[j] * D[j]; ok = ok && (fabs(d[j]) < INFINITY); }
    {
#pragma unroll
        for (int j = 0; j < 10; ++j) b[j] = 0.0;
        b[4] = D[4];
        lev_chol_solve<4>(L, b, x);
        Ninv_ll[0] = x[4] * D[4]; Ninv_ll[1] = x[5] * D[5]; Ninv_ll[2] = x[6] * D[6];
        b[4] = 0.0; b[5] = D[5];
        lev_chol_solve<5>(L, b, x);
        Ninv_ll[3] = x[4] * D[4]; Ninv_ll[4] = x[5] * D[5]; Ninv_ll[5] = x[6] * D[6];
        b[5] = 0.0; b[6] = D[6];
        lev_chol_solve<6>(L, b, x);
        Ninv_ll[6] = x[4] * D[4]; Ninv_ll[7] = x[5] * D[5]; Ninv_ll[8] = x[6] * D[6];
    }
    return ok;
}

// ---- R <- R exp([d]x) (Rodrigues): exp = I + a K + b K^2, a = sin(th) / th, b = (1 - cos(th)) / th^2, by their series below th^2 = 1e-6
GSF_HD void lev_rotate(double* R, double d0, double d1, double d2)
{
    const double t2 = d0 * d0 + d1 * d1 + d2 * d2;
    double ca, cb;
    if (t2 < 1e-6) { ca = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0)); cb = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0)); }
    else { const double th = sqrt(t2); ca = sin(th) / th; cb = (1.0 - cos(th)) / t2; }
    const double E[9] = { 1.0 - cb * (d1 * d1 + d2 * d2), cb * d0 * d1 - ca * d2, cb * d0 * d2 + ca * d1,
                          cb * d0 * d1 + ca * d2, 1.0 - cb * (d0 * d0 + d2 * d2), cb * d1 * d2 - ca * d0,
                          cb * d0 * d2 - ca * d1, cb * d1 * d2 + ca * d0, 1.0 - cb * (d0 * d0 + d1 * d1) };
    double Rn[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = R[r * 3] * E[c] + R[r * 3 + 1] * E[3 + c] + R[r * 3 + 2] * E[6 + c];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
}

GSF_HD bool lev_scale_bad(double s, double s0, double ratio_max)
{
    const double ratio = s / s0;
    return !(s > 1e-6) || !(ratio >= 1.0 / ratio_max) || !(ratio <= ratio_max);
}

// ---- the fit of one track.  Pass:  void scan(int64_t& first, int32_t& n, int32_t& n_bad)  -- first usable row (-1: none) and the counts;
//                                   void shift(double* pf, double* gf)                      -- pos / gps of that row;
//                                   void sums(const LevState&, const double* pf, const double* gf, LevSums&)  -- the totals of a round.
template <class Pass>
GSF_HD void lev_fit_track(Pass& pass, const LevRule& rule, const double* R0, const double* t0, double s0, const double* l0, int32_t run_status, LevOut& o)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) { o.R[k] = R0[k]; o.lcov[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.t[k] = t0[k]; o.l[k] = l0[k]; o.lcov[k * 4] = rule.sigma_prior[k] * rule.sigma_prior[k]; }
    o.s = s0; o.rms_before = o.rms_after = o.last_step = NAN;
    o.n_rows = o.n_bad_quat = 0;
    int32_t flags = 0;
    if (run_status != 0) flags = LEVER_TRACK;                              // the rows of a failed run are not read
    else {
        int64_t first;
        pass.scan(first, o.n_rows, o.n_bad_quat);
        if (o.n_rows < rule.min_rows) flags |= LEVER_FEW;
        if (o.n_rows >= 1) {
            double pf[3], gf[3];
            pass.shift(pf, gf);
            LevState x;
#pragma unroll
            for (int k = 0; k < 9; ++k) x.R[k] = R0[k];
            x.s = s0;
            const double e0 = t0[0] - gf[0], e1 = t0[1] - gf[1], e2 = t0[2] - gf[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {                                  // c = R0^T (t0 - gps_f) + s0 pos_f
                x.c[k] = (R0[k] * e0 + R0[3 + k] * e1 + R0[6 + k] * e2) + s0 * pf[k];
                x.l[k] = l0[k]; x.phi[k] = 0.0;
            }
            double Ninv[9], step = NAN;
            LevSums S;
            for (int it = 0; it < rule.iters; ++it) {
                pass.sums(x, pf, gf, S);
                if (it == 0) {
                    const double n = S.a[0];
                    o.rms_before = sqrt(S.a[48] / n);
                    const double var = fmax(0.0, S.a[1] - (S.a[2] * S.a[2] + S.a[3] * S.a[3] + S.a[4] * S.a[4]) / n) / n;
                    if (!(var >= 1e-12)) flags |= LEVER_VAR0;
                    if (flags) break;
                }
                double N[100], g[10], d[10];
                lev_build(S, x, rule, l0, N, g);
                if (!lev_solve(N, g, rule.pivot_min, d, Ninv)) { flags |= LEVER_SINGULAR; break; }
                x.s += d[0];
#pragma unroll
                for (int k = 0; k < 3; ++k) { x.c[k] += d[1 + k]; x.l[k] += d[4 + k]; x.phi[k] += d[7 + k]; }
                lev_rotate(x.R, d[7], d[8], d[9]);
                step = fmax(fabs(d[4]), fmax(fabs(d[5]), fabs(d[6])));
                if (lev_scale_bad(x.s, s0, rule.ratio_max)) { flags |= LEVER_SCALE; break; }
            }
            if (!flags) {
                pass.sums(x, pf, gf, S);
                o.rms_after = sqrt(S.a[48] / S.a[0]);
                o.last_step = step;
                const double sf2 = rule.sigma_fix * rule.sigma_fix;
                const double b0 = x.c[0] - x.s * pf[0], b1 = x.c[1] - x.s * pf[1], b2 = x.c[2] - x.s * pf[2];
#pragma unroll
                for (int k = 0; k < 9; ++k) { o.R[k] = x.R[k]; o.lcov[k] = sf2 * Ninv[k]; }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    o.t[k] = (x.R[k * 3] * b0 + x.R[k * 3 + 1] * b1 + x.R[k * 3 + 2] * b2) + gf[k];
                    o.l[k] = x.l[k];
                }
                o.s = x.s;
            } else o.rms_after = o.rms_before;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (o.lcov[k * 4] > rule.weak_ratio * (rule.sigma_prior[k] * rule.sigma_prior[k])) flags |= (LEVER_WEAK_X << k);
    if (o.last_step > rule.conv_tol) flags |= LEVER_NOT_CONVERGED;
    o.flags = flags;
}

// ---- one fix moved between antenna and camera:  out = gps + sign R (M(q) l).  A component whose shift is exactly zero returns the
// fix's own bytes (l = 0: the input), a NaN fix stays NaN, a quaternion that cannot be normalised gives a NaN row and LVP_BAD_QUAT.
GSF_HD int32_t lev_apply_row(const double* R, const double* l, double sign, const double* quat, const double* gps, double* out)
{
    Quat qn;
    if (!lev_quat_unit(Quat{ quat[0], quat[1], quat[2], quat[3] }, qn)) { out[0] = out[1] = out[2] = NAN; return LVP_BAD_QUAT; }
    const Mat3 M = quat_matrix(qn);
    const double a0 = M.m00 * l[0] + M.m01 * l[1] + M.m02 * l[2], a1 = M.m10 * l[0] + M.m11 * l[1] + M.m12 * l[2], a2 = M.m20 * l[0] + M.m21 * l[1] + M.m22 * l[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double d = sign * (R[r * 3] * a0 + R[r * 3 + 1] * a1 + R[r * 3 + 2] * a2);
        out[r] = (d == 0.0) ? gps[r] : gps[r] + d;
    }
    return 0;
}

}  // namespace gsf
