// gsf_local_core.hpp -- local Sim3 alignment (gsf_sim3_local_fit_dev / gsf_sim3_local_apply_dev): everything that decides an index or a
// flag, as plain host/device C++ without a HIP type.
//
// A monocular front end drifts in scale over minutes, and one Sim3 per track (ref :973-1006) cannot follow it.  Here a track carries Sim3
// KNOTS on a time grid -- knot k at tau_k = t0 + k spacing, fitted on the usable rows with |ts - tau_k| <= half_window -- and every pose is
// mapped by a blend of the nearest valid knot on either side.  This header holds the grid (loc_tau, loc_knot_count, loc_cell), a
// track's status (loc_stamp_bad, loc_track_status), the window bounds (loc_window), the row rule (loc_usable), the moments of a window as one row adds to them (loc_add_row), the closed form of a knot
// with its validity flags (loc_knot_fit), the neighbour tables and rule (loc_index_track, loc_neighbours), the weight (loc_weight) and the
// blend of a pose (loc_blend).  gsf_local.hip calls them; tests/host_harness_local.cpp compiles them with g++ and runs them on the cases
// of tests/local_align_ref.py, whose NumPy restatement is the specification (definitions: include/gsf.h).
//
// Written orders that decide a flag or an index are fixed here and nowhere else:
//   tau_k = fma(k, spacing, t0)                one rounding, whatever -ffp-contract says
//   row i is in the window of knot k  iff  -half_window <= (ts[i] - tau_k) <= half_window   (one subtraction, then the comparisons)
//   cell of a pose = min(floor((ts - t0) / spacing), K - 2)
//   w = (ts - tau_L) / (tau_Rr - tau_L)
#pragma once
#include "gsf_math.hpp"

namespace gsf {

constexpr int LOC_KMAX = 4096;         // knots per track of one call (the caller's knot stride is at most this)

enum : int32_t {                       // track_status bits (include/gsf.h)
    LOC_EMPTY = 1, LOC_UNSORTED = 2, LOC_TOO_MANY = 4, LOC_SKIPPED = 8
};
enum : int32_t {                       // knot_flags bits
    KNOT_FEW = 1, KNOT_VAR0 = 2, KNOT_SCALE = 4, KNOT_ROT_FALLBACK = 8,
    KNOT_INVALID = KNOT_FEW | KNOT_VAR0 | KNOT_SCALE
};
enum : int32_t {                       // pose_flags bits
    LP_BRIDGED = 1, LP_HELD = 2, LP_GLOBAL = 4, LP_BAD_QUAT = 8, LP_TRACK = 16
};
enum : int32_t { LOC_SCALE = 0, LOC_SIM3 = 1 };   // gsf_local_config.mode

// ---- grid
GSF_HD double loc_tau(double t0, double spacing, int k) { return fma((double)k, spacing, t0); }

// K_b = floor((t_last - t0) / spacing) + 2, so that every pose has a knot on each side; anything beyond LOC_KMAX (a quotient that is not
// finite included) reads LOC_KMAX + 1
GSF_HD int32_t loc_knot_count(double t0, double t_last, double spacing)
{
    const double q = floor((t_last - t0) / spacing);
    if (!(q >= 0.0)) return (q < 0.0) ? 2 : LOC_KMAX + 1;                  // (a sorted track has q >= 0; NaN: too many)
    if (!(q <= (double)(LOC_KMAX - 1))) return LOC_KMAX + 1;
    return (int32_t)q + 2;
}

// a track's stamps must be non-decreasing and none may be NaN (the test of GSF_GATE_UNSORTED): is stamp t, followed by t_next, a defect?
GSF_HD bool loc_stamp_bad(double t, bool has_next, double t_next) { return !(t == t) || (has_next && !(t_next >= t)); }
// track_status of a track of n poses whose grid has K knots under the caller's stride Kmax; a track with a status has no knots
GSF_HD int32_t loc_track_status(int64_t n, bool unsorted, int32_t K, int32_t Kmax)
{
    return n <= 0 ? LOC_EMPTY : (unsorted ? LOC_UNSORTED : (K > Kmax ? LOC_TOO_MANY : 0));
}

// the cell of a pose: k = min(floor((ts - t0) / spacing), K - 2), not below 0 (a NaN stamp reads 0)
GSF_HD int32_t loc_cell(double ts, double t0, double spacing, int32_t K)
{
    const double q = floor((ts - t0) / spacing);
    const int32_t top = K >= 2 ? K - 2 : 0;
    if (!(q >= 0.0)) return 0;
    return q >= (double)top ? top : (int32_t)q;
}

// ---- window of a knot in the sorted stamps ts[i0 .. i1): rows lo .. hi - 1 are the ones with -hw <= ts - tau <= hw
GSF_HD bool loc_before_window(double ts, double tau, double hw) { const double d = ts - tau; return d < -hw; }
GSF_HD bool loc_past_window(double ts, double tau, double hw) { const double d = ts - tau; return d > hw; }
GSF_HD void loc_window(const double* ts, int64_t i0, int64_t i1, double tau, double hw, int64_t& lo, int64_t& hi)
{
    int64_t a = i0, b = i1;
    while (a < b) { const int64_t m = a + ((b - a) >> 1); if (loc_before_window(ts[m], tau, hw)) a = m + 1; else b = m; }
    lo = a; b = i1;
    while (a < b) { const int64_t m = a + ((b - a) >> 1); if (!loc_past_window(ts[m], tau, hw)) a = m + 1; else b = m; }
    hi = a;
}

// a row feeds a fit when its mask byte is set and its fix is finite (the rule gsf_sim3_fit_rows_batch_dev states)
GSF_HD bool loc_usable(uint8_t valid, double g0, double g1, double g2)
{
    return valid != 0 && (fabs(g0) < INFINITY) && (fabs(g1) < INFINITY) && (fabs(g2) < INFINITY);
}

// ---- the 17 raw moments of a window's usable rows, shifted by the window's first usable row (as / bs): n, sum a, sum b, sum a b^T,
// sum |a|^2 with a = src - as, b = fix - bs.  |a|, |b| <= the window's extent, so UTM-sized coordinates cost nothing (the bound bR_shift
// of tests/sim3_ref.py); differences of prefix sums of the unshifted rows would cancel.
struct LocMoments { double n, Sa[3], Sb[3], Saa, Sab[9], as[3], bs[3]; };

GSF_HD void loc_moments_zero(LocMoments& m)
{
    m.n = 0.0; m.Saa = 0.0;
    for (int k = 0; k < 3; ++k) { m.Sa[k] = m.Sb[k] = m.as[k] = m.bs[k] = 0.0; }
    for (int k = 0; k < 9; ++k) m.Sab[k] = 0.0;
}
GSF_HD void loc_add_row(LocMoments& m, const double* src, const double* fix)
{
    const double a0 = src[0] - m.as[0], a1 = src[1] - m.as[1], a2 = src[2] - m.as[2];
    const double c0 = fix[0] - m.bs[0], c1 = fix[1] - m.bs[1], c2 = fix[2] - m.bs[2];
    m.n += 1.0; m.Sa[0] += a0; m.Sa[1] += a1; m.Sa[2] += a2; m.Sb[0] += c0; m.Sb[1] += c1; m.Sb[2] += c2;
    m.Saa += a0 * a0 + a1 * a1 + a2 * a2;
    m.Sab[0] += a0 * c0; m.Sab[1] += a0 * c1; m.Sab[2] += a0 * c2;
    m.Sab[3] += a1 * c0; m.Sab[4] += a1 * c1; m.Sab[5] += a1 * c2;
    m.Sab[6] += a2 * c0; m.Sab[7] += a2 * c1; m.Sab[8] += a2 * c2;
}

struct LocFitRule { int32_t mode, min_rows; double rot_open, ratio_max; };

// ---- the closed form of one knot -> knot_flags; Rk / tk / sk are written for a valid knot only.
// The centring is finalize_raw's of gsf_sim3.hip (H = Sab - n ma mb^T, ssq = max(0, Saa - n |ma|^2), centroids = shift + mean).
//   mode LOC_SCALE: Rk = the track's global Rg;  sk = tr(Rg H) / ssq
//   mode LOC_SIM3:  the closed form of ref :436-451 on the Jacobi SVD (umeyama_rotation_svd's arithmetic, so the scale carries
//                   sigma1 + sigma2 + sigma3 as :444 is written); a rotation-open window, (sigma2 + d sigma3) <= rot_open sigma1, takes
//                   the LOC_SCALE form for this knot and is flagged KNOT_ROT_FALLBACK
//   tk = mean(b) - sk Rk mean(a)
// Validity, every comparison written so that a NaN fails it: KNOT_FEW  n < min_rows;  KNOT_VAR0  not (ssq / n >= 1e-12);  KNOT_SCALE
// not (sk > 1e-6), or sk / sg outside [1 / ratio_max, ratio_max].
GSF_HD int32_t loc_knot_fit(const LocMoments& m, const LocFitRule& rule, const double* Rg, double sg, double* Rk, double* tk, double& sk)
{
    if (!(m.n >= (double)rule.min_rows)) return KNOT_FEW;
    const double rn = 1.0 / m.n;
    const double ma[3] = { m.Sa[0] * rn, m.Sa[1] * rn, m.Sa[2] * rn }, mb[3] = { m.Sb[0] * rn, m.Sb[1] * rn, m.Sb[2] * rn };
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = m.Sab[k] - m.n * ma[k / 3] * mb[k % 3];
    const double ssq = fmax(0.0, m.Saa - m.n * (ma[0] * ma[0] + ma[1] * ma[1] + ma[2] * ma[2]));
    const double sc[3] = { m.as[0] + ma[0], m.as[1] + ma[1], m.as[2] + ma[2] }, dc[3] = { m.bs[0] + mb[0], m.bs[1] + mb[1], m.bs[2] + mb[2] };
    int32_t flags = 0;
    if (!(ssq * rn >= 1e-12)) return KNOT_VAR0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) finite = finite && (fabs(H[i]) < INFINITY);
    double R[9], tr = NAN;
    bool own_rotation = false;
    if (rule.mode == LOC_SIM3 && finite) {
        Svd3 s; svd3(H, s);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                R[r * 3 + c] = s.V[r * 3 + 0] * s.U[c * 3 + 0] + s.V[r * 3 + 1] * s.U[c * 3 + 1] + s.V[r * 3 + 2] * s.U[c * 3 + 2];
        double d = 1.0;
        if (det3(R) < 0.0) {                                               // (:441-442) flip last row of Vt
            d = -1.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    R[r * 3 + c] = s.V[r * 3 + 0] * s.U[c * 3 + 0] + s.V[r * 3 + 1] * s.U[c * 3 + 1] - s.V[r * 3 + 2] * s.U[c * 3 + 2];
        }
        if ((s.S[1] + d * s.S[2]) <= rule.rot_open * s.S[0]) flags |= KNOT_ROT_FALLBACK;
        else { own_rotation = true; tr = s.S[0] + s.S[1] + s.S[2] * det3(R); }   // (:444, Q12)
    }
    if (!own_rotation) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rg[i];
        tr = (Rg[0] * H[0] + Rg[1] * H[3] + Rg[2] * H[6]) + (Rg[3] * H[1] + Rg[4] * H[4] + Rg[5] * H[7]) + (Rg[6] * H[2] + Rg[7] * H[5] + Rg[8] * H[8]);
    }
    const double s = tr / ssq;
    const double ratio = s / sg;
    if (!(s > 1e-6) || !(ratio >= 1.0 / rule.ratio_max) || !(ratio <= rule.ratio_max)) return flags | KNOT_SCALE;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rk[i] = R[i];
#pragma unroll
    for (int r = 0; r < 3; ++r) tk[r] = dc[r] - s * (R[r * 3] * sc[0] + R[r * 3 + 1] * sc[1] + R[r * 3 + 2] * sc[2]);
    sk = s;
    return flags;
}

// T(p) = s R p + t in the operation order of apply_sim3_kernel (ref :464)
GSF_HD Vec3 loc_map(const double* R, const double* t, double s, const Vec3& p)
{
    Vec3 o;
    o.x = s * (p.x * R[0] + p.y * R[1] + p.z * R[2]) + t[0];
    o.y = s * (p.x * R[3] + p.y * R[4] + p.z * R[5]) + t[1];
    o.z = s * (p.x * R[6] + p.y * R[7] + p.z * R[8]) + t[2];
    return o;
}

// ---- neighbour tables of one track: nl[k] = the nearest valid knot <= k, nr[k] = the nearest valid knot >= k, -1 where there is none
GSF_HD bool loc_knot_valid(int32_t flags) { return (flags & KNOT_INVALID) == 0; }
GSF_HD void loc_index_track(const int32_t* flags, int32_t K, int32_t* nl, int32_t* nr)
{
    int32_t last = -1;
    for (int32_t k = 0; k < K; ++k) { if (loc_knot_valid(flags[k])) last = k; nl[k] = last; }
    last = -1;
    for (int32_t k = K - 1; k >= 0; --k) { if (loc_knot_valid(flags[k])) last = k; nr[k] = last; }
}
// the two knots of a pose in cell k: L = nl[k], Rr = nr[k + 1] (-1: none)
GSF_HD void loc_neighbours(const int32_t* nl, const int32_t* nr, int32_t k, int32_t K, int32_t& L, int32_t& Rr)
{
    L = (k >= 0 && k < K) ? nl[k] : -1;
    Rr = (k + 1 >= 0 && k + 1 < K) ? nr[k + 1] : -1;
}
GSF_HD double loc_weight(double ts, double t0, double spacing, int32_t L, int32_t Rr)
{
    const double tl = loc_tau(t0, spacing, L), tr = loc_tau(t0, spacing, Rr);
    return (ts - tl) / (tr - tl);
}

// ---- one pose.  loc_pose_kind(L, Rr) names the case; A / B are the transforms it uses (R[9], t[3], s):
//   both (0 or LP_BRIDGED when Rr - L > 1), A = knot L, B = knot Rr:
//          pos' = T_A(p) + w (T_B(p) - T_A(p))  -- NOT (1 - w) x + w y: equal knots return T_A(p) to the bit --
//          quat' = quaternion_nlerp(R_A (x) q, R_B (x) q, w) (ref :94-105), and R_A (x) q itself where the two products are the same
//          numbers (nlerp of a quaternion with itself is that quaternion; taken exactly, equal knots return K3's bytes);
//          scale_at = s_A + w (s_B - s_A)
//   LP_HELD, A = the one knot there is: that knot alone;   LP_GLOBAL, A = the track's global transform
//   R (x) q is K3's: quat_mul(quat_from_matrix(R), q / |q|); a norm that is 0 / NaN / inf gives a NaN quaternion and LP_BAD_QUAT.
struct LocKnot { double R[9], t[3], s; };
struct LocPose { Vec3 p; Quat q; double scale; int32_t flags; };

GSF_HD int32_t loc_pose_kind(int32_t L, int32_t Rr)
{
    if (L >= 0 && Rr >= 0) return (Rr - L > 1) ? LP_BRIDGED : 0;
    return (L >= 0 || Rr >= 0) ? LP_HELD : LP_GLOBAL;
}

GSF_HD LocPose loc_blend(const Vec3& p, const Quat& qin, double w, int32_t kind, const LocKnot& A, const LocKnot& B)
{
    LocPose o;
    Quat qn; const bool ok = quat_unit(qin, qn);
    const Vec3 a = loc_map(A.R, A.t, A.s, p);
    const Quat qa = quat_mul(quat_from_matrix(A.R), qn);
    o.p = a; o.q = qa; o.scale = A.s; o.flags = kind;
    if ((kind & (LP_HELD | LP_GLOBAL)) == 0) {
        const Vec3 b = loc_map(B.R, B.t, B.s, p);
        o.p.x = a.x + w * (b.x - a.x); o.p.y = a.y + w * (b.y - a.y); o.p.z = a.z + w * (b.z - a.z);
        const Quat qb = quat_mul(quat_from_matrix(B.R), qn);
        const bool same = qa.x == qb.x && qa.y == qb.y && qa.z == qb.z && qa.w == qb.w;
        if (!same) o.q = quat_nlerp(qa, qb, w);
        o.scale = A.s + w * (B.s - A.s);
    }
    if (!ok) { o.q = Quat{ NAN, NAN, NAN, NAN }; o.flags |= LP_BAD_QUAT; }
    return o;
}

}  // namespace gsf
