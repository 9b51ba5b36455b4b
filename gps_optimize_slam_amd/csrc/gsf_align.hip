// gsf_align.hip -- GNSS positions interpolated onto the SLAM stamps: dynamic_time_alignment (EKFGPSSLAM.py:325-387), the
// step right before both the Sim3 fit and the EKF (SURVEY 8f "next-1").
//
// One 64-lane workgroup per trajectory, the GNSS track staged in LDS (t, y[3], second derivatives M[3], c': 64 B per fix;
// tracks of more than 2560 fixes are staged in a global scratch slab instead):
//   1. sort by stamp if needed (rank sort, stable by input order) and keep the first of equal stamps (np.unique, :339-346);
//   2. split at gaps > max_gps_gap_threshold (:348-352); a segment needs >= 2 fixes and stamps increasing by > 1e-9 (:364);
//   3. >= 4 fixes: not-a-knot cubic spline (scipy interp1d(kind='cubic'), :362/:368) -- the tridiagonal system for the knot
//      second derivatives is solved as three prefix scans over the rows (a Moebius scan for c', an affine scan for d', an affine
//      scan in reverse for the back substitution; all 64 lanes); 2-3 fixes: linear;
//   4. every SLAM stamp inside [t0-1e-9, t1+1e-9] (:372-373) is evaluated by its own lane (binary search of the interval);
//      stamps outside [t0, t1] get NaN like interp1d(bounds_error=False, fill_value=nan); valid = all three finite (:377-379).
// The clock-offset estimate of :336 is identically 0 and is not computed.
// NaN stamps sort last (np.argsort), which leaves the last segment without strictly increasing stamps: it is skipped (:364), as in
// the reference.  drop_masked != 0 (the chain from the geodetic log): fixes whose easting AND northing are NaN -- the mark
// gsf_gps_rows_to_utm_batch_dev leaves on rows that load_gps_data removes before the projection (:259-264) -- never reach the
// spline, exactly as if the loader had removed them.
#include "gsf_internal.hpp"
#include "gsf_ekf_core.hpp"
#include "gsf_wave_common.hpp"   // DPP scan stages, lane broadcasts

using namespace gsf;

namespace {

constexpr int ALIGN_THREADS = 64;

// The staging area is LDS when the track fits (<= 2 560 fixes), else a slab of global scratch.  The body is a template over the pointer
// type: with one generic pointer for both, every access of the serial spline sweeps was a FLAT instruction (hundreds of cycles of
// latency per dependent step instead of an LDS access) -- 93 of the kernel's 115 us.
// SEARCH (the clock-offset search below): track b is an argument, every stamp of the log is shifted by tau as it is staged (:338), gps_keep
// (may be NULL) drops fixes next to the loader's NaN mark, and nothing is evaluated or written: the splines stay in the staging area with one
// descriptor per segment in W[first fix of the segment] (its last fix; -(last fix) - 1 for a segment that is not interpolated), read by
// aligned_at.  Returns the number of staged fixes (0: no fix is aligned).  The alignment entries instantiate SEARCH = false.
template <class StagePtr, bool SEARCH = false>
__device__ __forceinline__ int time_align_body(StagePtr lds, const int64_t b, const double* __restrict__ slam_t, const int64_t* __restrict__ slam_off,
                                               const double* __restrict__ gps_t, const double* __restrict__ gps_p,
                                               const int64_t* __restrict__ gps_off, double max_gap, int max_g, int drop_masked,
                                               double* __restrict__ aligned, uint8_t* __restrict__ valid, int32_t* __restrict__ status,
                                               const double tau = 0.0, const uint8_t* __restrict__ gps_keep = nullptr);

__global__ __launch_bounds__(ALIGN_THREADS) void time_align_kernel(const double* __restrict__ slam_t, const int64_t* __restrict__ slam_off,
                                                                    const double* __restrict__ gps_t, const double* __restrict__ gps_p,
                                                                    const int64_t* __restrict__ gps_off, double max_gap, int max_g, int drop_masked,
                                                                    double* __restrict__ gscratch, double* __restrict__ aligned,
                                                                    uint8_t* __restrict__ valid, int32_t* __restrict__ status)
{
    extern __shared__ double lds_[];
    typedef __attribute__((address_space(3))) double* LdsPtr;
    if (gscratch) time_align_body<double*>(gscratch + (size_t)blockIdx.x * 8 * (size_t)max_g, blockIdx.x, slam_t, slam_off, gps_t, gps_p, gps_off, max_gap, max_g, drop_masked, aligned, valid, status);
    else time_align_body<LdsPtr>((LdsPtr)lds_, blockIdx.x, slam_t, slam_off, gps_t, gps_p, gps_off, max_gap, max_g, drop_masked, aligned, valid, status);
}

// one stamp t inside [x[0], x[m-1]] of a built segment: scipy's cubic (knot second derivatives Ms) or linear evaluation
template <class StagePtr>
__device__ __forceinline__ void spline_at(const StagePtr x, const StagePtr y, const StagePtr Ms, const int m, const bool cubic, const double t,
                                          double& v0, double& v1, double& v2)
{
    if (cubic) {
        int lo = 0, hi = m - 1;                      // interval [x[lo], x[lo+1]] containing t
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (x[mid] <= t) lo = mid; else hi = mid; }
        const double hh = x[lo + 1] - x[lo], A = (x[lo + 1] - t) / hh, Bc = (t - x[lo]) / hh;
        const double ca = (A * A * A - A) * hh * hh / 6.0, cb = (Bc * Bc * Bc - Bc) * hh * hh / 6.0;
        v0 = A * y[lo * 3] + Bc * y[(lo + 1) * 3] + ca * Ms[lo * 3] + cb * Ms[(lo + 1) * 3];
        v1 = A * y[lo * 3 + 1] + Bc * y[(lo + 1) * 3 + 1] + ca * Ms[lo * 3 + 1] + cb * Ms[(lo + 1) * 3 + 1];
        v2 = A * y[lo * 3 + 2] + Bc * y[(lo + 1) * 3 + 2] + ca * Ms[lo * 3 + 2] + cb * Ms[(lo + 1) * 3 + 2];
    } else {
        // scipy _call_linear: hi = clip(searchsorted(x, t, 'left'), 1, m-1); lo = hi-1
        int hi = 0;
        while (hi < m && x[hi] < t) ++hi;
        hi = hi < 1 ? 1 : (hi > m - 1 ? m - 1 : hi);
        const int lo = hi - 1;
        const double dx = x[hi] - x[lo], dtq = t - x[lo];
        v0 = (y[hi * 3] - y[lo * 3]) / dx * dtq + y[lo * 3];
        v1 = (y[hi * 3 + 1] - y[lo * 3 + 1]) / dx * dtq + y[lo * 3 + 1];
        v2 = (y[hi * 3 + 2] - y[lo * 3 + 2]) / dx * dtq + y[lo * 3 + 2];
    }
}

template <class StagePtr, bool SEARCH>
__device__ __forceinline__ int time_align_body(StagePtr lds, const int64_t b, const double* __restrict__ slam_t, const int64_t* __restrict__ slam_off,
                                               const double* __restrict__ gps_t, const double* __restrict__ gps_p,
                                               const int64_t* __restrict__ gps_off, double max_gap, int max_g, int drop_masked,
                                               double* __restrict__ aligned, uint8_t* __restrict__ valid, int32_t* __restrict__ status,
                                               const double tau, const uint8_t* __restrict__ gps_keep)
{
    const int lane = threadIdx.x;
    const int64_t s0 = slam_off[b], ns = slam_off[b + 1] - s0;
    const int64_t g0 = gps_off[b];
    int ng = (int)(gps_off[b + 1] - g0);
    const double* st = slam_t + s0;
    double* al = aligned + s0 * 3;
    uint8_t* va = valid + s0;
    if (!SEARCH) {
        for (int64_t i = lane; i < ns; i += ALIGN_THREADS) { al[i * 3] = NAN; al[i * 3 + 1] = NAN; al[i * 3 + 2] = NAN; va[i] = 0; }   // :331
        if (status && lane == 0) status[b] = 0;
    }
    if (ns == 0 || ng < 2) return 0;                                     // :332-334
    if (ng > max_g) { if (!SEARCH && status && lane == 0) status[b] = 1; return 0; }  // does not fit the LDS staging: reported, not computed
    StagePtr T = lds;                   // [ng] stamps
    StagePtr Y = T + max_g;             // [ng][3] positions
    StagePtr M = Y + 3 * (size_t)max_g; // [ng][3] second derivatives (cubic segments)
    StagePtr W = M + 3 * (size_t)max_g; // [ng] scratch: c' of the Thomas sweep / sort keys
    // ---- rows the loader would have removed (drop_masked): the kept fixes' input indices, compacted in input order into M (free
    // until the spline runs)
    if (drop_masked) {
        int kept = 0;
        for (int k0 = 0; k0 < ng; k0 += ALIGN_THREADS) {
            const int k = k0 + lane;
            bool keep = k < ng && !(isnan(gps_p[(g0 + k) * 3]) && isnan(gps_p[(g0 + k) * 3 + 1]));
            if (SEARCH && keep && gps_keep) keep = gps_keep[g0 + k] != 0;
            const unsigned long long m = __ballot(keep);
            if (keep) M[kept + __popcll(m & ((1ull << lane) - 1ull))] = (double)k;
            kept += __popcll(m);
        }
        __syncthreads();
        ng = kept;
        if (ng < 2) return 0;                                            // :332-334 on the rows that survive the loader
    }
#define GSF_AL_SRC(k) (g0 + (drop_masked ? (int)M[k] : (k)))
#define GSF_AL_T(k) (SEARCH ? gps_t[GSF_AL_SRC(k)] + tau : gps_t[GSF_AL_SRC(k)])   // adjusted_gps_times (:338)
    // ---- stage + order: rank of fix k = #{j : t_j < t_k or (t_j == t_k and j < k)} (stable argsort, :339); NaN stamps rank last
    bool sorted = true;
    for (int k = lane; k < ng; k += ALIGN_THREADS) {
        const double tk = GSF_AL_T(k);
        W[k] = tk;
        if (k > 0 && !(GSF_AL_T(k - 1) < tk)) sorted = false;
    }
    __syncthreads();
    sorted = (__ballot(!sorted) == 0ull);
    if (sorted) {
        for (int k = lane; k < ng; k += ALIGN_THREADS) {
            const int64_t src = GSF_AL_SRC(k);
            T[k] = W[k];
            Y[k * 3] = gps_p[src * 3]; Y[k * 3 + 1] = gps_p[src * 3 + 1]; Y[k * 3 + 2] = gps_p[src * 3 + 2];
        }
    } else {
        for (int k = lane; k < ng; k += ALIGN_THREADS) {
            const double tk = W[k];
            const bool nk = isnan(tk);
            int rank = 0;
            for (int j = 0; j < ng; ++j) {
                const double tj = W[j];
                const bool nj = isnan(tj);
                rank += (tj < tk || (!nj && nk) || ((tj == tk || (nj && nk)) && j < k)) ? 1 : 0;
            }
            const int64_t src = GSF_AL_SRC(k);
            T[rank] = tk;
            Y[rank * 3] = gps_p[src * 3]; Y[rank * 3 + 1] = gps_p[src * 3 + 1]; Y[rank * 3 + 2] = gps_p[src * 3 + 2];
        }
    }
#undef GSF_AL_T
#undef GSF_AL_SRC
    __syncthreads();
    // ---- np.unique(return_index=True): keep the first fix of every run of equal stamps (:341-346).  Compaction in place by
    // one lane -- duplicates are rare and ng is a few hundred.
    int nu = ng;
    if (!sorted) {
        if (lane == 0) {
            int w = 0;
            for (int k = 0; k < ng; ++k) {
                if (w > 0 && T[k] == T[w - 1]) continue;
                if (w != k) { T[w] = T[k]; Y[w * 3] = Y[k * 3]; Y[w * 3 + 1] = Y[k * 3 + 1]; Y[w * 3 + 2] = Y[k * 3 + 2]; }
                ++w;
            }
            W[0] = (double)w;
        }
        __syncthreads();
        nu = (int)W[0];
        __syncthreads();
    }
    if (nu < 2) return 0;                                                // :343-345
    // ---- segments (:348-352), processed one after the other (usually 1-3 per track)
    int seg_s = 0;
    while (seg_s < nu) {
        // end of the segment = first k >= seg_s with T[k+1] - T[k] > max_gap (or the last fix): 64 gaps per step, first set bit of the ballot
        int seg_e = nu - 1;
        for (int k0 = seg_s; k0 + 1 < nu; k0 += ALIGN_THREADS) {
            const int k = k0 + lane;
            const unsigned long long gaps = __ballot(k + 1 < nu && (T[k + 1] - T[k] > max_gap));
            if (gaps != 0ull) { seg_e = k0 + __ffsll((long long)gaps) - 1; break; }
        }
        const int m = seg_e - seg_s + 1;
        bool usable = false;
        if (m >= 2) {                                                    // :360
            bool inc = true;
            for (int k = seg_s + lane; k < seg_e; k += ALIGN_THREADS) if (!(T[k + 1] - T[k] > 1e-9)) inc = false;     // :364
            inc = (__ballot(!inc) == 0ull);
            usable = inc;
            if (inc) {
                const StagePtr x = T + seg_s;
                const StagePtr y = Y + (size_t)seg_s * 3;
                StagePtr Ms = M + (size_t)seg_s * 3;
                const bool cubic = m >= 4;                               // :362
                if (cubic) {
                    // knot second derivatives M_0..M_{m-1}:  h[i-1] M[i-1] + 2(h[i-1]+h[i]) M[i] + h[i] M[i+1] = 6 (d[i]-d[i-1]),
                    // not-a-knot ends folded into the first / last interior row.  Lanes 0..2 = components; c' is shared.
                    // right-hand sides 6 (d[i+1] - d[i]), d = divided differences: independent per row, all lanes (their divisions were
                    // most of the serial sweep's time); parked where the sweep leaves d'_i
                    const int kk = m - 2;
                    for (int i = lane; i < kk; i += ALIGN_THREADS) {
                        const double hl = x[i + 1] - x[i], hr = x[i + 2] - x[i + 1];
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            Ms[(i + 1) * 3 + c] = 6.0 * ((y[(i + 2) * 3 + c] - y[(i + 1) * 3 + c]) / hr - (y[(i + 1) * 3 + c] - y[i * 3 + c]) / hl);
                    }
                    __syncthreads();
                    // The tridiagonal solve as three prefix scans over the rows (64 per step, all lanes), instead of two serial sweeps on
                    // three lanes: with rows scaled by 1/b_i, the forward elimination's c'_i = c_i / (1 - a_i c'_{i-1}) is a Moebius
                    // recurrence (2x2 matrix prefix products), d'_i = (r_i - a_i d'_{i-1}) / (b_i - a_i c'_{i-1}) is affine in d'_{i-1}
                    // once the c' are known (one multiplier for the three components), and the back substitution
                    // M_i = d'_i - c'_i M_{i+1} is affine in reverse order.  Rows are diagonally dominant (|a| + |c| <= b / 2 inside, the
                    // not-a-knot ends included for increasing stamps), so the products stay O(1).
                    const double r0 = (x[1] - x[0]) / (x[2] - x[1]);
                    const double r1 = (x[m - 1] - x[m - 2]) / (x[m - 2] - x[m - 3]);
                    StagePtr cp = W + seg_s;                             // c'_i
                    double c_in = 0.0, d_in0 = 0.0, d_in1 = 0.0, d_in2 = 0.0;
                    for (int c0 = 0; c0 < kk; c0 += ALIGN_THREADS) {
                        const int i = c0 + lane;
                        const bool act = i < kk;
                        const int ic = act ? i : kk - 1;
                        const double hl = x[ic + 1] - x[ic], hr = x[ic + 2] - x[ic + 1];
                        double aa = hl, bb = 2.0 * (hl + hr), cc = hr;
                        if (ic == 0) { bb += aa * (1.0 + r0); cc -= aa * r0; aa = 0.0; }
                        if (ic == kk - 1) { bb += cc * (1.0 + r1); aa -= cc * r1; cc = 0.0; }
                        const double rb = fast_rcp(bb);
                        // f_i(c) = (0 c + cc/bb) / (-(aa/bb) c + 1); idle lanes carry the identity map
                        double A = act ? 0.0 : 1.0, Bm = act ? cc * rb : 0.0, Cm = act ? -(aa * rb) : 0.0, Dm = 1.0;
#define GSF_AL_MSTAGE(CTRL, RM) {                                                                                              \
                        const double oA = dpp<CTRL, RM>(1.0, A), oB = dpp0<CTRL, RM>(Bm), oC = dpp0<CTRL, RM>(Cm), oD = dpp<CTRL, RM>(1.0, Dm); \
                        const double nA = A * oA + Bm * oC, nB = A * oB + Bm * oD, nC = Cm * oA + Dm * oC, nD = Cm * oB + Dm * oD;                  \
                        A = nA; Bm = nB; Cm = nC; Dm = nD; }
                        GSF_SCAN_STAGES(GSF_AL_MSTAGE)
#undef GSF_AL_MSTAGE
                        const double cpi = (A * c_in + Bm) * fast_rcp(Cm * c_in + Dm);
                        const double cprev = prev_lane(c_in, cpi);
                        const double rden = fast_rcp(bb - aa * cprev);
                        double al = act ? -(aa * rden) : 1.0;
                        double be0 = act ? Ms[(ic + 1) * 3] * rden : 0.0, be1 = act ? Ms[(ic + 1) * 3 + 1] * rden : 0.0, be2 = act ? Ms[(ic + 1) * 3 + 2] * rden : 0.0;
#define GSF_AL_ASTAGE(CTRL, RM) { const double oa = dpp<CTRL, RM>(1.0, al), o0 = dpp0<CTRL, RM>(be0), o1 = dpp0<CTRL, RM>(be1), o2 = dpp0<CTRL, RM>(be2); \
                                  be0 = al * o0 + be0; be1 = al * o1 + be1; be2 = al * o2 + be2; al = al * oa; }
                        GSF_SCAN_STAGES(GSF_AL_ASTAGE)
                        const double dp0 = al * d_in0 + be0, dp1 = al * d_in1 + be1, dp2 = al * d_in2 + be2;
                        if (act) { cp[i] = cpi; Ms[(i + 1) * 3] = dp0; Ms[(i + 1) * 3 + 1] = dp1; Ms[(i + 1) * 3 + 2] = dp2; }
                        const int L = (kk - c0 < ALIGN_THREADS) ? (kk - c0 - 1) : ALIGN_THREADS - 1;
                        c_in = lane_bcast(cpi, L); d_in0 = lane_bcast(dp0, L); d_in1 = lane_bcast(dp1, L); d_in2 = lane_bcast(dp2, L);
                    }
                    __syncthreads();
                    double x_in0 = 0.0, x_in1 = 0.0, x_in2 = 0.0;
                    for (int c0 = 0; c0 < kk; c0 += ALIGN_THREADS) {         // back substitution, rows in reverse: j = kk-1-i
                        const int j = c0 + lane;
                        const bool act = j < kk;
                        const int i = act ? kk - 1 - j : 0;
                        double al = act ? -cp[i] : 1.0;
                        double be0 = act ? Ms[(i + 1) * 3] : 0.0, be1 = act ? Ms[(i + 1) * 3 + 1] : 0.0, be2 = act ? Ms[(i + 1) * 3 + 2] : 0.0;
                        GSF_SCAN_STAGES(GSF_AL_ASTAGE)
#undef GSF_AL_ASTAGE
                        const double m0 = al * x_in0 + be0, m1 = al * x_in1 + be1, m2 = al * x_in2 + be2;
                        if (act) { Ms[(i + 1) * 3] = m0; Ms[(i + 1) * 3 + 1] = m1; Ms[(i + 1) * 3 + 2] = m2; }
                        const int L = (kk - c0 < ALIGN_THREADS) ? (kk - c0 - 1) : ALIGN_THREADS - 1;
                        x_in0 = lane_bcast(m0, L); x_in1 = lane_bcast(m1, L); x_in2 = lane_bcast(m2, L);
                    }
                    __syncthreads();
                    if (lane < 3) {
                        const int c = lane;
                        Ms[c] = Ms[3 + c] * (1.0 + r0) - Ms[6 + c] * r0;
                        Ms[(m - 1) * 3 + c] = Ms[(m - 2) * 3 + c] * (1.0 + r1) - Ms[(m - 3) * 3 + c] * r1;
                    }
                }
                __syncthreads();
                if (!SEARCH) {
                    const double t0 = x[0], t1 = x[m - 1];
                    for (int64_t i = lane; i < ns; i += ALIGN_THREADS) {
                        const double t = st[i];
                        if (!(t >= t0 - 1e-9 && t <= t1 + 1e-9)) continue;   // :372-373
                        double v0 = NAN, v1 = NAN, v2 = NAN;
                        if (t >= t0 && t <= t1) spline_at(x, y, Ms, m, cubic, t, v0, v1, v2);
                        al[i * 3] = v0; al[i * 3 + 1] = v1; al[i * 3 + 2] = v2;                       // :375
                        if (!(isnan(v0) || isnan(v1) || isnan(v2))) va[i] = 1;                          // :377-379 (only ever set, never cleared)
                    }
                    __syncthreads();
                }
            }
        }
        if (SEARCH) {                                                    // (c' of this segment has been consumed: its first slot takes the descriptor)
            if (lane == 0) W[seg_s] = usable ? (double)seg_e : -(double)seg_e - 1.0;
        }
        seg_s = seg_e + 1;
    }
    if (SEARCH) __syncthreads();
    return nu;
}

// ---- clock-offset search (gsf_clock_offset_search_dev): for track b and candidate k, "how well does the track fit the fixes if the GNSS
// clock is shifted by tau[b][k]" -- dynamic_time_alignment with adjusted_gps_times = gps_t + tau (:338), the row choice of :973-998,
// compute_sim3_transform (:428-459) and the RMSE of the fit's residuals.  One 64-lane workgroup per (b, k): the log is staged and its splines
// are built by time_align_body<SEARCH>; the aligned rows are never stored -- the three passes over the poses (row walk, moments, residuals)
// evaluate the splines again, 64 poses at a time -- so a problem writes two numbers.  A second launch (one workgroup per track) takes the
// arg-min, the parabola and the status bits, and repeats the best candidate's fit for R, t, s.
struct ClkArgs {
    const double* ts; const double* pos; const int64_t* slam_off;
    const double* gps_t; const double* gps_p; const uint8_t* gps_keep; const int64_t* gps_off;
    const double* tau0; double dtau; int K;
    double max_gap; int max_g; int min_rows; double flat_thr; FitRows rows;
    double* J; int32_t* n_rows; int32_t* best_k; double* tau_best; double* tau_refined; double* R; double* t; double* s; int32_t* clk_status;
    int64_t B;
};

// tau[b][k] = tau0[b] + (double)k * dtau: a product and a sum, each rounded once (numpy's tau0 + k * dtau), never one fused operation
__device__ __forceinline__ double clk_tau(const ClkArgs& a, const int64_t b, const int k)
{
    double step = (double)k * a.dtau;
    asm volatile("" : "+v"(step));
    return (a.tau0 ? a.tau0[b] : 0.0) + step;
}

// the aligned fix at stamp t from the splines time_align_body<SEARCH> left in the staging area: the segments are visited in order and a later
// one overwrites an earlier one, as the alignment kernel's stores do.  Returns valid = all three components finite (:377-379).
template <class StagePtr>
__device__ __forceinline__ bool aligned_at(const StagePtr lds, const int max_g, const int nu, const double t, const bool act, double& v0, double& v1, double& v2)
{
    const StagePtr T = lds, Y = T + max_g, M = Y + 3 * (size_t)max_g, W = M + 3 * (size_t)max_g;
    v0 = NAN; v1 = NAN; v2 = NAN;
    for (int s = 0; s < nu;) {
        const double d = W[s];                                           // wave-uniform
        const int e = d >= 0.0 ? (int)d : (int)(-d) - 1;
        if (d >= 0.0) {
            const int m = e - s + 1;
            const StagePtr x = T + s;
            const double t0 = x[0], t1 = x[m - 1];
            if (act && t >= t0 - 1e-9 && t <= t1 + 1e-9) {              // :372-373
                v0 = NAN; v1 = NAN; v2 = NAN;
                if (t >= t0 && t <= t1) spline_at(x, Y + (size_t)s * 3, M + (size_t)s * 3, m, m >= 4, t, v0, v1, v2);
            }
        }
        s = e + 1;
    }
    return act && !(isnan(v0) || isnan(v1) || isnan(v2));
}

// one (track, candidate) problem.  write_fit == false: J[b][k] and n_rows[b][k]; true: R[b], t[b], s[b] of that candidate.
template <class StagePtr>
__device__ __forceinline__ void clk_problem(const StagePtr lds, const ClkArgs& a, const int64_t b, const int k, const bool write_fit)
{
    const int lane = threadIdx.x;
    const int64_t s0 = uniform64(a.slam_off[b]);
    const int ns = (int)(uniform64(a.slam_off[b + 1]) - s0);
    const double* __restrict__ st = a.ts + s0;
    const double* __restrict__ ps = a.pos + s0 * 3;
    const int nu = time_align_body<StagePtr, true>(lds, b, a.ts, a.slam_off, a.gps_t, a.gps_p, a.gps_off, a.max_gap, a.max_g, 1, nullptr, nullptr, nullptr,
                                                  clk_tau(a, b, k), a.gps_keep);
    double Jv = NAN, Rb[9], tb[3], sb = NAN;
#pragma unroll
    for (int c = 0; c < 9; ++c) Rb[c] = NAN;
    tb[0] = tb[1] = tb[2] = NAN;
    int total = 0;
    if (nu >= 2) {
        const FitRows rule = a.rows;
        // pass 1: the first valid row (GNSS-side shift, segment_start_time :988) and, under the reference's rule, the first gap of the valid
        // rows and what the duration limit keeps (the walk of sim3_rows_kernel, gsf_robust.hip)
        RowScan rs{ false, 0.0, 0, 0 };
        bool gap_found = false, have_t0 = false, carry_in_T = false;
        int row_end = ns, nF = 0, nT = 0;
        double tlim = 0.0, bs0 = 0.0, bs1 = 0.0, bs2 = 0.0;
        for (int c0 = 0; c0 < ns && !gap_found; c0 += 64) {
            const int i = c0 + lane;
            const double t = st[i < ns ? i : ns - 1];
            double v0, v1, v2;
            const bool ok = aligned_at(lds, a.max_g, nu, t, i < ns, v0, v1, v2);
            const u64 m = __ballot(ok);
            if (m == 0ull) continue;
            if (!have_t0) {
                const int f = __ffsll((long long)m) - 1;
                tlim = lane_bcast(t, f) + rule.max_dur;                   // segment_start_time + max_dur (:988-990)
                bs0 = lane_bcast(v0, f); bs1 = lane_bcast(v1, f); bs2 = lane_bcast(v2, f);
                have_t0 = true;
            }
            if (rule.mode == 0) { nF += __popcll(m); continue; }
            bool in_chunk = false;
            gap_found = rows_gap_in_chunk(rs, m, t, ok, lane, c0, rule.max_gap, row_end, nF, in_chunk);
            const u64 tm = __ballot(ok && t <= tlim);
            if (gap_found) {
                if (in_chunk) nT += __popcll(tm & bits(0, row_end - c0 - 1));
                else nT -= carry_in_T ? 1 : 0;                            // the row in front of the gap is the carried one: it was counted, and V[:k] leaves it out
            } else {
                nT += __popcll(tm);
                carry_in_T = ((tm >> (63 - __clzll((long long)m))) & 1ull) != 0ull;
            }
        }
        bool use_tlim = false, few = false;
        if (rule.mode != 0) {
            if (!gap_found) nF = rs.nvalid;
            use_tlim = true;
            if (nF < rule.min_samples) {                                  // :983
                use_tlim = false;
                if (!gap_found) few = true;                               // :975
                else row_end = ns;                                        // :984 (counted in pass 2; :975 if that is short as well)
            } else if (nT < rule.min_samples) use_tlim = false;           // :993-995
        }
        // pass 2: moments of the chosen rows, shifted by pose 0 / the first valid fix
        const double as0 = ps[0], as1 = ps[1], as2 = ps[2];
        double Sa0 = 0, Sa1 = 0, Sa2 = 0, Sb0 = 0, Sb1 = 0, Sb2 = 0, Saa = 0;
        double Sab[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        const int pass_end = row_end < ns ? row_end : ns;
        for (int c0 = 0; c0 < pass_end; c0 += 64) {
            const int i = c0 + lane;
            const int ic = i < ns ? i : ns - 1;
            const double t = st[ic];
            double v0, v1, v2;
            const bool ok = aligned_at(lds, a.max_g, nu, t, i < ns, v0, v1, v2);
            const bool o = ok && i < row_end && (!use_tlim || t <= tlim);
            total += __popcll(__ballot(o));
            const double a0 = o ? ps[ic * 3] - as0 : 0.0, a1 = o ? ps[ic * 3 + 1] - as1 : 0.0, a2 = o ? ps[ic * 3 + 2] - as2 : 0.0;
            const double b0 = o ? v0 - bs0 : 0.0, b1 = o ? v1 - bs1 : 0.0, b2 = o ? v2 - bs2 : 0.0;
            Sa0 += a0; Sa1 += a1; Sa2 += a2; Sb0 += b0; Sb1 += b1; Sb2 += b2;
            Saa += a0 * a0 + a1 * a1 + a2 * a2;
            Sab[0] += a0 * b0; Sab[1] += a0 * b1; Sab[2] += a0 * b2;
            Sab[3] += a1 * b0; Sab[4] += a1 * b1; Sab[5] += a1 * b2;
            Sab[6] += a2 * b0; Sab[7] += a2 * b1; Sab[8] += a2 * b2;
        }
        if (rule.mode != 0 && total < rule.min_samples) few = true;      // fewer than min_samples valid rows in all: ValueError (:975, :997)
        const int need = a.min_rows > 0 ? a.min_rows : rule.min_samples;
        if (!few && total >= 3 && total >= need) {                        // ref :430
            const Sums16 S = wave_sum16(Sa0, Sa1, Sa2, Sb0, Sb1, Sb2, Saa, Sab[0], Sab[1], Sab[2], Sab[3], Sab[4], Sab[5], Sab[6], Sab[7], Sab[8], lane);
            const double n = (double)total, rn = fast_rcp(n);
            const double ma[3] = { S.v[0] * rn, S.v[1] * rn, S.v[2] * rn };
            const double mb[3] = { S.v[3] * rn, S.v[4] * rn, S.v[5] * rn };
            const double ssq = fmax(0.0, S.v[6] - n * (ma[0] * ma[0] + ma[1] * ma[1] + ma[2] * ma[2]));
            double H[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) H[c] = S.v[7 + c] - n * ma[c / 3] * mb[c % 3];
            const double sc[3] = { as0 + ma[0], as1 + ma[1], as2 + ma[2] }, dc[3] = { bs0 + mb[0], bs1 + mb[1], bs2 + mb[2] };
            double Rf[9], tf[3], sf = NAN;
            const int32_t fit = umeyama_finalize<true>(H, ssq, sc, dc, n, Rf, tf, sf);   // every lane redundantly (wave-uniform inputs)
            if (fit != SIM3_NONE) {
#pragma unroll
                for (int c = 0; c < 9; ++c) Rb[c] = Rf[c];
                tb[0] = tf[0]; tb[1] = tf[1]; tb[2] = tf[2]; sb = sf;
                if (!write_fit) {
                    // pass 3: residuals dst - (s R src + t) of the same rows, about the two centroids (t = dc - s R sc, :451)
                    double r2 = 0.0;
                    for (int c0 = 0; c0 < pass_end; c0 += 64) {
                        const int i = c0 + lane;
                        const int ic = i < ns ? i : ns - 1;
                        const double t = st[ic];
                        double v0, v1, v2;
                        const bool ok = aligned_at(lds, a.max_g, nu, t, i < ns, v0, v1, v2);
                        const bool o = ok && i < row_end && (!use_tlim || t <= tlim);
                        const double a0 = ps[ic * 3] - sc[0], a1 = ps[ic * 3 + 1] - sc[1], a2 = ps[ic * 3 + 2] - sc[2];
                        const double e0 = (v0 - dc[0]) - sf * (Rf[0] * a0 + Rf[1] * a1 + Rf[2] * a2);
                        const double e1 = (v1 - dc[1]) - sf * (Rf[3] * a0 + Rf[4] * a1 + Rf[5] * a2);
                        const double e2 = (v2 - dc[2]) - sf * (Rf[6] * a0 + Rf[7] * a1 + Rf[8] * a2);
                        r2 += o ? e0 * e0 + e1 * e1 + e2 * e2 : 0.0;
                    }
                    Jv = sqrt(wave_sum(r2) / n);
                }
            }
        }
    }
    if (lane == 0) {
        if (write_fit) {
            for (int c = 0; c < 9; ++c) a.R[b * 9 + c] = Rb[c];
            a.t[b * 3] = tb[0]; a.t[b * 3 + 1] = tb[1]; a.t[b * 3 + 2] = tb[2]; a.s[b] = sb;
        } else {
            a.J[b * a.K + k] = Jv;
            if (a.n_rows) a.n_rows[b * a.K + k] = total;
        }
    }
    __syncthreads();                                                      // the staging area is reused by the workgroup's next problem
}

// arg-min of J[b][:], the parabola through (tau, J^2) at its neighbours, the status bits.  Returns best_k (wave-uniform).
__device__ __forceinline__ int clk_pick(const ClkArgs& a, const int64_t b)
{
    const int lane = threadIdx.x;
    const double* __restrict__ Jb = a.J + b * a.K;
    double best = INFINITY, top = -INFINITY; int bk = 0x7fffffff;
    for (int k = lane; k < a.K; k += 64) {
        const double j = Jb[k];
        if (isnan(j)) continue;
        if (bk == 0x7fffffff || j < best) { best = j; bk = k; }           // (k ascends: the first of equal values stays)
        top = fmax(top, j);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double ob = __shfl_xor(best, d, 64), ot = __shfl_xor(top, d, 64); const int ok = __shfl_xor(bk, d, 64);
        if (ok != 0x7fffffff && (bk == 0x7fffffff || ob < best || (ob == best && ok < bk))) { best = ob; bk = ok; }
        top = fmax(top, ot);
    }
    const bool none = bk == 0x7fffffff;
    if (none) bk = -1;
    if (lane == 0) {
        int32_t stw = 0;
        double tb_ = NAN, tr_ = NAN;
        if (none) stw = GSF_CLK_NONE;
        else {
            if (a.K > 1 && (bk == 0 || bk == a.K - 1)) stw |= GSF_CLK_AT_EDGE;
            if (a.flat_thr > 0.0 && top - best < a.flat_thr) stw |= GSF_CLK_FLAT;
            tb_ = clk_tau(a, b, bk); tr_ = tb_;
            if (bk > 0 && bk < a.K - 1) {
                const double ja = Jb[bk - 1], jc = Jb[bk + 1];
                const double qa = ja * ja, qm = best * best, qc = jc * jc, den = qa - 2.0 * qm + qc;
                if (!isnan(ja) && !isnan(jc) && den > 0.0) tr_ = tb_ + 0.5 * a.dtau * (qa - qc) / den;
            }
        }
        a.best_k[b] = bk; a.tau_best[b] = tb_; a.tau_refined[b] = tr_; a.clk_status[b] = stw;
    }
    return bk;
}

// pick == 0: problem p = (b, k) = (p / K, p % K) of the sweep; pick == 1: problem p = track b after the sweep.  A workgroup takes problems
// blockIdx.x, + gridDim.x, ...: the launcher gives every problem its own workgroup when the logs are staged in LDS, and as many workgroups as
// the scratch slab has rows when they are staged there.
__global__ __launch_bounds__(ALIGN_THREADS) void clock_search_kernel(const ClkArgs a, const int pick, double* __restrict__ gscratch)
{
    extern __shared__ double lds_[];
    typedef __attribute__((address_space(3))) double* LdsPtr;
    const int64_t total = pick ? a.B : a.B * a.K;
    for (int64_t p = blockIdx.x; p < total; p += gridDim.x) {
        int64_t b = p; int k = 0;
        if (!pick) { b = p / a.K; k = (int)(p - b * a.K); }
        else {
            k = clk_pick(a, b);
            if (!a.R) continue;
            if (k < 0) {
                if (threadIdx.x == 0) {
                    for (int c = 0; c < 9; ++c) a.R[b * 9 + c] = NAN;
                    a.t[b * 3] = a.t[b * 3 + 1] = a.t[b * 3 + 2] = NAN; a.s[b] = NAN;
                }
                continue;
            }
        }
        if (gscratch) clk_problem<double*>(gscratch + (size_t)blockIdx.x * 8 * (size_t)a.max_g, a, b, k, pick != 0);
        else clk_problem<LdsPtr>((LdsPtr)lds_, a, b, k, pick != 0);
    }
}

}  // namespace

extern "C" {

static int time_align_launch(gsf_ctx* ctx, const double* slam_t, const int64_t* slam_offsets, const double* gps_t, const double* gps_p,
                             const int64_t* gps_offsets, int64_t B, int32_t max_gps_per_trajectory, double max_gps_gap_threshold,
                             int drop_masked, double* aligned, uint8_t* valid, int32_t* status)
{
    GSF_REQUIRE(ctx && slam_offsets && gps_offsets && aligned && valid, "NULL argument");
    GSF_REQUIRE(B >= 0 && B <= 0x7fffffff, "bad B");
    GSF_REQUIRE(max_gps_per_trajectory >= 2 && max_gps_per_trajectory <= (1 << 24), "max_gps_per_trajectory out of range");
    if (B == 0) return GSF_OK;
    GSF_HIP(hipSetDevice(ctx->device));
    size_t lds = (size_t)max_gps_per_trajectory * 8 * sizeof(double);                // T + Y(3) + M(3) + W
    double* gscratch = nullptr;
    if (max_gps_per_trajectory > 2560) {                                             // does not fit 160 KB of LDS: stage in HBM scratch
        int rc = ensure_workspace(ctx, GSF_WS_KERNEL, lds * (size_t)B);
        if (rc) return rc;
        gscratch = workspace<double>(ctx, GSF_WS_KERNEL); lds = 0;
    } else if (lds > 64 * 1024) {
        GSF_HIP(hipFuncSetAttribute((const void*)time_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL(time_align_kernel, dim3((unsigned)B), dim3(ALIGN_THREADS), lds, ctx->stream, slam_t, slam_offsets, gps_t, gps_p, gps_offsets,
                       max_gps_gap_threshold, (int)max_gps_per_trajectory, drop_masked, gscratch, aligned, valid, status);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

int gsf_time_align_batch_dev(gsf_ctx* ctx, const double* slam_t, const int64_t* slam_offsets, const double* gps_t, const double* gps_p,
                             const int64_t* gps_offsets, int64_t B, int32_t max_gps_per_trajectory, double max_gps_gap_threshold,
                             double* aligned, uint8_t* valid, int32_t* status)
{
    return time_align_launch(ctx, slam_t, slam_offsets, gps_t, gps_p, gps_offsets, B, max_gps_per_trajectory, max_gps_gap_threshold, 0, aligned, valid, status);
}

int gsf_time_align_loaded_rows_batch_dev(gsf_ctx* ctx, const double* slam_t, const int64_t* slam_offsets, const double* gps_t, const double* gps_p,
                                         const int64_t* gps_offsets, int64_t B, int32_t max_gps_per_trajectory, double max_gps_gap_threshold,
                                         double* aligned, uint8_t* valid, int32_t* status)
{
    return time_align_launch(ctx, slam_t, slam_offsets, gps_t, gps_p, gps_offsets, B, max_gps_per_trajectory, max_gps_gap_threshold, 1, aligned, valid, status);
}

int gsf_time_align_batch(gsf_ctx* ctx, const double* slam_t, const int64_t* slam_offsets, const double* gps_t, const double* gps_p,
                         const int64_t* gps_offsets, int64_t B, double max_gps_gap_threshold, double* aligned, uint8_t* valid, int32_t* status)
{
    GSF_REQUIRE(ctx && slam_offsets && gps_offsets && B >= 0, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t ns = slam_offsets[B], ng = gps_offsets[B];
    GSF_REQUIRE(ns >= 0 && ng >= 0 && (ns == 0 || (slam_t && aligned && valid)) && (ng == 0 || (gps_t && gps_p)), "bad offsets / NULL arrays");
    int64_t maxg = 2;
    for (int64_t b = 0; b < B; ++b) { const int64_t g = gps_offsets[b + 1] - gps_offsets[b]; if (g > maxg) maxg = g; }
    Staging st(ctx);
    auto dst = st.in(slam_t, (size_t)ns); auto dgt = st.in(gps_t, (size_t)ng); auto dgp = st.in(gps_p, (size_t)ng * 3);
    auto dso = st.in(slam_offsets, (size_t)B + 1); auto dgo = st.in(gps_offsets, (size_t)B + 1);
    auto dal = st.out(aligned, (size_t)ns * 3); auto dva = st.out(valid, (size_t)ns); auto dstat = st.out(status, (size_t)B);
    ST_RUN(gsf_time_align_batch_dev(ctx, dst, dso, dgt, dgp, dgo, B, (int32_t)maxg, max_gps_gap_threshold, dal, dva, dstat));
}

int gsf_clock_offset_search_dev(gsf_ctx* ctx, const double* ts, const double* pos, const int64_t* slam_offsets, const double* gps_t, const double* gps_utm,
                                const uint8_t* gps_keep, const int64_t* gps_offsets, int64_t B, int32_t max_fixes, const double* tau0, double dtau,
                                int32_t K, double max_gps_gap_threshold, int32_t min_rows, double flat_threshold, double* J, int32_t* n_rows,
                                int32_t* best_k, double* tau_best, double* tau_refined, double* R, double* t, double* s, int32_t* clk_status)
{
    GSF_REQUIRE(ctx && slam_offsets && gps_offsets && J && best_k && tau_best && tau_refined && clk_status, "NULL argument");
    GSF_REQUIRE((R && t && s) || (!R && !t && !s), "R, t, s: all three or none");
    GSF_REQUIRE(B >= 0 && K >= 1 && K <= 4096 && B <= 0x7fffffff / (int64_t)K, "bad B / K");
    GSF_REQUIRE(max_fixes >= 0 && max_fixes <= (1 << 24), "max_fixes out of range");
    if (B == 0) return GSF_OK;
    GSF_HIP(hipSetDevice(ctx->device));
    const int max_g = max_fixes < 2 ? 2 : max_fixes;
    ClkArgs a{ ts, pos, slam_offsets, gps_t, gps_utm, gps_keep, gps_offsets, tau0, dtau, K, max_gps_gap_threshold, max_g, min_rows, flat_threshold,
               ctx->fit_rows, J, n_rows, best_k, tau_best, tau_refined, R, t, s, clk_status, B };
    size_t lds = (size_t)max_g * 8 * sizeof(double);                                 // T + Y(3) + M(3) + W, sized by the longest log
    double* gscratch = nullptr;
    int64_t slab_rows = 0;
    if (max_g > 2560) {                                                              // does not fit 160 KB of LDS: one slab row per RESIDENT workgroup
        int cus = 0;
        GSF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        slab_rows = (int64_t)(cus > 0 ? cus : 1) * 8;
        if (slab_rows > B * K) slab_rows = B * K;
        int rc = ensure_workspace(ctx, GSF_WS_KERNEL, lds * (size_t)slab_rows);
        if (rc) return rc;
        gscratch = workspace<double>(ctx, GSF_WS_KERNEL); lds = 0;
    } else if (lds > 64 * 1024) {
        GSF_HIP(hipFuncSetAttribute((const void*)clock_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    const int64_t sweep = B * K;
    hipLaunchKernelGGL(clock_search_kernel, dim3((unsigned)(gscratch ? slab_rows : sweep)), dim3(ALIGN_THREADS), lds, ctx->stream, a, 0, gscratch);
    GSF_HIP(hipGetLastError());
    hipLaunchKernelGGL(clock_search_kernel, dim3((unsigned)(gscratch && slab_rows < B ? slab_rows : B)), dim3(ALIGN_THREADS), lds, ctx->stream, a, 1, gscratch);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

int gsf_clock_offset_search(gsf_ctx* ctx, const double* ts, const double* pos, const int64_t* slam_offsets, const double* gps_t, const double* gps_utm,
                            const uint8_t* gps_keep, const int64_t* gps_offsets, int64_t B, const double* tau0, double dtau, int32_t K,
                            double max_gps_gap_threshold, int32_t min_rows, double flat_threshold, double* J, int32_t* n_rows, int32_t* best_k,
                            double* tau_best, double* tau_refined, double* R, double* t, double* s, int32_t* clk_status)
{
    GSF_REQUIRE(ctx && slam_offsets && gps_offsets && B >= 0 && K >= 1 && K <= 4096, "bad arguments");
    GSF_REQUIRE(J && best_k && tau_best && tau_refined && clk_status, "NULL output");
    GSF_REQUIRE((R && t && s) || (!R && !t && !s), "R, t, s: all three or none");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(slam_offsets[0] == 0 && gps_offsets[0] == 0, "offsets must start at 0");
    int64_t maxg = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = slam_offsets[b + 1] - slam_offsets[b], g = gps_offsets[b + 1] - gps_offsets[b];
        GSF_REQUIRE(n >= 0 && g >= 0 && g <= (1 << 24), "offsets must not decrease; at most 2^24 fixes per log");
        if (g > maxg) maxg = g;
    }
    const size_t P = (size_t)slam_offsets[B], G = (size_t)gps_offsets[B], BK = (size_t)B * (size_t)K;
    GSF_REQUIRE((P == 0 || (ts && pos)) && (G == 0 || (gps_t && gps_utm)), "NULL arrays");
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dpos = st.in(pos, P * 3); auto dso = st.in(slam_offsets, (size_t)B + 1);
    auto dgt = st.in(gps_t, G); auto dgp = st.in(gps_utm, G * 3); auto dgk = st.in_opt(gps_keep, G);
    auto dgo = st.in(gps_offsets, (size_t)B + 1); auto dt0 = st.in_opt(tau0, (size_t)B);
    auto dJ = st.out(J, BK); auto dnr = st.out_opt(n_rows, BK); auto dbk = st.out(best_k, (size_t)B);
    auto dtb = st.out(tau_best, (size_t)B); auto dtr = st.out(tau_refined, (size_t)B);
    auto dR = st.out_opt(R, (size_t)B * 9); auto dt = st.out_opt(t, (size_t)B * 3); auto ds = st.out_opt(s, (size_t)B);
    auto dcs = st.out(clk_status, (size_t)B);
    ST_RUN(gsf_clock_offset_search_dev(ctx, dts, dpos, dso, dgt, dgp, dgk, dgo, B, (int32_t)maxg, dt0, dtau, K, max_gps_gap_threshold, min_rows, flat_threshold,
                                       dJ, dnr, dbk, dtb, dtr, dR, dt, ds, dcs));
}

}  // extern "C"
