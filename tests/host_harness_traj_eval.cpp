// TEST-ONLY host harness: compiles the GSF_HD helpers of gsf_traj_eval_core.hpp (what gsf_traj_eval.hip calls per lane) with g++, so that
// tests/test_traj_eval_host.py can compare them with the 50-digit restatement in the CPU-only tier.  One track per call, walked the way the
// three kernels walk it, sequentially.  Never shipped, never loaded by the package.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../gps_optimize_slam_amd/csrc/gsf_traj_eval_core.hpp"

using namespace gsf;

static void stats_of(const std::vector<double>& x, double* out)
{
    const double nan = __builtin_nan("");
    const int64_t M = (int64_t)x.size();
    if (M == 0) { out[0] = 0.0; for (int c = 1; c < 8; ++c) out[c] = nan; return; }
    double sum = 0.0, sse = 0.0, lo = INFINITY, hi = 0.0;
    for (double v : x) { sum += v; sse = fma(v, v, sse); lo = fmin(lo, v); hi = fmax(hi, v); }
    const double mean = sum / (double)M;
    double dev2 = 0.0;
    for (double v : x) { const double e = v - mean; dev2 = fma(e, e, dev2); }
    auto bits = [](double v) { uint64_t w; memcpy(&w, &v, 8); return w; };
    auto kth = [&](int64_t k) {
        const uint64_t w = te_select_kth(k, [&](uint64_t mask, uint64_t prefix, uint64_t bit) {
            int64_t c = 0;
            for (double v : x) c += ((bits(v) & mask) == prefix && !(bits(v) & bit)) ? 1 : 0;
            return c;
        });
        double v; memcpy(&v, &w, 8); return v;
    };
    const double m_lo = kth((M - 1) >> 1), m_hi = kth(M >> 1);
    out[0] = (double)M; out[1] = mean; out[2] = (M & 1) ? m_lo : (m_lo + m_hi) * 0.5; out[3] = sqrt(sse / (double)M);
    out[4] = sqrt(dev2 / (double)M); out[5] = lo; out[6] = hi; out[7] = sse;
}

extern "C" {

int64_t ht_select_kth(const double* x, int64_t n, int64_t k, double* out)
{
    const uint64_t w = te_select_kth(k, [&](uint64_t mask, uint64_t prefix, uint64_t bit) {
        int64_t c = 0;
        for (int64_t i = 0; i < n; ++i) { uint64_t v; memcpy(&v, x + i, 8); c += ((v & mask) == prefix && !(v & bit)) ? 1 : 0; }
        return c;
    });
    memcpy(out, &w, 8);
    return 0;
}

double ht_angle(const double* q) { return te_angle(Quat{ q[0], q[1], q[2], q[3] }); }

// One track.  state_in: the TE_TRACK_* bits decided before the search (the Python side passes the yardstick's; te_unsorted below gives the
// header's own answer).  use_fit != 0: R / t / s are inputs (the alignment is not fitted).  Returns the track state.
int ht_unsorted(const double* t, int64_t n) { return query_track_unsorted(t, n) ? 1 : 0; }

int32_t ht_eval_track(const double* ts, const double* pos, const double* quat, int64_t n, const double* rts, const double* rpos,
                      const double* rquat, int64_t G, int32_t state_in, int32_t assoc, double max_diff, int32_t align, int32_t use_fit, int32_t K,
                      const int32_t* rpe_kind, const double* rpe_value, const int64_t* rpe_stride, int32_t trace_k, double* R, double* t, double* s,
                      uint8_t* pose_flags, int32_t* match_index, double* ape_t, double* ape_r, double* ape_stats, int64_t* rpe_n, double* rpe_sums,
                      int32_t* rpe_last, double* rpe_t, double* rpe_r)
{
    const double nan = __builtin_nan("");
    int32_t st = state_in;
    for (int64_t i = 0; i < n; ++i) {
        pose_flags[i] = (uint8_t)TE_TRACK; match_index[i] = -1; ape_t[i] = ape_r[i] = nan;
        rpe_last[i] = -1; rpe_t[i] = rpe_r[i] = nan;
    }
    std::vector<int64_t> matched;
    if (!st) {
        for (int64_t i = 0; i < n; ++i) {
            const TeMatch m = te_associate(assoc, max_diff, ts[i], Vec3{ pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] },
                                           Quat{ quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3] }, rts, rpos, rquat, G);
            pose_flags[i] = (uint8_t)m.flags; match_index[i] = (int32_t)m.index;
            if (m.flags == TE_MATCHED) matched.push_back(i);
        }
    }
    const int64_t M = (int64_t)matched.size();
    auto truth = [&](int64_t i, Vec3& g, Quat& qg, Quat& qe) {
        te_truth_pose(assoc, max_diff, ts[i], Quat{ quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3] }, rts, rpos, rquat,
                      (int64_t)match_index[i], g, qg, qe);
    };
    bool ok = st == 0;
    TeAlign A = te_align_identity();
    if (ok && align != TE_ALIGN_NONE) {
        if (M < 3) { st |= TE_TRACK_FEW; ok = false; }
        else if (use_fit) {
            for (int k = 0; k < 9; ++k) A.R[k] = R[k];
            for (int k = 0; k < 3; ++k) A.t[k] = t[k];
            A.s = *s; A.qR = quat_from_matrix(A.R);
        } else {
            Vec3 g0; Quat q0, q1;
            truth(matched[0], g0, q0, q1);
            const double* p0 = pos + matched[0] * 3;
            double sa[3] = { 0, 0, 0 }, sb[3] = { 0, 0, 0 };
            for (int64_t i : matched) {
                Vec3 g; Quat qg, qe; truth(i, g, qg, qe);
                for (int c = 0; c < 3; ++c) sa[c] += pos[i * 3 + c] - p0[c];
                sb[0] += g.x - g0.x; sb[1] += g.y - g0.y; sb[2] += g.z - g0.z;
            }
            const double cnt = (double)M;
            const double sc[3] = { p0[0] + sa[0] / cnt, p0[1] + sa[1] / cnt, p0[2] + sa[2] / cnt };
            const double dc[3] = { g0.x + sb[0] / cnt, g0.y + sb[1] / cnt, g0.z + sb[2] / cnt };
            double H[9] = { 0 }, ssq = 0.0;
            for (int64_t i : matched) {
                Vec3 g; Quat qg, qe; truth(i, g, qg, qe);
                const double x[3] = { pos[i * 3] - sc[0], pos[i * 3 + 1] - sc[1], pos[i * 3 + 2] - sc[2] }, y[3] = { g.x - dc[0], g.y - dc[1], g.z - dc[2] };
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[r * 3 + c] = fma(x[r], y[c], H[r * 3 + c]);
                ssq = fma(x[2], x[2], fma(x[1], x[1], fma(x[0], x[0], ssq)));
            }
            const int32_t fit = umeyama_finalize<false, false>(H, ssq, sc, dc, cnt, A.R, A.t, A.s);
            if (fit & SIM3_NONE) { st |= TE_TRACK_DEGENERATE; ok = false; }
            else {
                if (align == TE_ALIGN_SE3) {
                    A.s = 1.0;
                    for (int r = 0; r < 3; ++r) A.t[r] = dc[r] - (A.R[r * 3] * sc[0] + A.R[r * 3 + 1] * sc[1] + A.R[r * 3 + 2] * sc[2]);
                }
                A.qR = quat_from_matrix(A.R);
            }
        }
    }
    for (int k = 0; k < 9; ++k) R[k] = ok ? A.R[k] : nan;
    for (int k = 0; k < 3; ++k) t[k] = ok ? A.t[k] : nan;
    *s = ok ? A.s : nan;
    for (int k = 0; k < K; ++k) {
        rpe_n[k] = 0;
        for (int c = 0; c < 8; ++c) rpe_sums[k * 8 + c] = (c >= 6 && rpe_kind[k] != TE_METRES) ? nan : 0.0;
    }
    if (!ok) { stats_of({}, ape_stats); stats_of({}, ape_stats + 8); return st; }

    std::vector<double> rows((size_t)(M > 0 ? M : 1) * TE_ROW), xt, xr;
    Vec3 gprev{ 0, 0, 0 };
    double d = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        const int64_t i = matched[m];
        Vec3 g, pa; Quat qg, qe, qa; double et, er;
        truth(i, g, qg, qe);
        te_ape(A, Vec3{ pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] }, qe, g, qg, pa, qa, et, er);
        ape_t[i] = et; ape_r[i] = er; xt.push_back(et); xr.push_back(er);
        if (m > 0) d += te_norm3(g.x - gprev.x, g.y - gprev.y, g.z - gprev.z);
        gprev = g;
        double* row = rows.data() + m * TE_ROW;
        row[TE_ROW_G] = g.x; row[TE_ROW_G + 1] = g.y; row[TE_ROW_G + 2] = g.z;
        row[TE_ROW_QG] = qg.x; row[TE_ROW_QG + 1] = qg.y; row[TE_ROW_QG + 2] = qg.z; row[TE_ROW_QG + 3] = qg.w;
        row[TE_ROW_P] = pa.x; row[TE_ROW_P + 1] = pa.y; row[TE_ROW_P + 2] = pa.z;
        row[TE_ROW_Q] = qa.x; row[TE_ROW_Q + 1] = qa.y; row[TE_ROW_Q + 2] = qa.z; row[TE_ROW_Q + 3] = qa.w;
        row[TE_ROW_TS] = ts[i]; row[TE_ROW_D] = d;
    }
    stats_of(xt, ape_stats); stats_of(xr, ape_stats + 8);
    const double* tab = rows.data();
    for (int k = 0; k < K; ++k) {
        const int64_t stride = rpe_stride[k];
        if (stride < 1) continue;
        double* o = rpe_sums + k * 8;
        for (int64_t f = 0; f < M; f += stride) {
            const int64_t l = te_last_frame(rpe_kind[k], rpe_value[k], tab, M, f);
            if (l < 0) continue;
            double et, er;
            te_pair_error(tab + f * TE_ROW, tab + l * TE_ROW, et, er);
            o[0] += et; o[1] = fma(et, et, o[1]); o[2] = fmax(o[2], et); o[3] += er; o[4] = fma(er, er, o[4]); o[5] = fmax(o[5], er);
            if (rpe_kind[k] == TE_METRES) { o[6] += et / rpe_value[k]; o[7] += er / rpe_value[k]; }
            ++rpe_n[k];
            if (k == trace_k) { rpe_last[matched[f]] = (int32_t)matched[l]; rpe_t[matched[f]] = et; rpe_r[matched[f]] = er; }
        }
    }
    return st;
}
}
