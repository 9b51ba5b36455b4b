// gsf_traj_eval.hip -- trajectory evaluation against 6-DoF truth (gsf_traj_eval_dev): association, alignment, absolute pose error with
// evo's statistics, relative pose error over frame / metre / second deltas and KITTI's segment errors, for B ragged tracks at once.
// Definitions: include/gsf.h ("trajectory evaluation"); the maths: gsf_traj_eval_core.hpp; shapes and measurements: DESIGN.md 7r.
//
// Three launches, stream-ordered, no atomics:
//  1. te_associate_kernel, one 256-thread block per track.  The block decides the track's state first (run_status, empty, one pass over the
//     estimate and the truth stamps: sorted? NaN?), then one thread per estimate pose searches the truth stamps and writes pose_flags and
//     match_index.  It also writes the "no value" rows of every per-pose output, so the later launches only write what exists.
//  2. te_align_kernel, one 64-lane workgroup per track.  Counts the matched poses; with an alignment: centroids as sums about the first matched
//     pair, centred moments, umeyama_finalize (the SVD route).  Then 64 poses at a time, in order: the aligned pose and the two absolute
//     errors, and the matched poses compacted into the workspace table (16 doubles a row: truth pose, aligned estimate, stamp, truth path
//     length d[m] by a wave scan with a carry across the 64-row chunks).  Then the statistics from the lane's own per-pose values: two passes
//     for the moments, 64 counting rounds on the bit patterns for the median.
//  3. te_rpe_kernel, one wave per (track, scenario); lanes take first frames, 64 at a time.  Not launched for K = 0.
// Reductions: every lane adds its rows in ascending order, then an xor butterfly -- one fixed order, the same bits in every lane.
#include "gsf_internal.hpp"
#include "gsf_traj_eval_core.hpp"

namespace {

using namespace gsf;

typedef unsigned long long u64;

struct TeArgs {
    const double* ts; const double* pos; const double* quat; const int64_t* offsets;
    const double* rts; const double* rpos; const double* rquat; const int64_t* roffsets;
    const int32_t* run_status;
    int64_t B; int32_t assoc, align; double max_diff;
    int32_t K; const int32_t* rpe_kind; const double* rpe_value; const int64_t* rpe_stride; int32_t trace_k;
    double* R; double* t; double* s; int32_t* track_state; uint8_t* pose_flags; int32_t* match_index; double* ape_t; double* ape_r;
    double* ape_stats; int64_t* rpe_n; double* rpe_sums; int32_t* rpe_last; double* rpe_t; double* rpe_r;
    double* rows; int64_t* n_matched; int32_t* row_pose;       // workspace: the matched table, M per track, the estimate row of table row m
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ u64 wave_min_u64(u64 v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const u64 o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}

__device__ __forceinline__ Vec3 load3(const double* p, int64_t i) { return Vec3{ p[i * 3], p[i * 3 + 1], p[i * 3 + 2] }; }
__device__ __forceinline__ Quat load4(const double* p, int64_t i) { return Quat{ p[i * 4], p[i * 4 + 1], p[i * 4 + 2], p[i * 4 + 3] }; }

// ---- 1. track state and association
__global__ __launch_bounds__(256) void te_associate_kernel(const TeArgs a)
{
    const int64_t b = blockIdx.x;
    const int64_t base = a.offsets[b], n = a.offsets[b + 1] - base;
    int32_t st = 0;
    int64_t gb = 0, G = 0;
    if (a.run_status && a.run_status[b] != 0) st = TE_TRACK_SKIPPED;         // (block-uniform, as every branch on st below)
    if (!st) {
        gb = a.roffsets[b]; G = a.roffsets[b + 1] - gb;
        if (n <= 0 || G <= 0) st = TE_TRACK_EMPTY;
    }
    const double* __restrict__ t = a.ts + base;
    const double* __restrict__ rt = a.rts + gb;
    if (!st) {
        int bad = 0;
        for (int64_t i = threadIdx.x; i < n; i += 256) { const double cur = t[i]; bad |= (i == 0) ? (cur != cur) : query_stamp_breaks(t[i - 1], cur); }
        for (int64_t i = threadIdx.x; i < G; i += 256) { const double cur = rt[i]; bad |= (i == 0) ? (cur != cur) : query_stamp_breaks(rt[i - 1], cur); }
        if (__syncthreads_or(bad)) st = TE_TRACK_UNSORTED;
    }
    if (threadIdx.x == 0) a.track_state[b] = st;
    const double nan = __builtin_nan("");
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        int32_t flags = TE_TRACK;
        int64_t idx = -1;
        if (!st) {
            const TeMatch m = te_associate(a.assoc, a.max_diff, t[i], load3(a.pos, base + i), load4(a.quat, base + i), rt, a.rpos + gb * 3,
                                           a.rquat + gb * 4, G);
            flags = m.flags; idx = m.index;
        }
        const int64_t r = base + i;
        a.pose_flags[r] = (uint8_t)flags;
        a.match_index[r] = (int32_t)idx;
        a.ape_t[r] = nan; a.ape_r[r] = nan;
        if (a.rpe_last) a.rpe_last[r] = -1;
        if (a.rpe_t) a.rpe_t[r] = nan;
        if (a.rpe_r) a.rpe_r[r] = nan;
    }
}

// ---- 2. alignment, absolute errors, the matched table, statistics
// {n, mean, median, rmse, std, min, max, sse} of the non-NaN values of x[0 .. n): lane l reads rows l, l + 64, ... -- the rows it wrote
__device__ __forceinline__ void te_stats(const double* x, const int64_t n, const int64_t M, const int lane, double* out)
{
    const double nan = __builtin_nan("");
    if (M <= 0) {
        if (lane == 0) { out[0] = 0.0; for (int c = 1; c < 8; ++c) out[c] = nan; }
        return;
    }
    double sum = 0.0, sse = 0.0, lo = INFINITY, hi = 0.0;
    for (int64_t i = lane; i < n; i += 64) {
        const double v = x[i];
        if (v == v) { sum += v; sse = fma(v, v, sse); lo = fmin(lo, v); hi = fmax(hi, v); }
    }
    sum = wave_sum(sum); sse = wave_sum(sse); lo = wave_min(lo); hi = wave_max(hi);
    const double mean = sum / (double)M;
    double dev2 = 0.0;
    for (int64_t i = lane; i < n; i += 64) {
        const double v = x[i];
        if (v == v) { const double e = v - mean; dev2 = fma(e, e, dev2); }
    }
    dev2 = wave_sum(dev2);
    // the lower middle value by counting, the upper one from a last pass: the lower again if it occurs often enough, else the next larger
    const int64_t k_lo = (M - 1) >> 1, k_hi = M >> 1;
    const u64 b_lo = te_select_kth(k_lo, [&](const uint64_t mask, const uint64_t prefix, const uint64_t bit) {
        int64_t c = 0;
        for (int64_t i0 = 0; i0 < n; i0 += 64) {
            const int64_t i = i0 + lane;
            bool hit = false;
            if (i < n) { const double v = x[i]; const u64 w = (u64)__double_as_longlong(v); hit = v == v && (w & mask) == prefix && !(w & bit); }
            c += __popcll(__ballot(hit));
        }
        return c;
    });
    u64 b_hi = b_lo;
    if (k_hi != k_lo) {
        int64_t le = 0; u64 next = ~0ull;
        for (int64_t i0 = 0; i0 < n; i0 += 64) {
            const int64_t i = i0 + lane;
            bool hit = false;
            if (i < n) {
                const double v = x[i]; const u64 w = (u64)__double_as_longlong(v);
                hit = v == v && w <= b_lo;
                if (v == v && w > b_lo && w < next) next = w;
            }
            le += __popcll(__ballot(hit));
        }
        next = wave_min_u64(next);
        if (le <= k_hi) b_hi = next;
    }
    const double m_lo = __longlong_as_double((long long)b_lo), m_hi = __longlong_as_double((long long)b_hi);
    if (lane == 0) {
        out[0] = (double)M; out[1] = mean; out[2] = (k_hi != k_lo) ? (m_lo + m_hi) * 0.5 : m_lo; out[3] = sqrt(sse / (double)M);
        out[4] = sqrt(dev2 / (double)M); out[5] = lo; out[6] = hi; out[7] = sse;
    }
}

__global__ __launch_bounds__(64) void te_align_kernel(const TeArgs a)
{
    __shared__ double lds_g[64 * 3];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double nan = __builtin_nan("");
    int32_t st = a.track_state[b];
    const int64_t base = a.offsets[b], n = st ? 0 : a.offsets[b + 1] - base;
    const int64_t gb = st ? 0 : a.roffsets[b];
    const double* __restrict__ t = a.ts + base;
    const double* __restrict__ pos = a.pos + base * 3;
    const double* __restrict__ quat = a.quat + base * 4;
    const double* __restrict__ rt = a.rts + gb;
    const double* __restrict__ rpos = a.rpos + gb * 3;
    const double* __restrict__ rquat = a.rquat + gb * 4;
    const uint8_t* __restrict__ pf = a.pose_flags + base;
    const int32_t* __restrict__ mi = a.match_index + base;

    // ---- matched poses: how many, and the first
    int64_t M = 0, first = 0;
    for (int64_t i0 = 0; i0 < n; i0 += 64) {
        const int64_t i = i0 + lane;
        const u64 mask = __ballot(i < n && pf[i] == TE_MATCHED);
        if (mask && M == 0) first = i0 + (__ffsll((long long)mask) - 1);
        M += __popcll(mask);
    }
    bool ok = st == 0;
    TeAlign A = te_align_identity();
    if (ok && a.align != TE_ALIGN_NONE) {
        if (M < 3) { st |= TE_TRACK_FEW; ok = false; }
        else {
            // centroids about the first matched pair (UTM-sized coordinates: the sums then carry the track's extent, not its offset)
            Vec3 g0; Quat q0, q1;
            te_truth_pose(a.assoc, a.max_diff, t[first], load4(quat, first), rt, rpos, rquat, mi[first], g0, q0, q1);
            const Vec3 p0 = load3(pos, first);
            double sa[3] = { 0.0, 0.0, 0.0 }, sb[3] = { 0.0, 0.0, 0.0 };
            for (int64_t i = lane; i < n; i += 64) {
                if (pf[i] != TE_MATCHED) continue;
                Vec3 g; Quat qg, qe;
                te_truth_pose(a.assoc, a.max_diff, t[i], load4(quat, i), rt, rpos, rquat, mi[i], g, qg, qe);
                const Vec3 p = load3(pos, i);
                sa[0] += p.x - p0.x; sa[1] += p.y - p0.y; sa[2] += p.z - p0.z;
                sb[0] += g.x - g0.x; sb[1] += g.y - g0.y; sb[2] += g.z - g0.z;
            }
            const double cnt = (double)M;
            const double sc[3] = { p0.x + wave_sum(sa[0]) / cnt, p0.y + wave_sum(sa[1]) / cnt, p0.z + wave_sum(sa[2]) / cnt };
            const double dc[3] = { g0.x + wave_sum(sb[0]) / cnt, g0.y + wave_sum(sb[1]) / cnt, g0.z + wave_sum(sb[2]) / cnt };
            double H[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, ssq = 0.0;
            for (int64_t i = lane; i < n; i += 64) {
                if (pf[i] != TE_MATCHED) continue;
                Vec3 g; Quat qg, qe;
                te_truth_pose(a.assoc, a.max_diff, t[i], load4(quat, i), rt, rpos, rquat, mi[i], g, qg, qe);
                const Vec3 p = load3(pos, i);
                const double x[3] = { p.x - sc[0], p.y - sc[1], p.z - sc[2] }, y[3] = { g.x - dc[0], g.y - dc[1], g.z - dc[2] };
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) H[r * 3 + c] = fma(x[r], y[c], H[r * 3 + c]);
                ssq = fma(x[2], x[2], fma(x[1], x[1], fma(x[0], x[0], ssq)));
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) H[k] = wave_sum(H[k]);
            ssq = wave_sum(ssq);
            const int32_t fit = umeyama_finalize<false, false>(H, ssq, sc, dc, cnt, A.R, A.t, A.s);
            if (fit & SIM3_NONE) { st |= TE_TRACK_DEGENERATE; ok = false; }
            else {
                if (a.align == TE_ALIGN_SE3) {
                    A.s = 1.0;
#pragma unroll
                    for (int r = 0; r < 3; ++r) A.t[r] = dc[r] - (A.R[r * 3] * sc[0] + A.R[r * 3 + 1] * sc[1] + A.R[r * 3 + 2] * sc[2]);
                }
                A.qR = quat_from_matrix(A.R);
            }
        }
    }
    if (lane == 0) {
        a.track_state[b] = st;
        a.n_matched[b] = ok ? M : 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) a.R[b * 9 + k] = ok ? A.R[k] : nan;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.t[b * 3 + k] = ok ? A.t[k] : nan;
        a.s[b] = ok ? A.s : nan;
    }
    if (!ok) {
        te_stats(a.ape_t, 0, 0, lane, a.ape_stats + (b * 2) * 8);
        te_stats(a.ape_r, 0, 0, lane, a.ape_stats + (b * 2 + 1) * 8);
        return;
    }

    // ---- 64 poses at a time: errors, the matched table, d[m]
    double* const rows = a.rows + base * TE_ROW;
    int32_t* const row_pose = a.row_pose + base;
    int64_t mb = 0;
    bool have_prev = false;
    Vec3 gprev{ 0.0, 0.0, 0.0 };
    double carry = 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool matched = i < n && pf[i] == TE_MATCHED;
        const u64 mask = __ballot(matched);
        const int c = __popcll(mask);
        if (c == 0) continue;                                                // (wave-uniform)
        if (matched) {
            const int rank = __popcll(mask & ((1ull << lane) - 1ull));
            const double tau = t[i];
            Vec3 g, pa; Quat qg, qe, qa; double et, er;
            te_truth_pose(a.assoc, a.max_diff, tau, load4(quat, i), rt, rpos, rquat, mi[i], g, qg, qe);
            te_ape(A, load3(pos, i), qe, g, qg, pa, qa, et, er);
            a.ape_t[base + i] = et; a.ape_r[base + i] = er;
            double* const row = rows + (mb + rank) * TE_ROW;
            row[TE_ROW_G] = g.x; row[TE_ROW_G + 1] = g.y; row[TE_ROW_G + 2] = g.z;
            row[TE_ROW_QG] = qg.x; row[TE_ROW_QG + 1] = qg.y; row[TE_ROW_QG + 2] = qg.z; row[TE_ROW_QG + 3] = qg.w;
            row[TE_ROW_P] = pa.x; row[TE_ROW_P + 1] = pa.y; row[TE_ROW_P + 2] = pa.z;
            row[TE_ROW_Q] = qa.x; row[TE_ROW_Q + 1] = qa.y; row[TE_ROW_Q + 2] = qa.z; row[TE_ROW_Q + 3] = qa.w;
            row[TE_ROW_TS] = tau;
            row_pose[mb + rank] = (int32_t)i;
            lds_g[rank * 3] = g.x; lds_g[rank * 3 + 1] = g.y; lds_g[rank * 3 + 2] = g.z;
        }
        __syncthreads();
        double step = 0.0;
        if (lane < c && (lane > 0 || have_prev)) {
            const Vec3 g1{ lds_g[lane * 3], lds_g[lane * 3 + 1], lds_g[lane * 3 + 2] };
            const Vec3 gp = lane > 0 ? Vec3{ lds_g[lane * 3 - 3], lds_g[lane * 3 - 2], lds_g[lane * 3 - 1] } : gprev;
            step = te_norm3(g1.x - gp.x, g1.y - gp.y, g1.z - gp.z);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const double o = __shfl_up(step, off); if (lane >= off) step += o; }
        const double d = carry + step;
        if (lane < c) rows[(mb + lane) * TE_ROW + TE_ROW_D] = d;
        carry = __shfl(d, c - 1);
        gprev = Vec3{ lds_g[(c - 1) * 3], lds_g[(c - 1) * 3 + 1], lds_g[(c - 1) * 3 + 2] };
        have_prev = true;
        mb += c;
        __syncthreads();                                                     // the slice is read before the next chunk fills it
    }
    te_stats(a.ape_t + base, n, M, lane, a.ape_stats + (b * 2) * 8);
    te_stats(a.ape_r + base, n, M, lane, a.ape_stats + (b * 2 + 1) * 8);
}

// ---- 3. relative errors: one wave per (track, scenario)
__global__ __launch_bounds__(64) void te_rpe_kernel(const TeArgs a)
{
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / a.K;
    const int k = (int)(blockIdx.x % a.K);
    const int64_t M = a.n_matched[b], base = a.offsets[b];
    const double* __restrict__ rows = a.rows + base * TE_ROW;
    const int32_t* __restrict__ row_pose = a.row_pose + base;
    const int32_t kind = a.rpe_kind[k];
    const double value = a.rpe_value[k];
    int64_t stride = a.rpe_stride[k];
    const bool trace = a.rpe_last && k == a.trace_k;
    const bool metres = kind == TE_METRES;
    const double nan = __builtin_nan("");
    double st = 0.0, st2 = 0.0, mt = 0.0, sr = 0.0, sr2 = 0.0, mr = 0.0, stl = 0.0, srl = 0.0;
    int64_t cnt = 0;
    if (stride >= 1 && M > 1) {
        if (stride > M) stride = M;                                          // (the second first frame is past the end either way)
        const int64_t F = (M + stride - 1) / stride;
        for (int64_t q = lane; q < F; q += 64) {
            const int64_t f = q * stride;
            const int64_t l = te_last_frame(kind, value, rows, M, f);
            if (l < 0) continue;
            double et, er;
            te_pair_error(rows + f * TE_ROW, rows + l * TE_ROW, et, er);
            st += et; st2 = fma(et, et, st2); mt = fmax(mt, et);
            sr += er; sr2 = fma(er, er, sr2); mr = fmax(mr, er);
            if (metres) { stl += et / value; srl += er / value; }
            ++cnt;
            if (trace) {
                const int64_t r = base + row_pose[f];
                a.rpe_last[r] = row_pose[l];
                if (a.rpe_t) a.rpe_t[r] = et;
                if (a.rpe_r) a.rpe_r[r] = er;
            }
        }
    }
    st = wave_sum(st); st2 = wave_sum(st2); mt = wave_max(mt); sr = wave_sum(sr); sr2 = wave_sum(sr2); mr = wave_max(mr);
    stl = wave_sum(stl); srl = wave_sum(srl);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) {
        a.rpe_n[b * a.K + k] = cnt;
        double* const o = a.rpe_sums + (b * a.K + k) * 8;
        o[0] = st; o[1] = st2; o[2] = mt; o[3] = sr; o[4] = sr2; o[5] = mr; o[6] = metres ? stl : nan; o[7] = metres ? srl : nan;
    }
}

}  // namespace

extern "C" int gsf_traj_eval_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets, int64_t P,
                                 const double* ref_ts, const double* ref_pos, const double* ref_quat, const int64_t* ref_offsets,
                                 const int32_t* run_status, int64_t B, int32_t assoc_mode, double max_diff, int32_t align_mode, int32_t K,
                                 const int32_t* rpe_kind, const double* rpe_value, const int64_t* rpe_stride, int32_t trace_k, double* R,
                                 double* t, double* s, int32_t* track_state, uint8_t* pose_flags, int32_t* match_index, double* ape_t,
                                 double* ape_r, double* ape_stats, int64_t* rpe_n, double* rpe_sums, int32_t* rpe_last, double* rpe_t,
                                 double* rpe_r)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_REQUIRE(B >= 0 && P >= 0 && K >= 0, "negative B / P / K");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(assoc_mode == GSF_TE_NEAREST || assoc_mode == GSF_TE_INTERP, "assoc_mode is neither GSF_TE_NEAREST nor GSF_TE_INTERP");
    GSF_REQUIRE(align_mode == GSF_TE_ALIGN_NONE || align_mode == GSF_TE_ALIGN_SE3 || align_mode == GSF_TE_ALIGN_SIM3, "unknown align_mode");
    GSF_REQUIRE(max_diff == max_diff, "max_diff is NaN");
    GSF_REQUIRE(ts && pos && quat && offsets && ref_ts && ref_pos && ref_quat && ref_offsets, "NULL input array");
    GSF_REQUIRE(R && t && s && track_state && pose_flags && match_index && ape_t && ape_r && ape_stats, "NULL output array");
    GSF_REQUIRE(K == 0 || (rpe_kind && rpe_value && rpe_stride && rpe_n && rpe_sums), "K > 0 needs rpe_kind, rpe_value, rpe_stride, rpe_n and rpe_sums");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff && B * (int64_t)(K > 0 ? K : 1) <= (int64_t)0x7fffffff, "B x K too large for one launch");
    GSF_HIP(hipSetDevice(ctx->device));
    // workspace: the matched table (16 doubles a pose), the matched count of every track, the estimate row of every table row
    const size_t rows_bytes = (size_t)P * TE_ROW * sizeof(double), cnt_bytes = (size_t)B * sizeof(int64_t);
    int rc = ensure_workspace(ctx, GSF_WS_KERNEL, rows_bytes + cnt_bytes + (size_t)P * sizeof(int32_t) + 8);
    if (rc) return rc;
    char* const w = workspace<char>(ctx, GSF_WS_KERNEL);
    const TeArgs a{ ts, pos, quat, offsets, ref_ts, ref_pos, ref_quat, ref_offsets, run_status, B, assoc_mode, align_mode, max_diff,
                    K, rpe_kind, rpe_value, rpe_stride, trace_k, R, t, s, track_state, pose_flags, match_index, ape_t, ape_r,
                    ape_stats, rpe_n, rpe_sums, rpe_last, rpe_t, rpe_r,
                    (double*)w, (int64_t*)(w + rows_bytes), (int32_t*)(w + rows_bytes + cnt_bytes) };
    hipLaunchKernelGGL(te_associate_kernel, dim3((unsigned)B), dim3(256), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    hipLaunchKernelGGL(te_align_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    if (K > 0) {
        hipLaunchKernelGGL(te_rpe_kernel, dim3((unsigned)(B * K)), dim3(64), 0, ctx->stream, a);
        GSF_HIP(hipGetLastError());
    }
    return GSF_OK;
}
