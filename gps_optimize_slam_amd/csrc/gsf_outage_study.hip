// gsf_outage_study.hip -- drift and RTS gain of the fused track for K withheld GNSS windows per track (gsf_outage_study_dev).
//
// A withheld window changes nothing before the outage it creates, GNSS never touches the state quaternion and every covariance
// is diagonal, so the study is one base pass per track plus O(outage length) work per scenario (gsf_outage_core.hpp):
//  * base pass, one wave per track, 64 poses per chunk: the shared chunk body of gsf_track_chunk.hpp under cfg's own noise -- dt, the availability
//    ballot, the outage structure and the blend weight of a sharp-turn recovery, d[i], variance_chunk() and the three affine scans -- and
//    five prefix sums.  It writes one workspace row per pose (p_f - init_pos, Pf, D = sum d, T = sum dt, sum |d|: 88 B), one flag byte per
//    pose (avail; "the pair (i - 1, i) exceeds the yaw-rate threshold", for EVERY adjacent pair) and one word per track (stamps unsorted).
//    Positions stay relative to init_pos so that differences of prefix sums lose nothing at UTM magnitudes.
//  * scenario pass, one wave per (track, scenario): two 64-way searches over the stamps give W, ballots over the flag bytes walk a back and
//    b forward, the anchor's and the recovery's rows are read wave-uniformly, the 64 lanes stride over [a, b), the sums are reduced in a
//    fixed lane order and lane 0 writes the row.  No LDS, no atomics, no state shared between scenarios: a row is the same bytes for any K,
//    any order of the scenarios and any other tracks in the batch.
// Definitions: include/gsf.h.
#include "gsf_track_chunk.hpp"
#include "gsf_outage_core.hpp"

namespace {

struct BaseArgs {
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid;
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* init_quat;
    double* rows; uint8_t* flags; int32_t* unsorted;
};

__global__ __launch_bounds__(64) void outage_base_kernel(const BaseArgs a, const EkfConfig cfg)
{
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x;
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    if (N <= 0) return;                                                   // (the scenario pass reads no row of an empty or a stopped track)
    if (a.run_status && a.run_status[b] != 0) return;
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;
    double* __restrict__ rowb = a.rows + base * OUTAGE_ROW;
    uint8_t* __restrict__ flb = a.flags + base;
    ChunkIn nxt = load_chunk(tsb, posb, quatb, gpsb, valb, lane, N);

    // ---- carried from chunk to chunk (wave-uniform): the filter's last pose, the prefix sums, the pair / outage state of the sweep
    double cP[3] = { cfg.P0[0], cfg.P0[1], cfg.P0[2] };                   // Pf of the last pose (pose 0: P0)
    double cx[3] = { 0.0, 0.0, 0.0 };                                     // its position relative to init_pos
    double cD[3] = { 0.0, 0.0, 0.0 }, cT = 0.0, cS = 0.0;                 // D, T and sum |d| up to it
    int same1, same2;
    same_axes(cfg.P0, cfg.Qps, cfg.Rm, same1, same2);
    TrackCarry tc = track_carry_init(a.init_pos, a.init_quat, b, nxt, cfg);
    bool c_ok = tc.first_ok;                                             // a local, not a member of the carry: gsf_track_chunk.hpp
    u64 unsorted_m = (tc.c_t != tc.c_t) ? 1ull : 0ull;                    // a NaN first stamp

    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const ChunkIn in = nxt;
        nxt = load_chunk(tsb, posb, quatb, gpsb, valb, c0 + 64 + lane, N);   // the next chunk's rows are requested before this chunk's scans (clamped past the end)
        const ChunkFront f = chunk_front(in, tc, c_ok, c0, N, lane);
        const int64_t i = f.i;
        const int L = f.L;
        const bool active = f.active, stepping = f.stepping, avail = f.fix;
        const double dt = f.dt;
        unsorted_m |= __ballot(stepping && !(f.t >= f.t_pr));             // a stamp below the one before it, or a NaN one
        // ---- outage structure and the sharp-turn decision of the unmodified run: gsf_ekf_cov_ragged_dev's (gsf_cov_core.hpp); the pair
        // test itself runs for EVERY adjacent pair, since a scenario may put any of them inside an outage
        const u64 av_m = avail_mask(f, avail);
        const OutageMasks om = outage_masks(f.act_m, av_m, c0 == 0, tc.oc.prev_avail);
        const u64 pair_m = yaw_pair_mask<true>(f, 0ull, cfg.yaw_thr_rad, lane);
        const bool fpair = (pair_m >> lane) & 1ull;
        const u64 f_mask = pair_m & om.pair;
        const u64 sharp_m = sharp_recoveries(om, f_mask, c0, tc.oc, cfg.yaw_thr_rad < 0.0);
        const double wgt = ((sharp_m >> lane) & 1ull) ? tc.wgt_sharp : 1.0;   // the one-step blend at a sharp-turn recovery, else a hard update

        const Vec3 u = orientation_step<false>(tc, c_ok, f).u;                 // the predicted displacement d[i] (ref :707)
        const double d[3] = { u.x, u.y, u.z };
        const double zr[3] = { f.z.x - tc.p0.x, f.z.y - tc.p0.y, f.z.z - tc.p0.z };   // relative to init_pos

        // ---- the filter under cfg's own noise: variances, gains and the three affine scans of the noise sweep
        AxisVar v0, v1, v2;
        variance_chunk<6>(cfg, same1, same2, dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
        const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, kg[3] = { v0.kg, v1.kg, v2.kg };
        double x[3], Dk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = position_axis(avail, kg[c] * wgt, d[c], zr[c], cx[c]).x;   // p_f[i] - init_pos
            Dk[c] = cD[c] + wave_prefix(d[c]);
        }
        const double dlen = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        const double Tk = cT + wave_prefix(stepping ? dt : 0.0);
        const double Sk = cS + wave_prefix(stepping ? dlen : 0.0);
        if (active) {
            double* row = rowb + i * OUTAGE_ROW;
            row[0] = x[0]; row[1] = x[1]; row[2] = x[2];
            row[3] = Pf[0]; row[4] = Pf[1]; row[5] = Pf[2];
            row[6] = Dk[0]; row[7] = Dk[1]; row[8] = Dk[2];
            row[9] = Tk; row[10] = Sk;
            flb[i] = (uint8_t)((((av_m >> lane) & 1ull) ? OSF_AVAIL : 0) | (fpair ? OSF_PAIR : 0));
        }

        // ---- carry to the next 64 poses (from the last active lane L)
#pragma unroll
        for (int c = 0; c < 3; ++c) { cP[c] = lane_bcast(Pf[c], L); cx[c] = lane_bcast(x[c], L); cD[c] = lane_bcast(Dk[c], L); }
        cT = lane_bcast(Tk, L); cS = lane_bcast(Sk, L);
        track_carry_next(tc, f, c0, av_m, om.start, f_mask);
        c_ok = last_ok(f);
    }
    if (lane == 0) a.unsorted[b] = unsorted_m != 0ull ? 1 : 0;
}

struct StudyArgs {
    const double* ts; const double* gps; const double* truth; const uint8_t* truth_valid;
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* scen;
    const double* rows; const uint8_t* flags; const int32_t* unsorted;
    double* stats; int32_t* seg; int32_t* os_flags; double* err_dr; double* err_fused; double* trace_pos;
    double Q[3], R[3];
    int32_t neg_thr, K, trace_k;
};

// #{ i < n : t[i] < x } for non-decreasing stamps: a 64-way search, every round probes 64 evenly spaced stamps (wave-uniform result)
__device__ __forceinline__ int64_t count_below(const double* __restrict__ t, const int64_t n, const double x, const int lane)
{
    int64_t lo = 0, hi = n;                                               // the answer lies in [lo, hi]
    while (hi > lo) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t idx = lo + (int64_t)(lane + 1) * step - 1;
        const bool below = idx < hi && t[idx < hi ? idx : hi - 1] < x;
        const int cnt = __popcll(__ballot(below));                        // the probes below x are lanes 0..cnt-1
        const int64_t nlo = lo + (int64_t)cnt * step;
        const int64_t nhi = nlo + step - 1;
        hi = nhi < hi ? nhi : hi; lo = nlo;
    }
    return lo;
}

// a row without an outage: every entry = fill, seg = (-1, -1), NaN over the track's rows of the traced scenario
__device__ __forceinline__ void plain_row(const StudyArgs& a, const int64_t row, const int64_t base, const int64_t N, const int lane,
                                          const bool traced, const int32_t flag_word, const double fill)
{
    if (lane == 0) {
        if (a.stats) for (int j = 0; j < OUTAGE_NSTAT; ++j) a.stats[row * OUTAGE_NSTAT + j] = fill;
        if (a.seg) { a.seg[row * 2] = -1; a.seg[row * 2 + 1] = -1; }
        if (a.os_flags) a.os_flags[row] = flag_word;
    }
    if (traced) {
        const double nan = __builtin_nan("");
        for (int64_t k = lane; k < N; k += 64) {
            if (a.err_dr) a.err_dr[base + k] = nan;
            if (a.err_fused) a.err_fused[base + k] = nan;
            if (a.trace_pos) { a.trace_pos[(base + k) * 3] = nan; a.trace_pos[(base + k) * 3 + 1] = nan; a.trace_pos[(base + k) * 3 + 2] = nan; }
        }
    }
}

__global__ __launch_bounds__(64) void outage_scenario_kernel(const StudyArgs a)
{
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)(blockIdx.x / (unsigned)a.K);
    const int k = (int)(blockIdx.x % (unsigned)a.K);
    const int64_t row = b * a.K + k;
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    const bool traced = (a.err_dr || a.err_fused || a.trace_pos) && a.trace_k == k;
    const double nan = __builtin_nan("");
    if (a.run_status && a.run_status[b] != 0) { plain_row(a, row, base, N, lane, traced, OS_SKIPPED, nan); return; }   // inputs not read
    if (N <= 0) { plain_row(a, row, base, 0, lane, false, OS_EMPTY, 0.0); return; }
    if (a.unsorted[b] != 0) { plain_row(a, row, base, N, lane, traced, OS_UNSORTED, nan); return; }
    const double* __restrict__ tsb = a.ts + base;
    const uint8_t* __restrict__ fl = a.flags + base;
    const double* __restrict__ rows = a.rows + base * OUTAGE_ROW;

    // ---- the window W = [#{t < lo}, #{t < hi})
    const double s = a.scen[k * 2], len = a.scen[k * 2 + 1];
    int64_t w0 = 0, w1 = 0;
    if (outage_window_ok(s, len)) {
        const double lo = tsb[0] + s, hi = lo + len;
        w0 = uniform64(count_below(tsb, N, lo, lane)); w1 = uniform64(count_below(tsb, N, hi, lane));
    }
    if (w1 <= w0) { plain_row(a, row, base, N, lane, traced, OS_EMPTY, 0.0); return; }

    // ---- the outage [a, b) around W: the last available pose below w0, the first one from w1 on
    int64_t oa = 0, ob = N;
    for (int64_t hi = w0; hi > 0; hi -= 64) {                             // lane l looks at pose hi - 1 - l
        const int64_t idx = hi - 1 - lane;
        const u64 m = __ballot(idx >= 0 && (fl[idx >= 0 ? idx : 0] & OSF_AVAIL) != 0);
        if (m != 0ull) { oa = hi - (int64_t)__builtin_ctzll(m); break; }
    }
    for (int64_t lo = w1; lo < N; lo += 64) {
        const int64_t idx = lo + lane;
        const u64 m = __ballot(idx < N && (fl[idx < N ? idx : N - 1] & OSF_AVAIL) != 0);
        if (m != 0ull) { ob = lo + (int64_t)__builtin_ctzll(m); break; }
    }
    oa = uniform64(oa); ob = uniform64(ob);
    // ---- |H| and the pairs strictly inside (a, b): the flag bytes of [a, b)
    int nH = 0; u64 pairs = 0ull;
    for (int64_t k0 = oa; k0 < ob; k0 += 64) {
        const int64_t kk = k0 + lane;
        const bool in = kk < ob;
        const uint32_t f = fl[in ? kk : ob - 1];
        nH += __popcll(__ballot(in && kk >= w0 && kk < w1 && kk >= 1 && (f & OSF_AVAIL) != 0));
        pairs |= __ballot(in && kk > oa && (f & OSF_PAIR) != 0);
    }
    const bool rec = ob < N;
    const bool sharp = outage_sharp(oa, ob, pairs != 0ull, a.neg_thr != 0);
    const bool smooth = rec && !sharp;
    const int32_t flag_word = outage_flag_word(N, w0, w1, oa, ob, sharp);

    // ---- anchor and recovery (wave-uniform rows)
    const int64_t c = oa > 0 ? oa - 1 : 0, be = rec ? ob : N - 1;
    const double* __restrict__ rc = rows + c * OUTAGE_ROW;
    const double* __restrict__ rb = rows + be * OUTAGE_ROW;
    const double xc[3] = { rc[0], rc[1], rc[2] }, Pfc[3] = { rc[3], rc[4], rc[5] }, Dc[3] = { rc[6], rc[7], rc[8] };
    const double Tc = rc[9];
    const double p0[3] = { a.init_pos[b * 3], a.init_pos[b * 3 + 1], a.init_pos[b * 3 + 2] };
    const double gap = tsb[be] - tsb[c];
    const double dist = rb[10] - rc[10];
    double gy[3] = { 0.0, 0.0, 0.0 }, Ppb[3] = { 1.0, 1.0, 1.0 }, ynorm = nan, nis = nan;
    if (rec) {
        double y2[3], ni[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double pm = outage_dr_pos(xc[ax], Dc[ax], rb[6 + ax]);
            Ppb[ax] = outage_dr_var(Pfc[ax], a.Q[ax], Tc, rb[9]);
            const double zb = a.gps[(base + ob) * 3 + ax] - p0[ax];
            const OutageAxis o = outage_recovery(zb, pm, Ppb[ax], a.R[ax]);
            gy[ax] = o.gy;
            y2[ax] = o.y * o.y;
            ni[ax] = y2[ax] * fast_rcp(o.S);
        }
        ynorm = sqrt((y2[0] + y2[1]) + y2[2]);
        nis = (ni[0] + ni[1]) + ni[2];
    }

    // ---- the poses of [a, b), 64 at a time: lane sums in ascending pose order, reduced across the lanes in a fixed order below
    double nE = 0.0, s_dr = 0.0, s_fu = 0.0, h_dr = 0.0, h_fu = 0.0, m_dr = 0.0, m_fu = 0.0;
    for (int64_t k0 = oa; k0 < ob; k0 += 64) {
        const int64_t kk = k0 + lane;
        const bool in = kk < ob;
        const int64_t kl = in ? kk : ob - 1;
        const double* __restrict__ rk = rows + kl * OUTAGE_ROW;
        const double Tk = rk[9];
        const double tr[3] = { a.truth[(base + kl) * 3], a.truth[(base + kl) * 3 + 1], a.truth[(base + kl) * 3 + 2] };
        const bool usable = in && a.truth_valid[base + kl] != 0 && !(isnan(tr[0]) || isnan(tr[1]) || isnan(tr[2]));
        double pfu[3], edr[3], efu[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double pdr = outage_dr_pos(xc[ax], Dc[ax], rk[6 + ax]);
            const double Pdr = outage_dr_var(Pfc[ax], a.Q[ax], Tc, Tk);
            const double ps = outage_smooth(pdr, Pdr, Ppb[ax], gy[ax]);
            pfu[ax] = smooth ? ps : pdr;
            const double trel = tr[ax] - p0[ax];
            edr[ax] = pdr - trel; efu[ax] = pfu[ax] - trel;
        }
        const double hd = edr[0] * edr[0] + edr[1] * edr[1], hf = efu[0] * efu[0] + efu[1] * efu[1];
        const double ed2 = hd + edr[2] * edr[2], ef2 = hf + efu[2] * efu[2];
        const double ed = sqrt(ed2), ef = sqrt(ef2);
        if (usable) {
            nE += 1.0; s_dr += ed2; s_fu += ef2; h_dr += hd; h_fu += hf;
            m_dr = fmax(m_dr, ed); m_fu = fmax(m_fu, ef);
        }
        if (traced && in) {
            if (a.err_dr) a.err_dr[base + kk] = usable ? ed : nan;
            if (a.err_fused) a.err_fused[base + kk] = usable ? ef : nan;
            if (a.trace_pos) {
                a.trace_pos[(base + kk) * 3] = pfu[0] + p0[0]; a.trace_pos[(base + kk) * 3 + 1] = pfu[1] + p0[1];
                a.trace_pos[(base + kk) * 3 + 2] = pfu[2] + p0[2];
            }
        }
    }
    if (traced) {                                                         // NaN outside [a, b)
        for (int64_t kk = lane; kk < N; kk += 64) {
            if (kk >= oa && kk < ob) continue;
            if (a.err_dr) a.err_dr[base + kk] = nan;
            if (a.err_fused) a.err_fused[base + kk] = nan;
            if (a.trace_pos) { a.trace_pos[(base + kk) * 3] = nan; a.trace_pos[(base + kk) * 3 + 1] = nan; a.trace_pos[(base + kk) * 3 + 2] = nan; }
        }
    }
    const Sums16 sm = wave_sum16(nE, s_dr, s_fu, h_dr, h_fu, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, lane);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m_dr = fmax(m_dr, __shfl_xor(m_dr, off, 64)); m_fu = fmax(m_fu, __shfl_xor(m_fu, off, 64));
    }
    if (lane == 0) {
        if (a.stats) {
            double* st = a.stats + row * OUTAGE_NSTAT;
            st[0] = sm.v[0]; st[1] = (double)nH; st[2] = (double)(ob - oa); st[3] = gap; st[4] = dist;
            st[5] = sm.v[1]; st[6] = m_dr; st[7] = sm.v[2]; st[8] = m_fu; st[9] = sm.v[3]; st[10] = sm.v[4];
            st[11] = ynorm; st[12] = nis;
        }
        if (a.seg) { a.seg[row * 2] = (int32_t)oa; a.seg[row * 2 + 1] = (int32_t)ob; }
        if (a.os_flags) a.os_flags[row] = flag_word;
    }
}

}  // namespace

namespace gsf {

int launch_outage_study(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                        const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                        const gsf_ekf_config* cfg, int64_t B, const double* truth, const uint8_t* truth_valid, const double* scen, int32_t K,
                        int32_t trace_k, double* stats, int32_t* seg, int32_t* os_flags, double* err_dr, double* err_fused, double* trace_pos)
{
    GSF_REQUIRE(B * (int64_t)K <= (int64_t)0x7fffffff, "B x K too large for one launch");
    GSF_HIP(hipSetDevice(ctx->device));
    // the workspace holds one row per pose; the number of poses is offsets[B], a device value: one 8-byte read behind the stream's work
    int64_t total = 0;
    GSF_HIP(hipMemcpyAsync(&total, offsets + B, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    GSF_HIP(hipStreamSynchronize(ctx->stream));
    GSF_REQUIRE(total >= 0, "offsets[B] is negative");
    const size_t P = total > 0 ? (size_t)total : 1;
    const size_t row_bytes = P * OUTAGE_ROW * sizeof(double), flag_bytes = (P + 7) / 8 * 8, word_bytes = (size_t)B * sizeof(int32_t);
    const int rc = ensure_workspace(ctx, GSF_WS_KERNEL, row_bytes + flag_bytes + word_bytes);
    if (rc != GSF_OK) return rc;
    char* w = workspace<char>(ctx, GSF_WS_KERNEL);
    double* rows = (double*)w; uint8_t* flags = (uint8_t*)(w + row_bytes); int32_t* unsorted = (int32_t*)(w + row_bytes + flag_bytes);
    const EkfConfig k = to_core(cfg);
    const BaseArgs ba{ ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, rows, flags, unsorted };
    hipLaunchKernelGGL(outage_base_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, ba, k);
    GSF_HIP(hipGetLastError());
    StudyArgs sa{ ts, gps, truth ? truth : gps, truth_valid ? truth_valid : valid, offsets, run_status, init_pos, scen, rows, flags, unsorted,
                  stats, seg, os_flags, err_dr, err_fused, trace_pos, { k.Qps[0], k.Qps[1], k.Qps[2] }, { k.Rm[0], k.Rm[1], k.Rm[2] },
                  k.yaw_thr_rad < 0.0 ? 1 : 0, K, trace_k };
    hipLaunchKernelGGL(outage_scenario_kernel, dim3((unsigned)(B * K)), dim3(64), 0, ctx->stream, sa);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace gsf
