// gsf_noise_sweep.hip -- innovation statistics of the EKF for K noise candidates per track (gsf_ekf_noise_sweep_dev).
//
// The state quaternion is never touched by GNSS, so the world-frame odometry increments d[i] = R(q_state[i-1]) dp_local[i]
// are the same for every (P0, Q, R); RTS rewrites outputs only (ref :918-922), so the innovations do not depend on it.  One wave therefore
// reads a chunk of 64 poses ONCE (89 B per pose), forms what every candidate shares -- dt, the "fix used" flags, the outage structure and
// the blend weight of a sharp-turn recovery, d[i] -- and then runs its group of candidates one after the other on registers: the variance
// scans of the pose kernels (variance_chunk) give Pp and the gain, three affine scans give the positions, the twelve terms of
// gsf_sweep_core.hpp are summed with one wave_sum16, and nothing is written per pose (except the optional trace of one candidate).
// Grid: B x ceil(K / KC) workgroups of one wave; lane l of a wave holds the noise values, the carry and the twelve accumulators of the
// l-th candidate of its group and hands them to the wave with v_readlane, so a candidate's arithmetic is the same instructions on the
// same operands whatever its group: its row is the same bytes for every KC.  Definitions: include/gsf.h; KC: sweep_group(), gsf_wave_route.hpp.
#include "gsf_wave_common.hpp"
#include "gsf_cov_core.hpp"
#include "gsf_sweep_core.hpp"

namespace {

struct SweepArgs {
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid;
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* init_quat; const double* cand;
    double* stats; double* innov; double* innov_var;
    double skip_seconds;
    int32_t K, KC, G, trace_k;
};

// (two waves per SIMD: the register budget sweep_group() counts on)
__global__ __launch_bounds__(64, 2) void noise_sweep_kernel(const SweepArgs a, const EkfConfig cfg)
{
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)(blockIdx.x / (unsigned)a.G);
    const int k0 = (int)(blockIdx.x % (unsigned)a.G) * a.KC;              // first candidate of this wave's group
    const int kc = (a.K - k0 < a.KC) ? a.K - k0 : a.KC;                   // ... and how many it holds (>= 1 by the grid's construction)
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    const int tk = a.trace_k - k0;                                        // the traced candidate's place in this group, if it is here
    const bool traced = (a.innov || a.innov_var) && a.trace_k >= 0 && tk >= 0 && tk < kc;
    double* strow = a.stats ? a.stats + ((b * a.K + k0) * SWEEP_NSTAT) : nullptr;
    if (N <= 0) {                                                         // an empty track (ref :835): no update, all sums zero, no trace rows
        if (strow && lane < kc) for (int j = 0; j < SWEEP_NSTAT; ++j) strow[lane * SWEEP_NSTAT + j] = 0.0;
        return;
    }
    if (a.run_status && a.run_status[b] != 0) {                           // the run stopped before the filter: NaN rows, inputs not read
        const double nan = __builtin_nan("");
        if (strow && lane < kc) for (int j = 0; j < SWEEP_NSTAT; ++j) strow[lane * SWEEP_NSTAT + j] = nan;
        if (traced) {
            for (int64_t k = lane; k < N * 3; k += 64) {
                if (a.innov) a.innov[base * 3 + k] = nan;
                if (a.innov_var) a.innov_var[base * 3 + k] = nan;
            }
        }
        return;
    }
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;
    ChunkIn nxt = load_chunk(tsb, posb, quatb, gpsb, valb, lane, N);

    // ---- this lane's candidate (idle lanes of a short group repeat its first one; their registers are never read).  The noise values
    // themselves are wave-uniform in the loop over the group and come through the scalar cache there.
    const double* cr = a.cand + (int64_t)(k0 + (lane < kc ? lane : 0)) * 9;
    double mPf[3] = { cr[0], cr[1], cr[2] };                              // carried: Pf of the last pose (pose 0: P0) ...
    double mp[3] = { 0.0, 0.0, 0.0 };                                     // ... its position relative to init_pos ...
    double mnu[3] = { 0.0, 0.0, 0.0 };                                    // ... and its normalised innovation (zero if it was not a counted update)
    double acc[SWEEP_NSTAT];
#pragma unroll
    for (int j = 0; j < SWEEP_NSTAT; ++j) acc[j] = 0.0;

    // ---- carried from chunk to chunk, the same for every candidate (wave-uniform)
    const Vec3 p0{ a.init_pos[b * 3], a.init_pos[b * 3 + 1], a.init_pos[b * 3 + 2] };
    Quat cq = ekf_normalize(Quat{ a.init_quat[b * 4], a.init_quat[b * 4 + 1], a.init_quat[b * 4 + 2], a.init_quat[b * 4 + 3] });   // ref :842, :683
    chunk_arrived(nxt);
    Vec3 c_po = lane_bcast(nxt.p, 0);                                     // "previous original pose" of pose 0 is pose 0 itself (ref :858)
    Quat c_r; bool c_ok = quat_unit(lane_bcast(nxt.q, 0), c_r);
    double c_t = lane_bcast(nxt.t, 0);
    const double t_count = c_t + a.skip_seconds;                          // updates with a later stamp are counted
    const bool count_all = !(a.skip_seconds > 0.0);
    Quat Cq = lane_bcast(quat_mul(cq, quat_conj(c_r)), 0);               // q_i = Cq r_i while every quaternion is valid (see wave_serial_chunks)
    bool cq_fresh = true;
    OutageCarry oc{ true, 0, false };
    bool c_counted = false;                                               // the last pose of the chunk before was a counted update
    const double wgt_sharp = (cfg.sharp_turn_steps > 1) ? 1.0 / (double)cfg.sharp_turn_steps : 1.0;   // ref :752-768, :889

    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const int64_t i = c0 + lane;
        const int L = (int)((N - c0 < 64) ? (N - c0 - 1) : 63);
        const bool active = i < N, stepping = active && i != 0;
        const ChunkIn in = nxt;
        nxt = load_chunk(tsb, posb, quatb, gpsb, valb, c0 + 64 + lane, N);   // the next chunk's rows are requested before this chunk's scans (clamped past the end)
        const double t = in.t;
        const Vec3 p = in.p, z = in.z;
        // ---- calculate_relative_pose (ref :77-92) against the previous lane / the carry
        Quat r; const bool ok = quat_unit(in.q, r);
        const double t_pr = prev_lane(c_t, t);
        const Vec3 p_pr{ prev_lane(c_po.x, p.x), prev_lane(c_po.y, p.y), prev_lane(c_po.z, p.z) };
        const u64 act_m = mask_first(L + 1);
        const u64 ok_mask = __ballot(ok);
        const u64 both_m = ((ok_mask << 1) | (c_ok ? 1ull : 0ull)) & ok_mask;
        const bool both_ok = (both_m >> lane) & 1ull;
        const double dt = fmax(1e-6, t - t_pr);                          // ref :865
        const bool vraw = in.v != 0;
        const bool avail = stepping && vraw && !(isnan(z.x) || isnan(z.y) || isnan(z.z));   // ref :867-869
        // ---- outage structure and the sharp-turn decision: gsf_ekf_cov_ragged_dev's (gsf_cov_core.hpp)
        const u64 avail_m = __ballot(avail) & act_m;
        const u64 av_m = __ballot(i == 0 ? vraw : avail) & act_m;         // pose 0: the raw mask byte (:848)
        const OutageMasks om = outage_masks(act_m, av_m, c0 == 0, oc.prev_avail);
        const Quat r_pr = prev_lane(c_r, r);
        u64 f_mask = 0ull;
        if (om.pair != 0ull) {
            const bool outpair = (om.pair >> lane) & 1ull;
            bool f = false;
            if (outpair && t > t_pr) f = !both_ok || yaw_rate_exceeds_body(r_pr, r, t - t_pr, cfg.yaw_thr_rad);   // :817, :821-824
            f_mask = __ballot(f);
        }
        u64 sharp_m = 0ull;
        for (u64 rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
            const int rl = __builtin_ctzll(rm);
            const OutageSeg sg = outage_closed_at(om.start, f_mask, rl, c0, oc.ostart, oc.seg_sharp, cfg.yaw_thr_rad < 0.0);
            if (sg.sharp) sharp_m |= 1ull << rl;
        }
        const double wgt = ((sharp_m >> lane) & 1ull) ? wgt_sharp : 1.0;   // the one-step blend at a sharp-turn recovery, else a hard update
        // ---- which updates are counted (U) and which pairs (i - 1, i) lie in U
        const u64 cnt_m = count_all ? avail_m : (avail_m & __ballot(t > t_count));
        const u64 cntp_m = (cnt_m << 1) | (c_counted ? 1ull : 0ull);
        const bool counted = (cnt_m >> lane) & 1ull, counted_prev = (cntp_m >> lane) & 1ull;

        // ---- predicted displacement d[i] (ref :707), as the pose kernels form it: one rotation by the wave-uniform Cq while every
        // quaternion is valid, else calculate_relative_pose per pose and a prefix product of the increments
        const Vec3 dp{ p.x - p_pr.x, p.y - p_pr.y, p.z - p_pr.z };
        Vec3 u;
        const bool telescope = c_ok && ((ok_mask & act_m) == act_m);
        if (telescope) {
            u = quat_rotate(Cq, dp);
            u.x = stepping ? u.x : 0.0; u.y = stepping ? u.y : 0.0; u.z = stepping ? u.z : 0.0;
            cq_fresh = false;
        } else {
            if (!cq_fresh) { cq = quat_mul(Cq, c_r); cq_fresh = true; }
            const Quat r1i = quat_conj(r_pr);
            Vec3 dpl = quat_rotate(r1i, dp);
            Quat dq = quat_mul(r1i, r);
            const bool move = stepping && both_ok;
            dpl.x = move ? dpl.x : 0.0; dpl.y = move ? dpl.y : 0.0; dpl.z = move ? dpl.z : 0.0;
            dq.x = move ? dq.x : 0.0; dq.y = move ? dq.y : 0.0; dq.z = move ? dq.z : 0.0; dq.w = move ? dq.w : 1.0;
            Quat D = dq;
            const Quat QID{ 0.0, 0.0, 0.0, 1.0 };
#define GSF_QSTAGE(CTRL, RM) { const Quat o = dpp<CTRL, RM>(QID, D); D = quat_mul(o, D); }
            GSF_SCAN_STAGES(GSF_QSTAGE)
#undef GSF_QSTAGE
            const Quat qi = ekf_normalize(quat_mul(cq, D));
            const Quat q_prev = prev_lane(cq, qi);
            u = quat_rotate(q_prev, dpl);
            cq = lane_bcast(qi, L);
            if (((ok_mask >> L) & 1ull) != 0ull) Cq = lane_bcast(quat_mul(cq, quat_conj(lane_bcast(r, L))), 0);
        }
        const double d[3] = { u.x, u.y, u.z };
        const double zr[3] = { z.x - p0.x, z.y - p0.y, z.z - p0.z };       // relative to init_pos: y is a difference of two UTM northings

        // ---- the candidates of the group, one after the other: one code path, a run-time loop
        for (int kk = 0; kk < kc; ++kk) {
            EkfConfig kcfg = cfg;
            const double* ck = a.cand + (int64_t)(k0 + kk) * 9;           // { P0[3], Q[3], R[3] }
            double cP[3], cx[3], cnu[3], P0k[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                P0k[c] = ck[c]; kcfg.Qps[c] = ck[3 + c]; kcfg.Rm[c] = ck[6 + c];
                cP[c] = lane_bcast(mPf[c], kk); cx[c] = lane_bcast(mp[c], kk); cnu[c] = lane_bcast(mnu[c], kk);
            }
            int same1 = -1, same2 = -1;                                   // axes with identical (P0, Q, R) share their variance scan
            if (P0k[1] == P0k[0] && kcfg.Qps[1] == kcfg.Qps[0] && kcfg.Rm[1] == kcfg.Rm[0]) same1 = 0;
            if (P0k[2] == P0k[0] && kcfg.Qps[2] == kcfg.Qps[0] && kcfg.Rm[2] == kcfg.Rm[0]) same2 = 0;
            else if (P0k[2] == P0k[1] && kcfg.Qps[2] == kcfg.Qps[1] && kcfg.Rm[2] == kcfg.Rm[1]) same2 = 1;
            AxisVar v0, v1, v2;
            variance_chunk<6>(kcfg, same1, same2, dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
            const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, Pm[3] = { v0.Pm, v1.Pm, v2.Pm }, kg[3] = { v0.kg, v1.kg, v2.kg };
            double x[3], y[3], S[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Affine m = sweep_affine(avail, kg[c] * wgt, d[c], zr[c]);
#define GSF_ASTAGE(CTRL, RM) { const Affine o{ dpp<CTRL, RM>(1.0, m.a), dpp0<CTRL, RM>(m.b) }; m = affine_compose(m, o); }
                GSF_SCAN_STAGES(GSF_ASTAGE)
#undef GSF_ASTAGE
                x[c] = affine_apply(m, cx[c]);                            // p[i] - init_pos
                const double pm = prev_lane(cx[c], x[c]) + d[c];          // p-[i] - init_pos (ref :707)
                y[c] = zr[c] - pm;                                        // ref :722
                S[c] = Pm[c] + kcfg.Rm[c];                                // ref :723
            }
            double nu[3], nu_prev[3], term[SWEEP_NSTAT];
            sweep_pose_nu(y, S, counted, nu);
#pragma unroll
            for (int c = 0; c < 3; ++c) nu_prev[c] = prev_lane(cnu[c], nu[c]);
            sweep_pose_terms(y, S, nu, nu_prev, counted, counted_prev, term);
            const Sums16 sm = wave_sum16(term[0], term[1], term[2], term[3], term[4], term[5], term[6], term[7], term[8], term[9], term[10],
                                         term[11], 0.0, 0.0, 0.0, 0.0, lane);
            const bool mine = lane == kk;
#pragma unroll
            for (int j = 0; j < SWEEP_NSTAT; ++j) { const double s = acc[j] + sm.v[j]; acc[j] = mine ? s : acc[j]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double pf = lane_bcast(Pf[c], L), xl = lane_bcast(x[c], L), nl = lane_bcast(nu[c], L);
                mPf[c] = mine ? pf : mPf[c]; mp[c] = mine ? xl : mp[c]; mnu[c] = mine ? nl : mnu[c];
            }
            if (traced && kk == tk && active) {                          // y and S of every pose with an update, NaN elsewhere
                const double nan = __builtin_nan("");
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (a.innov) a.innov[(base + i) * 3 + c] = avail ? y[c] : nan;
                    if (a.innov_var) a.innov_var[(base + i) * 3 + c] = avail ? S[c] : nan;
                }
            }
        }

        // ---- carry to the next 64 poses (from the last active lane L)
        oc = outage_carry(oc, av_m, om.start, f_mask, L, c0);
        c_counted = ((cnt_m >> L) & 1ull) != 0ull;
        c_po = lane_bcast(p, L); c_r = lane_bcast(r, L); c_ok = ((ok_mask >> L) & 1ull) != 0ull; c_t = lane_bcast(t, L);
    }
    if (strow && lane < kc) {
#pragma unroll
        for (int j = 0; j < SWEEP_NSTAT; ++j) strow[lane * SWEEP_NSTAT + j] = acc[j];
    }
}

// this lane's better (score, k) of the wave: the first k with the smallest score; k = INT32_MAX where no row may be picked
__device__ __forceinline__ int wave_first_min(double s, int k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double os = __shfl_xor(s, off, 64); const int ok = __shfl_xor(k, off, 64);
        if (sweep_pick_before(os, ok, s, k)) { s = os; k = ok; }
    }
    return k;
}
// the two picks over K rows of 12 sums (wave-uniform result); -1 where n_upd < min_updates or no row is finite
__device__ __forceinline__ void pick_rows(const double* rows, const int K, const int32_t min_updates, const int lane, int& b0, int& b1)
{
    const bool enough = rows[0] >= (double)min_updates;                   // (false for NaN)
    int pick[2];
    for (int crit = 0; crit < 2; ++crit) {
        double bs = __builtin_huge_val(); int bk = 0x7fffffff;
        for (int k = lane; k < K; k += 64) {
            const double s = sweep_score(rows + (int64_t)k * SWEEP_NSTAT, crit);
            if (s < __builtin_huge_val() && sweep_pick_before(s, k, bs, bk)) { bs = s; bk = k; }
        }
        const int k = wave_first_min(bs, bk);
        pick[crit] = (enough && k != 0x7fffffff) ? k : -1;
    }
    b0 = pick[0]; b1 = pick[1];
}
__device__ __forceinline__ int32_t pick_status(const int b0, const int b1)
{
    return (b0 < 0 || b1 < 0) ? NS_NONE : (b0 != b1 ? NS_TIE : 0);
}

struct PickArgs {
    const double* stats; const int32_t* run_status; const int64_t* offsets;
    int32_t* best_k; double* pooled; int32_t* pooled_best; int32_t* ns_status;
    int64_t B; int32_t K, min_updates, pool_blocks;
};
// Blocks 0..B-1: the picks of one track each.  Blocks B..: 64 entries of pooled[K][12] each, every entry one lane's sum over the tracks in
// ascending b -- a fixed order, no atomics, so the bytes are reproducible.
__global__ __launch_bounds__(64) void noise_pick_kernel(const PickArgs a)
{
    const int lane = (int)threadIdx.x;
    const int64_t blk = blockIdx.x;
    if (blk < a.B) {
        if (!a.best_k && !a.ns_status) return;
        const bool stopped = a.run_status && a.run_status[blk] != 0;
        const bool empty = a.offsets[blk + 1] <= a.offsets[blk];
        int b0 = -1, b1 = -1;
        if (!stopped && !empty) pick_rows(a.stats + blk * a.K * SWEEP_NSTAT, a.K, a.min_updates, lane, b0, b1);
        if (lane == 0) {
            if (a.best_k) { a.best_k[blk * 2] = b0; a.best_k[blk * 2 + 1] = b1; }
            if (a.ns_status) a.ns_status[blk] = pick_status(b0, b1);
        }
        return;
    }
    const int64_t e = (blk - a.B) * 64 + lane;
    if (e >= (int64_t)a.K * SWEEP_NSTAT) return;
    double sum = 0.0;
    for (int64_t b = 0; b < a.B; ++b) {
        const bool stopped = a.run_status && a.run_status[b] != 0;
        if (stopped || a.offsets[b + 1] <= a.offsets[b]) continue;
        const double* rows = a.stats + b * a.K * SWEEP_NSTAT;
        if (rows[0] >= (double)a.min_updates) sum += rows[e];
    }
    a.pooled[e] = sum;
}
__global__ __launch_bounds__(64) void noise_pooled_pick_kernel(const double* pooled, const int K, const int32_t min_updates, int32_t* pooled_best)
{
    int b0, b1;
    pick_rows(pooled, K, min_updates, (int)threadIdx.x, b0, b1);
    if (threadIdx.x == 0) { pooled_best[0] = b0; pooled_best[1] = b1; }
}

}  // namespace

namespace gsf {

int launch_noise_sweep(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                       const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                       const gsf_ekf_config* cfg, int64_t B, const double* cand, int32_t K, double skip_seconds, int32_t min_updates,
                       int32_t trace_k, double* stats, int32_t* best_k, double* pooled, int32_t* pooled_best, int32_t* ns_status,
                       double* innov, double* innov_var)
{
    const int KC = sweep_group(B, K, ctx->noise_sweep_group);
    const int G = (K + KC - 1) / KC;
    GSF_REQUIRE(B * (int64_t)G + (int64_t)(K * SWEEP_NSTAT + 63) / 64 <= (int64_t)0x7fffffff, "B x groups too large for one launch");
    GSF_HIP(hipSetDevice(ctx->device));
    // the picks read the rows of sums: where the caller does not ask for stats (or for pooled, and wants its pick) they live in the kernel workspace
    const bool picks = best_k || ns_status || pooled || pooled_best;
    const size_t pooled_bytes = (size_t)K * SWEEP_NSTAT * sizeof(double), stats_bytes = (size_t)B * (size_t)K * SWEEP_NSTAT * sizeof(double);
    const bool ws_pooled = pooled_best && !pooled, ws_stats = picks && !stats;
    if (ws_pooled || ws_stats) {
        const int rc = ensure_workspace(ctx, GSF_WS_KERNEL, (ws_pooled ? pooled_bytes : 0) + (ws_stats ? stats_bytes : 0));
        if (rc != GSF_OK) return rc;
        char* w = workspace<char>(ctx, GSF_WS_KERNEL);
        if (ws_pooled) { pooled = (double*)w; w += pooled_bytes; }
        if (ws_stats) stats = (double*)w;
    }
    const EkfConfig k = to_core(cfg);
    const SweepArgs a{ ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, cand, stats, innov, innov_var, skip_seconds, K, KC, G, trace_k };
    hipLaunchKernelGGL(noise_sweep_kernel, dim3((unsigned)(B * G)), dim3(64), 0, ctx->stream, a, k);
    GSF_HIP(hipGetLastError());
    if (picks) {
        const int pool_blocks = (pooled || pooled_best) ? (K * SWEEP_NSTAT + 63) / 64 : 0;
        const PickArgs pa{ stats, run_status, offsets, best_k, pooled, pooled_best, ns_status, B, K, min_updates, pool_blocks };
        hipLaunchKernelGGL(noise_pick_kernel, dim3((unsigned)(B + pool_blocks)), dim3(64), 0, ctx->stream, pa);
        GSF_HIP(hipGetLastError());
        if (pooled_best) {
            hipLaunchKernelGGL(noise_pooled_pick_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)pooled, (int)K, min_updates, pooled_best);
            GSF_HIP(hipGetLastError());
        }
    }
    return GSF_OK;
}

}  // namespace gsf
