// gsf_noise_sweep.hip -- innovation statistics of the EKF for K noise candidates per track (gsf_ekf_noise_sweep_dev).
//
// The state quaternion is never touched by GNSS, so the world-frame odometry increments d[i] = R(q_state[i-1]) dp_local[i]
// are the same for every (P0, Q, R); RTS rewrites outputs only (ref :918-922), so the innovations do not depend on it.  One wave therefore
// reads a chunk of 64 poses ONCE (89 B per pose), forms what every candidate shares with the shared chunk body of gsf_track_chunk.hpp -- dt,
// the "fix used" flags, the outage structure and the blend weight of a sharp-turn recovery, d[i] -- and then runs its group of candidates one after the other on registers: the variance
// scans of the pose kernels (variance_chunk) give Pp and the gain, three affine scans give the positions, the twelve terms of
// gsf_sweep_core.hpp are summed with one wave_sum16, and nothing is written per pose (except the optional trace of one candidate).
// Grid: B x ceil(K / KC) workgroups of one wave; lane l of a wave holds the noise values, the carry and the twelve accumulators of the
// l-th candidate of its group and hands them to the wave with v_readlane, so a candidate's arithmetic is the same instructions on the
// same operands whatever its group: its row is the same bytes for every KC.  Definitions: include/gsf.h; KC: sweep_group(), gsf_wave_route.hpp.
#include "gsf_track_chunk.hpp"

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
    TrackCarry tc = track_carry_init(a.init_pos, a.init_quat, b, nxt, cfg);
    const double t_count = tc.c_t + a.skip_seconds;                       // updates with a later stamp are counted
    const bool count_all = !(a.skip_seconds > 0.0);
    bool c_ok = tc.first_ok;                                             // a local, not a member of the carry: gsf_track_chunk.hpp
    bool c_counted = false;                                               // the last pose of the chunk before was a counted update

    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const ChunkIn in = nxt;
        nxt = load_chunk(tsb, posb, quatb, gpsb, valb, c0 + 64 + lane, N);   // the next chunk's rows are requested before this chunk's scans (clamped past the end)
        const ChunkFront f = chunk_front(in, tc, c_ok, c0, N, lane);
        const int64_t i = f.i;
        const int L = f.L;
        const bool active = f.active, stepping = f.stepping, avail = f.fix;
        const double dt = f.dt;
        // ---- outage structure and the sharp-turn decision: gsf_ekf_cov_ragged_dev's (gsf_cov_core.hpp)
        const u64 avail_m = __ballot(avail) & f.act_m;
        const u64 av_m = avail_mask(f, avail);
        const OutageMasks om = outage_masks(f.act_m, av_m, c0 == 0, tc.oc.prev_avail);
        const u64 f_mask = yaw_pair_mask<false>(f, om.pair, cfg.yaw_thr_rad, lane);
        const u64 sharp_m = sharp_recoveries(om, f_mask, c0, tc.oc, cfg.yaw_thr_rad < 0.0);
        const double wgt = ((sharp_m >> lane) & 1ull) ? tc.wgt_sharp : 1.0;   // the one-step blend at a sharp-turn recovery, else a hard update
        // ---- which updates are counted (U) and which pairs (i - 1, i) lie in U
        const u64 cnt_m = count_all ? avail_m : (avail_m & __ballot(f.t > t_count));
        const u64 cntp_m = (cnt_m << 1) | (c_counted ? 1ull : 0ull);
        const bool counted = (cnt_m >> lane) & 1ull, counted_prev = (cntp_m >> lane) & 1ull;

        const Vec3 u = orientation_step<false>(tc, c_ok, f).u;                 // the predicted displacement d[i] (ref :707)
        const double d[3] = { u.x, u.y, u.z };
        const double zr[3] = { f.z.x - tc.p0.x, f.z.y - tc.p0.y, f.z.z - tc.p0.z };   // relative to init_pos: y is a difference of two UTM northings

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
            int same1, same2;
            same_axes(P0k, kcfg.Qps, kcfg.Rm, same1, same2);
            AxisVar v0, v1, v2;
            variance_chunk<6>(kcfg, same1, same2, dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
            const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, Pm[3] = { v0.Pm, v1.Pm, v2.Pm }, kg[3] = { v0.kg, v1.kg, v2.kg };
            double x[3], y[3], S[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const AxisPos ap = position_axis(avail, kg[c] * wgt, d[c], zr[c], cx[c]);
                x[c] = ap.x;                                              // p[i] - init_pos
                y[c] = zr[c] - ap.pm;                                     // ref :722
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
        track_carry_next(tc, f, c0, av_m, om.start, f_mask);
        c_counted = ((cnt_m >> L) & 1ull) != 0ull;
        c_ok = last_ok(f);
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
