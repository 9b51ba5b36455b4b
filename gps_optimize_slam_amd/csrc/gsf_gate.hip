// gsf_gate.hip -- innovation gate: reject the GNSS fixes the filter disbelieves, K gates per track in one launch (gsf_innovation_gate_dev).
//
// One wave per (track, gate), 64 poses per chunk.  What does not depend on a rejection is formed once per chunk with the shared chunk body of
// gsf_track_chunk.hpp -- the rows, dt, the "fix usable" ballot, the yaw-rate test of EVERY adjacent pair, d[i].  What does depend on it
// -- the availability mask, the outage structure and the blend weight of a sharp-turn recovery, variance_chunk() and the three
// position scans -- runs inside a speculate-and-repair loop (gsf_gate_core.hpp): scan under the current
// rejection mask, ballot the lanes that are tested, applied and over the gate, settle the LOWEST one (every decision before it is
// final), scan again.  The ballot decides the trip count, so the loop is wave-uniform: one pass for a chunk without a rejection, one
// more per rejection.  The carries (variance, position, outage state, the run of rejected fixes) are taken from the settled pass only.
// No LDS, no atomics, nothing shared between gates: a gate's rows are the same bytes for any K, any order and any neighbours.  A second
// small kernel ors the per-(track, gate) words into gate_status[B] in a fixed order.  Definitions: include/gsf.h.
#include "gsf_track_chunk.hpp"
#include "gsf_gate_core.hpp"

namespace {

struct GateArgs {
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid;
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* init_quat; const double* gates;
    uint8_t* valid_out; double* nis_out; double* stats; int32_t* words;
    double arm_seconds;
    int64_t B;
    int32_t K, max_run;
};

// a row that holds no filter run: every stats entry = fill, the track's NIS rows NaN, its mask bytes zero or copied
__device__ __forceinline__ void gate_plain_row(const GateArgs& a, const int64_t row, const int64_t at, const int64_t base, const int64_t N,
                                               const int lane, const int32_t word, const double fill, const bool copy_valid)
{
    const double nan = __builtin_nan("");
    for (int64_t k = lane; k < N; k += 64) {
        if (a.valid_out) a.valid_out[at + k] = copy_valid ? a.valid[base + k] : (uint8_t)0;
        if (a.nis_out) a.nis_out[at + k] = nan;
    }
    if (lane == 0) {
        if (a.stats) for (int j = 0; j < GATE_NSTAT; ++j) a.stats[row * GATE_NSTAT + j] = fill;
        a.words[row] = word;
    }
}

__global__ __launch_bounds__(64) void innovation_gate_kernel(const GateArgs a, const EkfConfig cfg)
{
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)(blockIdx.x / (unsigned)a.K);
    const int k = (int)(blockIdx.x % (unsigned)a.K);
    const int64_t row = b * a.K + k;
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    const int64_t P = uniform64(a.offsets[a.B]);
    const int64_t at = (int64_t)k * P + base;                             // this (gate, track)'s place in valid_out / nis_out
    if (a.run_status && a.run_status[b] != 0) {                           // the run stopped before the filter: inputs not read
        gate_plain_row(a, row, at, base, N > 0 ? N : 0, lane, GATE_SKIPPED, __builtin_nan(""), false);
        return;
    }
    if (N <= 0) {                                                         // an empty track (ref :835): no pose, no update
        if (lane == 0) {
            if (a.stats) for (int j = 0; j < GATE_NSTAT; ++j) a.stats[row * GATE_NSTAT + j] = (j == 5) ? -1.0 : 0.0;
            a.words[row] = GATE_EMPTY;
        }
        return;
    }
    const double gate = a.gates[k];
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;
    ChunkIn nxt = load_chunk(tsb, posb, quatb, gpsb, valb, lane, N);

    // ---- carried from chunk to chunk (wave-uniform), from the settled pass only
    double cP[3] = { cfg.P0[0], cfg.P0[1], cfg.P0[2] };                   // Pf of the last pose (pose 0: P0)
    double cx[3] = { 0.0, 0.0, 0.0 };                                     // its position relative to init_pos
    int same1, same2;
    same_axes(cfg.P0, cfg.Qps, cfg.Rm, same1, same2);
    TrackCarry tc = track_carry_init(a.init_pos, a.init_quat, b, nxt, cfg);
    bool c_ok = tc.first_ok;                                             // a local, not a member of the carry: gsf_track_chunk.hpp
    const double t_arm = tc.c_t + a.arm_seconds;                          // fixes with a later stamp are tested
    const bool test_all = !(a.arm_seconds > 0.0);
    u64 unsorted_m = (tc.c_t != tc.c_t) ? 1ull : 0ull;                    // a NaN first stamp
    GateCounts cnt = gate_counts_init();
    double nis_max = 0.0, nis_sum = 0.0;                                  // over the tested fixes that were applied

    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const ChunkIn in = nxt;
        nxt = load_chunk(tsb, posb, quatb, gpsb, valb, c0 + 64 + lane, N);   // the next chunk's rows are requested before this chunk's scans (clamped past the end)
        const ChunkFront f = chunk_front(in, tc, c_ok, c0, N, lane);
        const int64_t i = f.i;
        const int L = f.L;
        const bool active = f.active, stepping = f.stepping, fix = f.fix;   // fix: usable before any rejection
        const double dt = f.dt;
        unsorted_m |= __ballot(stepping && !(f.t >= f.t_pr));             // a stamp below the one before it, or a NaN one
        const u64 fix_m = __ballot(fix) & f.act_m;
        const u64 tested_m = test_all ? fix_m : (fix_m & __ballot(f.t > t_arm));
        const u64 pair_m = yaw_pair_mask<true>(f, 0ull, cfg.yaw_thr_rad, lane);   // EVERY adjacent pair: a rejection may put any of them inside an outage

        const Vec3 u = orientation_step<false>(tc, c_ok, f).u;                 // the predicted displacement d[i] (ref :707)
        const double d[3] = { u.x, u.y, u.z };
        const double zr[3] = { f.z.x - tc.p0.x, f.z.y - tc.p0.y, f.z.z - tc.p0.z };   // relative to init_pos: y is a difference of two UTM northings

        // ---- speculate and repair: the filter under the current rejection mask, then the lowest lane over the gate is settled
        GateRepair g{ 0ull, 0ull, 0 };
        u64 av_m, f_mask; OutageMasks om;
        double Pf[3], x[3], nis;
        for (;;) {
            const bool avail = fix && !((g.rej >> lane) & 1ull);          // a rejected fix is a pose without a fix, in every respect
            // outage structure and the sharp-turn decision under this mask: gsf_ekf_cov_ragged_dev's (gsf_cov_core.hpp)
            av_m = avail_mask(f, avail);
            om = outage_masks(f.act_m, av_m, c0 == 0, tc.oc.prev_avail);
            f_mask = pair_m & om.pair;
            const u64 sharp_m = sharp_recoveries(om, f_mask, c0, tc.oc, cfg.yaw_thr_rad < 0.0);
            const double wgt = ((sharp_m >> lane) & 1ull) ? tc.wgt_sharp : 1.0;   // the one-step blend at a sharp-turn recovery, else a hard update
            // variances, gains and the three affine scans of the noise sweep, cfg's own noise
            AxisVar v0, v1, v2;
            variance_chunk<6>(cfg, same1, same2, dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
            const double Pm[3] = { v0.Pm, v1.Pm, v2.Pm }, kg[3] = { v0.kg, v1.kg, v2.kg };
            Pf[0] = v0.Pf; Pf[1] = v1.Pf; Pf[2] = v2.Pf;
            double y[3], S[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const AxisPos ap = position_axis(avail, kg[c] * wgt, d[c], zr[c], cx[c]);
                x[c] = ap.x;                                              // p[i] - init_pos
                y[c] = zr[c] - ap.pm;                                     // ref :722
                S[c] = Pm[c] + cfg.Rm[c];                                 // ref :723
            }
            nis = gate_nis(y, S);                                         // of the predicted state: the same whether the fix is applied or not
            const u64 over_m = __ballot(nis > gate) & tested_m;           // (false for a NaN NIS and for gate = +inf)
            if (!gate_settle(g, over_m, fix_m, cnt.run, a.max_run)) break;   // wave-uniform: the ballot decides
        }

        // ---- the settled chunk: rows, counts, carries
        const bool rejected = (g.rej >> lane) & 1ull;
        if (active) {
            if (a.valid_out) a.valid_out[at + i] = rejected ? (uint8_t)0 : (uint8_t)in.v;
            if (a.nis_out) a.nis_out[at + i] = fix ? nis : __builtin_nan("");
        }
        const bool applied_tested = ((tested_m & ~g.rej) >> lane) & 1ull;
        nis_sum = nis_sum + wave_sum(applied_tested ? nis : 0.0);
        double mx = applied_tested ? nis : 0.0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
        nis_max = fmax(nis_max, mx);
        gate_chunk_counts(cnt, fix_m, tested_m, g.rej, g.forced, c0);
#pragma unroll
        for (int c = 0; c < 3; ++c) { cP[c] = lane_bcast(Pf[c], L); cx[c] = lane_bcast(x[c], L); }
        track_carry_next(tc, f, c0, av_m, om.start, f_mask);
        c_ok = last_ok(f);
    }

    if (unsorted_m != 0ull) {                                             // no filter run is defined: NaN rows, the mask as it came
        gate_plain_row(a, row, at, base, N, lane, GATE_UNSORTED, __builtin_nan(""), true);   // (lane l rewrites the rows lane l wrote)
        return;
    }
    if (lane == 0) {
        if (a.stats) {
            double* st = a.stats + row * GATE_NSTAT;
            st[0] = (double)cnt.n_avail; st[1] = (double)cnt.n_tested; st[2] = (double)cnt.n_rejected; st[3] = (double)cnt.n_forced;
            st[4] = (double)cnt.longest; st[5] = (double)cnt.first; st[6] = nis_max; st[7] = nis_sum;
        }
        a.words[row] = (cnt.n_rejected > 0 ? GATE_ANY_REJECTED : 0) | (cnt.n_forced > 0 ? GATE_ANY_FORCED : 0);
    }
}

// gate_status[b] = the words of the track's K gates or'ed, one thread per track, ascending k
__global__ __launch_bounds__(64) void gate_status_kernel(const int32_t* words, const int64_t B, const int32_t K, int32_t* gate_status)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int32_t w = 0;
    for (int k = 0; k < K; ++k) w |= words[b * K + k];
    gate_status[b] = w;
}

}  // namespace

namespace gsf {

int launch_innovation_gate(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                           const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                           const gsf_ekf_config* cfg, int64_t B, const double* gates, int32_t K, double arm_seconds, int32_t max_run,
                           uint8_t* valid_out, double* nis_out, double* stats, int32_t* gate_status)
{
    GSF_REQUIRE(B * (int64_t)K <= (int64_t)0x7fffffff, "B x K too large for one launch");
    GSF_HIP(hipSetDevice(ctx->device));
    const int rc = ensure_workspace(ctx, GSF_WS_KERNEL, (size_t)B * (size_t)K * sizeof(int32_t));   // one word per (track, gate)
    if (rc != GSF_OK) return rc;
    int32_t* words = workspace<int32_t>(ctx, GSF_WS_KERNEL);
    const EkfConfig kc = to_core(cfg);
    const GateArgs a{ ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, gates, valid_out, nis_out, stats, words,
                      arm_seconds, B, K, max_run };
    hipLaunchKernelGGL(innovation_gate_kernel, dim3((unsigned)(B * K)), dim3(64), 0, ctx->stream, a, kc);
    GSF_HIP(hipGetLastError());
    if (gate_status) {
        hipLaunchKernelGGL(gate_status_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx->stream, (const int32_t*)words, B, K, gate_status);
        GSF_HIP(hipGetLastError());
    }
    return GSF_OK;
}

}  // namespace gsf
