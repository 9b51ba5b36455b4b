// gsf_ekf_cov.hip -- per-pose covariance and smoothing flags of the fused track (gsf_ekf_cov_ragged_dev).
//
// The reference computes the filtered and predicted covariance of every pose (process_step, kept in ekf_covs_filt_hist / ekf_covs_pred_hist,
// ref :852-853, :902-903) and the smoothed covariance of every segment it hands to rts_smoother_segment (:777-803), and drops them (:917).
// They depend only on the stamps, the mask and the NaN-ness of the fixes -- plus, for the RTS decision, on the SLAM quaternions inside
// outages -- so they are a pass of their own beside the pose kernels: one wave per track, 64 poses per chunk, no LDS and no workspace,
// hence no length limit.  Definitions: include/gsf.h; derivation of the closed form and the traffic per pose: DESIGN.md.
//
// Per chunk: stamps, mask byte and fix of every pose (33 B; only the NaN-ness of the fix matters) -> the Moebius scans of
// gsf_wave_common.hpp for the three position axes (the same variance_chunk() as the pose kernels) and ONE prefix sum of dt for the four
// quaternion axes, which never see an update: Pf[c] = P0[c] + Q[c] * sum(dt).  The outage structure is bit work on the ballot of the
// "available" flag (gsf_cov_core.hpp); quaternions are read only for the pairs inside an outage, and the pair test is
// yaw_rate_exceeds_body -- the routine of the ragged fuse entry's kernel, so the RTS decisions are that entry's decisions.
// At a recovery b that is not a sharp turn, rows a..b-1 are rewritten with the closed form: those of this chunk in registers, those of
// earlier chunks by reading Pf[k] back from cov_out, 64 rows at a time on chunk boundaries -- so every lane re-reads rows it stored itself,
// and each row is rewritten at most once per track.
#include "gsf_track_chunk.hpp"

namespace {

struct CovArgs {
    const double* ts; const double* quat; const double* gps; const uint8_t* valid; const int64_t* offsets; const int32_t* run_status;
    double* cov_filt; double* cov_out; uint8_t* flags; int32_t* status;
};

__global__ __launch_bounds__(64) void ekf_cov_kernel(const CovArgs a, const EkfConfig cfg)
{
    const int64_t b = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    if (N <= 0) {                                                        // apply_ekf_correction's early return (:835): no rows
        if (lane == 0 && a.status) a.status[b] = 0;
        return;
    }
    double* cfb = a.cov_filt ? a.cov_filt + base * 7 : nullptr;
    double* cob = a.cov_out + base * 7;
    uint8_t* flb = a.flags ? a.flags + base : nullptr;
    if (a.run_status && a.run_status[b] != 0) {                          // the run stopped before the filter: NaN rows, no flags, inputs not read
        const double nan = __builtin_nan("");
        for (int64_t k = lane; k < N * 7; k += 64) { cob[k] = nan; if (cfb) cfb[k] = nan; }
        if (flb) for (int64_t k = lane; k < N; k += 64) flb[k] = 0;
        if (lane == 0 && a.status) a.status[b] = 0;
        return;
    }
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const uint8_t* __restrict__ valb = a.valid + base;
    int same1, same2;
    same_axes(cfg.P0, cfg.Qps, cfg.Rm, same1, same2);

    // carried from chunk to chunk (wave-uniform): Pf of the last pose, its stamp, the sum of dt so far, the open outage
    double cP[3] = { cfg.P0[0], cfg.P0[1], cfg.P0[2] };
    double c_t = tsb[0], c_sum = 0.0;
    OutageCarry oc{ true, 0, false };
    int32_t status = 0;

    struct HIn { double t, z0, z1, z2; uint32_t v; };
    auto hload = [&](const int64_t i) __attribute__((always_inline)) {
        const int64_t il = i < N ? i : N - 1;                            // idle lanes of the last chunk re-read the last pose
        return HIn{ tsb[il], gpsb[il * 3], gpsb[il * 3 + 1], gpsb[il * 3 + 2], valb[il] };
    };
    HIn nx = hload(lane);
    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const int64_t i = c0 + lane;
        const bool active = i < N, stepping = active && i != 0;
        const int L = (int)((N - c0 < 64) ? (N - c0 - 1) : 63);
        const HIn in = nx;
        if (c0 + 64 < N) nx = hload(c0 + 64 + lane);                     // the next chunk's rows are requested before this chunk's scans
        const double t = in.t;
        const bool vraw = in.v != 0;
        const double t_pr = prev_lane(c_t, t);
        const double dt = fmax(1e-6, t - t_pr);                          // ref :865
        const bool avail = stepping && vraw && !(isnan(in.z0) || isnan(in.z1) || isnan(in.z2));   // ref :867-869
        // ---- outage structure of the chunk (pose 0: the raw mask byte, :848)
        const u64 act_m = mask_first(L + 1);
        const u64 av_m = __ballot(i == 0 ? vraw : avail) & act_m;
        const OutageMasks om = outage_masks(act_m, av_m, c0 == 0, oc.prev_avail);
        status |= (om.start != 0ull) ? ST_HAD_OUTAGE : 0;
        const bool in_outage = ((act_m & ~av_m) >> lane) & 1ull;

        // ---- filtered variances: position axes by the scans (ref :712-713, :723-731), quaternion axes by one prefix sum of dt
        AxisVar v0, v1, v2;
        variance_chunk<6>(cfg, same1, same2, dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
        const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, Pm[3] = { v0.Pm, v1.Pm, v2.Pm };
        const double S = c_sum + wave_prefix(stepping ? dt : 0.0);
        double Pq[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) Pq[c] = cfg.P0[3 + c] + cfg.Qps[3 + c] * S;

        // ---- is_sharp_turn_in_segment (ref :808-826) over the pairs inside outages: the only place quaternions are read
        u64 f_mask = 0ull;
        if (om.pair != 0ull) {
            const bool need = ((om.pair | (om.pair >> 1)) >> lane) & 1ull;      // the pair's two poses
            Quat q{ 0.0, 0.0, 0.0, 1.0 }, qc{ 0.0, 0.0, 0.0, 1.0 };
            if (need) q = Quat{ quatb[i * 4], quatb[i * 4 + 1], quatb[i * 4 + 2], quatb[i * 4 + 3] };
            if ((om.pair & 1ull) != 0ull) {                              // lane 0 pairs with the last pose of the chunk before
                const int64_t ic = c0 - 1;
                qc = Quat{ quatb[ic * 4], quatb[ic * 4 + 1], quatb[ic * 4 + 2], quatb[ic * 4 + 3] };
            }
            Quat r, rc;
            const bool ok = quat_unit(q, r), okc = quat_unit(qc, rc);
            const Quat r_pr = prev_lane(rc, r);
            const u64 ok_m = __ballot(ok);
            const u64 both_m = ((ok_m << 1) | (okc ? 1ull : 0ull)) & ok_m;
            const bool both_ok = (both_m >> lane) & 1ull, outpair = (om.pair >> lane) & 1ull;
            bool f = false;
            if (outpair && t > t_pr) f = !both_ok || yaw_rate_exceeds_body(r_pr, r, t - t_pr, cfg.yaw_thr_rad);   // :817, :821-824
            f_mask = __ballot(f);
        }

        // ---- recoveries of the chunk, one after the other (wave-uniform): RTS decision (:879-894), flags, smoothed rows (:906-922)
        int fl = avail ? POSE_GNSS_USED : (in_outage ? POSE_IN_OUTAGE : 0);
        double Po[3] = { Pf[0], Pf[1], Pf[2] };
        for (u64 rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
            const int r = __builtin_ctzll(rm);
            const OutageSeg sg = outage_closed_at(om.start, f_mask, r, c0, oc.ostart, oc.seg_sharp, cfg.yaw_thr_rad < 0.0);
            status |= sg.sharp ? ST_SHARP_TURN : ST_RTS_APPLIED;
            const int mark = POSE_IN_OUTAGE | (sg.sharp ? POSE_SHARP_TURN : POSE_SMOOTHED);
            const double Ppb[3] = { lane_bcast(Pm[0], r), lane_bcast(Pm[1], r), lane_bcast(Pm[2], r) };
            const double Pfb[3] = { lane_bcast(Pf[0], r), lane_bcast(Pf[1], r), lane_bcast(Pf[2], r) };
            if (lane >= sg.start_lane && lane < r) {                     // rows of this chunk (start_lane -1: from lane 0)
                fl = mark;
                if (!sg.sharp) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) Po[c] = cov_smooth(Pf[c], Ppb[c], Pfb[c]);
                }
            }
            if (sg.start_lane < 0) {                                     // rows of earlier chunks: each lane revisits rows it stored itself
                for (int64_t k0 = (sg.first / 64) * 64; k0 < c0; k0 += 64) {
                    const int64_t k = k0 + lane;
                    if (k >= sg.first) {
                        if (flb) flb[k] = (uint8_t)mark;
                        if (!sg.sharp) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) cob[k * 7 + c] = cov_smooth(cob[k * 7 + c], Ppb[c], Pfb[c]);
                        }
                    }
                }
            }
        }

        // ---- this chunk's rows: [P][7] rows of 56 B, contiguous across lanes
        if (active) {
            if (cfb) {
                cfb[i * 7] = Pf[0]; cfb[i * 7 + 1] = Pf[1]; cfb[i * 7 + 2] = Pf[2];
                cfb[i * 7 + 3] = Pq[0]; cfb[i * 7 + 4] = Pq[1]; cfb[i * 7 + 5] = Pq[2]; cfb[i * 7 + 6] = Pq[3];
            }
            cob[i * 7] = Po[0]; cob[i * 7 + 1] = Po[1]; cob[i * 7 + 2] = Po[2];
            cob[i * 7 + 3] = Pq[0]; cob[i * 7 + 4] = Pq[1]; cob[i * 7 + 5] = Pq[2]; cob[i * 7 + 6] = Pq[3];
            if (flb) flb[i] = (uint8_t)fl;
        }

        // ---- carry to the next 64 poses (from the last active lane L)
        oc = outage_carry(oc, av_m, om.start, f_mask, L, c0);
        cP[0] = lane_bcast(Pf[0], L); cP[1] = lane_bcast(Pf[1], L); cP[2] = lane_bcast(Pf[2], L);
        c_t = lane_bcast(t, L); c_sum = lane_bcast(S, L);
    }
    if (lane == 0 && a.status) a.status[b] = status | (oc.prev_avail ? 0 : ST_ENDED_IN_OUTAGE);
}

}  // namespace

extern "C" int gsf_ekf_cov_ragged_dev(gsf_ctx* ctx, const double* ts, const double* quat, const double* gps, const uint8_t* valid,
                                      const int64_t* offsets, const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B,
                                      double* cov_filt, double* cov_out, uint8_t* pose_flags, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && quat && gps && valid && cov_out, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff, "B too large for one launch");
    GSF_HIP(hipSetDevice(ctx->device));
    const EkfConfig k = to_core(cfg);
    const CovArgs a{ ts, quat, gps, valid, offsets, run_status, cov_filt, cov_out, pose_flags, status };
    hipLaunchKernelGGL(ekf_cov_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, k);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}
