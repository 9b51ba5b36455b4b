// gsf_smooth.hip -- whole-track RTS smoothing: the fixed-interval smoother over the fused track (gsf_ekf_smooth_ragged_dev).
//
// One wave per track, 64 poses per chunk, lane = pose, two passes over the track; no LDS, no workspace, hence no length limit.
// PASS 1, ascending, is the chunk body of the noise sweep (gsf_noise_sweep.hip) for ONE candidate -- cfg's own noise: the rows, dt, the
// "fix used" flags, the outage structure and the sharp-turn decision (gsf_cov_core.hpp), the orientation telescoped or scanned as the pose
// kernels form it, variance_chunk() and three affine prefix scans relative to init_pos -- plus the filter's quaternion.  It stores the
// filtered track (pos_out, quat_out, the optional pos_filt / cov_filt), the flags, and PARKS in the track's own cov_out row what the
// backward pass needs of the filter: { Pf[0..2], g[0..2], sum of dt } with two tag bits in sign bits (gsf_smooth_core.hpp) -- 56 B.
// PASS 2, descending over the same chunk boundaries, re-reads the parked row, the stamp and the filtered position, forms A from Pf[k], Q
// and dt[k+1], and runs the e scans and the d scans of include/gsf.h as SUFFIX scans with the carried (e, d, g, Pf, t) of the chunk above.
// row_bcast:15 / :31 have no downward twin, so the operands are reversed across the wave (scan lane j = row c0 + 63 - j), the prefix
// stages of GSF_SCAN_STAGES run as they are, and the results are reversed back.  It overwrites the parked row with the final diagonal
// (Pf + d, and P0 + Q sum(dt) on the quaternion axes, as ekf_cov_kernel forms it) and rewrites the position only where a later fix of
// the row's own span reaches it; every other row keeps the filter's bytes.  Everything is in correction coordinates: nothing of UTM
// size enters a scan of pass 2, and pass 1 scans positions relative to init_pos.
// The reversal is ds_bpermute (__shfl(v, 63 - lane)), so every lane re-reads only rows it stored itself (program order, no fence between the
// passes).  Measured against row_mirror + v_permlane32_swap + v_permlane16_swap and against loading the rows mirrored behind a device-scope
// fence: DESIGN.md 7k.
#include "gsf_wave_common.hpp"
#include "gsf_cov_core.hpp"
#include "gsf_sweep_core.hpp"
#include "gsf_smooth_core.hpp"

namespace {

struct SmoothArgs {
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid;
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* init_quat;
    double* pos_out; double* quat_out; double* cov_out; double* pos_filt; double* cov_filt; uint8_t* flags; int32_t* status;
};

// value of lane 63 - lane, and a lane mask in the same order
__device__ __forceinline__ double lane_rev(const double v, const int lane) { return __shfl(v, 63 - lane, 64); }
__device__ __forceinline__ u64 mask_rev(const u64 m) { return __brevll(m); }

// variance of quaternion axis c after a total dt of S: the axes never see an update (ekf_cov_kernel forms it the same way)
__device__ __forceinline__ double quat_axis_var(const EkfConfig& cfg, const int c, const double S) { return cfg.P0[3 + c] + cfg.Qps[3 + c] * S; }

__global__ __launch_bounds__(64) void ekf_smooth_kernel(const SmoothArgs a, const EkfConfig cfg)
{
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    if (N <= 0) {                                                         // an empty track (ref :835): no rows
        if (lane == 0 && a.status) a.status[b] = 0;
        return;
    }
    double* pob = a.pos_out + base * 3;
    double* qob = a.quat_out + base * 4;
    double* cob = a.cov_out + base * 7;
    double* pfb = a.pos_filt ? a.pos_filt + base * 3 : nullptr;
    double* cfb = a.cov_filt ? a.cov_filt + base * 7 : nullptr;
    uint8_t* flb = a.flags ? a.flags + base : nullptr;
    if (a.run_status && a.run_status[b] != 0) {                           // the run stopped before the filter: NaN rows, no flags, inputs not read
        const double nan = __builtin_nan("");
        for (int64_t k = lane; k < N * 7; k += 64) { cob[k] = nan; if (cfb) cfb[k] = nan; }
        for (int64_t k = lane; k < N * 4; k += 64) qob[k] = nan;
        for (int64_t k = lane; k < N * 3; k += 64) { pob[k] = nan; if (pfb) pfb[k] = nan; }
        if (flb) for (int64_t k = lane; k < N; k += 64) flb[k] = 0;
        if (lane == 0 && a.status) a.status[b] = 0;
        return;
    }
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;
    ChunkIn nxt = load_chunk(tsb, posb, quatb, gpsb, valb, lane, N);

    int same1 = -1, same2 = -1;                                           // axes with identical (P0, Q, R) share their variance scan and their d scan
    if (cfg.P0[1] == cfg.P0[0] && cfg.Qps[1] == cfg.Qps[0] && cfg.Rm[1] == cfg.Rm[0]) same1 = 0;
    if (cfg.P0[2] == cfg.P0[0] && cfg.Qps[2] == cfg.Qps[0] && cfg.Rm[2] == cfg.Rm[0]) same2 = 0;
    else if (cfg.P0[2] == cfg.P0[1] && cfg.Qps[2] == cfg.Qps[1] && cfg.Rm[2] == cfg.Rm[1]) same2 = 1;

    int32_t status = 0;
    // ================================================================================================ pass 1: the filter, ascending
    {
        // carried from chunk to chunk (wave-uniform)
        double cP[3] = { cfg.P0[0], cfg.P0[1], cfg.P0[2] };               // Pf of the last pose (pose 0: P0) ...
        double cx[3] = { 0.0, 0.0, 0.0 };                                 // ... and its position relative to init_pos
        double c_sum = 0.0;                                               // the sum of dt so far
        const Vec3 p0{ a.init_pos[b * 3], a.init_pos[b * 3 + 1], a.init_pos[b * 3 + 2] };
        Quat cq = ekf_normalize(Quat{ a.init_quat[b * 4], a.init_quat[b * 4 + 1], a.init_quat[b * 4 + 2], a.init_quat[b * 4 + 3] });   // ref :842, :683
        const Quat cq0 = cq;
        chunk_arrived(nxt);
        Vec3 c_po = lane_bcast(nxt.p, 0);                                 // "previous original pose" of pose 0 is pose 0 itself (ref :858)
        Quat c_r; bool c_ok = quat_unit(lane_bcast(nxt.q, 0), c_r);
        double c_t = lane_bcast(nxt.t, 0);
        Quat Cq = lane_bcast(quat_mul(cq, quat_conj(c_r)), 0);           // q_i = Cq r_i while every quaternion is valid (see wave_serial_chunks)
        bool cq_fresh = true;
        OutageCarry oc{ true, 0, false };
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
            const double dt = fmax(1e-6, t - t_pr);                      // ref :865
            const bool vraw = in.v != 0;
            const bool avail = stepping && vraw && !(isnan(z.x) || isnan(z.y) || isnan(z.z));   // ref :867-869
            // ---- outage structure and the sharp-turn decision: gsf_ekf_cov_ragged_dev's (gsf_cov_core.hpp)
            const u64 av_m = __ballot(i == 0 ? vraw : avail) & act_m;     // pose 0: the raw mask byte (:848)
            const OutageMasks om = outage_masks(act_m, av_m, c0 == 0, oc.prev_avail);
            status |= (om.start != 0ull) ? ST_HAD_OUTAGE : 0;
            const bool in_outage = ((act_m & ~av_m) >> lane) & 1ull;
            const Quat r_pr = prev_lane(c_r, r);
            u64 f_mask = 0ull;
            if (om.pair != 0ull) {
                const bool outpair = (om.pair >> lane) & 1ull;
                bool f = false;
                if (outpair && t > t_pr) f = !both_ok || yaw_rate_exceeds_body(r_pr, r, t - t_pr, cfg.yaw_thr_rad);   // :817, :821-824
                f_mask = __ballot(f);
            }
            int fl = avail ? POSE_GNSS_USED : (in_outage ? POSE_IN_OUTAGE : 0);
            u64 sharp_m = 0ull;
            for (u64 rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
                const int rl = __builtin_ctzll(rm);
                const OutageSeg sg = outage_closed_at(om.start, f_mask, rl, c0, oc.ostart, oc.seg_sharp, cfg.yaw_thr_rad < 0.0);
                if (sg.sharp) {                                           // a span ends in front of this recovery; the outage's rows are marked
                    sharp_m |= 1ull << rl;
                    status |= ST_SHARP_TURN;
                    if (lane >= sg.start_lane && lane < rl) fl |= POSE_SHARP_TURN;   // rows of this chunk (start_lane -1: from lane 0)
                    if (sg.start_lane < 0 && flb) {                       // rows of earlier chunks: each lane revisits rows it stored itself
                        for (int64_t k0 = (sg.first / 64) * 64; k0 < c0; k0 += 64) {
                            const int64_t k = k0 + lane;
                            if (k >= sg.first) flb[k] = (uint8_t)(flb[k] | POSE_SHARP_TURN);
                        }
                    }
                }
            }
            const bool sharp_here = (sharp_m >> lane) & 1ull;
            const bool span_start = active && (i == 0 || sharp_here);
            fl |= span_start ? POSE_SPAN_START : 0;
            const double wgt = sharp_here ? wgt_sharp : 1.0;             // the one-step blend at a sharp-turn recovery, else a hard update

            // ---- the filter's quaternion (ref :708-709) and the predicted displacement d[i] (ref :707), as the pose kernels form them:
            // one product / rotation by the wave-uniform Cq while every quaternion is valid, else calculate_relative_pose per pose and a
            // prefix product of the increments
            const Vec3 dp{ p.x - p_pr.x, p.y - p_pr.y, p.z - p_pr.z };
            Vec3 u; Quat qi;
            const bool telescope = c_ok && ((ok_mask & act_m) == act_m);
            if (telescope) {
                qi = quat_mul(Cq, r);
                const bool is_init = i == 0;                              // pose 0 keeps the initial state (ref :842)
                qi.x = is_init ? cq0.x : qi.x; qi.y = is_init ? cq0.y : qi.y; qi.z = is_init ? cq0.z : qi.z; qi.w = is_init ? cq0.w : qi.w;
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
                if (__ballot(stepping && !both_ok) != 0ull) status |= ST_BAD_QUAT;
                Quat D = dq;
                const Quat QID{ 0.0, 0.0, 0.0, 1.0 };
#define GSF_QSTAGE(CTRL, RM) { const Quat o = dpp<CTRL, RM>(QID, D); D = quat_mul(o, D); }
                GSF_SCAN_STAGES(GSF_QSTAGE)
#undef GSF_QSTAGE
                qi = ekf_normalize(quat_mul(cq, D));
                const Quat q_prev = prev_lane(cq, qi);
                u = quat_rotate(q_prev, dpl);
                cq = lane_bcast(qi, L);
                if (((ok_mask >> L) & 1ull) != 0ull) Cq = lane_bcast(quat_mul(cq, quat_conj(lane_bcast(r, L))), 0);
            }
            const double d[3] = { u.x, u.y, u.z };
            const double zr[3] = { z.x - p0.x, z.y - p0.y, z.z - p0.z };   // relative to init_pos: y is a difference of two UTM northings

            // ---- variances (the pose kernels' scans), positions (three affine scans), the applied correction g = xf - xp
            AxisVar v0, v1, v2;
            variance_chunk<6>(cfg, same1, same2, dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
            const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, kg[3] = { v0.kg, v1.kg, v2.kg };
            double x[3], g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double kw = kg[c] * wgt;
                Affine m = sweep_affine(avail, kw, d[c], zr[c]);
#define GSF_ASTAGE(CTRL, RM) { const Affine o{ dpp<CTRL, RM>(1.0, m.a), dpp0<CTRL, RM>(m.b) }; m = affine_compose(m, o); }
                GSF_SCAN_STAGES(GSF_ASTAGE)
#undef GSF_ASTAGE
                x[c] = affine_apply(m, cx[c]);                            // xf[i] - init_pos
                const double pm = prev_lane(cx[c], x[c]) + d[c];          // xp[i] - init_pos (ref :707)
                const double gc = kw * (zr[c] - pm);                      // ref :722-728 and the blend of :752-768
                g[c] = avail ? gc : 0.0;
            }
            double dsum = stepping ? dt : 0.0;                            // the quaternion axes: one prefix sum of dt (ekf_cov_kernel's)
#define GSF_SSTAGE(CTRL, RM) { dsum += dpp0<CTRL, RM>(dsum); }
            GSF_SCAN_STAGES(GSF_SSTAGE)
#undef GSF_SSTAGE
            const double S = c_sum + dsum;

            // ---- carry to the next 64 poses (from the last active lane L)
            oc = outage_carry(oc, av_m, om.start, f_mask, L, c0);
#pragma unroll
            for (int c = 0; c < 3; ++c) { cP[c] = lane_bcast(Pf[c], L); cx[c] = lane_bcast(x[c], L); }
            c_sum = lane_bcast(S, L);
            c_po = lane_bcast(p, L); c_r = lane_bcast(r, L); c_ok = ((ok_mask >> L) & 1ull) != 0ull; c_t = lane_bcast(t, L);

            // ---- this chunk's rows.  pos_out, the parked cov_out row and the flags are read again by pass 2: plain stores
            chunk_arrived(nxt);
            if (active) {
                const double xf[3] = { p0.x + x[0], p0.y + x[1], p0.z + x[2] };
                pob[i * 3] = xf[0]; pob[i * 3 + 1] = xf[1]; pob[i * 3 + 2] = xf[2];
                __builtin_nontemporal_store(qi.x, &qob[i * 4]); __builtin_nontemporal_store(qi.y, &qob[i * 4 + 1]);
                __builtin_nontemporal_store(qi.z, &qob[i * 4 + 2]); __builtin_nontemporal_store(qi.w, &qob[i * 4 + 3]);
                cob[i * 7] = smooth_tag(Pf[0], avail); cob[i * 7 + 1] = Pf[1]; cob[i * 7 + 2] = Pf[2];
                cob[i * 7 + 3] = g[0]; cob[i * 7 + 4] = g[1]; cob[i * 7 + 5] = g[2];
                cob[i * 7 + 6] = smooth_tag(S, span_start);
                if (pfb) { __builtin_nontemporal_store(xf[0], &pfb[i * 3]); __builtin_nontemporal_store(xf[1], &pfb[i * 3 + 1]); __builtin_nontemporal_store(xf[2], &pfb[i * 3 + 2]); }
                if (cfb) {
                    __builtin_nontemporal_store(Pf[0], &cfb[i * 7]); __builtin_nontemporal_store(Pf[1], &cfb[i * 7 + 1]); __builtin_nontemporal_store(Pf[2], &cfb[i * 7 + 2]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) __builtin_nontemporal_store(quat_axis_var(cfg, c, S), &cfb[i * 7 + 3 + c]);
                }
                if (flb) flb[i] = (uint8_t)fl;
            }
        }
        status |= oc.prev_avail ? 0 : ST_ENDED_IN_OUTAGE;
    }

    // ================================================================================================ pass 2: the smoother, descending
    {
        // carried from the chunk above (wave-uniform): its first row's e, d (0 where no fix reaches it), g, Pf, stamp and tag bits.  Above
        // the last row there is nothing: a span start, which cuts the link whatever the other values are.
        double c_e[3] = { 0.0, 0.0, 0.0 }, c_d[3] = { 0.0, 0.0, 0.0 }, c_g[3] = { 0.0, 0.0, 0.0 }, c_Pf[3] = { 0.0, 0.0, 0.0 };
        double c_t = 0.0;
        bool c_fix = false, c_start = true, c_reach = false, any_reached = false;
        for (int64_t c0 = ((N - 1) >> 6) << 6; c0 >= 0; c0 -= 64) {
            const int64_t kr = c0 + 63 - lane;                            // the row of this SCAN lane
            const int64_t io = c0 + lane;                                  // the row this lane loads and stores: one it stored itself in pass 1
            const bool act_io = io < N;
            const int64_t il = act_io ? io : N - 1;
            double w[7], xf[3];
#pragma unroll
            for (int c = 0; c < 7; ++c) w[c] = cob[il * 7 + c];
#pragma unroll
            for (int c = 0; c < 3; ++c) xf[c] = pob[il * 3 + c];
            const double t_io = tsb[il];
            uint32_t fl_io = 0u;
            if (flb) fl_io = flb[il];
            const double S = smooth_untag(w[6]);
            const double Pf_io[3] = { smooth_untag(w[0]), w[1], w[2] };
            // ---- into scan order: scan lane j holds row c0 + 63 - j, so the row after is the lane before
            const u64 fix_m = mask_rev(__ballot(act_io && smooth_tag_of(w[0]))), start_m = mask_rev(__ballot(act_io && smooth_tag_of(w[6])));
            const double t = lane_rev(t_io, lane);
            double Pf[3], g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { Pf[c] = lane_rev(act_io ? Pf_io[c] : 0.0, lane); g[c] = lane_rev(act_io ? w[3 + c] : 0.0, lane); }
            const bool act = kr < N;
            const u64 fixn_m = (fix_m << 1) | (c_fix ? 1ull : 0ull), startn_m = (start_m << 1) | (c_start ? 1ull : 0ull);   // of the row after
            const bool fix_n = (fixn_m >> lane) & 1ull, start_n = (startn_m >> lane) & 1ull;
            const bool linked = act && kr != N - 1 && !start_n;           // A = 0 on a span's last pose
            const double t_n = prev_lane(c_t, t);
            const double dt_n = fmax(1e-6, t_n - t);                      // the forward pass's dt[k+1] (:865)
            // six independent scans (three where the axes share their noise): what a lone wave per SIMD wants
            double e[3], dd[3];
            Affine md[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double Pf_n = prev_lane(c_Pf[c], Pf[c]), g_n = prev_lane(c_g[c], g[c]);
                const double Pp_n = smooth_pred(Pf[c], cfg.Qps[c], dt_n);
                const double A = smooth_gain(Pf[c], Pp_n, linked);
                Affine m = smooth_map_e(A, g_n);
                md[c] = smooth_map_d(A, Pf_n, Pp_n, fix_n);
#define GSF_ASTAGE(CTRL, RM) { const Affine o{ dpp<CTRL, RM>(1.0, m.a), dpp0<CTRL, RM>(m.b) }; m = affine_compose(m, o); }
                GSF_SCAN_STAGES(GSF_ASTAGE)
                e[c] = affine_apply(m, c_e[c]);
            }
            // (scalar arguments and constant indices only; axes with equal (P0, Q, R) run the same recursion on the same values)
            auto dscan = [&](Affine m, const double carry) __attribute__((always_inline)) {
                GSF_SCAN_STAGES(GSF_ASTAGE)
                return affine_apply(m, carry);
            };
#undef GSF_ASTAGE
            dd[0] = dscan(md[0], c_d[0]);
            if (same1 == 0) dd[1] = dd[0]; else dd[1] = dscan(md[1], c_d[1]);
            if (same2 == 0) dd[2] = dd[0]; else if (same2 == 1) dd[2] = dd[1]; else dd[2] = dscan(md[2], c_d[2]);
            // ---- the rows a later fix of their own span reaches (GSF_POSE_SMOOTHED): the others keep the filter's bytes
            const bool reached = act && smooth_row_reached(fix_m, start_m, lane, c_reach);
            const u64 reach_m = __ballot(reached);
            any_reached = any_reached || reach_m != 0ull;
            // ---- carry to the chunk below (from scan lane 63, the chunk's first row)
            c_reach = smooth_reach_carry(fix_m, start_m, (reach_m >> 63) != 0ull);
            c_fix = (fix_m >> 63) != 0ull; c_start = (start_m >> 63) != 0ull;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[c] = reached ? e[c] : 0.0; dd[c] = reached ? dd[c] : 0.0;
                c_e[c] = lane_bcast(e[c], 63); c_d[c] = lane_bcast(dd[c], 63); c_g[c] = lane_bcast(g[c], 63); c_Pf[c] = lane_bcast(Pf[c], 63);
            }
            c_t = lane_bcast(t, 63);
            // ---- back into row order, and out: the final diagonal over the parked row, the position where it moved
            const bool reached_io = (mask_rev(reach_m) >> lane) & 1ull;
            double e_io[3], d_io[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) e_io[c] = lane_rev(e[c], lane);
            d_io[0] = lane_rev(dd[0], lane);
            if (same1 == 0) d_io[1] = d_io[0]; else d_io[1] = lane_rev(dd[1], lane);
            if (same2 == 0) d_io[2] = d_io[0]; else if (same2 == 1) d_io[2] = d_io[1]; else d_io[2] = lane_rev(dd[2], lane);
            if (act_io) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double Ps = Pf_io[c] + d_io[c];
                    cob[io * 7 + c] = reached_io ? Ps : Pf_io[c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) cob[io * 7 + 3 + c] = quat_axis_var(cfg, c, S);
                if (reached_io) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) pob[io * 3 + c] = xf[c] + e_io[c];
                    if (flb) flb[io] = (uint8_t)(fl_io | POSE_SMOOTHED);
                }
            }
        }
        if (lane == 0 && a.status) a.status[b] = status | (any_reached ? ST_RTS_APPLIED : 0);
    }
}

}  // namespace

extern "C" int gsf_ekf_smooth_ragged_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps,
                                         const uint8_t* valid, const int64_t* offsets, const double* init_pos, const double* init_quat,
                                         const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, double* pos_out, double* quat_out,
                                         double* cov_out, double* pos_filt, double* cov_filt, uint8_t* pose_flags, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && init_pos && init_quat && pos_out && quat_out && cov_out, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff, "B too large for one launch");
    GSF_HIP(hipSetDevice(ctx->device));
    const EkfConfig k = to_core(cfg);
    const SmoothArgs a{ ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, pos_out, quat_out, cov_out, pos_filt, cov_filt, pose_flags, status };
    hipLaunchKernelGGL(ekf_smooth_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, k);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}
