// gsf_weighted.hip -- per-fix GNSS noise: the whole-track filter and RTS smoother with a measurement variance per pose and axis
// (gsf_ekf_smooth_weighted_dev), and the kernel that carries per-fix variances onto SLAM stamps (gsf_fix_var_at_poses_dev).
//
// ekf_smooth_weighted_kernel has the structure of ekf_smooth_kernel (gsf_smooth.hip) and is built from the same pieces: one wave per track,
// 64 poses per chunk, lane = pose, two passes, no LDS, no workspace, any track length.  What differs:
//  * PASS 1 loads the row's three variances beside the chunk's rows.  avail[i] is the smoother's AND three usable variances
//    (gsf_weighted_core.hpp); a row that fails on its variances alone drops out of av_m like a cleared mask byte, so the outage structure,
//    the sharp-turn decision, the flags, the spans and the reach of pass 2 see a pose without a fix, and it carries POSE_BAD_SIGMA.
//  * the variance scan takes r as a per-lane value and renormalises the composed map twice (variance_scan_w below: the range argument);
//    the gain, the Joseph Pf and g use the row's own r through variance_finish() and sweep_affine() as they stand.
//  * no axis shares a scan with another: three variance scans and three d scans per chunk, whatever cfg holds (measured: DESIGN.md 7n).
//  * nis[i] = sum_c y_c^2 / (Pp_c + r_ic) on the rows that took an update, NaN elsewhere.
// PASS 2 reads only what pass 1 parked (Pf, g, sum of dt, two tag bits), Q and the stamps: R never enters it, so it is the smoother's
// backward pass line for line, without the shared d scans.
#include "gsf_wave_common.hpp"
#include "gsf_cov_core.hpp"
#include "gsf_sweep_core.hpp"
#include "gsf_smooth_core.hpp"
#include "gsf_weighted_core.hpp"

namespace {

struct WeightedArgs {
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid; const double* meas_var;
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* init_quat;
    double* pos_out; double* quat_out; double* cov_out; double* pos_filt; double* cov_filt; uint8_t* flags; int32_t* status; double* nis;
};

// value of lane 63 - lane, and a lane mask in the same order
__device__ __forceinline__ double lane_rev(const double v, const int lane) { return __shfl(v, 63 - lane, 64); }
__device__ __forceinline__ u64 mask_rev(const u64 m) { return __brevll(m); }

// variance of quaternion axis c after a total dt of S: the axes never see an update (ekf_cov_kernel forms it the same way)
__device__ __forceinline__ double quat_axis_var(const EkfConfig& cfg, const int c, const double S) { return cfg.P0[3 + c] + cfg.Qps[3 + c] * S; }

// variance_scan() of gsf_wave_common.hpp with r of the lane's own row, and the composed map rescaled on the way.
// RANGE.  Applied to P = 0 the denominator of the composed map of a run of used fixes is the product of S_i / D_i over the scaled D_i (S_i =
// P_{i-1} + q dt_i + r_i the innovation variance, D_i = q dt_i + r_i scaled into [1, 2)): every factor is (1 + P_{i-1} / D_i) times a value
// in [1, 2).  What keeps a factor small is P_{i-1} <= D_i.  With steps of one length it holds whatever the r_i are: P_{i-1} <=
// min(r_{i-1}, P_{i-2} + q dt), so rows alternating between 1e8 and 1e-8 under an even dt give factors below 4 (the unrescaled product of
// a chunk stays below 1e21 there).  It fails when the variance a row inherits is large against its OWN step and r: a long step (P climbs
// by q dt, up to 1e14) followed by a short one with a fix.  With one r that needs rows WITHOUT a fix on the long steps -- with a fix on
// every row P < r <= D bounds every factor by 4, the argument above variance_scan -- and variance_scan leaves the doubles there as well
// (an outage pose per long step, r = 1e-8, 32 times a chunk).  With r_i per row it happens with a fix on every row: r = 1e8 on the long
// steps lets P reach 1e8, r = 1e-8 on a step of q dt = 1e-7 behind it gives a factor of 1e15, and a chunk holds 32 such pairs (1e480;
// tests/weighted_ref.long_short_track).  So the step scaling stays as it is, and the COMPOSED map of every lane is scaled again by the power
// of two that brings its own D into [1, 2), after the third stage (maps of up to 8 poses: at most 4 such pairs of at most (1e8 + 1e14) /
// 1e-8 = 1e22, entries below 1e92 times 2^8) and after the fifth.  A Moebius map is unchanged by a common factor, per lane.  Relative to
// its D a composed map has B / D = the variance it gives P = 0 (at most 64 (1e8 + 1e14)), C / D <= the sum of 1 / r_i over its fixes (the
// information they can add: at most 64e8), A / D <= 1 + (B / D)(C / D) (the derivative of a posterior by its prior is at most 1): every
// entry is at most 1e26 after a rescale, 1e52 and 1e104 after the next two stages, and moebius_apply() multiplies by P <= 1e8 + 64e14.
// D >= 1 throughout (a product of scaled D_i plus non-negative terms), so the rescale never sees zero or a subnormal.  Entries that shrink
// (A: a chain of r_i / D_i) only underflow towards 0, as with one r.  Powers of two commute with every rounding here, so wherever the
// unrescaled product stays in range -- with meas_var equal to cfg's R on every row included -- the variances are variance_scan()'s BIT FOR
// BIT.  Stated range (include/gsf.h): P0 and Q dt as gsf_ekf_config states them, 1e-8 <= r_i <= 1e8 for every row, no bound on the ratio
// of two rows and none on the ratio of two steps.
__device__ __forceinline__ Moebius variance_scan_w(const double q, const double rr, const double dt, const bool stepping, const bool avail)
{
    const double b0 = q * dt;
    double A = 1.0, Bm = stepping ? b0 : 0.0, Cm = 0.0, Dm = 1.0;
    if (avail) { const double d = b0 + rr, sc = pow2_rcp_below(d); A = rr * sc; Bm = (rr * b0) * sc; Cm = sc; Dm = d * sc; }
    // mine (later) o other (earlier); lanes without a source see the identity map (1,0;0,1)
#define GSF_MSTAGE(CTRL, RM) {                                                                                              \
        const double oA = dpp<CTRL, RM>(1.0, A), oB = dpp0<CTRL, RM>(Bm), oC = dpp0<CTRL, RM>(Cm), oD = dpp<CTRL, RM>(1.0, Dm); \
        const double nA = A * oA + Bm * oC, nB = A * oB + Bm * oD, nC = Cm * oA + Dm * oC, nD = Cm * oB + Dm * oD;                  \
        A = nA; Bm = nB; Cm = nC; Dm = nD; }
#define GSF_MRESCALE { const double sc = pow2_rcp_below(Dm); A *= sc; Bm *= sc; Cm *= sc; Dm *= sc; }
    GSF_MSTAGE(DPP_ROW_SHR1, 0xf) GSF_MSTAGE(DPP_ROW_SHR2, 0xf) GSF_MSTAGE(DPP_ROW_SHR4, 0xf)
    GSF_MRESCALE
    GSF_MSTAGE(DPP_ROW_SHR8, 0xf) GSF_MSTAGE(DPP_ROW_BCAST15, 0xa)
    GSF_MRESCALE
    GSF_MSTAGE(DPP_ROW_BCAST31, 0xc)
#undef GSF_MRESCALE
#undef GSF_MSTAGE
    return Moebius{ A, Bm, Cm, Dm };
}
// (scalar arguments only, as variance_axis())
__device__ __forceinline__ AxisVar variance_axis_w(const double q, const double rr, const double dt, const bool stepping, const bool avail, const double cPc)
{
    return variance_finish(variance_scan_w(q, rr, dt, stepping, avail), q, rr, dt, cPc);
}

__global__ __launch_bounds__(64) void ekf_smooth_weighted_kernel(const WeightedArgs a, const EkfConfig cfg)
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
    double* nib = a.nis ? a.nis + base : nullptr;
    if (a.run_status && a.run_status[b] != 0) {                           // the run stopped before the filter: NaN rows, no flags, inputs not read
        const double nan = __builtin_nan("");
        for (int64_t k = lane; k < N * 7; k += 64) { cob[k] = nan; if (cfb) cfb[k] = nan; }
        for (int64_t k = lane; k < N * 4; k += 64) qob[k] = nan;
        for (int64_t k = lane; k < N * 3; k += 64) { pob[k] = nan; if (pfb) pfb[k] = nan; }
        for (int64_t k = lane; k < N; k += 64) { if (flb) flb[k] = 0; if (nib) nib[k] = nan; }
        if (lane == 0 && a.status) a.status[b] = 0;
        return;
    }
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;
    const double* __restrict__ mvb = a.meas_var + base * 3;
    ChunkIn nxt = load_chunk(tsb, posb, quatb, gpsb, valb, lane, N);
    // the row's variances, clamped like the chunk's rows
#define GSF_LOAD_VAR(dst, row) { const int64_t il_ = (row) < N ? (row) : N - 1;                                                   \
        dst[0] = __builtin_nontemporal_load(&mvb[il_ * 3]); dst[1] = __builtin_nontemporal_load(&mvb[il_ * 3 + 1]);               \
        dst[2] = __builtin_nontemporal_load(&mvb[il_ * 3 + 2]); }
    double mv_nxt[3];
    GSF_LOAD_VAR(mv_nxt, (int64_t)lane)

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
            const double mv[3] = { mv_nxt[0], mv_nxt[1], mv_nxt[2] };
            nxt = load_chunk(tsb, posb, quatb, gpsb, valb, c0 + 64 + lane, N);   // the next chunk's rows are requested before this chunk's scans (clamped past the end)
            GSF_LOAD_VAR(mv_nxt, c0 + 64 + lane)
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
            const bool base_avail = stepping && vraw && !(isnan(z.x) || isnan(z.y) || isnan(z.z));   // ref :867-869
            const WeightedAvail wa = weighted_avail(base_avail, mv[0], mv[1], mv[2]);   // ... and three usable variances
            const bool avail = wa.avail;
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
            fl |= wa.bad ? POSE_BAD_SIGMA : 0;
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

            // ---- the filter's quaternion (ref :708-709) and the predicted displacement d[i] (ref :707), as the pose kernels form them
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

            // ---- variances (one scan per axis, r of the row's own), positions (three affine scans), the applied correction g = xf - xp
            // a row that takes no update carries r = 1: nothing of what its meas_var holds reaches an operand
            const double rr0 = avail ? mv[0] : 1.0, rr1 = avail ? mv[1] : 1.0, rr2 = avail ? mv[2] : 1.0;
            const AxisVar v0 = variance_axis_w(cfg.Qps[0], rr0, dt, stepping, avail, cP[0]);
            const AxisVar v1 = variance_axis_w(cfg.Qps[1], rr1, dt, stepping, avail, cP[1]);
            const AxisVar v2 = variance_axis_w(cfg.Qps[2], rr2, dt, stepping, avail, cP[2]);
            const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, kg[3] = { v0.kg, v1.kg, v2.kg }, Pm[3] = { v0.Pm, v1.Pm, v2.Pm }, rr[3] = { rr0, rr1, rr2 };
            double x[3], g[3], nis = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double kw = kg[c] * wgt;
                Affine m = sweep_affine(avail, kw, d[c], zr[c]);
#define GSF_ASTAGE(CTRL, RM) { const Affine o{ dpp<CTRL, RM>(1.0, m.a), dpp0<CTRL, RM>(m.b) }; m = affine_compose(m, o); }
                GSF_SCAN_STAGES(GSF_ASTAGE)
#undef GSF_ASTAGE
                x[c] = affine_apply(m, cx[c]);                            // xf[i] - init_pos
                const double pm = prev_lane(cx[c], x[c]) + d[c];          // xp[i] - init_pos (ref :707)
                const double y = zr[c] - pm;                              // the innovation, before any blend
                const double gc = kw * y;                                 // ref :722-728 and the blend of :752-768
                g[c] = avail ? gc : 0.0;
                nis = nis + weighted_nis_term(y, Pm[c], rr[c]);
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
            asm volatile("" :: "v"(mv_nxt[0]), "v"(mv_nxt[1]), "v"(mv_nxt[2]) : "memory");
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
                if (nib) __builtin_nontemporal_store(avail ? nis : __builtin_nan(""), &nib[i]);
                if (flb) flb[i] = (uint8_t)fl;
            }
        }
        status |= oc.prev_avail ? 0 : ST_ENDED_IN_OUTAGE;
    }
#undef GSF_LOAD_VAR

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
            // six independent scans: what a lone wave per SIMD wants
            double e[3], dd[3];
#define GSF_ASTAGE(CTRL, RM) { const Affine o{ dpp<CTRL, RM>(1.0, m.a), dpp0<CTRL, RM>(m.b) }; m = affine_compose(m, o); }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double Pf_n = prev_lane(c_Pf[c], Pf[c]), g_n = prev_lane(c_g[c], g[c]);
                const double Pp_n = smooth_pred(Pf[c], cfg.Qps[c], dt_n);
                const double A = smooth_gain(Pf[c], Pp_n, linked);
                {
                    Affine m = smooth_map_e(A, g_n);
                    GSF_SCAN_STAGES(GSF_ASTAGE)
                    e[c] = affine_apply(m, c_e[c]);
                }
                {
                    Affine m = smooth_map_d(A, Pf_n, Pp_n, fix_n);
                    GSF_SCAN_STAGES(GSF_ASTAGE)
                    dd[c] = affine_apply(m, c_d[c]);
                }
            }
#undef GSF_ASTAGE
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
            for (int c = 0; c < 3; ++c) { e_io[c] = lane_rev(e[c], lane); d_io[c] = lane_rev(dd[c], lane); }
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

// ---- per-fix variances onto SLAM stamps: one thread per pose
struct FixVarArgs {
    const double* ts; const int64_t* slam_offsets; const double* gps_t; const int64_t* gps_offsets; const uint8_t* gps_keep;
    const double* fix_var; const uint8_t* valid; double* pose_var; int64_t B, P;
};

__global__ __launch_bounds__(256) void fix_var_at_poses_kernel(const FixVarArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const double inf = __builtin_huge_val();
    Vec3 v{ inf, inf, inf };
    if (!a.valid || a.valid[i] != 0) {
        // the pose's track: the last b with slam_offsets[b] <= i (an empty track shares its offset with the next one and is passed over)
        int64_t b = query_count_le(a.slam_offsets, a.B + 1, i) - 1;
        b = b < 0 ? 0 : (b > a.B - 1 ? a.B - 1 : b);
        const int64_t g0 = a.gps_offsets[b], n = a.gps_offsets[b + 1] - g0;
        v = fix_var_bracket(a.gps_t + g0, a.gps_keep ? a.gps_keep + g0 : (const uint8_t*)nullptr, a.fix_var + g0 * 3, n, a.ts[i]);
    }
    a.pose_var[i * 3] = v.x; a.pose_var[i * 3 + 1] = v.y; a.pose_var[i * 3 + 2] = v.z;
}

}  // namespace

namespace gsf {

int launch_ekf_smooth_weighted(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                               const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                               const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, double* pos_out, double* quat_out, double* cov_out,
                               double* pos_filt, double* cov_filt, uint8_t* pose_flags, int32_t* status, double* nis)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const EkfConfig k = to_core(cfg);
    const WeightedArgs a{ ts, pos, quat, gps, valid, meas_var, offsets, run_status, init_pos, init_quat, pos_out, quat_out, cov_out, pos_filt,
                          cov_filt, pose_flags, status, nis };
    hipLaunchKernelGGL(ekf_smooth_weighted_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, k);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

int launch_fix_var_at_poses(gsf_ctx* ctx, const double* ts, const int64_t* slam_offsets, const double* gps_t, const int64_t* gps_offsets,
                            const uint8_t* gps_keep, const double* fix_var, const uint8_t* valid, int64_t B, int64_t P, double* pose_var)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const FixVarArgs a{ ts, slam_offsets, gps_t, gps_offsets, gps_keep, fix_var, valid, pose_var, B, P };
    hipLaunchKernelGGL(fix_var_at_poses_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, a);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace gsf
