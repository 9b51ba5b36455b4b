// gsf_smooth.hip -- whole-track RTS smoothing: the fixed-interval smoother over the fused track (gsf_ekf_smooth_ragged_dev) and the same
// smoother with a measurement variance per pose and axis (gsf_ekf_smooth_weighted_dev), and that smoother made robust by Huber / Cauchy
// reweighting rounds (gsf_ekf_smooth_reweighted_dev).  ONE kernel body, ekf_smooth_kernel<MODE>: SMOOTH_PLAIN, SMOOTH_WEIGHTED (below:
// WEIGHTED, which SMOOTH_REWEIGHTED is as well) and SMOOTH_REWEIGHTED (below: REWEIGHT).
//
// One wave per track, 64 poses per chunk, lane = pose, two passes over the track; no LDS, no workspace, hence no length limit.
// PASS 1, ascending, is the shared chunk body of gsf_track_chunk.hpp under cfg's own noise: the rows, dt, the "fix used" flags, the outage
// structure and the sharp-turn decision (gsf_cov_core.hpp), the orientation step with the filter's quaternion, variance_chunk() and three
// affine prefix scans relative to init_pos.  It stores the filtered track (pos_out, quat_out, the optional pos_filt / cov_filt), the
// flags, and PARKS in the track's own cov_out row what the backward pass needs of the filter: { Pf[0..2], g[0..2], sum of dt } with two
// tag bits in sign bits (gsf_smooth_core.hpp) -- 56 B.
// WEIGHTED changes pass 1 only:
//  * it loads the row's three variances beside the chunk's rows.  avail[i] is the smoother's AND three usable variances
//    (gsf_weighted_core.hpp); a row that fails on its variances alone drops out of av_m like a cleared mask byte, so the outage structure,
//    the sharp-turn decision, the flags, the spans and the reach of pass 2 see a pose without a fix, and it carries POSE_BAD_SIGMA.
//  * the variance scan takes r as a per-lane value and renormalises the composed map twice (variance_scan<6, true>: the range argument);
//    the gain, the Joseph Pf and g use the row's own r through variance_finish() and sweep_affine() as they stand.
//  * no axis shares a scan with another: three variance scans and three d scans per chunk, whatever cfg holds (measured: DESIGN.md 7n).
//  * nis[i] = sum_c y_c^2 / (Pp_c + r_ic) on the rows that took an update, NaN elsewhere.
// REWEIGHT opens a loop over the SOLVES around both passes (one trip in the other two modes, where it folds away): solve 0 under the
// given variances, then up to `rounds` solves under r_eff = min(v / w, 1e8) (gsf_reweight_core.hpp), stopped per track at a fixed point
// of the weights.  meas_var may be NULL there: cfg's R on every row.
//  * pass 1 of a solve loads weight[i] beside the row's variances, a chunk ahead like them, and forms r_eff for the rows that take an
//    update; availability is judged on the GIVEN variances, and r_eff of a used row is usable, so every solve sees the same outages,
//    sharp-turn decisions, spans, flags and quaternions.  Solve 0 runs on w = 1.0: v / 1.0 and the min return v's bits.
//  * pass 1 parks the RELATIVE filtered position in the track's own pos_out row; pass 2 forms init_pos + xr with pass 1's expression
//    (the bytes the weighted mode stores) and + e on the rows a later fix reaches, and rewrites every row.
//  * pass 2 also loads the row's fix and given variances and forms res = (z - init_pos) - (xr + e), u2 and the weight of the NEXT
//    solve, stores it (NaN on rows without an update), and keeps the ballot "some used weight is not the one its solve used" and the
//    largest step of a weight.  The stop is wave-uniform.
//  * row k stays on lane k mod 64 in both passes and all solves: a lane reads back only rows it stored itself, program order is enough
//    (as for the parked cov_out row).  `weight` is neither restrict nor nontemporal.  The clamped load of an idle lane may touch another
//    lane's row: `avail` (pass 1) and `used` (pass 2) end it before any operand.
// PASS 2, descending over the same chunk boundaries, re-reads the parked row, the stamp and the filtered position, forms A from Pf[k], Q
// and dt[k+1], and runs the e scans and the d scans of include/gsf.h as SUFFIX scans with the carried (e, d, g, Pf, t) of the chunk above.
// It reads only what pass 1 parked, Q and the stamps: R never enters it.
// row_bcast:15 / :31 have no downward twin, so the operands are reversed across the wave (scan lane j = row c0 + 63 - j), the prefix
// stages of GSF_SCAN_STAGES run as they are, and the results are reversed back.  It overwrites the parked row with the final diagonal
// (Pf + d, and P0 + Q sum(dt) on the quaternion axes, as ekf_cov_kernel forms it) and rewrites the position only where a later fix of
// the row's own span reaches it; every other row keeps the filter's bytes.  Everything is in correction coordinates: nothing of UTM
// size enters a scan of pass 2, and pass 1 scans positions relative to init_pos.
// The reversal is ds_bpermute (__shfl(v, 63 - lane)), so every lane re-reads only rows it stored itself (program order, no fence between the
// passes).  Measured against row_mirror + v_permlane32_swap + v_permlane16_swap and against loading the rows mirrored behind a device-scope
// fence: DESIGN.md 7k.
#include "gsf_track_chunk.hpp"
#include "gsf_smooth_core.hpp"
#include "gsf_weighted_core.hpp"
#include "gsf_reweight_core.hpp"

namespace {

enum : int { SMOOTH_PLAIN = 0, SMOOTH_WEIGHTED = 1, SMOOTH_REWEIGHTED = 2 };

struct SmoothArgs {
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid; const double* meas_var;   // (WEIGHTED)
    const int64_t* offsets; const int32_t* run_status; const double* init_pos; const double* init_quat;
    double* pos_out; double* quat_out; double* cov_out; double* pos_filt; double* cov_filt; uint8_t* flags; int32_t* status; double* nis;   // (nis: WEIGHTED)
};
// (REWEIGHT) what the round loop adds; a parameter of its own BEHIND the others, so that the kernel arguments of the two modes without
// it lie where they lay and their code is the same instruction for instruction.  meas_var may be NULL in that mode: cfg's R on every row
struct ReweightArgs { double* weight; int32_t* rounds_used; double* w_change; double c2; int32_t loss, rounds; };

// (WEIGHTED) a row's three variances, clamped like the chunk's rows
__device__ __forceinline__ void load_row_var(const double* __restrict__ mvb, const int64_t row, const int64_t N, double& v0, double& v1, double& v2)
{
    const int64_t il = row < N ? row : N - 1;
    v0 = __builtin_nontemporal_load(&mvb[il * 3]); v1 = __builtin_nontemporal_load(&mvb[il * 3 + 1]); v2 = __builtin_nontemporal_load(&mvb[il * 3 + 2]);
}

// (REWEIGHT) ... or, without an array, cfg's R: a wave-uniform choice
template <bool REWEIGHT>
__device__ __forceinline__ void row_var(const double* __restrict__ mvb, const EkfConfig& cfg, const int64_t row, const int64_t N, double& v0, double& v1, double& v2)
{
    if (REWEIGHT && !mvb) { v0 = cfg.Rm[0]; v1 = cfg.Rm[1]; v2 = cfg.Rm[2]; }
    else load_row_var(mvb, row, N, v0, v1, v2);
}

template <int MODE>
__global__ __launch_bounds__(64) void ekf_smooth_kernel(const SmoothArgs a, const EkfConfig cfg, const ReweightArgs rw)
{
    constexpr bool WEIGHTED = MODE != SMOOTH_PLAIN, REWEIGHT = MODE == SMOOTH_REWEIGHTED;
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t base = uniform64(a.offsets[b]), N = uniform64(a.offsets[b + 1]) - base;
    if (N <= 0) {                                                         // an empty track (ref :835): no rows
        if (lane == 0 && a.status) a.status[b] = 0;
        if constexpr (REWEIGHT) if (lane == 0) { if (rw.rounds_used) rw.rounds_used[b] = 0; if (rw.w_change) rw.w_change[b] = 0.0; }
        return;
    }
    double* pob = a.pos_out + base * 3;
    double* qob = a.quat_out + base * 4;
    double* cob = a.cov_out + base * 7;
    double* pfb = a.pos_filt ? a.pos_filt + base * 3 : nullptr;
    double* cfb = a.cov_filt ? a.cov_filt + base * 7 : nullptr;
    uint8_t* flb = a.flags ? a.flags + base : nullptr;
    double* nib = (WEIGHTED && a.nis) ? a.nis + base : nullptr;
    double* wtb = REWEIGHT ? rw.weight + base : nullptr;                   // neither restrict nor nontemporal: the rounds' own store, read back by the lane that wrote
    if (a.run_status && a.run_status[b] != 0) {                           // the run stopped before the filter: NaN rows, no flags, inputs not read
        const double nan = __builtin_nan("");
        for (int64_t k = lane; k < N * 7; k += 64) { cob[k] = nan; if (cfb) cfb[k] = nan; }
        for (int64_t k = lane; k < N * 4; k += 64) qob[k] = nan;
        for (int64_t k = lane; k < N * 3; k += 64) { pob[k] = nan; if (pfb) pfb[k] = nan; }
        for (int64_t k = lane; k < N; k += 64) { if (flb) flb[k] = 0; if (nib) nib[k] = nan; if constexpr (REWEIGHT) wtb[k] = nan; }
        if (lane == 0 && a.status) a.status[b] = 0;
        if constexpr (REWEIGHT) if (lane == 0) { if (rw.rounds_used) rw.rounds_used[b] = 0; if (rw.w_change) rw.w_change[b] = 0.0; }
        return;
    }
    const double* __restrict__ tsb = a.ts + base;
    const double* __restrict__ posb = a.pos + base * 3;
    const double* __restrict__ quatb = a.quat + base * 4;
    const double* __restrict__ gpsb = a.gps + base * 3;
    const uint8_t* __restrict__ valb = a.valid + base;
    const double* __restrict__ mvb = (WEIGHTED && (!REWEIGHT || a.meas_var)) ? a.meas_var + base * 3 : nullptr;

    // the solves: ONE without REWEIGHT (the loop folds away); with it solve 0 under the given variances, then up to rw.rounds more under
    // r_eff = min(v / w, 1e8) with the weights the pass 2 before left in `weight` (gsf_reweight_core.hpp).  s is wave-uniform.
    for (int32_t s = 0;; ++s) {
    ChunkIn nxt = load_chunk(tsb, posb, quatb, gpsb, valb, lane, N);
    double mv_nxt[3] = { 1.0, 1.0, 1.0 };
    if constexpr (WEIGHTED) row_var<REWEIGHT>(mvb, cfg, (int64_t)lane, N, mv_nxt[0], mv_nxt[1], mv_nxt[2]);
    double wt_nxt = 1.0;                                                  // (REWEIGHT) the row's weight; solve 0 runs on 1.0
    if constexpr (REWEIGHT) if (s > 0) wt_nxt = wtb[lane < N ? lane : N - 1];

    int same1 = -1, same2 = -1;                                           // WEIGHTED: no axis shares a scan, and the branches on them fold away
    if constexpr (!WEIGHTED) same_axes(cfg.P0, cfg.Qps, cfg.Rm, same1, same2);

    int32_t status = 0;
    // ================================================================================================ pass 1: the filter, ascending
    {
        // carried from chunk to chunk (wave-uniform)
        double cP[3] = { cfg.P0[0], cfg.P0[1], cfg.P0[2] };               // Pf of the last pose (pose 0: P0) ...
        double cx[3] = { 0.0, 0.0, 0.0 };                                 // ... and its position relative to init_pos
        double c_sum = 0.0;                                               // the sum of dt so far
        TrackCarry tc = track_carry_init(a.init_pos, a.init_quat, b, nxt, cfg);
        bool c_ok = tc.first_ok;                                             // a local, not a member of the carry: gsf_track_chunk.hpp

        for (int64_t c0 = 0; c0 < N; c0 += 64) {
            const ChunkIn in = nxt;
            const double mv[3] = { mv_nxt[0], mv_nxt[1], mv_nxt[2] };
            const double wt = wt_nxt;
            nxt = load_chunk(tsb, posb, quatb, gpsb, valb, c0 + 64 + lane, N);   // the next chunk's rows are requested before this chunk's scans (clamped past the end)
            if constexpr (WEIGHTED) row_var<REWEIGHT>(mvb, cfg, c0 + 64 + lane, N, mv_nxt[0], mv_nxt[1], mv_nxt[2]);
            if constexpr (REWEIGHT) if (s > 0) { const int64_t in_ = c0 + 64 + lane; wt_nxt = wtb[in_ < N ? in_ : N - 1]; }
            const ChunkFront f = chunk_front(in, tc, c_ok, c0, N, lane);
            const int64_t i = f.i;
            const bool active = f.active, stepping = f.stepping;
            bool avail = f.fix, bad_sigma = false;
            if constexpr (WEIGHTED) {                                     // ... and three usable variances
                const WeightedAvail wa = weighted_avail(f.fix, mv[0], mv[1], mv[2]);
                avail = wa.avail; bad_sigma = wa.bad;
            }
            // ---- outage structure and the sharp-turn decision: gsf_ekf_cov_ragged_dev's (gsf_cov_core.hpp)
            const u64 av_m = avail_mask(f, avail);
            const OutageMasks om = outage_masks(f.act_m, av_m, c0 == 0, tc.oc.prev_avail);
            status |= (om.start != 0ull) ? ST_HAD_OUTAGE : 0;
            const bool in_outage = ((f.act_m & ~av_m) >> lane) & 1ull;
            const u64 f_mask = yaw_pair_mask<false>(f, om.pair, cfg.yaw_thr_rad, lane);
            int fl = avail ? POSE_GNSS_USED : (in_outage ? POSE_IN_OUTAGE : 0);
            fl |= bad_sigma ? POSE_BAD_SIGMA : 0;
            // sharp_recoveries() with the rows of the outage marked on the way
            u64 sharp_m = 0ull;
            for (u64 rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
                const int rl = __builtin_ctzll(rm);
                const OutageSeg sg = outage_closed_at(om.start, f_mask, rl, c0, tc.oc.ostart, tc.oc.seg_sharp, cfg.yaw_thr_rad < 0.0);
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
            const double wgt = sharp_here ? tc.wgt_sharp : 1.0;          // the one-step blend at a sharp-turn recovery, else a hard update

            const OrientStep<true> os = orientation_step<true>(tc, c_ok, f);
            status |= os.bad_quat ? ST_BAD_QUAT : 0;
            const Quat qi = os.q;
            const double d[3] = { os.u.x, os.u.y, os.u.z };
            const double zr[3] = { f.z.x - tc.p0.x, f.z.y - tc.p0.y, f.z.z - tc.p0.z };   // relative to init_pos: y is a difference of two UTM northings

            // ---- variances (the pose kernels' scans; WEIGHTED: one scan per axis, r of the row's own), positions (three affine scans), the
            // applied correction g = xf - xp
            AxisVar v0, v1, v2;
            double rr[3] = { cfg.Rm[0], cfg.Rm[1], cfg.Rm[2] };
            if constexpr (WEIGHTED) {
                // a row that takes no update carries r = 1: nothing of what its meas_var holds reaches an operand
                // (REWEIGHT: the effective variance, formed for the rows that take an update; wt = 1.0 returns mv's bits.  An idle lane's
                // clamped wt may be another lane's row, old or new: it ends here)
                if constexpr (REWEIGHT) {
                    rr[0] = avail ? reweight_var(mv[0], wt) : 1.0; rr[1] = avail ? reweight_var(mv[1], wt) : 1.0; rr[2] = avail ? reweight_var(mv[2], wt) : 1.0;
                } else {
                    rr[0] = avail ? mv[0] : 1.0; rr[1] = avail ? mv[1] : 1.0; rr[2] = avail ? mv[2] : 1.0;
                }
                v0 = variance_axis<6, true>(cfg.Qps[0], rr[0], f.dt, stepping, avail, cP[0]);
                v1 = variance_axis<6, true>(cfg.Qps[1], rr[1], f.dt, stepping, avail, cP[1]);
                v2 = variance_axis<6, true>(cfg.Qps[2], rr[2], f.dt, stepping, avail, cP[2]);
            } else {
                variance_chunk<6>(cfg, same1, same2, f.dt, stepping, avail, cP[0], cP[1], cP[2], v0, v1, v2);
            }
            const double Pf[3] = { v0.Pf, v1.Pf, v2.Pf }, kg[3] = { v0.kg, v1.kg, v2.kg }, Pm[3] = { v0.Pm, v1.Pm, v2.Pm };
            double x[3], g[3], nis = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double kw = kg[c] * wgt;
                const AxisPos ap = position_axis(avail, kw, d[c], zr[c], cx[c]);
                x[c] = ap.x;                                              // xf[i] - init_pos
                const double y = zr[c] - ap.pm;                           // the innovation, before any blend
                const double gc = kw * y;                                 // ref :722-728 and the blend of :752-768
                g[c] = avail ? gc : 0.0;
                if constexpr (WEIGHTED) nis = nis + weighted_nis_term(y, Pm[c], rr[c]);
            }
            const double S = c_sum + wave_prefix(stepping ? f.dt : 0.0);  // the quaternion axes: one prefix sum of dt (ekf_cov_kernel's)

            // ---- carry to the next 64 poses (from the last active lane L)
            const int L = f.L;
#pragma unroll
            for (int c = 0; c < 3; ++c) { cP[c] = lane_bcast(Pf[c], L); cx[c] = lane_bcast(x[c], L); }
            c_sum = lane_bcast(S, L);
            track_carry_next(tc, f, c0, av_m, om.start, f_mask);
            c_ok = last_ok(f);

            // ---- this chunk's rows.  pos_out, the parked cov_out row and the flags are read again by pass 2: plain stores
            chunk_arrived(nxt);
            if constexpr (WEIGHTED) asm volatile("" :: "v"(mv_nxt[0]), "v"(mv_nxt[1]), "v"(mv_nxt[2]) : "memory");
            if constexpr (REWEIGHT) asm volatile("" :: "v"(wt_nxt) : "memory");
            if (active) {
                const double xf[3] = { tc.p0.x + x[0], tc.p0.y + x[1], tc.p0.z + x[2] };
                // (REWEIGHT parks the RELATIVE position: pass 2 forms the residual from it and p0 + x with the expression above)
                if constexpr (REWEIGHT) { pob[i * 3] = x[0]; pob[i * 3 + 1] = x[1]; pob[i * 3 + 2] = x[2]; }
                else { pob[i * 3] = xf[0]; pob[i * 3 + 1] = xf[1]; pob[i * 3 + 2] = xf[2]; }
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
        status |= tc.oc.prev_avail ? 0 : ST_ENDED_IN_OUTAGE;
    }

    // ================================================================================================ pass 2: the smoother, descending
    {
        // carried from the chunk above (wave-uniform): its first row's e, d (0 where no fix reaches it), g, Pf, stamp and tag bits.  Above
        // the last row there is nothing: a span start, which cuts the link whatever the other values are.
        double c_e[3] = { 0.0, 0.0, 0.0 }, c_d[3] = { 0.0, 0.0, 0.0 }, c_g[3] = { 0.0, 0.0, 0.0 }, c_Pf[3] = { 0.0, 0.0, 0.0 };
        double c_t = 0.0;
        bool c_fix = false, c_start = true, c_reach = false, any_reached = false;
        // (REWEIGHT) init_pos again, "some used row's weight is not the one its solve used", and the largest step of a weight
        double p0[3] = { 0.0, 0.0, 0.0 }, w_step = 0.0;
        u64 changed_m = 0ull;
        if constexpr (REWEIGHT) { p0[0] = a.init_pos[b * 3]; p0[1] = a.init_pos[b * 3 + 1]; p0[2] = a.init_pos[b * 3 + 2]; }
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
            // (REWEIGHT) the row's fix, its given variances and the weight its solve used (this lane's own store; solve 0: 1.0)
            double z_io[3] = { 0.0, 0.0, 0.0 }, v_io[3] = { 1.0, 1.0, 1.0 }, w_used = 1.0;
            if constexpr (REWEIGHT) {
#pragma unroll
                for (int c = 0; c < 3; ++c) z_io[c] = gpsb[il * 3 + c];
                row_var<true>(mvb, cfg, io, N, v_io[0], v_io[1], v_io[2]);
                if (s > 0) w_used = wtb[il];
            }
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
                md[c] = smooth_map_d(A, Pf_n, Pp_n, fix_n);
                e[c] = affine_apply(affine_scan(smooth_map_e(A, g_n)), c_e[c]);
            }
            // (scalar arguments and constant indices only; axes with equal (P0, Q, R) run the same recursion on the same values)
            dd[0] = affine_apply(affine_scan(md[0]), c_d[0]);
            if (same1 == 0) dd[1] = dd[0]; else dd[1] = affine_apply(affine_scan(md[1]), c_d[1]);
            if (same2 == 0) dd[2] = dd[0]; else if (same2 == 1) dd[2] = dd[1]; else dd[2] = affine_apply(affine_scan(md[2]), c_d[2]);
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
                if constexpr (REWEIGHT) {                                 // the parked row is relative: every row is rewritten
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double xa = p0[c] + xf[c];                  // pass 1's xf
                        const double xs = xa + e_io[c];
                        pob[io * 3 + c] = reached_io ? xs : xa;
                    }
                    if (reached_io && flb) flb[io] = (uint8_t)(fl_io | POSE_SMOOTHED);
                } else if (reached_io) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) pob[io * 3 + c] = xf[c] + e_io[c];
                    if (flb) flb[io] = (uint8_t)(fl_io | POSE_SMOOTHED);
                }
            }
            if constexpr (REWEIGHT) {
                // ---- the weights of the next solve fall out here: the residual of every used row against the smoothed track (e_io is 0
                // on a row no later fix reaches), relative to init_pos.  Idle lanes hold whatever their clamped loads gave: `used` ends it.
                const bool used = act_io && smooth_tag_of(w[0]);
                double res[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { const double zr = z_io[c] - p0[c]; res[c] = reweight_residual(zr, xf[c], e_io[c]); }
                const double u2 = reweight_u2(res[0], res[1], res[2], v_io[0], v_io[1], v_io[2]);
                const double w_new = reweight_weight(rw.loss, u2, rw.c2);
                changed_m |= __ballot(used && !reweight_same_bits(w_new, w_used));
                w_step = fmax(w_step, used ? fabs(w_new - w_used) : 0.0);
                if (act_io) wtb[io] = used ? w_new : __builtin_nan("");
            }
        }
        if (lane == 0 && a.status) a.status[b] = status | (any_reached ? ST_RTS_APPLIED : 0);
        if constexpr (REWEIGHT) {
            // stop after rw.rounds reweighted solves, or at a fixed point: the next solve would run on the same bytes (wave-uniform)
            if (s >= rw.rounds || changed_m == 0ull) {
                for (int off = 32; off > 0; off >>= 1) w_step = fmax(w_step, __shfl_xor(w_step, off, 64));
                if (lane == 0) { if (rw.rounds_used) rw.rounds_used[b] = s; if (rw.w_change) rw.w_change[b] = w_step; }
                break;
            }
        }
    }
    if constexpr (!REWEIGHT) break;
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
    const SmoothArgs a{ ts, pos, quat, gps, valid, nullptr, offsets, run_status, init_pos, init_quat, pos_out, quat_out, cov_out, pos_filt, cov_filt,
                        pose_flags, status, nullptr };
    hipLaunchKernelGGL(ekf_smooth_kernel<SMOOTH_PLAIN>, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, k, ReweightArgs{});
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

namespace gsf {

int launch_ekf_smooth_weighted(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                               const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                               const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, double* pos_out, double* quat_out, double* cov_out,
                               double* pos_filt, double* cov_filt, uint8_t* pose_flags, int32_t* status, double* nis)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const EkfConfig k = to_core(cfg);
    const SmoothArgs a{ ts, pos, quat, gps, valid, meas_var, offsets, run_status, init_pos, init_quat, pos_out, quat_out, cov_out, pos_filt,
                        cov_filt, pose_flags, status, nis };
    hipLaunchKernelGGL(ekf_smooth_kernel<SMOOTH_WEIGHTED>, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, k, ReweightArgs{});
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

// robust smoothing: the same kernel with its round loop open (arguments checked by the entry, gsf_capi.hip)
int launch_ekf_smooth_reweighted(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                                 const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                                 const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, int32_t loss, double c2, int32_t rounds,
                                 double* pos_out, double* quat_out, double* cov_out, double* pos_filt, double* cov_filt, uint8_t* pose_flags,
                                 int32_t* status, double* nis, double* weight, int32_t* rounds_used, double* w_change)
{
    GSF_HIP(hipSetDevice(ctx->device));
    const EkfConfig k = to_core(cfg);
    const SmoothArgs a{ ts, pos, quat, gps, valid, meas_var, offsets, run_status, init_pos, init_quat, pos_out, quat_out, cov_out, pos_filt,
                        cov_filt, pose_flags, status, nis };
    const ReweightArgs rw{ weight, rounds_used, w_change, c2, loss, rounds };
    hipLaunchKernelGGL(ekf_smooth_kernel<SMOOTH_REWEIGHTED>, dim3((unsigned)B), dim3(64), 0, ctx->stream, a, k, rw);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

}  // namespace gsf
