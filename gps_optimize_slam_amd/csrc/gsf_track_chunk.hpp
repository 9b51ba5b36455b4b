// gsf_track_chunk.hpp -- the chunk body of the kernels that re-run the filter "one wave per track, 64 poses per chunk, lane = pose, no LDS":
// the noise sweep, the outage study's base pass, the innovation gate and the two smoothers.  Each rule of that body is written once here:
// the track's carry and its initialisation, the front of a chunk (rows, dt, "fix usable"), the yaw-rate test of the pairs, the walk
// over the recoveries, the orientation step, the affine position scans.  Device-only (DPP): not one of the host-shared *_core.hpp rule
// headers.  Plain forceinline functions and small by-value structs; scalar arguments and constant indices only (a helper that indexes its
// caller's arrays dynamically puts them into scratch).  -ffp-contract=on in every unit that includes it: which operations fuse is a
// property of these expressions, so the kernels round alike.
#pragma once
#include "gsf_wave_common.hpp"
#include "gsf_cov_core.hpp"
#include "gsf_sweep_core.hpp"

namespace {

// ---- small helpers
// inclusive prefix sum over the wave (lanes without a source add 0)
__device__ __forceinline__ double wave_prefix(double v)
{
#define GSF_PSTAGE(CTRL, RM) { v += dpp0<CTRL, RM>(v); }
    GSF_SCAN_STAGES(GSF_PSTAGE)
#undef GSF_PSTAGE
    return v;
}
// value of lane 63 - lane, and a lane mask in the same order
__device__ __forceinline__ double lane_rev(const double v, const int lane) { return __shfl(v, 63 - lane, 64); }
__device__ __forceinline__ u64 mask_rev(const u64 m) { return __brevll(m); }
// variance of quaternion axis c after a total dt of S: the axes never see an update (ekf_cov_kernel forms it the same way)
__device__ __forceinline__ double quat_axis_var(const EkfConfig& cfg, const int c, const double S) { return cfg.P0[3 + c] + cfg.Qps[3 + c] * S; }
// axes with identical (P0, Q, R) run the same recursion on the same values and share their scans: axis 1 repeats axis same1, axis 2
// repeats axis same2 (-1: scans of its own)
__device__ __forceinline__ void same_axes(const double* P0, const double* Q, const double* R, int& same1, int& same2)
{
    same1 = -1; same2 = -1;
    if (P0[1] == P0[0] && Q[1] == Q[0] && R[1] == R[0]) same1 = 0;
    if (P0[2] == P0[0] && Q[2] == Q[0] && R[2] == R[0]) same2 = 0;
    else if (P0[2] == P0[1] && Q[2] == Q[1] && R[2] == R[1]) same2 = 1;
}
// inclusive scan of affine maps, mine (later) o other (earlier); lanes without a source see the identity
__device__ __forceinline__ Affine affine_scan(Affine m)
{
#define GSF_ASTAGE(CTRL, RM) { const Affine o{ dpp<CTRL, RM>(1.0, m.a), dpp0<CTRL, RM>(m.b) }; m = affine_compose(m, o); }
    GSF_SCAN_STAGES(GSF_ASTAGE)
#undef GSF_ASTAGE
    return m;
}

// ---- the track's carry from chunk to chunk (wave-uniform).  ONE flag that goes with it stays a local of the kernel, handed to the helpers
// by value: c_ok, "the last pose's quaternion is a unit one" (first_ok, then last_ok()).  A local that no call sees by reference is promoted
// to a value before the helpers are inlined and stays a wave-uniform predicate in a scalar register pair; as a member of this struct, which
// the helpers take by reference, it is promoted after inlining as a BYTE that is fetched through a v_cndmask / v_readfirstlane pair, and
// the sweep, the outage base pass and the smoother ran 0.3 to 1 % slower for it (measured: DESIGN.md 7o).  The OutageCarry's flags were
// measured both ways and are as fast in here.
struct TrackCarry {
    Vec3 p0;                  // init_pos: positions are scanned relative to it
    Quat cq0, cq;             // the normalised initial quaternion; the filter's quaternion of the last pose (valid while cq_fresh)
    Quat Cq;                  // q_i = Cq r_i while every quaternion is valid (see wave_serial_chunks)
    bool cq_fresh;
    Vec3 c_po; Quat c_r; double c_t;              // the last pose's original position, unit quaternion (where it is one: c_ok), stamp
    bool first_ok;            // pose 0's quaternion is a unit one: where the kernel's c_ok starts (written once, never carried)
    OutageCarry oc;
    double wgt_sharp;         // the one-step blend at a sharp-turn recovery (ref :752-768, :889)
};
__device__ __forceinline__ TrackCarry track_carry_init(const double* init_pos, const double* init_quat, const int64_t b, const ChunkIn& first,
                                                       const EkfConfig& cfg)
{
    TrackCarry tc;
    tc.p0 = Vec3{ init_pos[b * 3], init_pos[b * 3 + 1], init_pos[b * 3 + 2] };
    tc.cq = ekf_normalize(Quat{ init_quat[b * 4], init_quat[b * 4 + 1], init_quat[b * 4 + 2], init_quat[b * 4 + 3] });   // ref :842, :683
    tc.cq0 = tc.cq;
    chunk_arrived(first);
    tc.c_po = lane_bcast(first.p, 0);                                     // "previous original pose" of pose 0 is pose 0 itself (ref :858)
    tc.first_ok = quat_unit(lane_bcast(first.q, 0), tc.c_r);
    tc.c_t = lane_bcast(first.t, 0);
    tc.Cq = lane_bcast(quat_mul(tc.cq, quat_conj(tc.c_r)), 0);
    tc.cq_fresh = true;
    tc.oc = OutageCarry{ true, 0, false };
    tc.wgt_sharp = (cfg.sharp_turn_steps > 1) ? 1.0 / (double)cfg.sharp_turn_steps : 1.0;
    return tc;
}

// ---- the front of a chunk: what follows from its rows and the carry alone
struct ChunkFront {
    int64_t i; int L; bool active, stepping;   // this lane's pose, the last active lane, i < N, ... and not pose 0
    double t, t_pr, dt; Vec3 p, p_pr, z;       // the row; the previous lane's / the carry's stamp and position
    Quat r, r_pr; bool both_ok;                // unit quaternions of the pose and of the one before; both are valid
    u64 act_m, ok_mask;
    bool vraw, fix;                            // the raw mask byte; the fix is usable (before any rejection, variance test or window)
};
__device__ __forceinline__ ChunkFront chunk_front(const ChunkIn& in, const TrackCarry& tc, const bool c_ok, const int64_t c0, const int64_t N, const int lane)
{
    ChunkFront f;
    f.i = c0 + lane;
    f.L = (int)((N - c0 < 64) ? (N - c0 - 1) : 63);
    f.active = f.i < N; f.stepping = f.active && f.i != 0;
    f.t = in.t; f.p = in.p; f.z = in.z;
    // calculate_relative_pose (ref :77-92) against the previous lane / the carry
    const bool ok = quat_unit(in.q, f.r);
    f.t_pr = prev_lane(tc.c_t, f.t);
    f.p_pr = Vec3{ prev_lane(tc.c_po.x, f.p.x), prev_lane(tc.c_po.y, f.p.y), prev_lane(tc.c_po.z, f.p.z) };
    f.act_m = mask_first(f.L + 1);
    f.ok_mask = __ballot(ok);
    const u64 both_m = ((f.ok_mask << 1) | (c_ok ? 1ull : 0ull)) & f.ok_mask;
    f.both_ok = (both_m >> lane) & 1ull;
    f.dt = fmax(1e-6, f.t - f.t_pr);                                      // ref :865
    f.vraw = in.v != 0;
    f.fix = f.stepping && f.vraw && !(isnan(f.z.x) || isnan(f.z.y) || isnan(f.z.z));   // ref :867-869
    f.r_pr = prev_lane(tc.c_r, f.r);
    return f;
}
// the availability ballot the outage structure is built from; pose 0: the raw mask byte (:848)
__device__ __forceinline__ u64 avail_mask(const ChunkFront& f, const bool avail) { return __ballot(f.i == 0 ? f.vraw : avail) & f.act_m; }
// c_ok for the next 64 poses
__device__ __forceinline__ bool last_ok(const ChunkFront& f) { return ((f.ok_mask >> f.L) & 1ull) != 0ull; }
// the carry to the next 64 poses, from the last active lane L (after the orientation step, which reads the old one)
__device__ __forceinline__ void track_carry_next(TrackCarry& tc, const ChunkFront& f, const int64_t c0, const u64 av_m, const u64 start_m, const u64 f_mask)
{
    tc.oc = outage_carry(tc.oc, av_m, start_m, f_mask, f.L, c0);
    tc.c_po = lane_bcast(f.p, f.L); tc.c_r = lane_bcast(f.r, f.L); tc.c_t = lane_bcast(f.t, f.L);
}

// ---- is_sharp_turn_in_segment's pair test (ref :808-826; :817, :821-824) as a lane mask.  EVERY = false: only the pairs of `sel` (the pairs
// inside outages, OutageMasks::pair) are tested, none where sel is empty.  EVERY = true: every adjacent pair -- the gate and the outage
// study, where a rejection or a scenario may put any pair inside an outage; the caller masks with the outage structure it settles on.
template <bool EVERY>
__device__ __forceinline__ u64 yaw_pair_mask(const ChunkFront& f, const u64 sel, const double yaw_thr_rad, const int lane)
{
    if (!EVERY && sel == 0ull) return 0ull;
    const bool wanted = EVERY ? f.stepping : (bool)((sel >> lane) & 1ull);
    bool over = false;
    if (wanted && f.t > f.t_pr) over = !f.both_ok || yaw_rate_exceeds_body(f.r_pr, f.r, f.t - f.t_pr, yaw_thr_rad);
    return __ballot(over);
}
// the recoveries of the chunk that follow a sharp turn (gsf_cov_core.hpp): the fix there is blended in, and a smoothing span ends in front of it
__device__ __forceinline__ u64 sharp_recoveries(const OutageMasks& om, const u64 f_mask, const int64_t c0, const OutageCarry& oc, const bool neg_thr)
{
    u64 sharp_m = 0ull;
    for (u64 rm = om.rec; rm != 0ull; rm &= rm - 1ull) {
        const int rl = __builtin_ctzll(rm);
        const OutageSeg sg = outage_closed_at(om.start, f_mask, rl, c0, oc.ostart, oc.seg_sharp, neg_thr);
        if (sg.sharp) sharp_m |= 1ull << rl;
    }
    return sharp_m;
}

// ---- the orientation step: the predicted displacement u = d[i] (ref :707) and, with WANT_Q, the filter's quaternion (ref :708-709), as the
// pose kernels form them: one product / rotation by the wave-uniform Cq while every quaternion is valid, else calculate_relative_pose per
// pose and a prefix product of the increments.  Updates cq, Cq and cq_fresh of the carry; reads c_r and c_ok of the chunk before.
// WANT_Q (the smoothers, which store the quaternion and have a status word): q is returned, and bad_quat says that a stepping pose of a
// scanned chunk lacks a valid pair -- ST_BAD_QUAT.  The sweep, the gate and the outage study have no word to report it in and take u alone.
// On the scanned route u is NOT cleared on the lanes that do not step (pose 0 and the idle lanes past L), as it is on the telescoped one:
// it is +0 there already, for every input.  dpl is the literal +0 on them (move is false).  q_prev is finite: pose 0's is cq, the idle
// lanes' is the qi of the lane before, and both leave ekf_normalize(), which returns finite components or, for a NaN, inf, overflowing or
// tiny norm, the identity (pose 0 of a later chunk steps).  quat_rotate(finite q, +0): every product is +-0, so t is +-0 in each
// component, fma(q.w, t, +0) = +-0 + +0 = +0 under round-to-nearest, and +0 + +-0 = +0 -- the word a clearing select would write.
template <bool WANT_Q> struct OrientStep;
template <> struct OrientStep<false> { Vec3 u; };
template <> struct OrientStep<true> { Vec3 u; Quat q; bool bad_quat; };
template <bool WANT_Q>
__device__ __forceinline__ OrientStep<WANT_Q> orientation_step(TrackCarry& tc, const bool c_ok, const ChunkFront& f)
{
    OrientStep<WANT_Q> o;
    const Vec3 dp{ f.p.x - f.p_pr.x, f.p.y - f.p_pr.y, f.p.z - f.p_pr.z };
    const bool stepping = f.stepping;
    const bool telescope = c_ok && ((f.ok_mask & f.act_m) == f.act_m);
    if (telescope) {
        if constexpr (WANT_Q) {
            o.q = quat_mul(tc.Cq, f.r);
            const bool is_init = f.i == 0;                                // pose 0 keeps the initial state (ref :842)
            o.q.x = is_init ? tc.cq0.x : o.q.x; o.q.y = is_init ? tc.cq0.y : o.q.y; o.q.z = is_init ? tc.cq0.z : o.q.z; o.q.w = is_init ? tc.cq0.w : o.q.w;
            o.bad_quat = false;
        }
        o.u = quat_rotate(tc.Cq, dp);
        o.u.x = stepping ? o.u.x : 0.0; o.u.y = stepping ? o.u.y : 0.0; o.u.z = stepping ? o.u.z : 0.0;
        tc.cq_fresh = false;
    } else {
        if (!tc.cq_fresh) { tc.cq = quat_mul(tc.Cq, tc.c_r); tc.cq_fresh = true; }
        const Quat r1i = quat_conj(f.r_pr);
        Vec3 dpl = quat_rotate(r1i, dp);
        Quat dq = quat_mul(r1i, f.r);
        const bool move = stepping && f.both_ok;
        dpl.x = move ? dpl.x : 0.0; dpl.y = move ? dpl.y : 0.0; dpl.z = move ? dpl.z : 0.0;
        dq.x = move ? dq.x : 0.0; dq.y = move ? dq.y : 0.0; dq.z = move ? dq.z : 0.0; dq.w = move ? dq.w : 1.0;
        Quat D = dq;
        const Quat QID{ 0.0, 0.0, 0.0, 1.0 };
#define GSF_QSTAGE(CTRL, RM) { const Quat e = dpp<CTRL, RM>(QID, D); D = quat_mul(e, D); }
        GSF_SCAN_STAGES(GSF_QSTAGE)
#undef GSF_QSTAGE
        const Quat qi = ekf_normalize(quat_mul(tc.cq, D));
        const Quat q_prev = prev_lane(tc.cq, qi);
        o.u = quat_rotate(q_prev, dpl);
        if constexpr (WANT_Q) { o.q = qi; o.bad_quat = __ballot(stepping && !f.both_ok) != 0ull; }
        tc.cq = lane_bcast(qi, f.L);
        if (((f.ok_mask >> f.L) & 1ull) != 0ull) tc.Cq = lane_bcast(quat_mul(tc.cq, quat_conj(lane_bcast(f.r, f.L))), 0);
    }
    return o;
}

// ---- one position axis of the chunk, relative to init_pos: x = the filtered position (an affine scan of the poses' own maps applied to the
// carry cx), pm = the predicted one (ref :707).  kw = gain times blend weight, d = the axis of u, zr = the fix relative to init_pos.
struct AxisPos { double x, pm; };
__device__ __forceinline__ AxisPos position_axis(const bool avail, const double kw, const double d, const double zr, const double cx)
{
    const Affine m = affine_scan(sweep_affine(avail, kw, d, zr));
    AxisPos a;
    a.x = affine_apply(m, cx);
    a.pm = prev_lane(cx, a.x) + d;
    return a;
}

}  // namespace
