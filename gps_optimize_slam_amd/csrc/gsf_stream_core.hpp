// gsf_stream_core.hpp -- streaming fusion: the EkfTraj recursion of gsf_ekf_core.hpp continued across calls (include/gsf.h, "streaming fusion").
//
// A stream keeps, per track, exactly what EkfTraj carries from one pose to the next -- in caller-owned memory, exactly in float64 / int64 --
// and the last `cap` fused rows with their stamps in a ring (global pose index i lives in slot i % cap), which is all that an open outage's
// RTS back-pass reaches back to.  This header holds everything of that which is not a launch: the state's layout with its pack / unpack, the
// ring as the `Out` of EkfTraj, the capacity rule, the n_final / revised_from bookkeeping and the per-track body of an append.  GSF_HD, no HIP
// include: gsf_stream.hip runs stream_append_track() with one lane per track, tests/host_harness_stream.cpp compiles the same code with g++.
//
// State layout (version STREAM_LAYOUT_VERSION): FIELD-MAJOR, field k of track b at state_f64[k * B + b] / state_i64[k * B + b], so the 64 tracks
// of a wave load and store each field as one contiguous 512-byte row.  The fields are the members of StreamF64 / StreamI64 below, in order.
#pragma once
#include "gsf_ekf_core.hpp"

namespace gsf {

constexpr int64_t STREAM_LAYOUT_VERSION = 1;
enum : int32_t { STREAM_FULL = 256, STREAM_BAD_STATE = 512 };          // GSF_STREAM_* of include/gsf.h, beside the GSF_ST_* bits

struct StreamF64 {                  // one track's float64 fields, in the order they are stored
    double p[3], q[4], P[7];        // filter state; before the first pose p / q hold the initial pose (EkfTraj::init's p0, q0)
    double po_prev[3], r_prev[4];   // previous original pose (r_prev already unit)
    double t_prev;
};
struct StreamI64 {
    int64_t version, cap;           // checked by every append: another layout or another ring is refused (STREAM_BAD_STATE)
    int64_t n_total;                // poses seen
    int64_t ostart;                 // first index of the open outage (meaningful while the outage is open)
    int64_t flags;                  // SFL_* bits
    int64_t status;                 // accumulated ST_* bits (without ST_ENDED_IN_OUTAGE, which is a statement about this moment)
};
constexpr int STREAM_F64 = (int)(sizeof(StreamF64) / sizeof(double));   // 22
constexpr int STREAM_I64 = (int)(sizeof(StreamI64) / sizeof(int64_t));  // 6
static_assert(STREAM_F64 == 22 && STREAM_I64 == 6, "the sizes include/gsf.h publishes (GSF_STREAM_F64, GSF_STREAM_I64)");
enum : int64_t { SFL_PREV_AVAIL = 1, SFL_OK_PREV = 2, SFL_SEG_SHARP = 4 };
enum { SI_VERSION = 0, SI_CAP, SI_NTOTAL, SI_OSTART, SI_FLAGS, SI_STATUS };

// The capacity rule.  A back-pass at pose i reads rows ostart .. i-1, so no ring slot may be reused while it can still be read: a track whose
// open outage (n_total - ostart rows) plus its new segment (m rows) does not fit the ring is refused BEFORE any work.
GSF_HD bool stream_refused(bool outage_open, int64_t n_total, int64_t ostart, int64_t m, int64_t cap)
{
    return (outage_open ? n_total - ostart : 0) + m > cap;
}

// The ring (and the outputs of the running call) as the Out of EkfTraj.  Every index an append touches lies in [n0 - cap, n0 + cap) by the
// capacity rule (n0 = n_total before the call), so a slot is s0 + (i - n0) wrapped once: one 64-bit remainder per track and call.
struct RingOut {
    double* rt; double* rp; double* rq;         // this track's ring: [cap], [cap][3], [cap][4]
    int64_t cap, n0, s0;                        // s0 = n0 % cap
    double* po; double* qo;                     // this track's rows of the call's outputs (row j = pose n0 + j), may be NULL
    int64_t lowest;                             // smallest index stored so far (revised_from)

    GSF_HD int64_t slot(int64_t i) const
    {
        int64_t s = s0 + (i - n0);
        s += (s < 0) ? cap : 0;
        s -= (s >= cap) ? cap : 0;
        return s;
    }
    GSF_HD void store(int64_t i, const Vec3& p, const Quat& q)
    {
        const int64_t s = slot(i);
        rp[s * 3] = p.x; rp[s * 3 + 1] = p.y; rp[s * 3 + 2] = p.z;
        rq[s * 4] = q.x; rq[s * 4 + 1] = q.y; rq[s * 4 + 2] = q.z; rq[s * 4 + 3] = q.w;
        const int64_t j = i - n0;
        if (j >= 0) {
            if (po) { po[j * 3] = p.x; po[j * 3 + 1] = p.y; po[j * 3 + 2] = p.z; }
            if (qo) { qo[j * 4] = q.x; qo[j * 4 + 1] = q.y; qo[j * 4 + 2] = q.z; qo[j * 4 + 3] = q.w; }
        }
        lowest = i < lowest ? i : lowest;
    }
    GSF_HD void load(int64_t i, Vec3& p, Quat& q) const
    {
        const int64_t s = slot(i);
        p = Vec3{ rp[s * 3], rp[s * 3 + 1], rp[s * 3 + 2] };
        q = Quat{ rq[s * 4], rq[s * 4 + 1], rq[s * 4 + 2], rq[s * 4 + 3] };
    }
    GSF_HD double stamp(int64_t i) const { return rt[slot(i)]; }
};

template <class Out>
GSF_HD void stream_unpack(const double* sf, const int64_t* si, int64_t B, int64_t b, EkfTraj<Out>& f)
{
    const double* s = sf + b;
    f.p = Vec3{ s[0], s[B], s[2 * B] };
    f.q = Quat{ s[3 * B], s[4 * B], s[5 * B], s[6 * B] };
#pragma unroll
    for (int c = 0; c < 7; ++c) f.P[c] = s[(7 + c) * B];
    f.po_prev = Vec3{ s[14 * B], s[15 * B], s[16 * B] };
    f.r_prev = Quat{ s[17 * B], s[18 * B], s[19 * B], s[20 * B] };
    f.t_prev = s[21 * B];
    const int64_t fl = si[SI_FLAGS * B + b];
    f.prev_avail = (fl & SFL_PREV_AVAIL) != 0; f.ok_prev = (fl & SFL_OK_PREV) != 0; f.seg_sharp = (fl & SFL_SEG_SHARP) != 0;
    f.ostart = si[SI_OSTART * B + b];
    f.status = (int32_t)si[SI_STATUS * B + b];
}

template <class Out>
GSF_HD void stream_pack(double* sf, int64_t* si, int64_t B, int64_t b, const EkfTraj<Out>& f, int64_t n_total)
{
    double* s = sf + b;
    s[0] = f.p.x; s[B] = f.p.y; s[2 * B] = f.p.z;
    s[3 * B] = f.q.x; s[4 * B] = f.q.y; s[5 * B] = f.q.z; s[6 * B] = f.q.w;
#pragma unroll
    for (int c = 0; c < 7; ++c) s[(7 + c) * B] = f.P[c];
    s[14 * B] = f.po_prev.x; s[15 * B] = f.po_prev.y; s[16 * B] = f.po_prev.z;
    s[17 * B] = f.r_prev.x; s[18 * B] = f.r_prev.y; s[19 * B] = f.r_prev.z; s[20 * B] = f.r_prev.w;
    s[21 * B] = f.t_prev;
    si[SI_NTOTAL * B + b] = n_total;
    si[SI_OSTART * B + b] = f.ostart;
    si[SI_FLAGS * B + b] = (f.prev_avail ? SFL_PREV_AVAIL : 0) | (f.ok_prev ? SFL_OK_PREV : 0) | (f.seg_sharp ? SFL_SEG_SHARP : 0);
    si[SI_STATUS * B + b] = (int64_t)f.status;
}

// gsf_stream_open for one track: zero poses seen, p / q = the initial pose, no outage open
GSF_HD void stream_open_track(double* sf, int64_t* si, int64_t B, int64_t b, int64_t cap, const double* init_pos, const double* init_quat)
{
    double* s = sf + b;
#pragma unroll
    for (int k = 0; k < STREAM_F64; ++k) s[k * B] = 0.0;
    s[0] = init_pos[b * 3]; s[B] = init_pos[b * 3 + 1]; s[2 * B] = init_pos[b * 3 + 2];
    s[3 * B] = init_quat[b * 4]; s[4 * B] = init_quat[b * 4 + 1]; s[5 * B] = init_quat[b * 4 + 2]; s[6 * B] = init_quat[b * 4 + 3];
    si[SI_VERSION * B + b] = STREAM_LAYOUT_VERSION; si[SI_CAP * B + b] = cap;
    si[SI_NTOTAL * B + b] = 0; si[SI_OSTART * B + b] = 0; si[SI_FLAGS * B + b] = SFL_PREV_AVAIL; si[SI_STATUS * B + b] = 0;
}

struct StreamSeg {                  // the flat ragged arrays of one append (rows lo .. lo + m - 1 are this track's)
    const double* ts; const double* pos; const double* quat; const double* gps; const uint8_t* valid;
    double* pos_out; double* quat_out; double* cov_out;                   // each may be NULL
};
struct StreamReport { int64_t n_total, n_final, revised_from; int32_t status; };

GSF_HD StepIn stream_load_step(const StreamSeg& g, int64_t r)
{
    StepIn s;
    s.t = g.ts[r];
    s.p = Vec3{ g.pos[r * 3], g.pos[r * 3 + 1], g.pos[r * 3 + 2] };
    s.q = Quat{ g.quat[r * 4], g.quat[r * 4 + 1], g.quat[r * 4 + 2], g.quat[r * 4 + 3] };
    s.z = Vec3{ g.gps[r * 3], g.gps[r * 3 + 1], g.gps[r * 3 + 2] };
    s.valid = g.valid[r];
    return s;
}

GSF_HD void stream_nan_rows(const StreamSeg& g, int64_t lo, int64_t m)
{
    for (int64_t r = lo; r < lo + m; ++r) {
        if (g.pos_out) { g.pos_out[r * 3] = NAN; g.pos_out[r * 3 + 1] = NAN; g.pos_out[r * 3 + 2] = NAN; }
        if (g.quat_out) { g.quat_out[r * 4] = NAN; g.quat_out[r * 4 + 1] = NAN; g.quat_out[r * 4 + 2] = NAN; g.quat_out[r * 4 + 3] = NAN; }
        if (g.cov_out)
            for (int c = 0; c < 7; ++c) g.cov_out[r * 7 + c] = NAN;
    }
}

// The parking policy of an append: what, beyond the ring, is kept of every pose's step.  NoPark keeps nothing and is what
// gsf_stream_append_dev runs; gsf_stream_lag_core.hpp's LagPark keeps the forward quantities of the fixed-lag smoother.  A policy names the
// Out its filter runs on, may refuse a segment on a capacity rule of its own, and sees every pose right after its step.
struct NoPark {
    using Out = RingOut;
    static constexpr bool parks = false;
    GSF_HD bool refused(int64_t, int64_t, int64_t) const { return false; }
    GSF_HD void row(const EkfConfig&, const EkfTraj<RingOut>&, const RingOut&, int64_t, bool) const {}
};

// One track of gsf_stream_append: continue the filter over rows lo .. lo + m - 1 of the segment arrays.  The first pose a track ever sees is
// EkfTraj::init, every later one EkfTraj::step; the state is read once, kept in registers, written once.
template <class Park = NoPark>
GSF_HD StreamReport stream_append_track(const EkfConfig& cfg, double* sf, int64_t* si, int64_t B, int64_t b, int64_t cap, double* ring_t,
                                        double* ring_pos, double* ring_quat, const StreamSeg& g, int64_t lo, int64_t m, const Park park = Park())
{
    using Out = typename Park::Out;
    StreamReport rep;
    m = m < 0 ? 0 : m;
    const int64_t n0 = si[SI_NTOTAL * B + b], os0 = si[SI_OSTART * B + b];
    const bool open0 = n0 > 0 && (si[SI_FLAGS * B + b] & SFL_PREV_AVAIL) == 0;
    if (si[SI_VERSION * B + b] != STREAM_LAYOUT_VERSION || si[SI_CAP * B + b] != cap || n0 < 0 || (open0 && (os0 < 0 || os0 >= n0))) {
        stream_nan_rows(g, lo, m);                                       // not a state this layout wrote for this ring: nothing is touched
        rep.n_total = 0; rep.n_final = 0; rep.revised_from = 0; rep.status = STREAM_BAD_STATE;
        return rep;
    }
    const int32_t st0 = (int32_t)si[SI_STATUS * B + b];
    if (stream_refused(open0, n0, os0, m, cap) || park.refused(n0, m, cap)) {
        stream_nan_rows(g, lo, m);
        rep.n_total = n0; rep.n_final = open0 ? os0 : n0; rep.revised_from = n0;
        rep.status = st0 | (open0 ? ST_ENDED_IN_OUTAGE : 0) | STREAM_FULL;
        return rep;
    }
    if (m == 0) {                                                        // the no-op
        rep.n_total = n0; rep.n_final = open0 ? os0 : n0; rep.revised_from = n0;
        rep.status = st0 | (open0 ? ST_ENDED_IN_OUTAGE : 0);
        return rep;
    }
    EkfTraj<Out> f;
    stream_unpack(sf, si, B, b, f);
    const RingOut ring{ ring_t + b * cap, ring_pos + b * cap * 3, ring_quat + b * cap * 4, cap, n0, n0 % cap,
                        g.pos_out ? g.pos_out + lo * 3 : nullptr, g.quat_out ? g.quat_out + lo * 4 : nullptr, n0 };
    Out out{ ring };
    StepIn nxt = stream_load_step(g, lo);
    for (int64_t j = 0; j < m; ++j) {
        const int64_t i = n0 + j;
        const StepIn in = nxt;
        nxt = stream_load_step(g, lo + (j + 1 < m ? j + 1 : j));         // one pose ahead (clamped re-read at the tail): the rows of a lane are its own
        out.rt[out.slot(i)] = in.t;                                      // the stamp first: a back-pass at this pose reads it
        [[maybe_unused]] const bool was_outage = !f.prev_avail;                          // (read by a parking policy only)
        if (i == 0) {
            const Vec3 p0 = f.p; const Quat q0 = f.q;
            f.init(cfg, p0, q0, in, out);
        } else {
            f.step(cfg, i, in, out);
        }
        if constexpr (Park::parks) park.row(cfg, f, out, i, was_outage);
        if (g.cov_out) {
#pragma unroll
            for (int c = 0; c < 7; ++c) g.cov_out[(lo + j) * 7 + c] = f.P[c];
        }
    }
    stream_pack(sf, si, B, b, f, n0 + m);
    rep.n_total = n0 + m;
    rep.n_final = f.prev_avail ? n0 + m : f.ostart;
    rep.revised_from = out.lowest;
    rep.status = f.status | (f.prev_avail ? 0 : ST_ENDED_IN_OUTAGE);
    return rep;
}

// One row of gsf_stream_gather: global index i of a track with n_total poses, NaN outside what the ring still holds
GSF_HD void stream_gather_row(const double* rt, const double* rp, const double* rq, int64_t cap, int64_t n_total, int64_t i, double& t, Vec3& p, Quat& q)
{
    if (i < 0 || i >= n_total || i < n_total - cap) {
        t = NAN; p = Vec3{ NAN, NAN, NAN }; q = Quat{ NAN, NAN, NAN, NAN };
        return;
    }
    const int64_t s = i % cap;
    t = rt[s];
    p = Vec3{ rp[s * 3], rp[s * 3 + 1], rp[s * 3 + 2] };
    q = Quat{ rq[s * 4], rq[s * 4 + 1], rq[s * 4 + 2], rq[s * 4 + 3] };
}

}  // namespace gsf
