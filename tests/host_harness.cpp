// TEST-ONLY host harness: compiles the PRODUCT's per-lane math headers (gsf_math.hpp,
// gsf_ekf_core.hpp) with g++ so that the exact code the HIP kernels inline can be checked
// against the oracle and the goldens in the CPU-only test tier (no GPU in the build
// container).  Never shipped, never loaded by gps_optimize_slam_amd.
#include <cstdint>
#include <cstring>
#include "../gps_optimize_slam_amd/csrc/gsf_ekf_core.hpp"

using namespace gsf;

namespace {
struct AosOut {
    const double* ts_; double* pos; double* quat;
    void store(int64_t i, const Vec3& p, const Quat& q) {
        pos[i * 3] = p.x; pos[i * 3 + 1] = p.y; pos[i * 3 + 2] = p.z;
        quat[i * 4] = q.x; quat[i * 4 + 1] = q.y; quat[i * 4 + 2] = q.z; quat[i * 4 + 3] = q.w;
    }
    void load(int64_t i, Vec3& p, Quat& q) const {
        p = Vec3{ pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] };
        q = Quat{ quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3] };
    }
    double stamp(int64_t i) const { return ts_[i]; }
};
StepIn load_step(const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid, int64_t i) {
    StepIn s;
    s.t = ts[i];
    s.p = Vec3{ pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2] };
    s.q = Quat{ quat[i * 4], quat[i * 4 + 1], quat[i * 4 + 2], quat[i * 4 + 3] };
    s.z = Vec3{ gps[i * 3], gps[i * 3 + 1], gps[i * 3 + 2] };
    s.valid = valid[i];
    return s;
}
}  // namespace

extern "C" {
int hh_ekf_config_size() { return (int)sizeof(EkfConfig); }

int hh_ekf_fuse(const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                int64_t n, const double* p0, const double* q0, const EkfConfig* cfg, double* pos_out, double* quat_out)
{
    if (n <= 0) return 0;
    AosOut out{ ts, pos_out, quat_out };
    EkfTraj<AosOut> f;
    f.init(*cfg, Vec3{ p0[0], p0[1], p0[2] }, Quat{ q0[0], q0[1], q0[2], q0[3] }, load_step(ts, pos, quat, gps, valid, 0), out);
    for (int64_t i = 1; i < n; ++i) f.step(*cfg, i, load_step(ts, pos, quat, gps, valid, i), out);
    return f.finish();
}

// The sharp-turn gate on n pairs: q1, q2 (n,4) raw quaternions, made unit as the kernels make them (quat_unit) before the call.
// out[i]: bit 0 = yaw_rate_exceeds, bit 1 = yaw_rate_exceeds_body, bit 2 = a quaternion is invalid (the callers then count the pair as sharp)
void hh_yaw_gate(const double* q1, const double* q2, const double* dt, const double* thr, int64_t n, uint8_t* out)
{
    for (int64_t i = 0; i < n; ++i) {
        Quat r1, r2;
        const bool ok1 = quat_unit(Quat{ q1[i * 4], q1[i * 4 + 1], q1[i * 4 + 2], q1[i * 4 + 3] }, r1);
        const bool ok2 = quat_unit(Quat{ q2[i * 4], q2[i * 4 + 1], q2[i * 4 + 2], q2[i * 4 + 3] }, r2);
        out[i] = (uint8_t)((yaw_rate_exceeds(r1, r2, dt[i], thr[i]) ? 1 : 0) | (yaw_rate_exceeds_body(r1, r2, dt[i], thr[i]) ? 2 : 0) | ((ok1 && ok2) ? 0 : 4));
    }
}
// the gate's polynomial sine (0 <= c <= 0.785)
void hh_gate_sin_poly(const double* c, int64_t n, double* s) { for (int64_t i = 0; i < n; ++i) s[i] = gate_sin_poly(c[i]); }

static int umeyama_impl(const double* src, const double* dst, int64_t n, double* R, double* t, double* s, bool polar)
{
    if (n < 3) return SIM3_NONE;
    double sc[3] = { 0, 0, 0 }, dc[3] = { 0, 0, 0 };
    for (int64_t i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { sc[k] += src[i * 3 + k]; dc[k] += dst[i * 3 + k]; }
    for (int k = 0; k < 3; ++k) { sc[k] /= (double)n; dc[k] /= (double)n; }
    double H[9] = { 0 }, ssq = 0;
    for (int64_t i = 0; i < n; ++i) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) { a[k] = src[i * 3 + k] - sc[k]; b[k] = dst[i * 3 + k] - dc[k]; }
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[r * 3 + c] += a[r] * b[c];
        ssq += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    }
    return polar ? umeyama_finalize<true>(H, ssq, sc, dc, (double)n, R, t, *s) : umeyama_finalize(H, ssq, sc, dc, (double)n, R, t, *s);
}
int hh_umeyama(const double* src, const double* dst, int64_t n, double* R, double* t, double* s) { return umeyama_impl(src, dst, n, R, t, s, false); }
// the fused pipeline's route (Newton polar iteration instead of the SVD where it applies)
int hh_umeyama_polar(const double* src, const double* dst, int64_t n, double* R, double* t, double* s) { return umeyama_impl(src, dst, n, R, t, s, true); }
// 1 if umeyama_rotation_polar accepts H (else the SVD route is taken)
int hh_polar_applies(const double* H) { double R[9], tr; return umeyama_rotation_polar(H, R, tr) ? 1 : 0; }
// the rotation and singular-value sum of umeyama_rotation_polar itself (R, tr untouched where it declines)
int hh_polar_rotation(const double* H, double* R, double* tr) { return umeyama_rotation_polar(H, R, *tr) ? 1 : 0; }
// the rotation of the Jacobi-SVD route from H
void hh_svd_rotation(const double* H, double* R, double* tr) { umeyama_rotation_svd(H, R, *tr); }

// Host restatement of the ONE-PASS reductions (the short-set path of umeyama_batch_kernel and the window kernels of gsf_sim3.hip, the
// moments pass of the fused pipeline): raw moments of the rows shifted by the first usable (unmasked, finite) row -- shift_last != 0: by
// the last one, the edit tests/test_sim3_yardstick_host.py uses to show what the outlier twins catch -- in 16 strided partial sums, then
// H = Sab - n ma mb^T and umeyama_finalize.  mask may be NULL.
int hh_umeyama_shifted(const double* src, const double* dst, const uint8_t* mask, int64_t n, int polar, int shift_last, double* R, double* t, double* s)
{
    auto usable = [&](int64_t i) {
        if (mask && !mask[i]) return false;
        for (int k = 0; k < 3; ++k) if (!(fabs(src[i * 3 + k]) < INFINITY) || !(fabs(dst[i * 3 + k]) < INFINITY)) return false;
        return true;
    };
    int64_t is = -1;
    if (shift_last) { for (int64_t i = n - 1; i >= 0; --i) if (usable(i)) { is = i; break; } }
    else { for (int64_t i = 0; i < n; ++i) if (usable(i)) { is = i; break; } }
    if (is < 0) return SIM3_NONE;
    double as[3], bs[3];
    for (int k = 0; k < 3; ++k) { as[k] = src[is * 3 + k]; bs[k] = dst[is * 3 + k]; }
    double part[16][17] = { { 0 } };                                      // per lane: n, Sa3, Sb3, Saa, Sab9
    for (int64_t i = 0; i < n; ++i) {
        if (mask && !mask[i]) continue;
        double* p = part[i & 15];
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) { a[k] = src[i * 3 + k] - as[k]; b[k] = dst[i * 3 + k] - bs[k]; }
        p[0] += 1.0;
        for (int k = 0; k < 3; ++k) { p[1 + k] += a[k]; p[4 + k] += b[k]; }
        p[7] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) p[8 + r * 3 + c] += a[r] * b[c];
    }
    double tot[17] = { 0 };
    for (int l = 0; l < 16; ++l) for (int k = 0; k < 17; ++k) tot[k] += part[l][k];
    const double cnt = tot[0];
    if (!(cnt >= 3.0)) return SIM3_NONE;
    const double rn = 1.0 / cnt;
    double ma[3], mb[3], H[9], sc[3], dc[3];
    for (int k = 0; k < 3; ++k) { ma[k] = tot[1 + k] * rn; mb[k] = tot[4 + k] * rn; sc[k] = as[k] + ma[k]; dc[k] = bs[k] + mb[k]; }
    for (int k = 0; k < 9; ++k) H[k] = tot[8 + k] - cnt * ma[k / 3] * mb[k % 3];
    const double ssq = fmax(0.0, tot[7] - cnt * (ma[0] * ma[0] + ma[1] * ma[1] + ma[2] * ma[2]));
    return polar ? umeyama_finalize<true>(H, ssq, sc, dc, cnt, R, t, *s) : umeyama_finalize(H, ssq, sc, dc, cnt, R, t, *s);
}

void hh_sincos(const double* x, int64_t n, double* s, double* c) { for (int64_t i = 0; i < n; ++i) gsf_sincos(x[i], s[i], c[i]); }

void hh_utm_forward(const double* lat, const double* lon, int64_t n, int zone, int south, double* e, double* nn)
{
    TmConsts c = tm_consts();
    for (int64_t i = 0; i < n; ++i) utm_forward_point(c, lat[i], lon[i], 6.0 * zone - 183.0, south ? 1e7 : 0.0, e[i], nn[i]);
}
void hh_utm_inverse(const double* e, const double* nn, int64_t n, int zone, int south, double* lat, double* lon)
{
    TmConsts c = tm_consts();
    for (int64_t i = 0; i < n; ++i) utm_inverse_point(c, e[i], nn[i], 6.0 * zone - 183.0, south ? 1e7 : 0.0, lat[i], lon[i]);
}
void hh_quat_from_matrix(const double* M, double* q) { Quat r = quat_from_matrix(M); q[0] = r.x; q[1] = r.y; q[2] = r.z; q[3] = r.w; }
}
