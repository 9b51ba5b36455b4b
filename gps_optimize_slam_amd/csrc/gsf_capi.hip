// gsf_capi.hip -- context / error plumbing of the C ABI (include/gsf.h) and the host-pointer
// convenience entry points (copy in, launch the *_dev form, copy out, synchronise).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include <vector>

#include "gsf_internal.hpp"
#include "gsf_sweep_core.hpp"
#include "gsf_outage_core.hpp"
#include "gsf_gate_core.hpp"
#include "gsf_reweight_core.hpp"

namespace gsf {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int fail_hip(hipError_t e, const char* what)
{
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return GSF_ERR_HIP;
}

// growth per slot: the kernel workspace is allocated at exactly the bytes asked for (hundreds of MB at the largest batches: headroom there
// would be footprint), the others with a quarter on top so that slowly growing calls stop allocating
static const bool WS_HEADROOM[GSF_WS_COUNT] = { /* KERNEL */ false, /* RNG */ true, /* K2B */ true, /* ROWS */ true, /* RUN */ true, /* STREAM */ true };

int ensure_workspace(gsf_ctx* ctx, int slot, size_t bytes)
{
    auto& w = ctx->ws[slot];
    if (w.bytes >= bytes) return GSF_OK;
    if (w.p) {
        GSF_HIP(hipStreamSynchronize(ctx->stream));
        GSF_HIP(hipFree(w.p));
        w.p = nullptr; w.bytes = 0;
    }
    const size_t want = WS_HEADROOM[slot] ? bytes + bytes / 4 : bytes;
    GSF_HIP(hipMalloc(&w.p, want));
    w.bytes = want;
    if (ctx->poison >= 0) return launch_fill_words(ctx, w.p, w.bytes, (uint64_t)ctx->poison);
    return GSF_OK;
}

static int ensure_arena(void** p, size_t* have, size_t bytes, bool pinned, hipStream_t stream)
{
    if (*have >= bytes) return GSF_OK;
    if (*p) {
        GSF_HIP(hipStreamSynchronize(stream));
        GSF_HIP(pinned ? hipHostFree(*p) : hipFree(*p));
        *p = nullptr; *have = 0;
    }
    size_t want = bytes + bytes / 2;                                      // grow-only with headroom: repeated calls stop allocating
    if (want < ((size_t)1 << 20)) want = (size_t)1 << 20;
    hipError_t e = pinned ? hipHostMalloc(p, want, hipHostMallocDefault) : hipMalloc(p, want);
    if (e != hipSuccess && want != bytes) { want = bytes; e = pinned ? hipHostMalloc(p, want, hipHostMallocDefault) : hipMalloc(p, want); }
    if (e != hipSuccess) { *p = nullptr; return fail_hip(e, pinned ? "hipHostMalloc(staging)" : "hipMalloc(staging)"); }
    *have = want;
    return GSF_OK;
}

static void fill_words_host(void* p, size_t bytes, uint64_t word)
{
    for (size_t i = 0; i < bytes; ++i) ((unsigned char*)p)[i] = (unsigned char)(word >> (8 * (i & 7)));
}

int Staging::add(void* host, size_t bytes, int kind, int from)
{
    const int i = tab_.add(bytes, kind, host != nullptr);
    if (i < 0) {
        if (rc_ == GSF_OK) { set_error("staging: more than %d arrays declared", STAGE_MAX_BLOCKS); rc_ = GSF_ERR_INVALID_ARG; }
        return -1;
    }
    host_[i] = host; bind_[i] = nullptr; from_[i] = from;
    return i;
}

int Staging::upload()
{
    if (rc_ != GSF_OK) return rc_;
    plan_ = stage_plan(tab_.b, tab_.n);
    direct_ = plan_.cap > PINNED_MAX;
    GSF_HIP(hipSetDevice(ctx_->device));
    gsf_ctx* const ctx = ctx_;
    const void* const stage0 = ctx->stage; const void* const pinned0 = ctx->pinned;
    if ((rc_ = ensure_arena(&ctx->stage, &ctx->stage_bytes, plan_.cap, false, ctx->stream))) return rc_;
    if (!direct_ && (rc_ = ensure_arena(&ctx->pinned, &ctx->pinned_bytes, plan_.cap, true, ctx->stream))) return rc_;
    d_ = (char*)ctx->stage; h_ = (char*)ctx->pinned;
    if (ctx->poison >= 0) {                                               // an arena that has just grown is dirtied like the others
        if (ctx->stage != stage0 && (rc_ = launch_fill_words(ctx, ctx->stage, ctx->stage_bytes, (uint64_t)ctx->poison))) return rc_;
        if (ctx->pinned && ctx->pinned != pinned0) fill_words_host(ctx->pinned, ctx->pinned_bytes, (uint64_t)ctx->poison);
    }
    for (int i = 0; i < tab_.n; ++i) {
        const StageBlock& b = tab_.b[i];
        if (bind_[i]) *bind_[i] = d_ + b.off;
        if (b.kind != STAGE_IN || !b.host) continue;
        if (direct_) GSF_HIP(hipMemcpyAsync(d_ + b.off, host_[i], b.bytes, hipMemcpyHostToDevice, ctx->stream));
        else memcpy(h_ + b.off, host_[i], b.bytes);
    }
    if (!direct_ && plan_.in_end) GSF_HIP(hipMemcpyAsync(d_, h_, plan_.in_end, hipMemcpyHostToDevice, ctx->stream));
    for (int i = 0; i < tab_.n; ++i)
        if (from_[i] >= 0) GSF_HIP(hipMemcpyAsync(d_ + tab_.b[i].off, d_ + tab_.b[from_[i]].off, tab_.b[i].bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return GSF_OK;
}

int Staging::finish()
{
    if (rc_ != GSF_OK) return rc_;
    if (!direct_ && plan_.d2h_hi > plan_.d2h_lo)
        GSF_HIP(hipMemcpyAsync(h_ + plan_.d2h_lo, d_ + plan_.d2h_lo, plan_.d2h_hi - plan_.d2h_lo, hipMemcpyDeviceToHost, ctx_->stream));
    if (!direct_) GSF_HIP(hipStreamSynchronize(ctx_->stream));
    for (int i = 0; i < tab_.n; ++i) {
        const StageBlock& b = tab_.b[i];
        if (b.kind != STAGE_OUT || !b.host) continue;
        if (direct_) GSF_HIP(hipMemcpyAsync(host_[i], d_ + b.off, b.bytes, hipMemcpyDeviceToHost, ctx_->stream));
        else memcpy(host_[i], h_ + b.off, b.bytes);
    }
    if (direct_) GSF_HIP(hipStreamSynchronize(ctx_->stream));
    return GSF_OK;
}

}  // namespace gsf

using namespace gsf;

extern "C" {

// The wave-per-trajectory kernels live in two translation units that are compiled with different instruction schedulers (Makefile); which
// scheduler and which floating-point contraction mode actually produced each object is part of the version string, so a build that took
// the Makefile's fall-back path cannot ship unnoticed (bench.py prints this string).
const char* gsf_version(void)
{
    // a function-local static is initialised once, also under concurrent first calls (C++11)
    static const std::string v = std::string("gsf 0.5.0 (gfx950, fp64) | ") + gsf::wave_small_build_info() + " | " + gsf::wave_big_build_info() + " | " +
                                 gsf::wave_block_build_info() + " | " + gsf::wave_early_build_info();
    return v.c_str();
}
int gsf_abi_version(void) { return GSF_ABI_VERSION; }

int gsf_last_error(char* buf, int n)
{
    int len = (int)strlen(g_err);
    if (buf && n > 0) { strncpy(buf, g_err, (size_t)n - 1); buf[n - 1] = '\0'; }
    return len;
}

int gsf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int create_common(int device_id, hipStream_t stream, bool owns, gsf_ctx** out)
{
    if (!out) { set_error("gsf_create: out is NULL"); return GSF_ERR_INVALID_ARG; }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("gsf_create: no HIP device is visible (this library has no CPU fallback)");
        return GSF_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= n) { set_error("gsf_create: device %d out of range [0,%d)", device_id, n); return GSF_ERR_INVALID_ARG; }
    GSF_HIP(hipSetDevice(device_id));
    gsf_ctx* c = new gsf_ctx();
    c->device = device_id; c->stream = stream; c->owns_stream = owns;     // (everything else: the defaults of gsf_ctx)
    if (owns) {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail_hip(e, "hipStreamCreateWithFlags"); }
    }
    // on a failure everything created so far is released again, and the message names the call that failed
    bool have_ev0 = false, have_ev1 = false;
    const char* what = "hipEventCreate";
    hipError_t e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) { have_ev0 = true; e = hipEventCreate(&c->ev1); }
    if (e == hipSuccess) { have_ev1 = true; what = "hipMalloc(small_scratch)"; e = hipMalloc(&c->small_scratch, 512); }
    if (e != hipSuccess) {
        if (have_ev0) (void)hipEventDestroy(c->ev0);
        if (have_ev1) (void)hipEventDestroy(c->ev1);
        if (owns) (void)hipStreamDestroy(c->stream);
        delete c;
        return fail_hip(e, what);
    }
    *out = c;
    return GSF_OK;
}

int gsf_create(int device_id, gsf_ctx** out) { return create_common(device_id, nullptr, true, out); }
int gsf_create_on_stream(int device_id, void* hip_stream, gsf_ctx** out) { return create_common(device_id, (hipStream_t)hip_stream, false, out); }

void gsf_destroy(gsf_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& w : ctx->ws)
        if (w.p) (void)hipFree(w.p);
    if (ctx->small_scratch) (void)hipFree(ctx->small_scratch);
    if (ctx->stage) (void)hipFree(ctx->stage);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    (void)hipEventDestroy(ctx->ev0);
    (void)hipEventDestroy(ctx->ev1);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int gsf_trim(gsf_ctx* ctx)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_HIP(hipSetDevice(ctx->device));
    GSF_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& w : ctx->ws)                                              // (the 512-byte small_scratch stays)
        if (w.p) { GSF_HIP(hipFree(w.p)); w.p = nullptr; w.bytes = 0; }
    if (ctx->stage) { GSF_HIP(hipFree(ctx->stage)); ctx->stage = nullptr; ctx->stage_bytes = 0; }
    if (ctx->pinned) { GSF_HIP(hipHostFree(ctx->pinned)); ctx->pinned = nullptr; ctx->pinned_bytes = 0; }
    return GSF_OK;
}

int gsf_synchronize(gsf_ctx* ctx)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_HIP(hipStreamSynchronize(ctx->stream));
    return GSF_OK;
}

// the integer options that are a field and an inclusive range (what each one does: at the field, gsf_internal.hpp)
static const struct { const char* key; int gsf_ctx::*field; int64_t lo, hi; const char* message; } INT_OPTIONS[] = {
    { "ekf_variant", &gsf_ctx::ekf_variant, INT64_MIN, INT64_MAX, "" },
    { "synth_variant", &gsf_ctx::synth_variant, 0, 1, "synth_variant must be 0 (white SLAM noise) or 1 (random-walk drift, SURVEY 8d)" },
    { "block_kernel", &gsf_ctx::block_kernel, -1, 1, "block_kernel must be -1 (automatic), 0 (never) or 1 (whenever it applies)" },
    { "k2b_screen", &gsf_ctx::k2b_screen, 0, 1, "k2b_screen must be 1 (single-precision screen + exact re-check, default) or 0 (double throughout)" },
    { "ransac_early_exit", &gsf_ctx::ransac_early_exit, 0, 1,
      "ransac_early_exit must be 0 (every trajectory draws all max_trials: the generator ends where the reference leaves it) or 1 (a trajectory stops at the first "
      "trial that counts every row: same R, t, s, mask and poses)" },
    { "prefilter_speculate", &gsf_ctx::prefilter_speculate, 0, 1, "prefilter_speculate must be 0 or 1" },
    { "prefilter_miss_batch", &gsf_ctx::prefilter_miss_batch, 1, 64, "prefilter_miss_batch must be in [1, 64]" },
    { "prefilter_first_batch", &gsf_ctx::prefilter_first_batch, 1, 64, "prefilter_first_batch must be in [1, 64]" },
    { "ransac_probe_trials", &gsf_ctx::ransac_probe_trials, 1, 1 << 20, "ransac_probe_trials must be in [1, 2^20]" },
    { "duo_kernel", &gsf_ctx::duo_kernel, -1, 1, "duo_kernel must be -1 (automatic), 0 (one wave) or 1 (two-wave blocks)" },
    { "early_variances", &gsf_ctx::early_variances, -1, 1,
      "early_variances must be -1 (automatic), 0 (never) or 1 (always where the build applies); the results are the same bits" },
    { "tail_scan_stages", &gsf_ctx::tail_scan_stages, 0, 1,
      "tail_scan_stages must be 1 (the scans of a short last chunk run only the stages that reach its lanes, default) or 0 (always six stages); the results are the "
      "same bits" },
    { "noise_sweep_group", &gsf_ctx::noise_sweep_group, 0, 64,
      "noise_sweep_group must be 0 (automatic) or the number of candidates one wave of the EKF noise sweep takes, 1..64; the results are the same bits" },
};

int gsf_set_option(gsf_ctx* ctx, const char* key, int64_t value)
{
    GSF_REQUIRE(ctx && key, "NULL argument");
    for (const auto& o : INT_OPTIONS) {
        if (strcmp(key, o.key) != 0) continue;
        if (value < o.lo || value > o.hi) { set_error("gsf_set_option: %s", o.message); return GSF_ERR_INVALID_ARG; }
        ctx->*o.field = (int)value;
        return GSF_OK;
    }
    if (strcmp(key, "tape_draws") == 0) {                                     // (not in the table: 1 is not a value)
        if (value < -1 || value > 2 || value == 1) { set_error("gsf_set_option: tape_draws must be -1 (automatic: a few streams are drawn chip-wide), 0 (always one wave per stream) or 2 (tests: a tape cut short, so that the one-wave kernel takes over)"); return GSF_ERR_INVALID_ARG; }
        ctx->tape_draws = (int)value; return GSF_OK;
    }
    if (strcmp(key, "lane_min_traj") == 0) {                                  // (64-bit, no upper bound)
        if (value < 0) { set_error("gsf_set_option: lane_min_traj must be >= 0"); return GSF_ERR_INVALID_ARG; }
        ctx->lane_min_traj = value; return GSF_OK;
    }
    if (strcmp(key, "poison_workspaces") == 0) {
        if (value < -1 || value > 255) { set_error("gsf_set_option: poison_workspaces must be -1 (off) or a fill word in [0, 255]"); return GSF_ERR_INVALID_ARG; }
        ctx->poison = value;
        if (value < 0) return GSF_OK;
        // every call fills what the context holds now; the pinned mirror is idle between calls (the host-pointer entries synchronise)
        GSF_HIP(hipSetDevice(ctx->device));
        GSF_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->pinned) fill_words_host(ctx->pinned, ctx->pinned_bytes, (uint64_t)value);
        for (auto& w : ctx->ws)
            if (w.p) { const int rc = launch_fill_words(ctx, w.p, w.bytes, (uint64_t)value); if (rc != GSF_OK) return rc; }
        void* const more[2] = { ctx->stage, ctx->small_scratch };
        const size_t nb[2] = { ctx->stage_bytes, 512 };
        for (int k = 0; k < 2; ++k)
            if (more[k]) { const int rc = launch_fill_words(ctx, more[k], nb[k], (uint64_t)value); if (rc != GSF_OK) return rc; }
        return GSF_OK;
    }
    set_error("gsf_set_option: unknown key '%s'", key);
    return GSF_ERR_INVALID_ARG;
}

int gsf_set_sim3_rows(gsf_ctx* ctx, int32_t mode, int32_t min_samples, double max_gps_gap_threshold, double max_initial_duration)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (all valid rows) or 1 (the reference's choice, EKFGPSSLAM.py:973-998)");
    GSF_REQUIRE(mode == 0 || min_samples >= 0, "min_samples must be >= 0");
    ctx->fit_rows = gsf::FitRows{ mode, min_samples, max_gps_gap_threshold, max_initial_duration };
    return GSF_OK;
}

int gsf_timer_start(gsf_ctx* ctx)
{
    GSF_REQUIRE(ctx, "ctx is NULL");
    GSF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    return GSF_OK;
}

int gsf_timer_stop(gsf_ctx* ctx, float* elapsed_ms)
{
    GSF_REQUIRE(ctx && elapsed_ms, "NULL argument");
    GSF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    GSF_HIP(hipEventSynchronize(ctx->ev1));
    GSF_HIP(hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    return GSF_OK;
}

// ------------------------------------------------------------------------------------------
// host-pointer forms: pack -> one H2D -> *_dev launch -> one D2H -> synchronise (gsf::Staging)
// ------------------------------------------------------------------------------------------
static int utm_host(gsf_ctx* ctx, bool inverse, const double* a, const double* b, int64_t n, int32_t zone, int32_t south, double* oa, double* ob)
{
    GSF_REQUIRE(ctx && (n == 0 || (a && b && oa && ob)) && n >= 0, "bad arguments");
    if (n == 0) return GSF_OK;
    Staging st(ctx);
    const int64_t off[2] = { 0, n }; const int32_t zs[2] = { zone, south };
    auto da = st.in(a, (size_t)n); auto db = st.in(b, (size_t)n);
    auto doff = st.in(off, 2); auto dzs = st.in(zs, 2);
    auto doa = st.out(oa, (size_t)n); auto dob = st.out(ob, (size_t)n);
    if (inverse) ST_RUN(gsf_utm_inverse_batch_dev(ctx, da, db, doff, dzs, dzs + 1, 1, doa, dob));
    ST_RUN(gsf_utm_forward_batch_dev(ctx, da, db, doff, dzs, dzs + 1, 1, doa, dob));
}

int gsf_utm_forward(gsf_ctx* ctx, const double* lat, const double* lon, int64_t n, int32_t zone, int32_t south, double* e, double* nn)
{
    return utm_host(ctx, false, lat, lon, n, zone, south, e, nn);
}

int gsf_utm_inverse(gsf_ctx* ctx, const double* e, const double* nn, int64_t n, int32_t zone, int32_t south, double* lat, double* lon)
{
    return utm_host(ctx, true, e, nn, n, zone, south, lat, lon);
}

int gsf_sim3_umeyama_batch(gsf_ctx* ctx, const double* src, const double* dst, const uint8_t* mask, const int64_t* offsets,
                           int64_t B, double* R, double* t, double* s, int32_t* status)
{
    GSF_REQUIRE(ctx && offsets && B >= 0 && R && t && s && status, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (src && dst)), "bad offsets / NULL points");
    Staging st(ctx);
    auto dsrc = st.in(src, (size_t)total * 3); auto ddst = st.in(dst, (size_t)total * 3);
    auto doff = st.in(offsets, (size_t)B + 1);
    auto dmask = st.in_opt(mask, (size_t)total);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B);
    auto dst_ = st.out(status, (size_t)B);
    ST_RUN(gsf_sim3_umeyama_batch_dev(ctx, dsrc, ddst, dmask, doff, B, dR, dt, ds, dst_));
}

int gsf_sim3_ransac_batch(gsf_ctx* ctx, const double* src, const double* dst, const int64_t* offsets, int64_t B,
                          const int32_t* sample_idx, int32_t trials, int32_t min_samples, double thr, int32_t min_inliers,
                          double* R, double* t, double* s, int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers)
{
    GSF_REQUIRE(ctx && offsets && B >= 0 && R && t && s && status && inlier_mask && n_inliers, "bad arguments");
    GSF_REQUIRE(trials >= 0 && min_samples >= 1 && (trials == 0 || sample_idx), "bad trials/min_samples/sample_idx");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (src && dst)), "bad offsets / NULL points");
    const size_t nidx = (size_t)B * (size_t)trials * (size_t)min_samples;
    Staging st(ctx);
    auto dsrc = st.in(src, (size_t)total * 3); auto ddst = st.in(dst, (size_t)total * 3);
    auto doff = st.in(offsets, (size_t)B + 1);
    auto didx = st.in(sample_idx, nidx);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B);
    auto dst_ = st.out(status, (size_t)B); auto dni = st.out(n_inliers, (size_t)B);
    auto dmask = st.out(inlier_mask, (size_t)total);
    ST_RUN(gsf_sim3_ransac_batch_rows_dev(ctx, dsrc, ddst, doff, total, B, didx, trials, min_samples, thr, min_inliers, dR, dt, ds, dst_, dmask, dni));
}

// compute_sim3_transform_robust with the draws made on the device: mt_state[B][625] (host, in/out) is NumPy's legacy generator state
int gsf_sim3_ransac_mt_batch(gsf_ctx* ctx, const double* src, const double* dst, const int64_t* offsets, int64_t B, uint32_t* mt_state,
                             int32_t trials, int32_t min_samples, double thr, int32_t min_inliers, double* R, double* t, double* s,
                             int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers)
{
    GSF_REQUIRE(ctx && offsets && B >= 0 && B <= 0x7fffffff && mt_state && R && t && s && status && inlier_mask && n_inliers, "bad arguments");
    GSF_REQUIRE(trials >= 0 && trials <= (1 << 20) && min_samples >= 1 && min_samples <= 64, "bad trials / min_samples (1..64: the device sampler traces up to 64 positions per trial)");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (src && dst)), "bad offsets / NULL points");
    std::vector<int32_t> counts((size_t)B);
    int32_t n_max = 1;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        GSF_REQUIRE(n >= 0 && n <= 28000, "a point set has more than 28000 rows (device-side draws) or negative length");
        counts[(size_t)b] = (int32_t)n;
        if ((int32_t)n > n_max) n_max = (int32_t)n;
    }
    const size_t nidx = (size_t)B * (size_t)trials * (size_t)min_samples;
    Staging st(ctx);
    auto dsrc = st.in(src, (size_t)total * 3); auto ddst = st.in(dst, (size_t)total * 3);
    auto doff = st.in(offsets, (size_t)B + 1);
    auto dcnt = st.in(counts.data(), (size_t)B);
    auto dstate = st.inout(mt_state, (size_t)B * 625);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B);
    auto dst_ = st.out(status, (size_t)B); auto dni = st.out(n_inliers, (size_t)B);
    auto dmask = st.out(inlier_mask, (size_t)total);
    auto didx = st.tmp<int32_t>(nidx + 1);
    ST_UPLOAD();
    int rc;
    if (trials > 0 && (rc = launch_mt_choice(ctx, dstate, dcnt, B, trials, min_samples, didx, n_max))) return rc;
    if ((rc = launch_sim3_ransac(ctx, dsrc, ddst, doff, nullptr, B, didx, trials, min_samples, thr, min_inliers, dR, dt, ds, dst_, dmask, dni, total))) return rc;
    return st.finish();
}

int gsf_apply_sim3_batch(gsf_ctx* ctx, const double* pos, const double* quat, const int64_t* offsets, int64_t B, const double* R,
                         const double* t, const double* s, double* pos_out, double* quat_out, int32_t* bad_quat)
{
    GSF_REQUIRE(ctx && offsets && B >= 0 && R && t && s, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (pos && quat && pos_out && quat_out)), "bad offsets / NULL poses");
    Staging st(ctx);
    auto dpos = st.in(pos, (size_t)total * 3); auto dquat = st.in(quat, (size_t)total * 4);
    auto doff = st.in(offsets, (size_t)B + 1);
    auto dR = st.in(R, (size_t)B * 9); auto dt = st.in(t, (size_t)B * 3); auto ds = st.in(s, (size_t)B);
    auto dpo = st.out(pos_out, (size_t)total * 3); auto dqo = st.out(quat_out, (size_t)total * 4);
    auto dbad = st.out(bad_quat, (size_t)B);
    ST_RUN(gsf_apply_sim3_batch_dev(ctx, dpos, dquat, doff, B, dR, dt, ds, dpo, dqo, dbad));
}

int gsf_ekf_fuse_batch(gsf_ctx* ctx, int32_t layout, const double* ts, const double* pos, const double* quat, const double* gps,
                       const uint8_t* valid, const double* init_pos, const double* init_quat, const gsf_ekf_config* cfg, int64_t B,
                       int64_t N, double* pos_out, double* quat_out, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && B >= 0 && N >= 0, "bad arguments");
    if (B == 0 || N == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && init_pos && init_quat && pos_out && quat_out, "NULL array");
    const size_t P = (size_t)B * (size_t)N;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dpos = st.in(pos, P * 3); auto dquat = st.in(quat, P * 4);
    auto dgps = st.in(gps, P * 3); auto dval = st.in(valid, P);
    auto dip = st.in(init_pos, (size_t)B * 3); auto diq = st.in(init_quat, (size_t)B * 4);
    auto dpo = st.out(pos_out, P * 3); auto dqo = st.out(quat_out, P * 4); auto dst_ = st.out(status, (size_t)B);
    ST_RUN(gsf_ekf_fuse_batch_dev(ctx, layout, dts, dpos, dquat, dgps, dval, dip, diq, cfg, B, N, dpo, dqo, dst_));
}

// steps 3-5 of main_process_gui with the plain fit, host arrays in / out (one upload, one launch, one download)
int gsf_fuse_pipeline_batch(gsf_ctx* ctx, int32_t layout, const double* ts, const double* pos, const double* quat, const double* gps,
                            const uint8_t* valid, const gsf_ekf_config* cfg, int64_t B, int64_t N, double* R, double* t, double* s,
                            double* pos_out, double* quat_out, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && B >= 0 && N >= 0, "bad arguments");
    if (B == 0 || N == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && R && t && s && pos_out && quat_out && status, "NULL array");
    const size_t P = (size_t)B * (size_t)N;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dpos = st.in(pos, P * 3); auto dquat = st.in(quat, P * 4);
    auto dgps = st.in(gps, P * 3); auto dval = st.in(valid, P);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B);
    auto dpo = st.out(pos_out, P * 3); auto dqo = st.out(quat_out, P * 4); auto dst_ = st.out(status, (size_t)B);
    ST_RUN(gsf_fuse_pipeline_batch_dev(ctx, layout, dts, dpos, dquat, dgps, dval, cfg, B, N, dR, dt, ds, dpo, dqo, dst_));
}

// main_process_gui's row choice (ref :973-998), host arrays
int gsf_sim3_fit_rows_batch(gsf_ctx* ctx, const double* ts, const double* gps, const uint8_t* valid, const int64_t* offsets, int64_t B, int64_t N,
                            int32_t min_samples, double max_gps_gap_threshold, double max_initial_duration, uint8_t* row_mask, int32_t* n_rows,
                            int32_t* status)
{
    GSF_REQUIRE(ctx && B >= 0 && (offsets || N >= 0), "bad arguments");
    if (B == 0 || (!offsets && N == 0)) return GSF_OK;
    GSF_REQUIRE(ts && valid && row_mask && n_rows, "NULL array");
    const int64_t total = offsets ? offsets[B] : B * N;
    GSF_REQUIRE(total >= 0, "bad offsets");
    if (total == 0) { for (int64_t b = 0; b < B; ++b) { n_rows[b] = -1; if (status) status[b] = GSF_SIM3_FLAG_FEW_ROWS; } return GSF_OK; }
    const size_t P = (size_t)total;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dgps = st.in_opt(gps, P * 3); auto dval = st.in(valid, P);
    auto doff = st.in_opt(offsets, (size_t)B + 1);
    auto dmask = st.out(row_mask, P); auto dn = st.out(n_rows, (size_t)B); auto dst_ = st.out_opt(status, (size_t)B);
    ST_RUN(gsf_sim3_fit_rows_batch_dev(ctx, dts, dgps, dval, doff, B, N, min_samples, max_gps_gap_threshold, max_initial_duration, dmask, dn, dst_));
}

// the same steps with the reference's robust fit; mt_state[B][625] (host, in/out) is each trajectory's NumPy legacy generator state
int gsf_fuse_pipeline_robust_batch(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps,
                                   const uint8_t* valid, const gsf_ekf_config* cfg, int64_t B, int64_t N, int32_t min_samples,
                                   double residual_threshold, int32_t max_trials, int32_t min_inliers_needed, uint32_t* mt_state, double* R,
                                   double* t, double* s, double* pos_out, double* quat_out, int32_t* status, int32_t* n_inliers,
                                   uint8_t* inlier_mask)
{
    GSF_REQUIRE(ctx && cfg && B >= 0 && N >= 0 && mt_state, "bad arguments");
    if (B == 0 || N == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && R && t && s && pos_out && quat_out && status && n_inliers, "NULL array");
    const size_t P = (size_t)B * (size_t)N;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dpos = st.in(pos, P * 3); auto dquat = st.in(quat, P * 4);
    auto dgps = st.in(gps, P * 3); auto dval = st.in(valid, P);
    auto dstate = st.inout(mt_state, (size_t)B * 625);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B);
    auto dpo = st.out(pos_out, P * 3); auto dqo = st.out(quat_out, P * 4); auto dst_ = st.out(status, (size_t)B);
    auto dni = st.out(n_inliers, (size_t)B);
    auto dmask = st.out_opt(inlier_mask, P);
    ST_RUN(gsf_fuse_pipeline_robust_batch_dev(ctx, dts, dpos, dquat, dgps, dval, cfg, B, N, min_samples, residual_threshold, max_trials,
                                              min_inliers_needed, dstate, dR, dt, ds, dpo, dqo, dst_, dni, dmask));
}

// tracks of different lengths (flat [total][C] host arrays, trajectory b = rows offsets[b]..offsets[b+1])
int gsf_ekf_fuse_ragged(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                        const int64_t* offsets, const double* init_pos, const double* init_quat, const gsf_ekf_config* cfg, int64_t B,
                        double* pos_out, double* quat_out, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && offsets && B >= 0 && init_pos && init_quat && status, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (ts && pos && quat && gps && valid && pos_out && quat_out)), "bad offsets / NULL arrays");
    const size_t P = (size_t)total;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dpos = st.in(pos, P * 3); auto dquat = st.in(quat, P * 4);
    auto dgps = st.in(gps, P * 3); auto dval = st.in(valid, P); auto doff = st.in(offsets, (size_t)B + 1);
    auto dip = st.in(init_pos, (size_t)B * 3); auto diq = st.in(init_quat, (size_t)B * 4);
    auto dpo = st.out(pos_out, P * 3); auto dqo = st.out(quat_out, P * 4); auto dst_ = st.out(status, (size_t)B);
    ST_RUN(gsf_ekf_fuse_ragged_dev(ctx, dts, dpos, dquat, dgps, dval, doff, dip, diq, cfg, B, dpo, dqo, dst_));
}
int gsf_fuse_pipeline_ragged(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                             const int64_t* offsets, const gsf_ekf_config* cfg, int64_t B, double* R, double* t, double* s, double* pos_out,
                             double* quat_out, int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && offsets && B >= 0 && R && t && s && status, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (ts && pos && quat && gps && valid && pos_out && quat_out)), "bad offsets / NULL arrays");
    const size_t P = (size_t)total;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dpos = st.in(pos, P * 3); auto dquat = st.in(quat, P * 4);
    auto dgps = st.in(gps, P * 3); auto dval = st.in(valid, P); auto doff = st.in(offsets, (size_t)B + 1);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B);
    auto dpo = st.out(pos_out, P * 3); auto dqo = st.out(quat_out, P * 4); auto dst_ = st.out(status, (size_t)B);
    ST_RUN(gsf_fuse_pipeline_ragged_dev(ctx, dts, dpos, dquat, dgps, dval, doff, cfg, B, dR, dt, ds, dpo, dqo, dst_));
}

// per-pose covariance and flags of the fused tracks, host arrays (the outputs that are NULL are neither staged nor computed)
int gsf_ekf_cov_ragged(gsf_ctx* ctx, const double* ts, const double* quat, const double* gps, const uint8_t* valid, const int64_t* offsets,
                       const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, double* cov_filt, double* cov_out, uint8_t* pose_flags,
                       int32_t* status)
{
    GSF_REQUIRE(ctx && cfg && offsets && B >= 0, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (ts && quat && gps && valid && cov_out)), "bad offsets / NULL arrays");
    const size_t P = (size_t)total;
    Staging st(ctx);
    auto dts = st.in(ts, P); auto dquat = st.in(quat, P * 4); auto dgps = st.in(gps, P * 3);
    auto dval = st.in(valid, P); auto doff = st.in(offsets, (size_t)B + 1);
    auto drs = st.in_opt(run_status, (size_t)B);
    auto dcf = st.out_opt(cov_filt, P * 7); auto dco = st.out(cov_out, P * 7);
    auto dfl = st.out_opt(pose_flags, P); auto dst_ = st.out_opt(status, (size_t)B);
    ST_RUN(gsf_ekf_cov_ragged_dev(ctx, dts, dquat, dgps, dval, doff, drs, cfg, B, dcf, dco, dfl, dst_));
}

// B equal-size windows of W point pairs (sliding-window re-alignment) held by the host
int gsf_sim3_umeyama_windows(gsf_ctx* ctx, const double* src, const double* dst, const uint8_t* mask, int64_t B, int32_t W, double* R, double* t,
                             double* s, int32_t* status)
{
    GSF_REQUIRE(ctx && B >= 0 && W >= 0 && R && t && s && status, "bad arguments");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(W == 0 || (src && dst), "NULL points");
    const size_t P = (size_t)B * (size_t)W;
    Staging st(ctx);
    auto dsrc = st.in(src, P * 3); auto ddst = st.in(dst, P * 3);
    auto dmask = st.in_opt(mask, P);
    auto dR = st.out(R, (size_t)B * 9); auto dt = st.out(t, (size_t)B * 3); auto ds = st.out(s, (size_t)B); auto dst_ = st.out(status, (size_t)B);
    ST_RUN(gsf_sim3_umeyama_windows_dev(ctx, dsrc, ddst, dmask, B, W, dR, dt, ds, dst_));
}

// WGS84 -> local ENU about per-trajectory origins, host arrays
int gsf_geodetic_to_enu_batch(gsf_ctx* ctx, const double* lat_deg, const double* lon_deg, const double* alt, const int64_t* offsets,
                              const double* ref_llh, int64_t B, double* east, double* north, double* up)
{
    GSF_REQUIRE(ctx && offsets && ref_llh && B >= 0, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (lat_deg && lon_deg && alt && east && north && up)), "bad offsets / NULL arrays");
    const size_t P = (size_t)total;
    Staging st(ctx);
    auto dla = st.in(lat_deg, P); auto dlo = st.in(lon_deg, P); auto dal = st.in(alt, P);
    auto doff = st.in(offsets, (size_t)B + 1); auto dref = st.in(ref_llh, (size_t)B * 3);
    auto de = st.out(east, P); auto dn = st.out(north, P); auto du = st.out(up, P);
    ST_RUN(gsf_geodetic_to_enu_batch_dev(ctx, dla, dlo, dal, doff, dref, B, de, dn, du));
}

// load_gps_data's geodesy slice for B ragged logs held by the host
int gsf_gps_rows_to_utm_batch(gsf_ctx* ctx, const double* llh, const int64_t* offsets, int64_t B, double* utm_rows, int32_t* zone, int32_t* south)
{
    GSF_REQUIRE(ctx && offsets && B >= 0 && zone && south, "bad arguments");
    if (B == 0) return GSF_OK;
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (llh && utm_rows)), "bad offsets / NULL rows");
    Staging st(ctx);
    auto dllh = st.in(llh, (size_t)total * 3); auto doff = st.in(offsets, (size_t)B + 1);
    auto dutm = st.out(utm_rows, (size_t)total * 3); auto dz = st.out(zone, (size_t)B); auto dso = st.out(south, (size_t)B);
    ST_RUN(gsf_gps_rows_to_utm_batch_dev(ctx, dllh, doff, B, dutm, dz, dso));
}

// one RANSACRegressor.fit per problem with host-drawn sample sets, host arrays in / out
int gsf_ransac_poly_batch(gsf_ctx* ctx, const double* t, const double* y, const int64_t* offsets, int64_t P, const int32_t* sample_idx,
                          int32_t max_trials, int32_t min_samples, int32_t degree, double residual_threshold, double stop_probability,
                          uint8_t* inlier_mask, int32_t* n_trials, int32_t* n_inliers, int32_t* status)
{
    GSF_REQUIRE(ctx && offsets && P >= 0 && n_trials && n_inliers && status, "bad arguments");
    GSF_REQUIRE(max_trials >= 1 && min_samples >= 1, "bad max_trials / min_samples");
    if (P == 0) return GSF_OK;
    const int64_t total = offsets[P];
    GSF_REQUIRE(total >= 0 && (total == 0 || (t && y && inlier_mask)) && sample_idx, "bad offsets / NULL arrays");
    const size_t nidx = (size_t)P * (size_t)max_trials * (size_t)min_samples;
    Staging st(ctx);
    auto dt = st.in(t, (size_t)total); auto dy = st.in(y, (size_t)total); auto doff = st.in(offsets, (size_t)P + 1);
    auto didx = st.in(sample_idx, nidx);
    auto dmask = st.out(inlier_mask, (size_t)total); auto dnt = st.out(n_trials, (size_t)P); auto dni = st.out(n_inliers, (size_t)P);
    auto dst_ = st.out(status, (size_t)P);
    ST_RUN(gsf_ransac_poly_batch_dev(ctx, dt, dy, doff, P, didx, max_trials, min_samples, degree, residual_threshold, stop_probability, dmask, dnt, dni, dst_));
}

// the fused track at M query stamps, host arrays (the outputs that are NULL are neither staged nor computed)
int gsf_pose_query(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets, const int32_t* run_status,
                   const uint8_t* pose_flags, int64_t B, const double* q_t, const int64_t* q_offsets, int64_t M, double max_gap, double* out_pos,
                   double* out_quat, uint8_t* q_flags, int32_t* q_index, uint8_t* q_pose_flags, int32_t* track_state)
{
    GSF_REQUIRE(ctx && B >= 0 && M >= 0, "bad arguments");
    if (B == 0 || M == 0) return GSF_OK;
    GSF_REQUIRE(offsets && q_t && q_offsets && out_pos && out_quat && q_flags && track_state, "NULL array");
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (ts && pos && quat)), "bad offsets / NULL arrays");
    const size_t P = total > 0 ? (size_t)total : 1, Mq = (size_t)M;      // (no poses at all: one unread row stands in for the arrays)
    const double zero_row[8] = { 0.0 };
    Staging st(ctx);
    auto dts = st.in(total > 0 ? ts : zero_row, P); auto dpos = st.in(total > 0 ? pos : zero_row, P * 3);
    auto dquat = st.in(total > 0 ? quat : zero_row, P * 4); auto doff = st.in(offsets, (size_t)B + 1);
    auto drs = st.in_opt(run_status, (size_t)B);
    auto dpf = st.in_opt(total > 0 ? pose_flags : nullptr, P);
    auto dqt = st.in(q_t, Mq); auto dqo = st.in(q_offsets, (size_t)B + 1);
    auto dop = st.out(out_pos, Mq * 3); auto doq = st.out(out_quat, Mq * 4); auto dfl = st.out(q_flags, Mq);
    auto dqi = st.out_opt(q_index, Mq); auto dqp = st.out_opt(q_pose_flags, Mq);
    auto dst_ = st.out(track_state, (size_t)B);
    ST_RUN(gsf_pose_query_dev(ctx, dts, dpos, dquat, doff, drs, dpf, B, dqt, dqo, M, max_gap, dop, doq, dfl, dqi, dqp, dst_));
}

// sensor points carried into the fused track's frame, host arrays
int gsf_georef_points(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets, const int32_t* run_status,
                      const uint8_t* pose_flags, int64_t B, const double* q_t, const int64_t* q_offsets, int64_t M, double max_gap, const double* x,
                      const double* ext_q, const double* ext_t, const double* scale, double* out_xyz, uint8_t* q_flags, int32_t* q_index,
                      uint8_t* q_pose_flags, int32_t* track_state)
{
    GSF_REQUIRE(ctx && B >= 0 && M >= 0, "bad arguments");
    if (B == 0 || M == 0) return GSF_OK;
    GSF_REQUIRE(offsets && q_t && q_offsets && x && out_xyz && q_flags && track_state, "NULL array");
    const int64_t total = offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (ts && pos && quat)), "bad offsets / NULL arrays");
    const size_t P = total > 0 ? (size_t)total : 1, Mq = (size_t)M;
    const double zero_row[8] = { 0.0 };
    Staging st(ctx);
    auto dts = st.in(total > 0 ? ts : zero_row, P); auto dpos = st.in(total > 0 ? pos : zero_row, P * 3);
    auto dquat = st.in(total > 0 ? quat : zero_row, P * 4); auto doff = st.in(offsets, (size_t)B + 1);
    auto drs = st.in_opt(run_status, (size_t)B);
    auto dpf = st.in_opt(total > 0 ? pose_flags : nullptr, P);
    auto dqt = st.in(q_t, Mq); auto dqo = st.in(q_offsets, (size_t)B + 1); auto dx = st.in(x, Mq * 3);
    auto deq = st.in_opt(ext_q, (size_t)B * 4); auto det = st.in_opt(ext_t, (size_t)B * 3);
    auto dsc = st.in_opt(scale, (size_t)B);
    auto dxyz = st.out(out_xyz, Mq * 3); auto dfl = st.out(q_flags, Mq);
    auto dqi = st.out_opt(q_index, Mq); auto dqp = st.out_opt(q_pose_flags, Mq);
    auto dst_ = st.out(track_state, (size_t)B);
    ST_RUN(gsf_georef_points_dev(ctx, dts, dpos, dquat, doff, drs, dpf, B, dqt, dqo, M, max_gap, dx, deq, det, dsc, dxyz, dfl, dqi, dqp, dst_));
}

// EKF noise sweep: device form only (include/gsf.h; the Python binding uploads host arrays itself)
int gsf_ekf_noise_sweep_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                            const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                            const gsf_ekf_config* cfg, int64_t B, const double* cand, int32_t K, double skip_seconds, int32_t min_updates,
                            int32_t trace_k, double* stats, int32_t* best_k, double* pooled, int32_t* pooled_best, int32_t* ns_status,
                            double* innov, double* innov_var)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    GSF_REQUIRE(K >= 1 && K <= SWEEP_MAX_K, "K must be in [1, 4096]");
    GSF_REQUIRE(trace_k < K, "trace_k must be below K (negative: no trace)");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && init_pos && init_quat && cand, "NULL array");
    GSF_REQUIRE(skip_seconds == skip_seconds, "skip_seconds is NaN");
    return launch_noise_sweep(ctx, ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, cfg, B, cand, K, skip_seconds, min_updates,
                              trace_k, stats, best_k, pooled, pooled_best, ns_status, innov, innov_var);
}

// GNSS outage study: device form only (include/gsf.h; the Python binding uploads host arrays itself)
int gsf_outage_study_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                         const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                         const gsf_ekf_config* cfg, int64_t B, const double* truth, const uint8_t* truth_valid, const double* scen, int32_t K,
                         int32_t trace_k, double* stats, int32_t* seg, int32_t* os_flags, double* err_dr, double* err_fused, double* trace_pos)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    GSF_REQUIRE(K >= 1 && K <= OUTAGE_MAX_K, "K must be in [1, 4096]");
    GSF_REQUIRE(trace_k < K, "trace_k must be below K (negative: no trace)");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && init_pos && init_quat && scen, "NULL array");
    GSF_REQUIRE((truth == nullptr) == (truth_valid == nullptr), "truth and truth_valid go together (both NULL: the fixes themselves)");
    return launch_outage_study(ctx, ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, cfg, B, truth, truth_valid, scen, K,
                               trace_k, stats, seg, os_flags, err_dr, err_fused, trace_pos);
}

// innovation gate: device form only (include/gsf.h; the Python binding uploads host arrays itself)
int gsf_innovation_gate_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                            const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                            const gsf_ekf_config* cfg, int64_t B, const double* gates, int32_t K, double arm_seconds, int32_t max_run,
                            uint8_t* valid_out, double* nis_out, double* stats, int32_t* gate_status)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    GSF_REQUIRE(K >= 1 && K <= GATE_MAX_K, "K must be in [1, 64]");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && init_pos && init_quat && gates, "NULL array");
    GSF_REQUIRE(arm_seconds == arm_seconds, "arm_seconds is NaN");
    return launch_innovation_gate(ctx, ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, cfg, B, gates, K, arm_seconds, max_run,
                                  valid_out, nis_out, stats, gate_status);
}

// local Sim3 alignment: device forms only (include/gsf.h; the Python binding uploads host arrays itself)
int gsf_sim3_local_fit_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* gps, const uint8_t* valid, const int64_t* offsets,
                           int64_t B, const double* R, const double* t, const double* s, const gsf_local_config* cfg, int32_t Kmax,
                           double* knot_R, double* knot_t, double* knot_s, int32_t* knot_n, double* knot_rms, int32_t* knot_flags,
                           int32_t* n_knots, int32_t* track_status)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0 && B <= 0x7fffffff, "bad B");
    GSF_REQUIRE(Kmax >= 1 && Kmax <= 4096, "Kmax must be in [1, 4096]");
    GSF_REQUIRE(cfg->mode == GSF_LOC_SCALE || cfg->mode == GSF_LOC_SIM3, "mode must be GSF_LOC_SCALE or GSF_LOC_SIM3");
    GSF_REQUIRE(cfg->min_rows >= (cfg->mode == GSF_LOC_SIM3 ? 3 : 2), "min_rows must be >= 2 (mode 0) / >= 3 (mode 1)");
    GSF_REQUIRE(cfg->spacing > 0.0 && cfg->spacing < INFINITY, "spacing must be positive and finite");
    GSF_REQUIRE(cfg->half_window >= 0.0, "half_window must be >= 0");
    GSF_REQUIRE(cfg->rot_open >= 0.0 && cfg->ratio_max >= 1.0, "rot_open must be >= 0 and ratio_max >= 1");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && gps && valid && R && t && s, "NULL input array");
    GSF_REQUIRE(knot_R && knot_t && knot_s && knot_n && knot_rms && knot_flags && n_knots && track_status, "NULL output array");
    return launch_local_fit(ctx, ts, pos, gps, valid, offsets, B, R, t, s, cfg, Kmax, knot_R, knot_t, knot_s, knot_n, knot_rms, knot_flags,
                            n_knots, track_status);
}

int gsf_sim3_local_apply_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets, int64_t B,
                             const double* R, const double* t, const double* s, double spacing, int32_t Kmax, const double* knot_R,
                             const double* knot_t, const double* knot_s, const int32_t* knot_flags, const int32_t* n_knots,
                             const int32_t* track_status, double* pos_out, double* quat_out, double* scale_at, int32_t* pose_flags)
{
    GSF_REQUIRE(ctx && offsets, "ctx/offsets is NULL");
    GSF_REQUIRE(B >= 0 && B <= 0x7fffffff, "bad B");
    GSF_REQUIRE(Kmax >= 1 && Kmax <= 4096, "Kmax must be in [1, 4096]");
    GSF_REQUIRE(spacing > 0.0 && spacing < INFINITY, "spacing must be positive and finite");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && R && t && s, "NULL input array");
    GSF_REQUIRE(knot_R && knot_t && knot_s && knot_flags && n_knots && track_status, "NULL knot array");
    GSF_REQUIRE(pos_out && quat_out && scale_at && pose_flags, "NULL output array");
    return launch_local_apply(ctx, ts, pos, quat, offsets, B, R, t, s, spacing, Kmax, knot_R, knot_t, knot_s, knot_flags, n_knots, track_status,
                              pos_out, quat_out, scale_at, pose_flags);
}

// antenna lever arm: device forms only (include/gsf.h; the Python binding uploads host arrays itself)
int gsf_lever_fit_dev(gsf_ctx* ctx, const double* pos, const double* quat, const double* gps, const uint8_t* valid, const int64_t* offsets,
                      int64_t B, const double* R, const double* t, const double* s, const double* l0, const int32_t* run_status,
                      const gsf_lever_config* cfg, double* R_out, double* t_out, double* s_out, double* l_out, double* l_cov, int32_t* n_rows,
                      int32_t* n_bad_quat, double* rms_before, double* rms_after, double* last_step, int32_t* flags)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0 && B <= 0x7fffffff, "bad B");
    GSF_REQUIRE(cfg->iters >= 1 && cfg->iters <= 8, "iters must be in [1, 8]");
    GSF_REQUIRE(cfg->min_rows >= 1, "min_rows must be >= 1");
    GSF_REQUIRE(cfg->sigma_fix > 0.0 && cfg->sigma_fix < INFINITY, "sigma_fix must be positive and finite");
    GSF_REQUIRE(cfg->sigma_prior[0] > 0.0 && cfg->sigma_prior[1] > 0.0 && cfg->sigma_prior[2] > 0.0 && cfg->sigma_rot > 0.0,
                "sigma_prior and sigma_rot must be positive (infinite: no prior)");
    GSF_REQUIRE(cfg->ratio_max >= 1.0 && cfg->pivot_min >= 0.0 && cfg->weak_ratio >= 0.0 && cfg->conv_tol >= 0.0,
                "ratio_max must be >= 1, pivot_min, weak_ratio and conv_tol >= 0");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(pos && quat && gps && valid && R && t && s && l0, "NULL input array");
    GSF_REQUIRE(R_out && t_out && s_out && l_out && l_cov && n_rows && n_bad_quat && rms_before && rms_after && last_step && flags, "NULL output array");
    return launch_lever_fit(ctx, pos, quat, gps, valid, offsets, B, R, t, s, l0, run_status, cfg, R_out, t_out, s_out, l_out, l_cov, n_rows,
                            n_bad_quat, rms_before, rms_after, last_step, flags);
}

int gsf_lever_apply_dev(gsf_ctx* ctx, const double* quat, const double* xyz, const int64_t* offsets, int64_t B, const double* R, const double* l,
                        double sign, double* xyz_out, int32_t* pose_flags)
{
    GSF_REQUIRE(ctx && offsets, "ctx/offsets is NULL");
    GSF_REQUIRE(B >= 0 && B <= 0x7fffffff, "bad B");
    GSF_REQUIRE(sign == 1.0 || sign == -1.0, "sign must be +1 or -1");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(quat && xyz && R && l, "NULL input array");
    GSF_REQUIRE(xyz_out && pose_flags, "NULL output array");
    return launch_lever_apply(ctx, quat, xyz, offsets, B, R, l, sign, xyz_out, pose_flags);
}

// per-fix GNSS noise: device forms only (include/gsf.h; the Python binding uploads host arrays itself)
int gsf_ekf_smooth_weighted_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                                const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                                const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, double* pos_out, double* quat_out,
                                double* cov_out, double* pos_filt, double* cov_filt, uint8_t* pose_flags, int32_t* status, double* nis)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && meas_var && init_pos && init_quat && pos_out && quat_out && cov_out, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff, "B too large for one launch");
    return launch_ekf_smooth_weighted(ctx, ts, pos, quat, gps, valid, meas_var, offsets, init_pos, init_quat, run_status, cfg, B, pos_out, quat_out,
                                      cov_out, pos_filt, cov_filt, pose_flags, status, nis);
}

// robust smoothing: device form only (include/gsf.h).  meas_var may be NULL: cfg's meas_noise_diag on every row
int gsf_ekf_smooth_reweighted_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                                  const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                                  const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, int32_t loss, double c2, int32_t rounds,
                                  double* pos_out, double* quat_out, double* cov_out, double* pos_filt, double* cov_filt, uint8_t* pose_flags,
                                  int32_t* status, double* nis, double* weight, int32_t* rounds_used, double* w_change)
{
    GSF_REQUIRE(ctx && cfg && offsets, "ctx/cfg/offsets is NULL");
    GSF_REQUIRE(B >= 0, "negative B");
    GSF_REQUIRE(gsf::reweight_args_ok(loss, c2, rounds), "loss must be GSF_REWEIGHT_HUBER or _CAUCHY, c2 finite and > 0, rounds in [0, 32]");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && gps && valid && init_pos && init_quat && pos_out && quat_out && cov_out && weight, "NULL array");
    GSF_REQUIRE(B <= (int64_t)0x7fffffff, "B too large for one launch");
    return launch_ekf_smooth_reweighted(ctx, ts, pos, quat, gps, valid, meas_var, offsets, init_pos, init_quat, run_status, cfg, B, loss, c2, rounds,
                                        pos_out, quat_out, cov_out, pos_filt, cov_filt, pose_flags, status, nis, weight, rounds_used, w_change);
}

int gsf_fix_var_at_poses_dev(gsf_ctx* ctx, const double* ts, const int64_t* slam_offsets, const double* gps_t, const int64_t* gps_offsets,
                             const uint8_t* gps_keep, const double* fix_var, const uint8_t* valid, int64_t B, int64_t P, double* pose_var)
{
    GSF_REQUIRE(ctx && slam_offsets && gps_offsets, "ctx/slam_offsets/gps_offsets is NULL");
    GSF_REQUIRE(B >= 0 && P >= 0, "negative B or P");
    if (B == 0 || P == 0) return GSF_OK;
    GSF_REQUIRE(P <= (int64_t)0x7fffffff * 256, "P too large for one launch");
    GSF_REQUIRE(ts && pose_var, "NULL array");                           // (gps_t / fix_var may be NULL when every log is empty)
    return launch_fix_var_at_poses(ctx, ts, slam_offsets, gps_t, gps_offsets, gps_keep, fix_var, valid, B, P, pose_var);
}

}  // extern "C"
