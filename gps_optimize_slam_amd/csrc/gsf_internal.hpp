// gsf_internal.hpp -- context, error plumbing and layout indexing shared by the .hip units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gsf.h"
#include "gsf_ekf_core.hpp"
#include "gsf_stage_plan.hpp"

// The grow-only device workspaces of a context, one slot each.  They are separate allocations because a slot may grow (free + malloc) while a
// caller further up the chain still holds pointers into another one; no two of them may be merged.
enum gsf_ws_slot {
    GSF_WS_KERNEL,   // kernel workspace (time-alignment slabs, the transposed copy of a small time-major batch, robust_chain's layout), sized exactly
    GSF_WS_RNG,      // tape, transition tables and swap partners of the chip-wide draws (gsf_rng_tape.hip); separate from the kernel slot, whose
                     // layout the caller of launch_mt_choice (robust_chain) may hold pointers into
    GSF_WS_K2B,      // K2b's rows as floats (screened residual counts, gsf_sim3.hip); grows below robust_chain as well
    GSF_WS_ROWS,     // row mask + flags of the Sim3 row choice for the kernels that take it as a pre-pass (gsf_ekf_block.hip); below robust_chain too
    GSF_WS_RUN,      // temporaries of the whole-run chain (gsf_run.hip), which holds pointers into it while its stages grow the kernel slot
    GSF_WS_STREAM,   // the per-track plan the forward launch of gsf_stream_append_lag_dev leaves for its back-pass launch (gsf_stream_lag.hip): 16 B per track
    GSF_WS_COUNT
};

struct gsf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct { void* p = nullptr; size_t bytes = 0; } ws[GSF_WS_COUNT];   // gsf::ensure_workspace / gsf::workspace
    // staging of the host-pointer entry points: one grow-only device arena + a pinned host mirror (see gsf::Staging)
    void* stage = nullptr;
    size_t stage_bytes = 0;
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    void* small_scratch = nullptr;   // 512 B: arg-max keys of the split K2b launch (gsf_sim3.hip: up to 32 sets x 16 B)
    int k2b_screen = 1;        // K2b residual counts screened in packed single precision, exact re-check in the band (gsf_set_option "k2b_screen"): 1 default, 0 all double
    int tape_draws = -1;       // chip-wide draws for a few streams (gsf_set_option "tape_draws"): -1 automatic, 0 never, 2 tests (tape cut short)
    int ekf_variant = 0;       // reserved tuning knob (gsf_set_option "ekf_variant"); 0 = default
    int synth_variant = 0;     // synthetic workload (gsf_set_option "synth_variant"): 0 = white SLAM noise (default), 1 = SURVEY 8d's random-walk drift
    int block_kernel = -1;     // workgroup-per-trajectory kernel for 64 < N <= 1024 (gsf_set_option "block_kernel"): -1 automatic, 0 never, 1 always
    int ransac_early_exit = 0; // robust chain: stop a trajectory's trials at the first one that counts every row (gsf_set_option "ransac_early_exit"): 0 default, 1 on
    int prefilter_miss_batch = 4; // ... and the largest batch the sequential walk opens with after the speculative pass has missed (gsf_set_option "prefilter_miss_batch")
    int prefilter_speculate = 1;  // the pre-filter chain tries "every axis of the window stops after its first trial" first (gsf_set_option "prefilter_speculate")
    int prefilter_first_batch = 1; // trials the pre-filter chain draws and scores before its first look at scikit-learn's stopping rule (gsf_set_option "prefilter_first_batch")
    int ransac_probe_trials = 64; // ... trials the early-exit probe draws and scores itself before the wide kernels take the rest (gsf_set_option "ransac_probe_trials")
    int duo_kernel = -1;       // two-wave pipeline kernel for small batches (gsf_set_option "duo_kernel"): -1 automatic, 0 never, 1 always
    int early_variances = -1;  // one-wave pipeline build for short tracks with the first chunk's variances computed under the input burst (gsf_set_option "early_variances"): -1 automatic, 0 never, 1 always where it applies (same bits)
    int tail_scan_stages = 1;  // wave kernels: scans of a short last chunk sized by its last active lane (gsf_set_option "tail_scan_stages"): 1 default, 0 always six stages (same bits)
    int noise_sweep_group = 0; // candidates per wave of the EKF noise sweep (gsf_set_option "noise_sweep_group"): 0 automatic (sweep_group(), gsf_wave_route.hpp), 1..64 forced (same bits)
    // rows of the fused chains' Sim3 fit (gsf_set_sim3_rows); mode 0 = all valid rows.  Default: the rows main_process_gui hands to its fit
    // (ref :973-998) under the reference's CONFIG defaults (:34, :53, :37), so a raw C caller of gsf_fuse_pipeline_* gets steps 3-5 as the reference runs them
    gsf::FitRows fit_rows{ 1, 4, 5.0, 180.0 };
    int64_t poison = -1;       // tests: every workspace is filled with this 64-bit word when the option is set and after it grows (gsf_set_option "poison_workspaces"); -1 = off
    int64_t lane_min_traj = 32768; // time-major batches with fewer trajectories are transposed and run by the wave kernel (gsf_set_option "lane_min_traj")
};

namespace gsf {

void set_error(const char* fmt, ...);
int fail_hip(hipError_t e, const char* what);

#define GSF_HIP(call)                                         \
    do {                                                      \
        hipError_t e__ = (call);                              \
        if (e__ != hipSuccess) return gsf::fail_hip(e__, #call); \
    } while (0)

#define GSF_REQUIRE(cond, msg)                                \
    do {                                                      \
        if (!(cond)) { gsf::set_error("%s: %s", __func__, msg); return GSF_ERR_INVALID_ARG; } \
    } while (0)

// Element index of component c (of C) of pose i of trajectory b.
template <int LAYOUT>
struct Idx {
    int64_t B, N;
    __host__ __device__ __forceinline__ int64_t at(int64_t b, int64_t i, int c, int C) const
    {
        if (LAYOUT == GSF_LAYOUT_TIME_MAJOR) return (i * C + c) * B + b;
        return (b * N + i) * C + c;
    }
};

// how each wave-level translation unit was compiled (scheduler, -ffp-contract mode, compiler): recorded by the Makefile's -D flags
#ifndef GSF_TU_SCHED
#define GSF_TU_SCHED "default"
#endif
#ifndef GSF_TU_CONTRACT
#define GSF_TU_CONTRACT "fast (hipcc default)"
#endif
#define GSF_TU_BUILD_INFO(file) file ": sched=" GSF_TU_SCHED ", fp-contract=" GSF_TU_CONTRACT ", clang " __clang_version__
const char* wave_small_build_info();
const char* wave_big_build_info();
const char* wave_block_build_info();
const char* wave_early_build_info();

// slot `slot` (gsf_ws_slot) holds at least `bytes` afterwards; a regrowth synchronises the stream, frees the old block and invalidates pointers into it
int ensure_workspace(gsf_ctx* ctx, int slot, size_t bytes);
template <class T = char> inline T* workspace(const gsf_ctx* ctx, int slot) { return (T*)ctx->ws[slot].p; }
// `bytes` at p (device memory, 8-byte aligned) <- the 64-bit word repeated, on the context's stream (gsf_util.hip)
int launch_fill_words(gsf_ctx* ctx, void* p, size_t bytes, uint64_t word);

// gsf_ekf_config -> the kernels' form of it (np.deg2rad, ref :886)
inline EkfConfig to_core(const gsf_ekf_config* c)
{
    EkfConfig k;
    for (int i = 0; i < 7; ++i) { k.P0[i] = c->initial_cov_diag[i]; k.Qps[i] = c->process_noise_diag[i]; }
    for (int i = 0; i < 3; ++i) k.Rm[i] = c->meas_noise_diag[i];
    k.yaw_thr_rad = c->sharp_turn_yaw_rate_threshold_deg_per_sec * (M_PI / 180.0);
    k.sharp_turn_steps = c->default_ekf_transition_steps_on_sharp_turn;
    k._pad = 0;
    return k;
}

// wave-per-trajectory K4 / fused pipeline for the trajectory-major layout (gsf_ekf_wave.hip), by the build that wave_route() names
// (gsf_wave_route.hpp): one wave, two waves, early variances, big batch or a workgroup per trajectory -- the same bits from each
int launch_ekf_wave(gsf_ctx* ctx, bool pipeline, const double* ts, const double* pos, const double* quat, const double* gps,
                    const uint8_t* valid, const double* init_pos, const double* init_quat, const gsf_ekf_config* cfg, int64_t B,
                    int64_t N, double* R, double* t, double* s, double* pos_out, double* quat_out, int32_t* status,
                    const int64_t* offsets = nullptr);

// EKF noise sweep (gsf_noise_sweep.hip): the body of gsf_ekf_noise_sweep_dev, arguments checked by the caller
int launch_noise_sweep(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                       const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                       const gsf_ekf_config* cfg, int64_t B, const double* cand, int32_t K, double skip_seconds, int32_t min_updates,
                       int32_t trace_k, double* stats, int32_t* best_k, double* pooled, int32_t* pooled_best, int32_t* ns_status,
                       double* innov, double* innov_var);

// GNSS outage study (gsf_outage_study.hip): the body of gsf_outage_study_dev, arguments checked by the caller
int launch_outage_study(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                        const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                        const gsf_ekf_config* cfg, int64_t B, const double* truth, const uint8_t* truth_valid, const double* scen, int32_t K,
                        int32_t trace_k, double* stats, int32_t* seg, int32_t* os_flags, double* err_dr, double* err_fused, double* trace_pos);

// innovation gate (gsf_gate.hip): the body of gsf_innovation_gate_dev, arguments checked by the caller
int launch_innovation_gate(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                           const int64_t* offsets, const int32_t* run_status, const double* init_pos, const double* init_quat,
                           const gsf_ekf_config* cfg, int64_t B, const double* gates, int32_t K, double arm_seconds, int32_t max_run,
                           uint8_t* valid_out, double* nis_out, double* stats, int32_t* gate_status);

// local Sim3 alignment (gsf_local.hip): the bodies of gsf_sim3_local_fit_dev / gsf_sim3_local_apply_dev, arguments checked by the caller
int launch_local_fit(gsf_ctx* ctx, const double* ts, const double* pos, const double* gps, const uint8_t* valid, const int64_t* offsets,
                     int64_t B, const double* R, const double* t, const double* s, const gsf_local_config* cfg, int32_t Kmax, double* knot_R,
                     double* knot_t, double* knot_s, int32_t* knot_n, double* knot_rms, int32_t* knot_flags, int32_t* n_knots,
                     int32_t* track_status);
int launch_local_apply(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* offsets, int64_t B, const double* R,
                       const double* t, const double* s, double spacing, int32_t Kmax, const double* knot_R, const double* knot_t,
                       const double* knot_s, const int32_t* knot_flags, const int32_t* n_knots, const int32_t* track_status, double* pos_out,
                       double* quat_out, double* scale_at, int32_t* pose_flags);

// antenna lever arm (gsf_lever.hip): the bodies of gsf_lever_fit_dev / gsf_lever_apply_dev, arguments checked by the caller
int launch_lever_fit(gsf_ctx* ctx, const double* pos, const double* quat, const double* gps, const uint8_t* valid, const int64_t* offsets, int64_t B,
                     const double* R, const double* t, const double* s, const double* l0, const int32_t* run_status, const gsf_lever_config* cfg,
                     double* R_out, double* t_out, double* s_out, double* l_out, double* l_cov, int32_t* n_rows, int32_t* n_bad_quat,
                     double* rms_before, double* rms_after, double* last_step, int32_t* flags);
int launch_lever_apply(gsf_ctx* ctx, const double* quat, const double* xyz, const int64_t* offsets, int64_t B, const double* R, const double* l,
                       double sign, double* xyz_out, int32_t* pose_flags);
// robust smoothing: the weighted smoother with Huber / Cauchy reweighting rounds in one launch (gsf_smooth.hip, ekf_smooth_kernel<SMOOTH_REWEIGHTED>)
int launch_ekf_smooth_reweighted(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                                 const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                                 const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, int32_t loss, double c2, int32_t rounds,
                                 double* pos_out, double* quat_out, double* cov_out, double* pos_filt, double* cov_filt, uint8_t* pose_flags,
                                 int32_t* status, double* nis, double* weight, int32_t* rounds_used, double* w_change);
// per-fix GNSS noise: the weighted whole-track smoother (gsf_smooth.hip, ekf_smooth_kernel<SMOOTH_WEIGHTED>), and per-fix variances carried onto SLAM stamps (gsf_weighted.hip)
int launch_ekf_smooth_weighted(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                               const double* meas_var, const int64_t* offsets, const double* init_pos, const double* init_quat,
                               const int32_t* run_status, const gsf_ekf_config* cfg, int64_t B, double* pos_out, double* quat_out, double* cov_out,
                               double* pos_filt, double* cov_filt, uint8_t* pose_flags, int32_t* status, double* nis);
int launch_fix_var_at_poses(gsf_ctx* ctx, const double* ts, const int64_t* slam_offsets, const double* gps_t, const int64_t* gps_offsets,
                            const uint8_t* gps_keep, const double* fix_var, const uint8_t* valid, int64_t B, int64_t P, double* pose_var);

// filter_gps_outliers_ransac as a whole, windows found on the device (gsf_gpsfilter.hip); counts (may be NULL): log b = rows offsets[b] .. +counts[b]
int check_gps_prefilter(const gsf_prefilter_config* f, int32_t max_log_rows, int64_t B, int* jseq_elems = nullptr, size_t* lds = nullptr);
int launch_gps_prefilter_auto(gsf_ctx* ctx, const double* t, const double* pos, const int64_t* offsets, const int32_t* counts, int64_t B,
                              int32_t max_log_rows, const gsf_prefilter_config* f, uint32_t* mt_state, uint8_t* keep, int32_t* log_status, int32_t* log_info);

// step 6 for raw SLAM / Sim3 / EKF in one launch (gsf_eval.hip): stats[3][B][4], errors[3][B][N]
int launch_apply_sim3(gsf_ctx* ctx, const double* pos, const double* quat, const int64_t* offsets, int64_t B, const double* R, const double* t,
                      const double* s, double* pos_out, double* quat_out, int32_t* bad_quat, bool bad_quat_zeroed);
// (offsets: a ragged batch, trajectory b = rows offsets[b] .. offsets[b + 1], N >= the longest; errors then [3][offsets[B]])
int launch_eval_errors3(gsf_ctx* ctx, const double* ts, const double* traj0, const double* traj1, const double* traj2, const double* aligned_gps,
                        const uint8_t* valid, int64_t B, int64_t N, double skip_seconds, double* stats, double* errors,
                        const int64_t* offsets = nullptr, int64_t total_rows = 0);

// steps 3-5 of the robust chain (gsf_robust.hip): the body of gsf_fuse_pipeline_robust_info_batch_dev; offsets == NULL: B x N rows, else
// trajectory b = rows offsets[b] .. offsets[b + 1] of total_rows, N >= the longest (host-known: sizes the draws' LDS)
int robust_chain(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const double* gps, const uint8_t* valid,
                 const gsf_ekf_config* cfg, int64_t B, int64_t N, const int64_t* offsets, int64_t total_rows, int32_t min_samples,
                 double residual_threshold, int32_t max_trials, int32_t min_inliers_needed, uint32_t* mt_state, double* R, double* t, double* s,
                 double* pos_out, double* quat_out, int32_t* status, int32_t* n_inliers, uint8_t* inlier_mask, int32_t* trial_info);

// main_process_gui's row choice as a launch of its own (gsf_robust.hip: sim3_rows_kernel; ref :973-998): row_mask[B*N] / ragged, n_rows[B], status[B]
int launch_sim3_rows(gsf_ctx* ctx, const double* ts, const double* gps, const uint8_t* valid, const int64_t* offsets, int64_t B, int64_t N,
                     const FitRows& rule, uint8_t* row_mask, int32_t* n_rows, int32_t* status);

// K2b launch with optional per-set row counts (sets in fixed-stride slots: rows offsets[b] .. offsets[b] + counts[b])
int launch_sim3_ransac(gsf_ctx* ctx, const double* src, const double* dst, const int64_t* offsets, const int32_t* counts, int64_t B,
                       const int32_t* sample_idx, int32_t trials, int32_t min_samples, double thr, int32_t min_inliers, double* R, double* t,
                       double* s, int32_t* status, uint8_t* inlier_mask, int32_t* n_inliers,
                       int64_t total_rows = 0 /* rows of src / dst if the host knows them: enables the single-precision screen */,
                       int32_t trial0 = 0 /* hypotheses below this one were scored by the early-exit probe (gsf_robust.hip) ... */,
                       unsigned long long* keys_io = nullptr /* ... whose arg-max key per set comes in here ([B][2]) and the merged one goes out */,
                       const int32_t* decided = nullptr /* ... and sets it decided (a trial counted every row, ref :413) are not scanned again */);
// sample sets of the reference's RNG call, generated on the device (gsf_rng.hip): permutation(n_b)[:k] per trial from each set's
// legacy MT19937 state; n_b = counts[b] (int32) -- asynchronous on the context's stream
int launch_mt_choice(gsf_ctx* ctx, uint32_t* state, const int32_t* counts, int64_t B, int32_t trials, int32_t k, int32_t* sample_idx,
                     int32_t n_max /* largest counts[b] if the host knows it, else 0 */);
int launch_mt_choice_rest(gsf_ctx* ctx, uint32_t* state, const int32_t* counts, int64_t B, int32_t total_trials, int32_t trial0, int32_t k,
                          int32_t* sample_idx, int32_t n_max, const int32_t* skip);
// the same draws for a few streams, spread over the chip (gsf_rng_tape.hip); launch_mt_choice picks it when mt_tape_applies
bool mt_tape_applies(const gsf_ctx* ctx, int64_t B, int32_t trials, int32_t k, int32_t n_max);
int launch_mt_tape(gsf_ctx* ctx, uint32_t* state, const int32_t* counts, int64_t B, int32_t trials, int32_t k, int32_t* sample_idx, int32_t n_max,
                   const int32_t** done_flags, int* done_stride);

// Staging of the host-pointer entry points.  ONE grow-only device arena per context plus a pinned host mirror of it: the
// inputs of a call are packed into the mirror and cross PCIe in one hipMemcpyAsync, the outputs come back in one, and no call
// pays hipMalloc/hipFree (which synchronise the device).  Calls whose arrays exceed PINNED_MAX copy straight from/to the caller's
// pageable arrays instead (a bulk transfer, where the extra host memcpy would cost more than the runtime's own staging).
// Declare, then commit: an entry declares its arrays (in any order) and gets a handle for each; upload() lays the arena out from what was
// declared (stage_plan, gsf_stage_plan.hpp), grows it, packs and sends the inputs, and a handle converts to its device pointer only after
// that: nothing is sized by hand.  The host arrays an entry declares are read in upload(), so they must live until then.
//   in / out: a caller's array of n elements; a NULL host pointer still gets a device block (an input that is not copied in, an output that is
//   scratch and not copied back).  in_opt / out_opt: a NULL host pointer gives a NULL device pointer.  tmp: scratch.  inout: staged as an input
//   and as an output, upload() copies the one onto the other on the device; the handle is the output's.  bind: upload() writes the handle's
//   device pointer into a field (entries that hand a struct of pointers on).
// Order of use: declarations; upload(); launches; finish().  A full table makes upload() fail with GSF_ERR_INVALID_ARG.
class Staging {
public:
    static constexpr size_t PINNED_MAX = (size_t)32 << 20;
    template <class T> struct Handle {
        const Staging* st = nullptr; int idx = -1;
        operator T*() const { return idx < 0 ? nullptr : (T*)(st->d_ + st->tab_.b[idx].off); }
    };
    explicit Staging(gsf_ctx* ctx) : ctx_(ctx) {}
    template <class T> Handle<const T> in(const T* host, size_t n) { return { this, add((void*)host, n * sizeof(T), STAGE_IN) }; }
    template <class T> Handle<const T> in_opt(const T* host, size_t n) { return host ? in(host, n) : Handle<const T>{}; }
    template <class T> Handle<T> out(T* host, size_t n) { return { this, add(host, n * sizeof(T), STAGE_OUT) }; }
    template <class T> Handle<T> out_opt(T* host, size_t n) { return host ? out(host, n) : Handle<T>{}; }
    template <class T> Handle<T> tmp(size_t n) { return { this, add(nullptr, n * sizeof(T), STAGE_TMP) }; }
    template <class T> Handle<T> inout(T* host, size_t n) { return { this, add(host, n * sizeof(T), STAGE_OUT, add(host, n * sizeof(T), STAGE_IN)) }; }
    template <class T> void bind(T*& field, Handle<T> h) { if (h.idx >= 0) bind_[h.idx] = (void**)&field; else field = nullptr; }
    int upload();      // lay out, grow, pack, one H2D (+ the in-out copies); handles are valid afterwards
    int finish();      // device -> caller arrays, then hipStreamSynchronize

private:
    int add(void* host, size_t bytes, int kind, int from = -1);   // from: the block that upload() copies onto this one (inout)
    gsf_ctx* ctx_; char* d_ = nullptr; char* h_ = nullptr; bool direct_ = false; int rc_ = GSF_OK;
    StageTable tab_; StagePlan plan_{}; void* host_[STAGE_MAX_BLOCKS]; void** bind_[STAGE_MAX_BLOCKS]; int from_[STAGE_MAX_BLOCKS];
};

// host-pointer forms: declare -> upload (pack, one H2D) -> *_dev launch -> finish (one D2H, synchronise)
#define ST_UPLOAD() do { int rc__ = st.upload(); if (rc__) return rc__; } while (0)
#define ST_RUN(call) do { ST_UPLOAD(); int rc__ = (call); if (rc__) return rc__; return st.finish(); } while (0)

int launch_transpose_set(gsf_ctx* ctx, bool to_time, int n, const void* const* src, void* const* dst, const int* C, const int* elem_bytes, int64_t B, int64_t N);
}  // namespace gsf
