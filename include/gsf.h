/*
 * gsf.h -- C ABI of libgsf.so: the MI355X (gfx950) GPS<->SLAM trajectory-fusion hot path.
 *
 * The reference (A2ureeE/GPS-optimize-SLAM) has no FFI: its hot path sits behind
 * module-level Python functions of EKFGPSSLAM.py.  Each entry point below names the
 * reference function (file:line) whose arithmetic it replaces; the Python module
 * gps_optimize_slam_amd.ekfgpsslam binds them with ctypes and re-exports the reference's
 * own function names (INTEGRATION.md shows the stub a maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is caller-owned, the library never
 *     retains or frees it.  All floating-point arrays are IEEE float64 and results are those of
 *     float64 arithmetic (gsf_set_option "k2b_screen" describes the one internal exception).  Quaternions are
 *     scalar-last [x,y,z,w] (SciPy convention, as in the reference's TUM files).
 *   - `*_dev` entry points take DEVICE pointers and are asynchronous on the context's
 *     HIP stream; the matching host-pointer entry points copy in/out and synchronise.
 *   - return value: 0 = GSF_OK, otherwise a gsf_error; gsf_last_error() gives the
 *     thread-local message.  Per-item results (the reference's `None` returns, outage
 *     bookkeeping) come back in `status` arrays, never as failures of the call.
 *   - there is NO CPU fallback: without a HIP device gsf_create fails.
 */
#ifndef GSF_H
#define GSF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSF_ABI_VERSION 1

#if defined(__GNUC__)
#define GSF_API __attribute__((visibility("default")))
#else
#define GSF_API
#endif

typedef enum {
    GSF_OK = 0,
    GSF_ERR_INVALID_ARG = 1,
    GSF_ERR_HIP = 2,
    GSF_ERR_NO_DEVICE = 3,
    GSF_ERR_UNSUPPORTED = 4
} gsf_error;

/* batch memory layouts of the fusion kernels */
typedef enum {
    /* trajectory-major AoS (what B stacked TUM files look like):
       ts[B][N] pos[B][N][3] quat[B][N][4] gps[B][N][3] valid[B][N], outputs alike */
    GSF_LAYOUT_TRAJ_MAJOR = 0,
    /* time-major SoA (trajectory index fastest: every wave access is one contiguous 512-B row):
       ts[N][B] pos[N][3][B] quat[N][4][B] gps[N][3][B] valid[N][B], outputs alike */
    GSF_LAYOUT_TIME_MAJOR = 1
} gsf_layout;

/* CONFIG['ekf'] + CONFIG['rts_decision'] of the reference (EKFGPSSLAM.py:24-29, :67-70).
   Stated range of the noise values, per position axis (P0 = initial_cov_diag, Q = process_noise_diag, R = meas_noise_diag, dt = the step
   between two stamps in whatever unit the stamps are in, clamped to 1e-6 from below):
       0 <= P0 <= 1e8,   1e-8 <= R <= 1e8,   0 <= Q dt <= 1e14,   finite inputs.
   Inside it every route -- wave, two-wave, big-batch, early-variance, block, lane kernel, the covariance entry -- agrees with the oracle to
   the stated gates (1e-6 m, status words exact; variances 1e-10 relative): tests/test_ekf_noise_domain.py.  The scan-based routes scale
   every step matrix of their variance scans by a power of two, so the range does not depend on how Q dt and R compare or on the time unit
   of the stamps.  Outside the range the behaviour is undocumented.
   The sharp-turn threshold thr (rad/s after deg2rad), with dt the step between two poses of an outage: thr < 0 makes every outage of two or
   more poses a sharp turn (no RTS), also one whose stamps all repeat (:813, :826); thr dt >= pi can never be exceeded; between, every route
   decides a pair like the reference's atan2 form down to thr dt = 1e-7, unless its rate is closer to thr than the float64 error of the yaw
   angles themselves ("Domain of the sharp-turn gate"; tests/test_sharp_turn_gate.py). */
typedef struct {
    double initial_cov_diag[7];        /* :25 */
    double process_noise_diag[7];      /* :26  per second, used as variances */
    double meas_noise_diag[3];         /* :27  used as variances (Q4) */
    double sharp_turn_yaw_rate_threshold_deg_per_sec;   /* :68 */
    int32_t default_ekf_transition_steps_on_sharp_turn; /* :69 */
    int32_t reserved;
} gsf_ekf_config;

/* CONFIG['gps_filtering_ransac'] / CONFIG['ground_truth_gps_filtering'] of the reference (EKFGPSSLAM.py:39-48, :55-64) */
typedef struct {
    int32_t enabled;                   /* :40  0: the log passes unfiltered and nothing is drawn (:139-141) */
    int32_t use_sliding_window;        /* :41  0: one fit over the whole log (:148-182) */
    double window_duration_seconds;    /* :42 */
    double window_step_factor;         /* :43 */
    int32_t polynomial_degree;         /* :44 */
    int32_t min_samples;               /* :45 */
    double residual_threshold_meters;  /* :46 */
    int32_t max_trials;                /* :47 */
    int32_t max_windows;               /* not a reference value: cap on the windows the device loop visits per log (0 = 4096) */
    double stop_probability;           /* scikit-learn's RANSACRegressor default 0.99 (0 = that) */
} gsf_prefilter_config;

/* everything main_process_gui reads from CONFIG between its step 1 and its step 6 (EKFGPSSLAM.py:22-71) */
typedef struct {
    gsf_ekf_config ekf;                /* :24-29, :67-70 */
    gsf_prefilter_config gps_filter;   /* :39-48 */
    double sim3_residual_threshold;    /* :34 */
    double sim3_max_initial_duration;  /* :37 */
    double max_gps_gap_threshold;      /* :53 */
    double eval_skip_seconds;          /* 5.0, literal in :1018 */
    int32_t sim3_min_samples;          /* :33 */
    int32_t sim3_max_trials;           /* :35 */
    int32_t sim3_min_inliers_needed;   /* :36 */
    int32_t reserved;
} gsf_run_config;

/* per-trajectory outcome of gsf_run_fusion_batch_dev: where the reference's run would have stopped */
#define GSF_RUN_OK 0
#define GSF_RUN_GPS_EMPTY 1            /* no GNSS row passes the lat/lon range mask: load_gps_data raises ValueError (EKFGPSSLAM.py:264) */
#define GSF_RUN_GPS_FEW 2              /* fewer than 2 fixes left after the pre-filter: ValueError (:283, :967) */
#define GSF_RUN_PREFILTER_UNHANDLED 4  /* the device pre-filter does not cover this log (unsorted stamps in the sliding-window mode, more than
                                          max_windows windows): NaN outputs; the caller runs that track through the host route from its saved
                                          generator state.  Every ratio min_samples / n of scikit-learn's sampler is covered (permutation,
                                          tracking selection, n == min_samples) */
#define GSF_RUN_SIM3_FAILED 8          /* ValueError of the row choice (:975, :997) or RuntimeError of the failed fit (:1003): see status >> 8 */
#define GSF_RUN_BAD_QUAT 16            /* a SLAM quaternion of the track cannot be normalised: SciPy raises in transform_trajectory (:466) */
/* set only by gsf_run_fusion_ragged[_dev] (the optional ground-truth log of :962-966, the empty SLAM track of :967) */
#define GSF_RUN_GT_EMPTY 32            /* no ground-truth row passes the lat/lon range mask: load_gps_data raises, the whole run fails (:264, :964) */
#define GSF_RUN_GT_FEW 64              /* fewer than 2 ground-truth fixes left after its pre-filter: load_gps_data raises (:283; :966 is never reached) */
#define GSF_RUN_GT_UNHANDLED 128       /* the device pre-filter does not cover the ground-truth log (as GSF_RUN_PREFILTER_UNHANDLED) */
#define GSF_RUN_SLAM_EMPTY 256         /* a SLAM track with 0 poses: ValueError at :967, after both logs were loaded and filtered */

/* status of a Sim3 fit: GSF_SIM3_NONE <=> the reference returned (None, None, None) */
#define GSF_SIM3_OK 0
#define GSF_SIM3_NONE 1
#define GSF_SIM3_FLAG_VAR0 2          /* var_src < 1e-12 -> scale := 1   (EKFGPSSLAM.py:445-447) */
#define GSF_SIM3_FLAG_SMALL_SCALE 4   /* scale <= 1e-6  -> scale := 1   (EKFGPSSLAM.py:450) */
#define GSF_SIM3_FLAG_BAD_INDEX 8     /* a caller-fed sample set named a row outside [0, n): that trial was skipped */
#define GSF_SIM3_FLAG_SVD_FALLBACK 16 /* informational (fused pipeline): the closed form's rotation came from the Jacobi SVD because the
                                         polar iteration declined this cross-covariance (rank-deficient / weakly separated reflection);
                                         same result to ~1e-14, only slower */
/* row choice of the fused chains under gsf_set_sim3_rows mode 1 (main_process_gui, EKFGPSSLAM.py:973-998) */
#define GSF_SIM3_FLAG_FEW_ROWS 32     /* fewer than min_samples time-synchronised rows: the reference raises ValueError (:975, :997);
                                         comes with GSF_SIM3_NONE, NaN outputs, and (robust chain) an untouched generator */
#define GSF_SIM3_FLAG_ROWS_ALL 64     /* informational: the first gap-free segment is shorter than min_samples -> all valid rows (:984-986) */
#define GSF_SIM3_FLAG_ROWS_SEGMENT 128 /* informational: fewer than min_samples rows inside max_initial_duration -> the whole first segment (:993-995) */
/* robust chain with gsf_set_option "ransac_early_exit" 1 (compute_sim3_transform_robust, EKFGPSSLAM.py:404-414) */
#define GSF_SIM3_FLAG_SATURATED 256   /* informational: a trial counted EVERY row of the fit, so by the strict '>' of :413 no later trial could
                                         have replaced it and the trajectory stopped drawing there: R, t, s, inlier mask, n_inliers and
                                         the fused poses are the all-max_trials result bit for bit; only its generator was advanced by
                                         fewer trials (trial_info of gsf_fuse_pipeline_robust_info_batch_dev says how many) */

/* status bits of a fused trajectory */
#define GSF_ST_HAD_OUTAGE 1
#define GSF_ST_RTS_APPLIED 2
#define GSF_ST_SHARP_TURN 4
#define GSF_ST_ENDED_IN_OUTAGE 8
#define GSF_ST_BAD_QUAT 16            /* a zero/NaN SLAM quaternion took the zero-motion branch (:84-86) */

typedef struct gsf_ctx gsf_ctx;       /* opaque: device id + HIP stream + scratch */

/* ---- context ------------------------------------------------------------------------- */
GSF_API const char *gsf_version(void);
GSF_API int gsf_abi_version(void);
/* copies the calling thread's last error message (NUL-terminated) into buf; returns its length */
GSF_API int gsf_last_error(char *buf, int n);
/* number of HIP devices visible (0 if none / no driver) */
GSF_API int gsf_device_count(void);
/* creates a context on `device_id` with its own non-blocking stream */
GSF_API int gsf_create(int device_id, gsf_ctx **out);
/* same, but launches on a caller-owned hipStream_t (e.g. torch's current stream); not destroyed by gsf_destroy */
GSF_API int gsf_create_on_stream(int device_id, void *hip_stream, gsf_ctx **out);
GSF_API void gsf_destroy(gsf_ctx *ctx);
GSF_API int gsf_synchronize(gsf_ctx *ctx);
/* Workspaces.  A context owns grow-only device arenas that are kept between calls (no call pays hipMalloc / hipFree once they have
   grown): the kernel workspace (time alignment slabs, the transposed copy of a small time-major batch: 145 B/pose; the robust chain:
   ~54 B/pose + 4 B x max_trials x min_samples per trajectory), the staging arena + pinned mirror of the host-pointer entry points
   (the size of the largest call, up to 32 MB pinned), the float rows of the K2b screen (28 B per row + 25 %) and -- chosen
   automatically for <= 16 MT19937 streams of <= 2 040 rows -- the tape and transition tables of the chip-wide draws (up to 768 MB,
   960 MB with the growth margin; a few MB at the reference's own shape of one stream of 271 rows).  gsf_trim synchronises the stream
   and releases all of them (they grow again on demand); call it before sizing a large allocation to what the device has free.
   A hipGraph captured from calls on this context holds workspace addresses as kernel arguments: after gsf_trim -- and after any call
   that made a workspace grow -- such a graph must be captured again before it is replayed. */
GSF_API int gsf_trim(gsf_ctx *ctx);
/* tuning knobs; keys:
     "duo_kernel"     -1 automatic (default) / 0 never / 1 always: two-wave build of the fused pipeline for small batches of short tracks
     "tail_scan_stages"  1 (default): the wave-per-trajectory kernels run the scans of a track's last chunk with the stages that reach its
                      lanes only (4 of 6 for a tail of <= 16 poses, 5 for <= 32; equal-length batches of up to 2 048 tracks) / 0: always six stages.  Bit-identical results; the
                      switch exists so that both paths can be compared inside one build
     "early_variances"  -1 automatic (default) / 0 never / 1 always where the build applies: the one-wave build of the fused pipeline that computes
                      its first chunk's variances from stamps and mask bytes while the rest of the track's rows are still in flight (equal-length
                      batches of up to 2 048 tracks of 65..384 poses, x and y sharing their noise and z not -- the default CONFIG; a forced
                      "duo_kernel" 1 goes first).  Bit-identical results; -1 takes the build for 1 000..1 024 tracks of 256..384 poses (measured, see wave_route() in csrc/gsf_wave_route.hpp)
     "lane_min_traj"  time-major batches with fewer trajectories than this (default 32768) are transposed and run by the
                      wave-per-trajectory kernel; 0 = always the lane-per-trajectory kernel
     "block_kernel"   -1 / 0 never (what -1 means today) / 1 whenever it applies: workgroup-per-trajectory EKF kernel for 64 < N <= 1024
                      (under gsf_set_sim3_rows mode 1 its launcher marks the rows of the fit with a launch of their own first)
     "tape_draws"     -1 automatic (default): up to 16 MT19937 streams of <= 2040 rows are drawn chip-wide (csrc/gsf_rng_tape.hip) /
                      0 always one wave per stream / 2 tests only (a tape cut short: the one-wave kernel must take over)
     "k2b_screen"     1 (default): the residual counts of the RANSAC hypotheses are screened in packed single precision and re-checked in
                      double inside the rounding band (identical counts) / 0: double throughout.  The band carries 1e-6 m of slack for
                      the double path's own rounding, which covers coordinates up to ~1e9 m in magnitude (UTM: 1e7); rows beyond
                      that should be fitted with the screen off
     "ransac_early_exit"  0 (default): every trajectory of the robust chain draws and scores all max_trials hypotheses, so its generator
                      ends where np.random ends after compute_sim3_transform_robust (EKFGPSSLAM.py:404-405) / 1: a trajectory stops at
                      the first trial that counts every row of its fit -- :413 keeps a trial only on a STRICTLY larger count, so no later
                      trial can change the mask, the count or the final fit; outputs identical bit for bit, GSF_SIM3_FLAG_SATURATED in the
                      status word, the generator left after the round of eight trials that held the deciding one.  A trajectory that
                      never saturates (one GNSS outlier beyond the threshold among its rows is enough) runs all max_trials as before.
                      The Python batch binding switches it ON, the single-track drop-in never uses it
     "ransac_probe_trials"  (default 64) how many trials the early-exit probe draws and scores per trajectory (one wave each) before
                      the wide kernels take the rest of an undecided trajectory's trials
     "prefilter_speculate"  1 (default): the GPS pre-filter chain (gsf_gps_prefilter_chain_*, gsf_gps_prefilter_auto_dev, the whole-run entries)
                      first tries "every axis of the window stops after its first trial" -- three consecutive trials drawn, fitted and
                      counted at once; an axis whose first trial does not end RANSACRegressor's loop goes through the sequential walk
                      from the stream position where it starts.  0: the sequential walk only.  Same kept rows, same generator state.
     "prefilter_miss_batch"  (default 4, 1..64) after the speculative pass has missed at an axis, its first trial says how many trials
                      RANSACRegressor will want unless a later one counts more rows: the sequential walk opens with a batch of that many,
                      at most this value (a poor first sample asks for many; a better one among the next few shrinks that).  Same words.
     "prefilter_first_batch"  (default 1, 1..64) trials the sequential walk draws and scores before its first look at scikit-learn's
                      stopping rule (the batches then double); any value gives the same words, clean logs are fastest with 1
     "synth_variant"  workload of gsf_synth_batch: 0 white SLAM noise (default), 1 random-walk drift
     "poison_workspaces"  tests only.  -1 (default): off, no cost anywhere / v in [0, 255]: EVERY call of the option (also with the value it
                      has) fills every workspace the context holds at that moment -- kernel, RNG, K2b, rows and run workspaces, the
                      staging arena (device, on the context's stream) and its pinned mirror (on the host, after synchronising the
                      stream) -- with the 64-bit word v repeated, and while it is on a workspace that grows is filled the same way right
                      after its allocation.  No call keeps state in a workspace from one call to the next, so results must not depend on
                      it (tests/test_buffer_hygiene.py).  The word reads as a small number through every type, so a kernel that
                      does read a count or an offset nobody wrote gives a wrong value, not a wild address
     "noise_sweep_group"  0 automatic (default): gsf_ekf_noise_sweep_dev splits its K candidates into just enough equal groups to put 2 048
                      waves on the chip, at most 64 candidates per wave (sweep_group() in csrc/gsf_wave_route.hpp) / 1..64: that many
                      candidates per wave.  Bit-identical results
     "ekf_variant"    reserved (0) */
GSF_API int gsf_set_option(gsf_ctx *ctx, const char *key, int64_t value);
/* Which rows feed the Sim3 fit of the fused chains (gsf_fuse_pipeline_*, gsf_fuse_pipeline_robust_*, gsf_run_fusion_batch_*) on this context
   from now on.  A context STARTS in mode 1 with the reference's CONFIG defaults (min_samples 4, max_gps_gap_threshold 5.0 s,
   max_initial_duration 180.0 s; EKFGPSSLAM.py:34, :53, :37), so a caller that sets nothing gets steps 3-5 as main_process_gui runs them;
   the Python binding (batch.py, fit_rows="reference") sets the same mode from its CONFIG dict on every call.
     mode 0            every row with valid, finite GNSS (the operator SURVEY 8(b)/(d) defined for the batch configs)
     mode 1 (default)  what main_process_gui does between its alignment and its fit (EKFGPSSLAM.py:973-998): of the valid rows V (in row
                       order), the rows before the first k with ts[V[k+1]] - ts[V[k]] > max_gps_gap_threshold -- V[k] itself is left out,
                       :981-982 -- or all of V when there is no such k; if those are fewer than min_samples: all of V (:984-986); else
                       the rows of that segment with ts <= ts[V[0]] + max_initial_duration, or the whole segment when fewer than
                       min_samples of them remain (:988-996).  Fewer than min_samples valid rows: the reference raises ValueError
                       (:975, :997) -> GSF_SIM3_NONE | GSF_SIM3_FLAG_FEW_ROWS in the status word.
   min_samples = CONFIG['sim3_ransac']['min_samples'], the other two CONFIG['time_alignment'] / CONFIG['sim3_ransac'] values. */
GSF_API int gsf_set_sim3_rows(gsf_ctx *ctx, int32_t mode, int32_t min_samples, double max_gps_gap_threshold, double max_initial_duration);
/* The same choice on its own, for B trajectories of N rows (offsets == NULL) or ragged ones (rows offsets[b]..offsets[b+1], N ignored):
   row_mask[total] = 1 on the chosen rows, n_rows[b] their number (-1 where the reference raises ValueError), status[b] (may be NULL) the
   GSF_SIM3_FLAG_FEW_ROWS / _ROWS_ALL / _ROWS_SEGMENT bit.  A row is "valid" when valid[i] != 0 and -- if gps != NULL -- its fix is
   free of NaN (what the fused chains use).  Device pointers, asynchronous. */
GSF_API int gsf_sim3_fit_rows_batch_dev(gsf_ctx *ctx, const double *ts, const double *gps, const uint8_t *valid, const int64_t *offsets,
                                        int64_t B, int64_t N, int32_t min_samples, double max_gps_gap_threshold,
                                        double max_initial_duration, uint8_t *row_mask, int32_t *n_rows, int32_t *status);
GSF_API int gsf_sim3_fit_rows_batch(gsf_ctx *ctx, const double *ts, const double *gps, const uint8_t *valid, const int64_t *offsets,
                                    int64_t B, int64_t N, int32_t min_samples, double max_gps_gap_threshold, double max_initial_duration,
                                    uint8_t *row_mask, int32_t *n_rows, int32_t *status);                     /* host arrays */
/* opens / closes a HIP-event bracket on the context's stream; gsf_timer_stop returns the elapsed ms */
GSF_API int gsf_timer_start(gsf_ctx *ctx);
GSF_API int gsf_timer_stop(gsf_ctx *ctx, float *elapsed_ms);

/* ---- K1: WGS84 -> UTM  (replaces pyproj Proj(...)(lons, lats), EKFGPSSLAM.py:266-271) ------ */
/* zone/hemisphere pick of auto_utm_projection (EKFGPSSLAM.py:127-134), one per trajectory:
   zone = int((mean(lon)+180)//6+1), south = mean(lat) < 0.  offsets: int64[B+1] into lat/lon. */
GSF_API int gsf_utm_zone_batch_dev(gsf_ctx *ctx, const double *lat_deg, const double *lon_deg, const int64_t *offsets,
                           int64_t B, int32_t *zone, int32_t *south);
/* forward projection of B ragged trajectories, each in its own zone; invalid input rows
   (EKFGPSSLAM.py:259: |lat|>90, |lon|>180, lat==0, lon==0) produce NaN */
GSF_API int gsf_utm_forward_batch_dev(gsf_ctx *ctx, const double *lat_deg, const double *lon_deg, const int64_t *offsets,
                              const int32_t *zone, const int32_t *south, int64_t B, double *easting, double *northing);
/* inverse projection (utm_to_wgs84, EKFGPSSLAM.py:291-296) */
GSF_API int gsf_utm_inverse_batch_dev(gsf_ctx *ctx, const double *easting, const double *northing, const int64_t *offsets,
                              const int32_t *zone, const int32_t *south, int64_t B, double *lat_deg, double *lon_deg);
/* host-pointer, single-zone convenience forms used by the drop-in load_gps_data / utm_to_wgs84 */
GSF_API int gsf_utm_forward(gsf_ctx *ctx, const double *lat_deg, const double *lon_deg, int64_t n, int32_t zone, int32_t south,
                    double *easting, double *northing);
GSF_API int gsf_utm_inverse(gsf_ctx *ctx, const double *easting, const double *northing, int64_t n, int32_t zone, int32_t south,
                    double *lat_deg, double *lon_deg);

/* The whole geodesy slice of load_gps_data (EKFGPSSLAM.py:258-271) for B ragged GNSS logs in one launch: rows llh[total][3] =
   (lat deg, lon deg, alt m) -- columns 1,2,3 of the reference's text file -- are masked (:259-264), each log's zone / hemisphere
   is picked from the means over its valid rows (:131-133), and rows utm_rows[total][3] = (E, N, alt) come back (:271).  Rows the
   reference drops are NaN rows here (a device array cannot shrink); zone[b] = 0 for a log without a valid row. */
GSF_API int gsf_gps_rows_to_utm_batch_dev(gsf_ctx *ctx, const double *llh, const int64_t *offsets, int64_t B, double *utm_rows, int32_t *zone,
                                          int32_t *south);
GSF_API int gsf_gps_rows_to_utm_batch(gsf_ctx *ctx, const double *llh, const int64_t *offsets, int64_t B, double *utm_rows, int32_t *zone,
                                      int32_t *south);                                   /* the same with host arrays */

/* WGS84 geodetic -> local East-North-Up about a per-trajectory origin ref_llh[B][3] = (lat0 deg, lon0 deg, h0 m).  Offered in
   addition to UTM: the reference's pipeline projects with UTM (EKFGPSSLAM.py:266-271); BASELINE.json words the step as
   "WGS84 -> local ENU". */
GSF_API int gsf_geodetic_to_enu_batch_dev(gsf_ctx *ctx, const double *lat_deg, const double *lon_deg, const double *alt, const int64_t *offsets,
                                          const double *ref_llh, int64_t B, double *east, double *north, double *up);
GSF_API int gsf_geodetic_to_enu_batch(gsf_ctx *ctx, const double *lat_deg, const double *lon_deg, const double *alt, const int64_t *offsets,
                                      const double *ref_llh, int64_t B, double *east, double *north, double *up);   /* host arrays */

/* ---- next-3: GPS outlier pre-filter (filter_gps_outliers_ransac, EKFGPSSLAM.py:136-247) ------------------------------------
   One problem = one RANSACRegressor.fit of the reference (one window x one coordinate axis): rows offsets[p]..offsets[p+1] of
   (t, y).  sample_idx[P][max_trials][min_samples] are the sample sets of every trial, drawn by the host with scikit-learn's
   sample_without_replacement on NumPy's legacy RNG (the call of sklearn/linear_model/_ransac.py), so a seeded run reproduces the
   reference.  Per problem: inlier_mask over its rows (|y - poly(t)| <= residual_threshold for the accepted model), n_trials (the
   number of sample sets scikit-learn's loop would have consumed: acceptance rule + dynamic trial count with stop_probability),
   n_inliers, status (bit 0: no consensus set -- the reference's ValueError; bit 1: a fed sample set named a row outside the problem
   and was skipped).  degree 1..8, min_samples <= 64, max_trials <= 2^20; inside degree <= 3, min_samples <= 16, max_trials <= 1024
   one thread scores one trial in one pass, beyond that a slower kernel strides the trials (per-trial results in the context's
   workspace).
   DOMAIN OF THE FIT (every pre-filter entry: this one, gsf_gps_prefilter_chain*, gsf_gps_prefilter_auto_dev, the whole-run entries).
   Fit and prediction run in WINDOW-LOCAL TIME: the stamp of the first row of the problem (here) or of the window (the chain) is
   subtracted from every stamp where it is loaded, so the outputs do not depend on where the clock's zero lies -- stamps in seconds,
   milliseconds or microseconds, track-relative or Unix.  That first stamp must be FINITE: a NaN or infinite one makes every local stamp,
   every prediction and so every row of the problem / window an outlier (status bit 0 here, win_status 1 in the chain), where a non-finite
   stamp on any other row spoils only the samples that hold it and that row's own residual; the entries do not check stamps, and the
   reference's loader hands on the stamps of the file as they are.  A prediction at stamp t is within C x b(t) of the least-squares polynomial of the
   stored rows, b(t) = u kappa Lambda(t) max|y_i - ybar| + 4 u max|y| (u = 2^-53; kappa: condition of the sample's centred, unit-norm power
   columns in local time; Lambda(t): sum of the prediction's |weights| on the sample's targets; C = 5.44, measured).
   The reference's float64 solve on RAW stamps is not: at Unix magnitude and degree 2 it is tens of metres from that polynomial, so on
   such logs the entries follow the exact fit and the reference does not.  RANK RULE: a power column whose norm after the Gram-Schmidt
   sweep is at most 4 x 2^-52 x min_samples x its norm as loaded counts as dependent and gets coefficient 0 -- a sample with m <= degree
   distinct stamps (a receiver that repeats stamps) gets the least-squares polynomial of degree m - 1; scikit-learn returns the
   minimum-norm solution in its own basis (raw t, t^2, ..), which agrees at the sample's stamps and differs away from them. */
GSF_API int gsf_ransac_poly_batch_dev(gsf_ctx *ctx, const double *t, const double *y, const int64_t *offsets, int64_t P,
                                      const int32_t *sample_idx, int32_t max_trials, int32_t min_samples, int32_t degree,
                                      double residual_threshold, double stop_probability, uint8_t *inlier_mask, int32_t *n_trials,
                                      int32_t *n_inliers, int32_t *status);
GSF_API int gsf_ransac_poly_batch(gsf_ctx *ctx, const double *t, const double *y, const int64_t *offsets, int64_t P,
                                  const int32_t *sample_idx, int32_t max_trials, int32_t min_samples, int32_t degree,
                                  double residual_threshold, double stop_probability, uint8_t *inlier_mask, int32_t *n_trials,
                                  int32_t *n_inliers, int32_t *status);                  /* the same with host arrays */

/* The WHOLE pre-filter of B GNSS logs as one device chain, draws included.  Log b = rows offsets[b]..offsets[b+1] of t[] and
   pos[][3] (UTM E, N, alt); its windows are rows win_rows[2w], win_rows[2w+1] (relative to the log's first row; found by the host
   from the stamps, ref :205-206; one window = the whole log for the global mode, ref :148) for w in win_offsets[b]..win_offsets[b+1].
   Per window, per axis in the reference's order: max_trials sample sets from the log's legacy MT19937 stream (mt_state[B][625],
   in/out) exactly as scikit-learn's sample_without_replacement draws them, RANSACRegressor's acceptance walk, the stream rewound to
   where n_trials_ draws leave it; a failing axis drops its window and consumes nothing further for it (ref :228-229).
   keep[total] = OR over successful windows of the AND over axes; win_status[w] = 0 ok / 1 no consensus / 2 fewer rows than
   min_samples (not processed) / 3 not handled; log_status[b] = 0 (2 is kept for a window the device sampler does not cover, which no
   window of min_samples <= 16 is).  scikit-learn's sampler is restated on all its routes, chosen per window by min_samples / n in double
   precision: permutation(n)[:k] for 0.01 < k/n < 0.99, tracking selection (one randint(n) per selection, duplicates drawn again) for
   k/n <= 0.01, i.e. n >= 100 min_samples, and -- a window of exactly min_samples rows, ratio 1 -- reservoir sampling, which returns rows
   0 .. min_samples-1 without a draw.  max_trials <= 1024, min_samples <= 16, degree <= 3, max_window_rows <= 14000. */
GSF_API int gsf_gps_prefilter_chain_dev(gsf_ctx *ctx, const double *t, const double *pos, const int64_t *offsets, int64_t B,
                                        const int32_t *win_rows, const int64_t *win_offsets, int32_t max_window_rows, int32_t max_trials,
                                        int32_t min_samples, int32_t degree, double residual_threshold, double stop_probability,
                                        uint32_t *mt_state, uint8_t *keep, int32_t *win_status, int32_t *log_status);
GSF_API int gsf_gps_prefilter_chain(gsf_ctx *ctx, const double *t, const double *pos, const int64_t *offsets, int64_t B,
                                    const int32_t *win_rows, const int64_t *win_offsets, int32_t max_window_rows, int32_t max_trials,
                                    int32_t min_samples, int32_t degree, double residual_threshold, double stop_probability,
                                    uint32_t *mt_state, uint8_t *keep, int32_t *win_status, int32_t *log_status);
/* filter_gps_outliers_ransac AS A WHOLE for B logs (EKFGPSSLAM.py:136-247), no host step: the windows are found on the device from the
   stamps the way the reference walks them (:199-234: [w0, w0 + duration) advanced by duration x step_factor, one extra tail window, windows
   with fewer than min_samples rows skipped), or one global window (:148-182; a failing fit passes the log unfiltered), plus the
   reference's early-outs (disabled, fewer rows than min_samples: everything kept, nothing drawn).  Sorted stamps only in the
   sliding-window mode, and at most max_windows windows (log_status 3 otherwise: the log's generator is then not written back);
   max_log_rows >= the longest log, <= 14000.  log_info[B][2] (may be NULL) = { windows fitted, windows that found a consensus }.
   Draws, acceptance walk, generator handling: as gsf_gps_prefilter_chain_dev. */
GSF_API int gsf_gps_prefilter_auto_dev(gsf_ctx *ctx, const double *t, const double *pos, const int64_t *offsets, int64_t B, int32_t max_log_rows,
                                       const gsf_prefilter_config *filter, uint32_t *mt_state, uint8_t *keep, int32_t *log_status,
                                       int32_t *log_info);

/* ---- K2: Sim3 / Umeyama (compute_sim3_transform, EKFGPSSLAM.py:428-459) ------------------- */
/* B ragged point sets: src/dst are [total][3]; offsets int64[B+1].  Optional `mask` (uint8[total], may be NULL)
   selects the rows that take part (used for "valid GNSS only" fits).  Outputs R[B][9] (row-major), t[B][3],
   s[B], status[B]. */
GSF_API int gsf_sim3_umeyama_batch_dev(gsf_ctx *ctx, const double *src, const double *dst, const uint8_t *mask,
                               const int64_t *offsets, int64_t B, double *R, double *t, double *s, int32_t *status);
/* B equal-size windows of W point pairs each (BASELINE config C4: sliding-window re-alignment, 1 M windows of 50 pairs):
   src/dst are [B][W][3], mask (may be NULL) [B][W].  Same results as gsf_sim3_umeyama_batch_dev on offsets b*W; the streaming
   moments pass and the per-window 3x3 SVD run as two launches (a 192-byte record per window in the context's workspace). */
GSF_API int gsf_sim3_umeyama_windows_dev(gsf_ctx *ctx, const double *src, const double *dst, const uint8_t *mask, int64_t B, int32_t W,
                                         double *R, double *t, double *s, int32_t *status);
GSF_API int gsf_sim3_umeyama_windows(gsf_ctx *ctx, const double *src, const double *dst, const uint8_t *mask, int64_t B, int32_t W,
                                     double *R, double *t, double *s, int32_t *status);               /* host arrays */
GSF_API int gsf_sim3_umeyama_batch(gsf_ctx *ctx, const double *src, const double *dst, const uint8_t *mask,
                           const int64_t *offsets, int64_t B, double *R, double *t, double *s, int32_t *status);

/* ---- K2b: RANSAC wrapper (compute_sim3_transform_robust, EKFGPSSLAM.py:389-426) ------------ */
/* sample_idx: int32[B][trials][min_samples], drawn BY THE HOST with the reference's RNG call
   (np.random.choice(n, min_samples, replace=False), :405) so results are reproducible against it.
   inlier_mask: uint8[total] out; n_inliers: int32[B] out (best count, -1 if no trial succeeded). */
GSF_API int gsf_sim3_ransac_batch_dev(gsf_ctx *ctx, const double *src, const double *dst, const int64_t *offsets, int64_t B,
                              const int32_t *sample_idx, int32_t trials, int32_t min_samples, double residual_threshold,
                              int32_t min_inliers_needed, double *R, double *t, double *s, int32_t *status,
                              uint8_t *inlier_mask, int32_t *n_inliers);
/* the same with the number of rows of src / dst (= offsets[B]) known to the HOST: the library can then keep the rows a second time
   as floats in its workspace and SCREEN the residual counts of the hypotheses in packed single precision, re-checking in double
   every row inside the rounding band -- the counts, masks and fits are those of the double count, in ~0.6 of the time
   (gsf_set_option "k2b_screen" 0 switches the screen off).  The host-pointer forms use it by themselves. */
GSF_API int gsf_sim3_ransac_batch_rows_dev(gsf_ctx *ctx, const double *src, const double *dst, const int64_t *offsets, int64_t total_rows,
                                           int64_t B, const int32_t *sample_idx, int32_t trials, int32_t min_samples,
                                           double residual_threshold, int32_t min_inliers_needed, double *R, double *t, double *s,
                                           int32_t *status, uint8_t *inlier_mask, int32_t *n_inliers);
GSF_API int gsf_sim3_ransac_batch(gsf_ctx *ctx, const double *src, const double *dst, const int64_t *offsets, int64_t B,
                          const int32_t *sample_idx, int32_t trials, int32_t min_samples, double residual_threshold,
                          int32_t min_inliers_needed, double *R, double *t, double *s, int32_t *status,
                          uint8_t *inlier_mask, int32_t *n_inliers);

/* The same with the draws made ON THE DEVICE from NumPy's legacy generator state (host pointers; mt_state[B][625] uint32 in/out =
   np.random.get_state()[1:3] per set, see gsf_mt19937_*): one call instead of `trials` host-side np.random.choice calls, and the
   caller's generator ends where the reference leaves it. */
GSF_API int gsf_sim3_ransac_mt_batch(gsf_ctx *ctx, const double *src, const double *dst, const int64_t *offsets, int64_t B, uint32_t *mt_state,
                                     int32_t trials, int32_t min_samples, double residual_threshold, int32_t min_inliers_needed, double *R,
                                     double *t, double *s, int32_t *status, uint8_t *inlier_mask, int32_t *n_inliers);

/* ---- the reference's random draws on the device (np.random.choice(n, k, replace=False), EKFGPSSLAM.py:405) ---------- */
/* state: uint32[B][625] = NumPy's legacy MT19937 state per stream, key[624] then pos -- exactly np.random.get_state()[1:3], so a
   host can hand over its global generator (B = 1) or seed one stream per trajectory.
   gsf_mt19937_seed_batch_dev: np.random.seed(seeds[b]) for every stream.
   gsf_mt19937_choice_batch_dev: sample_idx[b][trial][0..k) = RandomState.permutation(n_population[b])[:k] for `trials`
   consecutive trials of stream b (what np.random.choice(n, k, replace=False) draws; also scikit-learn's
   sample_without_replacement for 0.01 < k/n < 0.99 -- all ratios: gsf_mt19937_sample_without_replacement_batch_dev), the state advanced exactly as NumPy advances it.  Streams with
   n_population[b] < k are left untouched and their sets zero-filled (the reference returns before drawing, :395-397).  n_population[b] <= 28000, k <= 64.
   gsf_mt19937_choice_bounded_batch_dev: the same, with n_max >= every n_population[b] known to the HOST (0 = unknown).  The
   populations live in device memory, so only with this bound can the library size the workspace of the chip-wide route
   (csrc/gsf_rng_tape.hip): up to 16 streams of n_max <= 2040 are then drawn by thousands of waves instead of one wave per stream
   (the reference's own case is ONE stream); results and final states are identical either way.  A stream whose population
   exceeds n_max is drawn by the one-wave route. */
GSF_API int gsf_mt19937_seed_batch_dev(gsf_ctx *ctx, const uint32_t *seeds, int64_t B, uint32_t *state);
GSF_API int gsf_mt19937_choice_batch_dev(gsf_ctx *ctx, uint32_t *state, const int32_t *n_population, int64_t B, int32_t trials,
                                         int32_t k, int32_t *sample_idx);
GSF_API int gsf_mt19937_choice_bounded_batch_dev(gsf_ctx *ctx, uint32_t *state, const int32_t *n_population, int32_t n_max, int64_t B,
                                                 int32_t trials, int32_t k, int32_t *sample_idx);
/* scikit-learn's sample_without_replacement(n_population[b], k) (method "auto", the sampler of RANSACRegressor and of the GPS
   pre-filter) for `trials` consecutive calls on stream b: sample_idx[b][trial][0..k), in the order scikit-learn returns them.  Routed per
   stream by k / n in double precision as scikit-learn routes it: RandomState.permutation(n)[:k] for 0.01 < k/n < 0.99; tracking selection
   for k/n <= 0.01 (k times randint(n), a value already in the set drawn again); reservoir sampling above 0.99, which for k <= 64 means
   n == k: rows 0 .. k-1, nothing drawn.  The state is advanced exactly as NumPy advances it.  Streams with n_population[b] < k (scikit-
   learn raises) are left untouched and their sets zero-filled.  k <= 64, n_population[b] <= 2^31 - 1.  The sets feed
   gsf_ransac_poly_batch_dev at any ratio. */
GSF_API int gsf_mt19937_sample_without_replacement_batch_dev(gsf_ctx *ctx, uint32_t *state, const int32_t *n_population, int64_t B,
                                                             int32_t trials, int32_t k, int32_t *sample_idx);

/* ---- K3: apply Sim3 (transform_trajectory, EKFGPSSLAM.py:461-467) -------------------------- */
/* pos[total][3], quat[total][4]; per-trajectory R[B][9], t[B][3], s[B].  A zero-norm quaternion (SciPy raises
   ValueError there) yields NaN quaternion output and sets bad_quat[b] (int32[B], may be NULL). */
GSF_API int gsf_apply_sim3_batch_dev(gsf_ctx *ctx, const double *pos, const double *quat, const int64_t *offsets, int64_t B,
                             const double *R, const double *t, const double *s, double *pos_out, double *quat_out,
                             int32_t *bad_quat);
GSF_API int gsf_apply_sim3_batch(gsf_ctx *ctx, const double *pos, const double *quat, const int64_t *offsets, int64_t B,
                         const double *R, const double *t, const double *s, double *pos_out, double *quat_out,
                         int32_t *bad_quat);

/* ---- K4: EKF + per-outage RTS (apply_ekf_correction, EKFGPSSLAM.py:831-935, after its :847 alignment) -- */
/* B trajectories of N poses each.  ts/pos/quat = ORIGINAL SLAM track, gps/valid = GNSS time-aligned to the SLAM
   stamps (NaN allowed), init_pos[B][3]/init_quat[B][4] = row 0 of the Sim3-aligned track.
   Outputs pos_out/quat_out in the same layout, status[B] (GSF_ST_* bits). */
GSF_API int gsf_ekf_fuse_batch_dev(gsf_ctx *ctx, int32_t layout, const double *ts, const double *pos, const double *quat,
                           const double *gps, const uint8_t *valid, const double *init_pos, const double *init_quat,
                           const gsf_ekf_config *cfg, int64_t B, int64_t N, double *pos_out, double *quat_out,
                           int32_t *status);
GSF_API int gsf_ekf_fuse_batch(gsf_ctx *ctx, int32_t layout, const double *ts, const double *pos, const double *quat,
                       const double *gps, const uint8_t *valid, const double *init_pos, const double *init_quat,
                       const gsf_ekf_config *cfg, int64_t B, int64_t N, double *pos_out, double *quat_out,
                       int32_t *status);

/* ---- fused pipeline: Umeyama on the chosen rows -> Sim3 of pose 0 -> EKF+RTS, one launch chain --------- */
/* (steps 3-5 of main_process_gui, EKFGPSSLAM.py:1002-1010, with the plain fit of :428 instead of RANSAC; the rows of the fit are
   every valid row or the reference's choice of :973-998 -- gsf_set_sim3_rows).
   Trajectories whose fit is None get status GSF_ST_* | (GSF_SIM3_NONE << 8) and NaN outputs. */
GSF_API int gsf_fuse_pipeline_batch_dev(gsf_ctx *ctx, int32_t layout, const double *ts, const double *pos, const double *quat,
                                const double *gps, const uint8_t *valid, const gsf_ekf_config *cfg, int64_t B, int64_t N,
                                double *R, double *t, double *s, double *pos_out, double *quat_out, int32_t *status);
GSF_API int gsf_fuse_pipeline_batch(gsf_ctx *ctx, int32_t layout, const double *ts, const double *pos, const double *quat,
                            const double *gps, const uint8_t *valid, const gsf_ekf_config *cfg, int64_t B, int64_t N,
                            double *R, double *t, double *s, double *pos_out, double *quat_out, int32_t *status);   /* host arrays */

/* ---- the same steps with the reference's ROBUST fit (compute_sim3_transform_robust, EKFGPSSLAM.py:1002, :389-426) ---------- */
/* One device chain, no host round trip: rows with valid finite GNSS (all of them, or the reference's choice of :973-998:
   gsf_set_sim3_rows) -> max_trials hypotheses drawn from each trajectory's
   legacy MT19937 stream (mt_state[B][625], in/out: see gsf_mt19937_*) -> first-best inlier set, final Umeyama on the inliers ->
   Sim3 of pose 0 -> EKF+RTS.  Trajectory-major layout.  Outputs as gsf_fuse_pipeline_batch_dev plus n_inliers[B] (best count,
   -1 if no hypothesis succeeded) and inlier_mask[B][N] (uint8, original row order, may be NULL).  The workspace (about
   53 B/pose + 4 B x max_trials x min_samples per trajectory) is the context's, grown on demand. */
GSF_API int gsf_fuse_pipeline_robust_batch_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                               const uint8_t *valid, const gsf_ekf_config *cfg, int64_t B, int64_t N, int32_t min_samples,
                                               double residual_threshold, int32_t max_trials, int32_t min_inliers_needed, uint32_t *mt_state,
                                               double *R, double *t, double *s, double *pos_out, double *quat_out, int32_t *status,
                                               int32_t *n_inliers, uint8_t *inlier_mask);
/* the same with trial_info[B][2] (int32, may be NULL): { the trial whose inlier set was kept -- the first one with the best count, :413 --
   or -1 when no trial was usable, the number of trials drawn from the trajectory's generator } (max_trials unless
   gsf_set_option "ransac_early_exit" stopped it early; 0 where the reference returns before drawing, :395-397) */
GSF_API int gsf_fuse_pipeline_robust_info_batch_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                                    const uint8_t *valid, const gsf_ekf_config *cfg, int64_t B, int64_t N, int32_t min_samples,
                                                    double residual_threshold, int32_t max_trials, int32_t min_inliers_needed,
                                                    uint32_t *mt_state, double *R, double *t, double *s, double *pos_out, double *quat_out,
                                                    int32_t *status, int32_t *n_inliers, uint8_t *inlier_mask, int32_t *trial_info);
/* host arrays; mt_state[B][625] in/out as in gsf_sim3_ransac_mt_batch (np.random.get_state(): key[624] + pos) */
GSF_API int gsf_fuse_pipeline_robust_batch(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                           const uint8_t *valid, const gsf_ekf_config *cfg, int64_t B, int64_t N, int32_t min_samples,
                                           double residual_threshold, int32_t max_trials, int32_t min_inliers_needed, uint32_t *mt_state,
                                           double *R, double *t, double *s, double *pos_out, double *quat_out, int32_t *status,
                                           int32_t *n_inliers, uint8_t *inlier_mask);

/* ---- steps 1-6 of main_process_gui for B trajectories as ONE device chain (EKFGPSSLAM.py:959-1033) -------------------------------
   In: B SLAM tracks of N poses (ts[B][N], pos[B][N][3], quat[B][N][4]: what load_slam_trajectory returns, :959) and their GNSS logs as
   load_gps_data reads them (:258): fixes gps_offsets[b]..gps_offsets[b+1] of gps_t[total] and gps_llh[total][3] = (col 1, col 2, col 3 of
   the text file: read as lat deg, lon deg, alt m).  total_fixes = gps_offsets[B], max_fixes >= the longest log (both known to the HOST:
   they size the workspace).  mt_state[B][625] in/out: each trajectory's NumPy legacy generator (np.random.get_state(): key[624] + pos);
   the pre-filter of step 1 and the robust fit of step 3 draw from it in the reference's order.
   Chain: lat/lon range mask, zone pick, UTM forward (:259-271) -> sliding-window RANSAC pre-filter (:275, :136-247) -> dynamic_time_alignment
   to the SLAM stamps (:971) -> the rows of the global fit (:973-998; this entry always applies the reference's choice with cfg's values,
   whatever gsf_set_sim3_rows says) -> compute_sim3_transform_robust (:1002; gsf_set_option "ransac_early_exit" applies) ->
   transform_trajectory (:1006) -> apply_ekf_correction (:1010) -> the error metric of step 6 against the primary GPS (:1013-1033).
   Out: R[B][9], t[B][3], s[B], pos_out[B][N][3], quat_out[B][N][4], status[B] (GSF_ST_* | GSF_SIM3_* << 8), n_inliers[B];
   zone[B] / south[B]; gps_utm[total][3] = (E, N, alt), NaN rows where the loader drops the fix; gps_keep[total] = 1 on the fixes that
   survive loader and pre-filter (what load_gps_data returns); aligned[B][N][3] / valid[B][N] = step 2's output; sim3_pos[B][N][3] (may be
   NULL) = step 4's positions; err_stats[3][B][4] = { count, mean, median, RMSE } of raw SLAM / Sim3 / EKF (:1027-1033);
   run_status[B] = GSF_RUN_* (a trajectory on which the reference raises has NaN outputs and its generator where the reference left it);
   gps_llh == NULL: gps_utm is an INPUT -- the logs as load_gps_data's projection left them, (E, N, alt) per fix, NaN easting and northing
   on a fix the loader drops -- and the chain starts at the pre-filter (zone / south are not written and may be NULL);
   inlier_mask[B][N] and trial_info[B][2] as in gsf_fuse_pipeline_robust_info_batch_dev (may be NULL). */
GSF_API int gsf_run_fusion_batch_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, int64_t B, int64_t N,
                                     const double *gps_t, const double *gps_llh, const int64_t *gps_offsets, int64_t total_fixes,
                                     int32_t max_fixes, const gsf_run_config *cfg, uint32_t *mt_state, double *R, double *t, double *s,
                                     double *pos_out, double *quat_out, int32_t *status, int32_t *n_inliers, int32_t *zone, int32_t *south,
                                     double *gps_utm, uint8_t *gps_keep, double *aligned, uint8_t *valid, double *sim3_pos,
                                     double *err_stats, int32_t *run_status, uint8_t *inlier_mask, int32_t *trial_info);
/* the same with host arrays (gps_llh must be given; total_fixes and max_fixes are read from gps_offsets) */
GSF_API int gsf_run_fusion_batch(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, int64_t B, int64_t N, const double *gps_t,
                                 const double *gps_llh, const int64_t *gps_offsets, const gsf_run_config *cfg, uint32_t *mt_state, double *R,
                                 double *t, double *s, double *pos_out, double *quat_out, int32_t *status, int32_t *n_inliers, int32_t *zone,
                                 int32_t *south, double *gps_utm, uint8_t *gps_keep, double *aligned, uint8_t *valid, double *sim3_pos,
                                 double *err_stats, int32_t *run_status, uint8_t *inlier_mask, int32_t *trial_info);

/* ---- steps 1-6 of main_process_gui for B SLAM tracks of ANY lengths, with the optional ground-truth GNSS log (EKFGPSSLAM.py:959-1075) ----
   The chain of gsf_run_fusion_batch_dev on ragged input: track b = rows slam_offsets[b]..slam_offsets[b+1] of ts[P], pos[P][3], quat[P][4]
   (P = total_poses; max_poses >= the longest track, host-known: it sizes LDS and the draws' workspace); primary log b = fixes
   gps_offsets[b]..gps_offsets[b+1] as in the dense entry; ground-truth log b = fixes gt_offsets[b]..gt_offsets[b+1] of gt_t / gt_llh
   (gt_offsets == NULL: no track has one -- the gt_* outputs may then be NULL --; an empty range: that track has none).  gps_llh == NULL /
   gt_llh == NULL: gps_utm / gt_utm are inputs holding the projected logs, as in the dense entry (zone / south resp. gt_zone / gt_south unused).
   Per track, in the reference's order of draws and raises: primary log (mask, zone, UTM, pre-filter with cfg->gps_filter; a failure there
   stops the run before any ground-truth draw) -> ground-truth log (its OWN zone, UTM, pre-filter with gt_filter = CONFIG['ground_truth_gps_
   filtering'], :55-64) -> the empty-track check (:967) -> steps 2-5 as in the dense entry -> step 6 against the primary fixes and, with a
   ground-truth log, against it after the same time alignment (:1035-1062).
   Out, per-pose arrays flat over P rows: as gsf_run_fusion_batch_dev, plus gt_zone[B] / gt_south[B], gt_utm[gt_total][3], gt_keep[gt_total],
   gt_aligned[P][3] / gt_valid[P]; err_stats[2][3][B][4] = { primary, ground truth } x { raw SLAM, Sim3, EKF } x { count, mean, median, RMSE }
   (count 0 and NaN where a track has no ground truth); plot_ref[B] (may be NULL) = the error reference of the plot (:1064-1075): 2 ground
   truth, 1 primary, 0 none; run_status[B] = GSF_RUN_* including the four bits above (a failed run: NaN outputs, count-0 rows, plot_ref 0).
   Limits: at most 28 000 poses per track, at most 14 000 fixes per log (a longer log fails the call, as in the dense entry); one thread per
   context at a time (the call swaps the context's Sim3 row rule for the duration, as the dense entry does). */
GSF_API int gsf_run_fusion_ragged_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *slam_offsets, int64_t B,
                                      int64_t total_poses, int32_t max_poses, const double *gps_t, const double *gps_llh, const int64_t *gps_offsets,
                                      int64_t total_fixes, int32_t max_fixes, const double *gt_t, const double *gt_llh, const int64_t *gt_offsets,
                                      int64_t gt_total, int32_t gt_max_fixes, const gsf_run_config *cfg, const gsf_prefilter_config *gt_filter,
                                      uint32_t *mt_state, double *R, double *t, double *s, double *pos_out, double *quat_out, int32_t *status,
                                      int32_t *n_inliers, int32_t *zone, int32_t *south, double *gps_utm, uint8_t *gps_keep, double *aligned,
                                      uint8_t *valid, double *sim3_pos, int32_t *gt_zone, int32_t *gt_south, double *gt_utm, uint8_t *gt_keep,
                                      double *gt_aligned, uint8_t *gt_valid, double *err_stats, int32_t *plot_ref, int32_t *run_status,
                                      uint8_t *inlier_mask, int32_t *trial_info);
/* the same with host arrays (gps_llh / gt_llh must be given): the sizes are read from the offsets, which are checked (non-decreasing, the
   limits above) before any device work; then one staged upload, the chain, one download */
GSF_API int gsf_run_fusion_ragged(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *slam_offsets, int64_t B,
                                  const double *gps_t, const double *gps_llh, const int64_t *gps_offsets, const double *gt_t, const double *gt_llh,
                                  const int64_t *gt_offsets, const gsf_run_config *cfg, const gsf_prefilter_config *gt_filter, uint32_t *mt_state,
                                  double *R, double *t, double *s, double *pos_out, double *quat_out, int32_t *status, int32_t *n_inliers, int32_t *zone,
                                  int32_t *south, double *gps_utm, uint8_t *gps_keep, double *aligned, uint8_t *valid, double *sim3_pos,
                                  int32_t *gt_zone, int32_t *gt_south, double *gt_utm, uint8_t *gt_keep, double *gt_aligned, uint8_t *gt_valid,
                                  double *err_stats, int32_t *plot_ref, int32_t *run_status, uint8_t *inlier_mask, int32_t *trial_info);

/* ragged forms (trajectories of different lengths): flat [total][C] arrays, trajectory b = rows offsets[b]..offsets[b+1].
   An empty trajectory (offsets[b] == offsets[b+1], apply_ekf_correction's early return, :835) gets status[b] = 0 and has no rows; the
   pipeline form writes NaN into its R[b], t[b] and s[b] (there is no fit). */
GSF_API int gsf_ekf_fuse_ragged_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                    const uint8_t *valid, const int64_t *offsets, const double *init_pos, const double *init_quat,
                                    const gsf_ekf_config *cfg, int64_t B, double *pos_out, double *quat_out, int32_t *status);
GSF_API int gsf_fuse_pipeline_ragged_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                         const uint8_t *valid, const int64_t *offsets, const gsf_ekf_config *cfg, int64_t B, double *R,
                                         double *t, double *s, double *pos_out, double *quat_out, int32_t *status);
/* the same with host arrays */
GSF_API int gsf_ekf_fuse_ragged(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                const uint8_t *valid, const int64_t *offsets, const double *init_pos, const double *init_quat,
                                const gsf_ekf_config *cfg, int64_t B, double *pos_out, double *quat_out, int32_t *status);
GSF_API int gsf_fuse_pipeline_ragged(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                     const uint8_t *valid, const int64_t *offsets, const gsf_ekf_config *cfg, int64_t B, double *R,
                                     double *t, double *s, double *pos_out, double *quat_out, int32_t *status);

/* ---- per-pose covariance and smoothing flags of the fused track ------------------------------------------------------------------------
   What apply_ekf_correction computes and drops: process_step returns the filtered and the predicted covariance of every pose (kept in
   ekf_covs_filt_hist / ekf_covs_pred_hist, EKFGPSSLAM.py:852-853, :902-903) and rts_smoother_segment the smoothed covariance of every
   segment it rewrites (:777-803; bound to `_` at :917).  Every one of these matrices is exactly diagonal (P0, Q, R come from np.diag,
   H = [I3 0], the Joseph form :731 keeps the diagonal), so a row of 7 doubles [x y z qx qy qz qw] is the whole matrix.
   For a track of N poses, dt[i] = max(1e-6, ts[i] - ts[i-1]) (:865), avail[i] = valid[i] && fix i free of NaN for i >= 1 (:867-869):
   - filtered: Pf[0] = P0; Pp[i] = Pf[i-1] + Q dt[i] (:712-714); on axes 0-2 with avail[i]: Pf[i] = (1-k) Pp (1-k) + k R k, k = Pp / (Pp + R)
     (:723-731); otherwise Pf[i] = Pp[i].  A sharp-turn recovery blends the state, not the covariance (:767).
   - outages, recoveries and the RTS decision: as in gsf_ekf_fuse_ragged_dev (:848-928).  The initial outage state is the raw valid[0] (:848);
     the sharp-turn test runs over the pose pairs inside the outage, and only for an outage of >= 2 poses (:882-889).
   - smoothed, for a segment [a..b] handed to the smoother (a = outage start, b = the recovery, no sharp turn): Ps[b] = Pf[b] (:783);
     Ps[k] = Pf[k] + A^2 (Ps[k+1] - Pp[k+1]), A = Pf[k] / Pp[k+1] for k < b (:786-801).  Poses a..b-1 take no update, so this equals
     Ps[k] = Pf[k] + (Pf[k] / Pp[b])^2 (Pf[b] - Pp[b]); axes 3-6 have Pf[b] = Pp[b] and stay as filtered. */
#define GSF_POSE_GNSS_USED 1   /* a GNSS update was applied at this pose (never pose 0) */
#define GSF_POSE_IN_OUTAGE 2   /* pose without a usable fix: rows a..b-1 of an outage, or an outage still open at the end; pose 0 by valid[0] (:848) */
#define GSF_POSE_SMOOTHED  4   /* pose rewritten by rts_smoother_segment: rows a..b-1 of a smoothed segment (the recovery b keeps its filtered state, :783) */
#define GSF_POSE_SHARP_TURN 8  /* row of an outage whose recovery was judged a sharp turn: left unsmoothed (:886-889) */
/* Ragged device form: ts[P], quat[P][4] (the ORIGINAL SLAM quaternions; read only inside outages), gps[P][3] / valid[P] = the time-aligned
   fixes and their mask, offsets int64[B+1].  Out: cov_filt[P][7] (may be NULL) = the diagonal of ekf_covs_filt_hist; cov_out[P][7] = the
   covariance that belongs to the pose the fuse entries return: smoothed on GSF_POSE_SMOOTHED rows, filtered elsewhere; pose_flags[P]
   (may be NULL) = GSF_POSE_* bits; status[B] (may be NULL) = GSF_ST_HAD_OUTAGE | _RTS_APPLIED | _SHARP_TURN | _ENDED_IN_OUTAGE with the
   meaning they have in gsf_ekf_fuse_ragged_dev (GSF_ST_BAD_QUAT is never set here: quaternions outside outages are not read).
   An empty track has no rows and gets status 0.  run_status (may be NULL): a track with run_status[b] != 0 gets NaN rows, zero flags
   and status 0, and its inputs are not read.  One wave per track, no workspace, any track length. */
GSF_API int gsf_ekf_cov_ragged_dev(gsf_ctx *ctx, const double *ts, const double *quat, const double *gps, const uint8_t *valid,
                                   const int64_t *offsets, const int32_t *run_status, const gsf_ekf_config *cfg, int64_t B,
                                   double *cov_filt, double *cov_out, uint8_t *pose_flags, int32_t *status);
/* the same with host arrays: staged upload, kernel, download */
GSF_API int gsf_ekf_cov_ragged(gsf_ctx *ctx, const double *ts, const double *quat, const double *gps, const uint8_t *valid,
                               const int64_t *offsets, const int32_t *run_status, const gsf_ekf_config *cfg, int64_t B,
                               double *cov_filt, double *cov_out, uint8_t *pose_flags, int32_t *status);

/* ---- whole-track RTS smoothing: the fixed-interval smoother over the fused track -----------------------------------------------------------
   apply_ekf_correction (EKFGPSSLAM.py:831-935) runs a causal filter and hands rts_smoother_segment (:777-803) only the poses of a GNSS
   outage (:906-923): wherever GNSS is present the fused pose at stamp t uses the fixes up to t and none after it.  The reference keeps
   everything the fixed-interval smoother needs (ekf_states_*_hist, ekf_covs_*_hist) and never makes the call; this entry makes it.
   Forward pass -- the filter of gsf_ekf_fuse_ragged_dev / gsf_ekf_cov_ragged_dev, exactly: dt[i] = max(1e-6, ts[i] - ts[i-1]) (:865),
   avail[i] as at :867-869, Pp[i] = Pf[i-1] + Q dt[i]; with a fix the gain k = Pp / (Pp + R) and the Joseph Pf; a sharp-turn recovery takes
   the one-step blend weight 1 / steps (:752-768, :889); outages and the sharp-turn decision are gsf_ekf_cov_ragged_dev's.  xf, xp = the
   filtered and the predicted position, g[i] = xf[i] - xp[i] = the applied correction (0 without an update).
   Spans -- every recovery b that the filter judges a sharp turn starts a new span: [0..b1-1], [b1..b2-1], ..., [bm..N-1].  The reference's
   judgement that RTS is not to be trusted across such an outage is kept; a caller who wants to smooth through turns raises
   sharp_turn_yaw_rate_threshold_deg_per_sec (a pair never exceeds once thr dt >= pi).
   Backward pass, per span and axis -- rts_smoother_segment (:777-803) on the span: A[k] = Pf[k] / Pp[k+1] (A[k] = 0 where Pp[k+1] == 0:
   the reference lands there through pinv); xs[last] = xf[last], Ps[last] = Pf[last]; xs[k] = xf[k] + A[k] (xs[k+1] - xp[k+1]);
   Ps[k] = Pf[k] + A[k]^2 (Ps[k+1] - Pp[k+1]).  In correction coordinates e = xs - xf, d = Ps - Pf:
       e[k] = A[k] (e[k+1] + g[k+1]),   d[k] = A[k]^2 (d[k+1] + (Pf[k+1] - Pp[k+1])),   e = d = 0 at a span's last pose
   -- two affine suffix scans per axis, and A := 0 on a span's last pose makes it one scan per track.  Consequences: the quaternion axes
   are never updated, so Ps = Pf on axes 3-6 and the smoothed quaternion is the filter's (the reference re-normalises it: <= 2.2e-16);
   poses of a sharp-turn outage, and poses after the last update of a span, keep their filtered values exactly; a zero-variance axis
   (P0 = Q = 0) comes back unsmoothed and free of NaN.  A <= 1, so products only underflow to 0: the stated range of the noise values
   (gsf_ekf_config: 0 <= P0 <= 1e8, 1e-8 <= R <= 1e8, 0 <= Q dt <= 1e14) holds unchanged.
   In: as gsf_ekf_fuse_ragged_dev, plus run_status as in gsf_ekf_cov_ragged_dev (may be NULL: NaN rows, zero flags, status 0, inputs not
   read).  Out: pos_out[P][3], quat_out[P][4] = the smoothed track; cov_out[P][7] = the smoothed diagonal; pos_filt[P][3], cov_filt[P][7]
   (the filter's own track and diagonal), pose_flags[P], status[B]: each may be NULL.  pose_flags = GSF_POSE_GNSS_USED | _IN_OUTAGE |
   _SHARP_TURN with their meanings above; GSF_POSE_SMOOTHED means HERE "a later fix of the same span was applied" -- exactly the rows
   where e, d are not structurally zero (every other row returns the filter's bytes); GSF_POSE_SPAN_START marks row 0 and every
   sharp-turn recovery.  status = GSF_ST_* bits as gsf_ekf_fuse_ragged_dev sets them, with GSF_ST_RTS_APPLIED set when any row is
   GSF_POSE_SMOOTHED.  An empty track has no rows and status 0.  One wave per track, two passes over it (the backward pass re-reads what
   the forward pass parked in the track's own cov_out rows), no workspace, any track length.  Device pointers, asynchronous on the
   context's stream; there is no host-pointer form: the Python binding uploads host arrays itself. */
#define GSF_POSE_SPAN_START 16 /* gsf_ekf_smooth_ragged_dev: first row of a smoothing span (row 0, every sharp-turn recovery) */
GSF_API int gsf_ekf_smooth_ragged_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                      const uint8_t *valid, const int64_t *offsets, const double *init_pos, const double *init_quat,
                                      const int32_t *run_status, const gsf_ekf_config *cfg, int64_t B, double *pos_out, double *quat_out,
                                      double *cov_out, double *pos_filt, double *cov_filt, uint8_t *pose_flags, int32_t *status);

/* ---- per-fix GNSS noise: the whole-track filter and smoother with a measurement variance per pose ------------------------------------------
   Every other filter entry weighs every fix with the one meas_noise_diag of its cfg.  Receivers report how good each fix is (NMEA GST, fix
   type, satellite count; GPSmerge.py:41-60 writes numsats and velmode behind lat lon alt), and an RTK-fixed fix and a single-point fix
   under trees differ by four orders of magnitude in variance.  This entry is gsf_ekf_smooth_ragged_dev with R replaced by the row's own.
   meas_var[P][3] = the measurement variance of pose i per position axis, in the unit of meas_noise_diag (a variance: np.diag of it is R,
   EKFGPSSLAM.py:686).  cfg's meas_noise_diag is not read.
   Usable -- a variance v is usable when 1e-8 <= v <= 1e8 (finite, inside the stated range of meas_noise_diag, both ends included).  There
   is no bound on the ratio of two variances of a track, nor on the ratio of two steps: rows at both ends of the range may follow each
   other, over long and short steps (the variance scans rescale their composed maps; the argument stands above variance_scan in
   gsf_wave_common.hpp).  P0 and Q dt as gsf_ekf_config states them.
   Available -- avail[i] = the smoother's avail[i] (i >= 1, valid[i] != 0, fix i free of NaN; :867-869) AND all three variances of row i
   usable.  A row that would be available but for its variances is a pose without a fix IN EVERY RESPECT -- the outage structure, the
   sharp-turn decision, flags, spans and the reach of the backward pass are those of the same call with valid[i] = 0 -- and it carries
   GSF_POSE_BAD_SIGMA.  Exception: all three variances +inf, the caller's way of saying "no information": no fix, and no bit.
   meas_var of row 0 decides nothing (pose 0 takes no update; its outage state is the raw valid[0], :848), nor does meas_var of a row
   whose mask byte is clear or whose fix holds a NaN: any bytes there change no output byte and set no bit.
   Filter and smoother -- exactly as documented above gsf_ekf_smooth_ragged_dev, with r_i = meas_var[i] for R on every available row:
   k = Pp / (Pp + r_i), the Joseph Pf = (1-k) Pp (1-k) + k r_i k, g = w k (z - xp) with the one-step blend w at a sharp-turn recovery;
   A[k] = Pf[k] / Pp[k+1] and the e and d suffix scans read Pf, g and dt only and are unchanged.
   nis[P] (may be NULL) = sum over the three axes of y_c^2 / (Pp_c + r_ic) on GSF_POSE_GNSS_USED rows, NaN elsewhere; y = z - xp is formed
   relative to init_pos and is the innovation before any blend.  Mean 3 for a consistent filter: the caller's check on the variances given.
   Everything else -- inputs, outputs and which may be NULL, run_status (NaN rows, nis included, zero flags, status 0, inputs not read),
   empty tracks, pose_flags, status words -- as gsf_ekf_smooth_ragged_dev.  Every call writes every output byte.  With meas_var[i] =
   cfg's meas_noise_diag on every row the variances are that entry's bit for bit (three scans here where axes with equal noise share one
   there: the same values).  One wave per track, two passes, no workspace, any track length.  Device pointers, asynchronous on the
   context's stream; there is no host-pointer form. */
#define GSF_POSE_BAD_SIGMA 32 /* gsf_ekf_smooth_weighted_dev: the row had a fix, but a variance that is not usable (and not all three +inf) */
GSF_API int gsf_ekf_smooth_weighted_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                        const uint8_t *valid, const double *meas_var, const int64_t *offsets, const double *init_pos,
                                        const double *init_quat, const int32_t *run_status, const gsf_ekf_config *cfg, int64_t B,
                                        double *pos_out, double *quat_out, double *cov_out, double *pos_filt, double *cov_filt,
                                        uint8_t *pose_flags, int32_t *status, double *nis);
/* ---- robust smoothing: Huber / Cauchy reweighting rounds of the weighted smoother, in one launch --------------------------------------------
   gsf_ekf_smooth_weighted_dev is a least-squares estimator: a multipath fix 25 m off pulls the smoothed track with the full weight of its
   stated variance.  The RANSAC pre-filter works on the log before alignment; the innovation gate is causal, all-or-nothing, and keeps one
   R per run.  This entry is the M-estimator a smoother takes, solved by iteratively reweighted least squares: every round smooths the
   track, forms each used fix's residual against the SMOOTHED track (which has seen the fixes on both sides), turns it into a weight and
   inflates that fix's variance by 1 / weight.  One kernel: the weight of the next round falls out of the backward pass.
   Solve 0 -- gsf_ekf_smooth_weighted_dev on meas_var[P][3].  meas_var may be NULL here: cfg's meas_noise_diag on every row.
   Residual -- after a solve, on every GSF_POSE_GNSS_USED row: res_c = (z_c - init_pos_c) - (xr_c + e_c), xr = the filtered position relative
   to init_pos, e = the smoother's correction (0 where no later fix reaches the row); u2 = sum_c res_c^2 / meas_var_ic with the GIVEN
   variance, not the inflated one.  Relative to init_pos: formed from UTM positions the residual would carry 1e-9 m of rounding.
   Weight -- loss GSF_REWEIGHT_HUBER: w = 1 for u2 <= c2, else sqrt(c2 / u2); GSF_REWEIGHT_CAUCHY: w = 1 / (1 + u2 / c2).  Both are
   continuous in u2.  c2 is a threshold on a chi-square of 3 degrees of freedom (7.81: 95 %).  weight[i] is NaN on rows without an update.
   Effective variance -- the next solve runs with r_eff_ic = min(meas_var_ic / w_i, 1e8): inside the usable range whatever w is (w = 0, from
   u2 = inf, gives 1e8), so availability is judged on the GIVEN variances once, and outages, sharp-turn decisions, spans, flags, status and
   quaternions are the same in every solve.
   Stop -- after `rounds` reweighted solves (0 <= rounds <= 32), or for a track as soon as every weight just computed equals, bit for bit,
   the weight its solve used (solve 0 used 1.0 everywhere): the next solve would reproduce the same bytes.  rounds_used[B] (may be NULL) =
   the reweighted solves done; w_change[B] (may be NULL) = max |w_new - w_used| over the used rows of the last solve, 0 at a fixed point
   and on a track without a used row.
   Out -- everything gsf_ekf_smooth_weighted_dev returns (nis included) is of the LAST solve, under its effective variances.  weight[P]
   (required) is the rounds' own store and holds, on return, the weights computed from the last solve's track; its incoming bytes are
   not read.  Two laws: (A) rounds = 0 returns gsf_ekf_smooth_weighted_dev's bytes on every shared output (with meas_var NULL: those of
   that entry fed cfg's meas_noise_diag on every row); (B) rounds = R returns the bytes of gsf_ekf_smooth_weighted_dev fed
   min(meas_var / w, 1e8) on the rows where w is a number and meas_var elsewhere, w = the weight output of the call with rounds = R - 1.
   run_status[b] != 0: NaN rows (weight included), rounds_used 0, w_change 0.  An empty track has no rows, status 0, rounds_used 0,
   w_change 0.  c2 not finite or <= 0, another loss, rounds outside [0, 32]: GSF_ERR_INVALID_ARG.  Everything else as
   gsf_ekf_smooth_weighted_dev.  One wave per track, two passes per solve (between them the track's own pos_out row holds the filtered
   position relative to init_pos), no workspace, any track length.  Device pointers, asynchronous on the context's stream; there is no
   host-pointer form. */
#define GSF_REWEIGHT_HUBER 0
#define GSF_REWEIGHT_CAUCHY 1
GSF_API int gsf_ekf_smooth_reweighted_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                          const uint8_t *valid, const double *meas_var, const int64_t *offsets, const double *init_pos,
                                          const double *init_quat, const int32_t *run_status, const gsf_ekf_config *cfg, int64_t B,
                                          int32_t loss, double c2, int32_t rounds, double *pos_out, double *quat_out, double *cov_out,
                                          double *pos_filt, double *cov_filt, uint8_t *pose_flags, int32_t *status, double *nis,
                                          double *weight, int32_t *rounds_used, double *w_change);
/* Per-fix variances carried onto SLAM stamps: pose_var[P][3] for gsf_ekf_smooth_weighted_dev from fix_var[T][3] of the GNSS logs.
   In: ts[P] with slam_offsets int64[B+1]; gps_t[T] with gps_offsets int64[B+1] (ascending stamps per log); gps_keep[T] = the pre-filter's
   mask (NULL: every fix kept); fix_var[T][3]; valid[P] (may be NULL).  For pose i of track b:
   - valid given and valid[i] == 0: +inf x3, and the log is not read;
   - otherwise, among the KEPT fixes of log b, lo = the last with stamp <= ts[i] and hi = the first with stamp >= ts[i]; either missing
     (a pose before the first or after the last kept fix, an empty log, a NaN stamp): +inf x3;
   - otherwise per axis the larger of the two variances; a NaN in either gives NaN, which the filter then flags.  A pose on a kept fix's
     stamp takes that fix's own variance; with repeated stamps the larger of the last and the first of them.
   The aligned fix is an interpolant of its neighbours (dynamic_time_alignment, :325-387), so the worse neighbour bounds it; the cubic
   spline reaches further than the bracket -- a stated approximation, and nis is the caller's check on it.  One thread per pose: a binary
   search on the log's stamps, then a walk over removed fixes; nothing outside [gps_offsets[b], gps_offsets[b+1]) is read, whatever the
   stamps hold.  Device pointers, asynchronous on the context's stream. */
GSF_API int gsf_fix_var_at_poses_dev(gsf_ctx *ctx, const double *ts, const int64_t *slam_offsets, const double *gps_t,
                                     const int64_t *gps_offsets, const uint8_t *gps_keep, const double *fix_var, const uint8_t *valid,
                                     int64_t B, int64_t P, double *pose_var);

/* ---- EKF noise sweep: innovation statistics of the filter for K noise candidates per track ------------------------------------------------
   CONFIG['ekf'] (initial_cov_diag, process_noise_diag, meas_noise_diag, EKFGPSSLAM.py:25-27) is tuned by hand; the standard way to choose
   and check such values is the filter's own innovation sequence: its normalised innovation squared (NIS; mean 3 for a consistent 3-axis
   filter), its Gaussian negative log-likelihood and its whiteness.  This entry runs the position filter of apply_ekf_correction for K
   candidates at once and returns the sums those figures are made of.  GNSS never touches the state quaternion, so the world-frame odometry
   increments are the same for every candidate; RTS rewrites outputs only (:918-922), so the innovations do not depend on it.
   In: ts, pos, quat, gps, valid, offsets, init_pos, init_quat, cfg as in gsf_ekf_fuse_ragged_dev; run_status as in gsf_ekf_cov_ragged_dev
   (may be NULL); cand[K][9] = { P0x, P0y, P0z, Qx, Qy, Qz, Rx, Ry, Rz } per candidate, a DEVICE array, values inside the range stated at
   gsf_ekf_config (outside it: undocumented, as for cfg).  From cfg, shared by all candidates: the sharp-turn threshold and
   default_ekf_transition_steps_on_sharp_turn (its position noise is not read; its quaternion axes influence no innovation).
   For track b, candidate k, axis c in {0, 1, 2}, with dt[i] = max(1e-6, ts[i] - ts[i-1]) (:865) and avail[i] as in gsf_ekf_cov_ragged_dev
   (:867-869), p[0] = init_pos[b], Pf[0] = P0:
   - prediction (_predict, :702-715): p-[i] = p[i-1] + d[i], Pp[i] = Pf[i-1] + Q dt[i]; d[i] = R(q_state[i-1]) dp_local[i] from
     calculate_relative_pose (:77-92) and the state quaternion chain, formed as the fuse kernels form it.
   - update, on avail[i]: y[i] = z[i] - p-[i] (:722), S[i] = Pp[i] + R (:723), g = Pp / S, Pf = (1-g)^2 Pp + g^2 R (:731),
     p[i] = p-[i] + w[i] g y[i].  w[i] = 1 except at the recovery pose of an outage judged a sharp turn when steps =
     default_ekf_transition_steps_on_sharp_turn > 1: there w = 1 / steps, the one-step blend of :752-768 with the override of :889, :899; the
     covariance is the updated one (:767).  The sharp-turn decision is gsf_ekf_cov_ragged_dev's; outages of fewer than 2 poses are hard
     updates (:893-894).
   - without a usable fix: p[i] = p-[i], Pf = Pp.
   - counted updates U = { i >= 1 : avail[i] and ts[i] > ts[0] + skip_seconds } (the burn-in of step 6, :1018); skip_seconds <= 0 counts
     every update.  Normalised innovation nu = y / sqrt(S).
   Out (each may be NULL):
   stats[B][K][12] = { n_upd = |U|;  sum_U y_c^2 / S_c, c = 0..2 (NIS per axis);  sum_U log S_c;  sum_U y_c^2 (in the stamps' length unit
     squared);  sum_c sum nu_c[i] nu_c[i-1] over the pairs with i and i-1 both in U;  the number of such pairs }.  Entries 0 and 11 are the
     same for every candidate.  Derived (the Python binding computes them): nll = (3 n_upd ln 2pi + sum stats[4..6] + sum stats[1..3]) / 2,
     mean_nis = sum stats[1..3] / n_upd, rho1 = stats[10] / (3 stats[11]).
   best_k[B][2] = the first k with the smallest nll (criterion 0) and the first k with the smallest |mean_nis - 3| (criterion 1); -1 when
     n_upd < min_updates.  A candidate whose row is not finite is never picked.
   pooled[K][12] = the sum of the rows of all tracks with run_status[b] == 0, at least one pose and n_upd >= min_updates, added in ascending
     b by one fixed-order pass (no atomics: the bytes are reproducible); pooled_best[2] = the picks over the pooled rows.  Noise is a
     property of the receiver, not of one run, so the pooled pick is the one to use.
   ns_status[B] = GSF_NS_* bits.
   innov[P][3] / innov_var[P][3] = y and S of candidate trace_k (0 <= trace_k < K; negative: no trace) on every pose with an update,
     whatever skip_seconds says, NaN elsewhere.
   An empty track gets rows of zeros, best_k = -1 and GSF_NS_NONE.  A track with run_status[b] != 0 gets NaN rows (stats and trace),
   best_k = -1 and GSF_NS_NONE, and its inputs are not read.  1 <= K <= 4096, any track length.  One wave per (track, group of candidates),
   64 poses per chunk, 89 B read per pose and group, nothing written per pose; gsf_set_option "noise_sweep_group" sets the group size, and a
   candidate's row is the same bytes for every group size.  Where stats (or pooled, with pooled_best given) is NULL and a pick is asked
   for, the rows live in the context's kernel workspace.  Device pointers, asynchronous on the context's stream.  There is no host-pointer
   form: the Python binding uploads host arrays itself. */
#define GSF_NS_NONE 1      /* no pick: fewer than min_updates counted updates, or no candidate with a finite row */
#define GSF_NS_TIE 2       /* the two criteria pick different candidates */
GSF_API int gsf_ekf_noise_sweep_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                    const uint8_t *valid, const int64_t *offsets, const int32_t *run_status, const double *init_pos,
                                    const double *init_quat, const gsf_ekf_config *cfg, int64_t B, const double *cand, int32_t K,
                                    double skip_seconds, int32_t min_updates, int32_t trace_k, double *stats, int32_t *best_k,
                                    double *pooled, int32_t *pooled_best, int32_t *ns_status, double *innov, double *innov_var);

/* ---- GNSS outage study: drift and RTS gain of the fused track for K withheld windows per track ----------------------------------------------
   How far does the fused track drift during a GNSS outage of L seconds, and how much of that does the per-outage RTS smoother take back?
   The standard method withholds the fixes of a window, runs the fusion and measures against the withheld fixes.  This entry does that for
   K windows per track at once.  GNSS never touches the state quaternion, so the world-frame odometry increments d[i] are the same in
   every scenario; all covariances are diagonal; and a withheld window changes nothing before the outage it creates: one base pass per
   track plus O(outage length) work per scenario gives the whole study.
   In: ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, cfg as in gsf_ekf_noise_sweep_dev (cfg's own noise is used);
   truth[P][3] / truth_valid[P] = what errors are measured against (both NULL: gps / valid; both or neither); scen[K][2] = { start, length }
   in the stamps' unit, start relative to the track's first stamp, a DEVICE array shared by all tracks.
   For track b (n poses, stamps t) and scenario (s, L), with avail[i] as in gsf_ekf_cov_ragged_dev (pose 0: the raw mask byte; every other
   pose: the byte set and a fix free of NaN) and dt[i] = max(1e-6, t[i] - t[i-1]) (:865):
   - stamps that are not non-decreasing, or a NaN stamp: GSF_OS_UNSORTED on every scenario of the track, NaN rows, seg = (-1, -1).
   - window: lo = t[0] + s, hi = lo + L, W = the index range [#{t < lo}, #{t < hi}); s or L NaN, or L <= 0: W is empty.  An empty W gives
     GSF_OS_EMPTY, a row of zeros and seg = (-1, -1).
   - modified run: apply_ekf_correction with the mask bytes of W cleared, avail'[i] = avail[i] && i not in W.
   - outage [a, b): the maximal run of !avail' that contains W; b = the recovery pose, or n when there is none (GSF_OS_NO_RECOVERY).
     GSF_OS_MERGED: [a, b) is larger than W.  GSF_OS_FROM_START: a = 0.
   - anchor c = max(a - 1, 0): the unmodified run's filtered position p_f[c] and variance Pf[c] are the modified run's as well.
   - dead reckoning, a <= k < b: p_dr[k] = p_f[c] + sum_{c<i<=k} d[i], Pdr[k] = Pf[c] + Q sum_{c<i<=k} dt[i] per position axis (k = c = 0:
     init_pos, P0).
   - recovery, when b < n: p-[b], Pp[b] formed likewise; y = gps[b] - p-[b] (:722), S = Pp[b] + R (:723), g = Pp[b] / S.
     sharp = (b - a >= 2) && (a pair (j-1, j) with a < j < b and t[j] > t[j-1] exceeds the yaw-rate threshold -- the pair test of
     gsf_ekf_cov_ragged_dev, an invalid quaternion in the pair counts -- or threshold < 0) (:882-889, :826).
   - fused position: not sharp: GSF_OS_SMOOTHED, p_fu[k] = p_dr[k] + (Pdr[k] / Pp[b]) g y per axis, the telescoped rts_smoother_segment
     (:777-803; no pose of [a, b) takes an update, so the smoother gains multiply to Pdr[k] / Pp[b]).  Sharp (GSF_OS_SHARP_TURN) or no
     recovery: p_fu = p_dr.  The one-step blend at a sharp recovery (:752-768) alters pose b only, which lies outside [a, b).
   - evaluated set E = { k in [a, b) : truth_valid[k] and truth[k] free of NaN }; withheld updates H = { i in W : i >= 1, avail[i] };
     e_dr[k] = |p_dr[k] - truth[k]|, e_fu[k] = |p_fu[k] - truth[k]| (Euclidean, 3-D).
   Out (each may be NULL):
   stats[B][K][13] = { |E|;  |H|;  b - a;  gap = t[min(b, n-1)] - t[c] (one subtraction of stamps);  dist = sum_{c<i<=min(b, n-1)} |d[i]|;
     sum_E e_dr^2;  max_E e_dr;  sum_E e_fu^2;  max_E e_fu;  sum_E of the horizontal (x, y) part of e_dr^2;  the same of e_fu^2;  |y| at the
     recovery;  NIS at the recovery sum_c y_c^2 / S_c }.  Entries 11 and 12 are NaN without a recovery; entries 6 and 8 are 0 where E is empty.
     Derived (the Python binding computes them): rms_dr = sqrt(stats[5] / stats[0]), rms_fused = sqrt(stats[7] / stats[0]),
     drift_pct = 100 stats[11] / stats[4].
   seg[B][K][2] = (a, b) relative to the track.  os_flags[B][K] = GSF_OS_* bits.
   err_dr[P], err_fused[P], trace_pos[P][3] = e_dr, e_fu and p_fu of scenario trace_k (0 <= trace_k < K; negative: no trace): errors are NaN
     outside E, trace_pos is NaN outside [a, b).
   An empty track gets GSF_OS_EMPTY rows.  A track with run_status[b] != 0 gets GSF_OS_SKIPPED: NaN rows (stats and trace), seg = (-1, -1),
   and its inputs are not read.  A scenario's row does not depend on K, on the other scenarios, on their order or on the other tracks: it is
   the same bytes in every call that holds it.  1 <= K <= 4096, any track length.  Base pass: one wave per track, 89 B read and 89 B written
   per pose into the context's kernel workspace; scenario pass: one wave per (track, scenario), about 58 B read per pose of [a, b).
   Device pointers; the launches are asynchronous on the context's stream, after one 8-byte read of offsets[B] (it sizes the workspace)
   for which the call waits on that stream.  There is no host-pointer form: the Python binding uploads host arrays itself. */
#define GSF_OS_EMPTY 1         /* the window holds no pose (or the track is empty): a row of zeros */
#define GSF_OS_NO_RECOVERY 2   /* the outage runs to the end of the track */
#define GSF_OS_SMOOTHED 4      /* the recovery hands [a..b] to the RTS smoother */
#define GSF_OS_SHARP_TURN 8    /* the recovery is judged a sharp turn: [a, b) stays dead-reckoned */
#define GSF_OS_MERGED 16       /* the outage is larger than the window: it merged with an outage of the data */
#define GSF_OS_FROM_START 32   /* the outage begins at pose 0 */
#define GSF_OS_UNSORTED 64     /* the track's stamps are not non-decreasing, or one is NaN: NaN rows */
#define GSF_OS_SKIPPED 128     /* run_status[b] != 0: NaN rows, inputs not read */
GSF_API int gsf_outage_study_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                 const uint8_t *valid, const int64_t *offsets, const int32_t *run_status, const double *init_pos,
                                 const double *init_quat, const gsf_ekf_config *cfg, int64_t B, const double *truth,
                                 const uint8_t *truth_valid, const double *scen, int32_t K, int32_t trace_k, double *stats, int32_t *seg,
                                 int32_t *os_flags, double *err_dr, double *err_fused, double *trace_pos);

/* ---- innovation gate: reject the GNSS fixes the filter disbelieves, K gates per track -----------------------------------------------------
   The reference's only outlier defence is the polynomial RANSAC pre-filter (filter_gps_outliers_ransac, EKFGPSSLAM.py:136-247) with a
   threshold of 10 m; every surviving fix is applied with meas_noise_diag = 0.2, so a multipath jump of 3-9 m drags the fused track almost
   all the way to it.  The standard remedy is a chi-square gate on the normalised innovation squared (NIS): a fix whose NIS exceeds a
   quantile is not applied.  A rejection changes the state and the variance of every later pose, so the decisions are sequential and the
   ungated trace of gsf_ekf_noise_sweep_dev is right only up to the first rejection: this entry runs the gated filter itself, for K gates
   at once.  The reference has no such step; nothing of its flow changes.
   In: ts, pos, quat, gps, valid, offsets, run_status, init_pos, init_quat, cfg as in gsf_ekf_noise_sweep_dev (cfg's own noise is used);
   gates[K] = the thresholds, a DEVICE array shared by all tracks, 1 <= K <= 64; arm_seconds; max_run.
   For track b and gate k the position filter runs exactly as defined at gsf_ekf_noise_sweep_dev (dt, avail, d[i], Pp, S, g and the
   sharp-turn blend w) with one change.  At a pose i with avail[i]:
   - nis[i] = (y0^2 / S0 + y1^2 / S1) + y2^2 / S2, from the predicted state of the GATED run.
   - the pose is tested iff ts[i] > ts[0] + arm_seconds; arm_seconds <= 0 tests every update.
   - a tested pose is REJECTED iff nis[i] > gates[k] and the forced-accept rule does not apply.  So a NaN NIS is never rejected, and
     gate = +inf (or NaN) rejects nothing.
   - forced accept: iff max_run > 0 and the max_run available fixes immediately before i were all rejected (poses without a usable fix
     neither count towards the run nor reset it), the pose is applied whatever its NIS and counted in n_forced.  max_run <= 0: no limit.
   - a rejected pose is treated IN EVERY RESPECT as a pose with valid[i] = 0: no update, Pf = Pp; it opens or extends an outage; the
     sharp-turn ballot and the blend weight at the next recovery see it as part of the outage; it may merge with an outage of the data on
     either side.
   That is what makes the entry compose: valid_out is valid with the rejected bytes cleared and every other byte copied (pose 0
   included), and gsf_ekf_fuse_ragged_dev, gsf_ekf_cov_ragged_dev or gsf_eval_errors_batch_dev on valid_out give the gated fusion, its
   covariance and its error.  No fuse kernel knows of the gate.
   Out (each may be NULL), P = offsets[B]:
   valid_out[K][P] uint8.
   nis_out[K][P] = the NIS at every pose with avail -- tested or not, rejected or not -- NaN elsewhere.
   stats[B][K][8] = { n_avail;  n_tested;  n_rejected;  n_forced;  the longest run of consecutive rejected available fixes;  the index of
     the first rejected pose relative to the track, -1: none;  the largest NIS among the tested poses that were applied (0: none);  their
     NIS sum }.  The first six are exact counts.  A forced accept is a tested pose that was applied: its NIS is in the last two.  A NaN NIS
     of such a pose makes the sum NaN and leaves the maximum alone.
   gate_status[B] = GSF_GATE_* bits, or'ed over the track's K gates.
   A track with run_status[b] != 0 gets GSF_GATE_SKIPPED: NaN rows (stats and nis_out), valid_out bytes 0, and its inputs are not read.
   An empty track gets GSF_GATE_EMPTY and rows of zeros with first = -1.  Stamps that are not non-decreasing, or a NaN stamp
   (GSF_GATE_UNSORTED, the test of GSF_OS_UNSORTED): NaN rows, valid_out = valid.
   A gate's rows do not depend on K, on the other gates, on their order or on the other tracks: they are the same bytes in every call
   that holds the gate.  One wave per (track, gate), 64 poses per chunk, 89 B read per pose; a chunk is scanned once plus once per
   rejection in it (speculate and repair: of the lanes over the gate the lowest has seen only settled decisions), so at most 65 times.
   B x K words of the context's kernel workspace.  Device pointers, asynchronous on the context's stream.  There is no host-pointer
   form: the Python binding uploads host arrays itself. */
#define GSF_GATE_SKIPPED 1        /* run_status[b] != 0: NaN rows, valid_out bytes 0, inputs not read */
#define GSF_GATE_EMPTY 2          /* the track has no pose */
#define GSF_GATE_UNSORTED 4       /* the track's stamps are not non-decreasing, or one is NaN: NaN rows, valid_out = valid */
#define GSF_GATE_ANY_REJECTED 8   /* at least one gate rejected a fix of the track */
#define GSF_GATE_ANY_FORCED 16    /* at least one gate applied a fix by the forced-accept rule */
GSF_API int gsf_innovation_gate_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const double *gps,
                                    const uint8_t *valid, const int64_t *offsets, const int32_t *run_status, const double *init_pos,
                                    const double *init_quat, const gsf_ekf_config *cfg, int64_t B, const double *gates, int32_t K,
                                    double arm_seconds, int32_t max_run, uint8_t *valid_out, double *nis_out, double *stats,
                                    int32_t *gate_status);

/* ---- streaming fusion: append poses to live tracks, finished rows marked ------------------------------------------------------------------
   Every fuse entry above takes a whole track and returns a whole track.  The filter itself is a recursion with a small state, and only an
   open outage reaches back (the RTS back-pass, EKFGPSSLAM.py:906-922), as far as the outage's first pose.  A STREAM is a set of B tracks that
   can be continued: the cost of an append depends on the new poses only, and every call says which rows are final.

   The whole state of a stream lives in caller-owned DEVICE buffers.  No handle, no allocation inside the library.  There is no host-pointer
   form (a stream that crossed PCIe with its ring on every call would cost what it saves): a binding uploads its segment itself, as the
   Python one does, and examples/stream_track.c shows it from plain C.
     state_f64[GSF_STREAM_F64 * B], state_i64[GSF_STREAM_I64 * B]: opaque; field-major (field k of track b at [k * B + b]).  The layout
       version and cap are stored in the state and checked by every append: a state of another version or ring size is refused with
       GSF_STREAM_BAD_STATE (NaN rows, counters 0, nothing written).  The state is exact float64 / int64, so it is a checkpoint: copy the
       buffers and the ring anywhere, continue there, and get the same bits.
     ring_t[B][cap], ring_pos[B][cap][3], ring_quat[B][cap][4]: the history ring, stamps and fused poses; global pose index i of track b
       lives in slot i % cap.  It need not be initialised.

   gsf_stream_open_dev: zero poses seen; init_pos[B][3] / init_quat[B][4] mean what they mean at gsf_ekf_fuse_ragged_dev (the Sim3-transformed
     pose 0).  track_mask[B] (may be NULL = all): only the tracks with a non-zero byte are (re-)opened, the others are left untouched.
   gsf_stream_append_dev: ts / pos / quat / gps / valid are flat ragged arrays as at gsf_ekf_fuse_ragged_dev (original SLAM poses, time-aligned
     fixes, mask); track b contributes rows seg_offsets[b] .. seg_offsets[b+1], possibly none (the no-op).  Each track's filter continues
     exactly where it stopped: how a track is cut into segments does not change one bit of any output.  Outputs, each may be NULL:
       pos_out / quat_out  the fused rows of this segment as they stand when the call ends (the segment's ragged shape);
       cov_out[.][7]       the filtered covariance diagonal after each pose of the segment (cov_filt of gsf_ekf_cov_ragged_dev);
       n_total[B]          poses the track holds;
       n_final[B]          rows [0, n_final) will never be written again: the open outage's first pose, else n_total;
       revised_from[B]     the smallest global index this call wrote: n_total before the call, or the start of an outage whose back-pass
                           reached further back;
       status[B]           the accumulated GSF_ST_* bits as of now (GSF_ST_ENDED_IN_OUTAGE = an outage is open at this moment) | GSF_STREAM_*.
     CAPACITY.  A back-pass reads the rows of its outage, so a ring slot must not be reused while it can still be read.  Before any work a
     track with (outage open ? n_total - outage start : 0) + segment length > cap is refused with GSF_STREAM_FULL: state and ring untouched,
     its segment rows NaN, counters as before the call, the other tracks proceed.  An RTS segment is never silently truncated; a stream that
     stays within capacity is the reference's filter.  Remedies: a larger cap (a new stream), shorter segments, or re-opening that track.
   gsf_stream_gather_dev: rows [lo[b], lo[b] + out_offsets[b+1] - out_offsets[b]) of each track's ring into ragged ts_out / pos_out / quat_out
     (each may be NULL); rows outside [n_total - cap, n_total) are NaN.  This is how a caller fetches revised or final rows.
   One launch each, lane per track, asynchronous on the context's stream. */
#define GSF_STREAM_F64 22
#define GSF_STREAM_I64 6
#define GSF_STREAM_LAYOUT_VERSION 1
#define GSF_STREAM_FULL 256       /* this call's segment was refused by the capacity rule */
#define GSF_STREAM_BAD_STATE 512  /* the state was not written by this layout version for this cap */
GSF_API int gsf_stream_open_dev(gsf_ctx *ctx, int64_t B, int64_t cap, const double *init_pos, const double *init_quat,
                                const uint8_t *track_mask, double *state_f64, int64_t *state_i64);
GSF_API int gsf_stream_append_dev(gsf_ctx *ctx, const gsf_ekf_config *cfg, int64_t B, int64_t cap, double *state_f64, int64_t *state_i64,
                                  double *ring_t, double *ring_pos, double *ring_quat, const double *ts, const double *pos,
                                  const double *quat, const double *gps, const uint8_t *valid, const int64_t *seg_offsets,
                                  double *pos_out, double *quat_out, double *cov_out, int64_t *n_total, int64_t *n_final,
                                  int64_t *revised_from, int32_t *status);
GSF_API int gsf_stream_gather_dev(gsf_ctx *ctx, int64_t B, int64_t cap, const int64_t *state_i64, const double *ring_t,
                                  const double *ring_pos, const double *ring_quat, const int64_t *lo, const int64_t *out_offsets,
                                  double *ts_out, double *pos_out, double *quat_out);

/* ---- streaming fusion with a fixed-lag RTS smoother ----------------------------------------------------------------------------------------
   gsf_stream_append_dev returns the causal filter: where GNSS is present row i uses no fix after stamp i.  gsf_stream_append_lag_dev is a
   SUPERSET of it -- every argument of that entry with the same meaning, the same outputs, state and ring bit for bit -- that also smooths
   every row with the fixes of the next `lag` rows, at a cost that depends on lag and the new poses, never on the history.
   With the forward quantities of gsf_ekf_smooth_ragged_dev (xf, Pf filtered; xp, Pp predicted; g = xf - xp; a span starts at row 0 and at
   every sharp-turn recovery), row i of a track that holds n poses, s(i) the last row of i's span:
       we(i) = min(i + lag, s(i), n - 1);   e = d = 0 at we(i);   for k = we(i) - 1 .. i:
           A[k] = Pf[k] / Pp[k+1]  (0 where Pp[k+1] == 0),   e = A[k] (e + g[k+1]),   d = A[k]^2 (d + Pf[k+1] - Pp[k+1])
       xs[i] = xf[i] + e,   Ps[i] = Pf[i] + d
   i.e. rts_smoother_segment on rows [i .. we(i)], row i of the whole-track smoother run on the prefix [0 .. min(i + lag, n - 1)].  Rows that no
   later fix of their span reaches inside the window keep xf, Pf exactly; a zero-variance axis comes back unsmoothed, free of NaN.  The
   orientation is never touched by a fix: row i's quaternion is the ring's, no smoothed quaternion is produced.
   Row i is FINAL once i + lag <= n - 1: n_smooth_final = max(0, n - lag).  The rows above are PROVISIONAL: the whole-track smoother's answer
   on what has arrived so far, rewritten by every call.  How a track is cut into calls does not change one bit of a final row, of
   smooth_from / n_smooth_final, or of the three rings at equal n_total.
     lag                 1 .. GSF_STREAM_LAG_MAX.  A property of a stream's life: a final row is the row of the lag in force when it became
                         final; rows that were final are not revisited when a later call names another lag.
     ring_lag[B][cap][GSF_STREAM_LAG_F64]   opaque: the forward quantities of every row the ring holds.  Need not be initialised.
     ring_spos[B][cap][3], ring_svar[B][cap][3]   smoothed position and variance of every row the ring holds (slot i % cap), final below
                         n_smooth_final, provisional above.  The layout of ring_pos: gsf_stream_gather_dev fetches either in ring_pos's place.
   New outputs, each may be NULL:
     spos_out[P][3], svar_out[P][3], sflags_out[P] (uint8)   the rows that BECAME FINAL IN THIS CALL, in the segment's ragged shape: row j of
                         track b's segment is final row smooth_from[b] + j (a call on m poses finalises at most m rows); the rest of the
                         segment's rows are NaN, flags 0.  Flags: GSF_POSE_SMOOTHED (a later fix inside the window was applied) and
                         GSF_POSE_SPAN_START.
     smooth_from[B], n_smooth_final[B]   the number of final rows before and after the call.
   CAPACITY.  A track is refused with GSF_STREAM_FULL if gsf_stream_append_dev's rule refuses it or if min(lag, n_total) + segment length
   > cap (the rows a call's back-pass rewrites need a slot each).  A refused track and one with a bad state leave all three new rings
   untouched; their new output rows are NaN.
   Two launches on the context's stream: the append (lane per track) and the back-pass (wave per track, lane = row, <= lag + m rows).  The
   context keeps 16 bytes per track of workspace between the two (allocated on the first call, gsf_trim releases it). */
#define GSF_STREAM_LAG_MAX 512
#define GSF_STREAM_LAG_F64 12
GSF_API int gsf_stream_append_lag_dev(gsf_ctx *ctx, const gsf_ekf_config *cfg, int64_t B, int64_t cap, int64_t lag, double *state_f64,
                                      int64_t *state_i64, double *ring_t, double *ring_pos, double *ring_quat, double *ring_lag,
                                      double *ring_spos, double *ring_svar, const double *ts, const double *pos, const double *quat,
                                      const double *gps, const uint8_t *valid, const int64_t *seg_offsets, double *pos_out, double *quat_out,
                                      double *cov_out, int64_t *n_total, int64_t *n_final, int64_t *revised_from, int32_t *status,
                                      double *spos_out, double *svar_out, uint8_t *sflags_out, int64_t *smooth_from, int64_t *n_smooth_final);

/* ---- local Sim3 alignment: windowed knots against SLAM scale drift ------------------------------------------------------------------------
   The chain fits ONE Sim3 per track (EKFGPSSLAM.py:973-1006) and applies its scale to the whole run, while a monocular front end drifts in
   scale over minutes.  These two entries fit Sim3 KNOTS on a time grid along each track and map every pose by a blend of the neighbouring
   knots.  The locally aligned track is a track like any other: handed to gsf_ekf_fuse_ragged_dev (and the sweep, outage and gate entries)
   as the motion source it scales the filter's increments by the local scale, because calculate_relative_pose is linear in the positions
   and invariant under a common rotation.  No fuse kernel knows of it; the reference has no such step and nothing of its flow changes.
   In, per track b = rows offsets[b] .. offsets[b + 1]: ts, pos[.][3], quat[.][4] of the original SLAM track; gps[.][3] / valid as
   dynamic_time_alignment returns them (NaN allowed); the track's global R[9], t[3], s.  A row is USABLE when valid != 0 and its fix is
   finite (the rule of gsf_sim3_fit_rows_batch_dev).
   [grid]  t0 = ts[first];  K_b = floor((ts[last] - t0) / spacing) + 2;  tau_k = fma(k, spacing, t0): every pose has a knot on each side.
     Kmax = the caller's knot stride, 1 .. 4096: knot k of track b is slot b * Kmax + k of every knot array.
     K_b > Kmax gives GSF_LOC_TOO_MANY, stamps that decrease inside a track (or a NaN stamp) GSF_LOC_UNSORTED, a track of 0 poses
     GSF_LOC_EMPTY.  A track with any of these gets NaN rows and n_knots = 0; it is never truncated.
   [window]  of knot k: the usable rows with -half_window <= (ts - tau_k) <= half_window, in double precision, the difference formed first.
   [fit]  a_i / b_i the window's SLAM rows / fixes minus their means, H = sum a_i b_i^T:
     GSF_LOC_SCALE (mode 0): R_k = the track's global R;  s_k = tr(R H) / sum |a_i|^2;  t_k = mean(b) - s_k R mean(a).  min_rows >= 2.
       Well posed on a straight road, where the rotation of a full fit is not.
     GSF_LOC_SIM3 (mode 1): the closed form of :436-451 as gsf_sim3_umeyama_batch_dev computes it from shifted raw moments (the scale
       carries sigma1 + sigma2 + sigma3 as :444 is written).  min_rows >= 3.  A knot whose window is rotation-open,
       (sigma2 + d sigma3) <= rot_open sigma1 (d = -1 where :441 flips), takes the mode-0 form and is flagged GSF_KNOT_ROT_FALLBACK.
   [validity]  a knot is valid unless GSF_KNOT_FEW (fewer than min_rows rows), GSF_KNOT_VAR0 (sum |a_i|^2 / n < 1e-12) or GSF_KNOT_SCALE
     (s_k <= 1e-6, or s_k / s outside [1 / ratio_max, ratio_max]) is set; a NaN fails every one of these tests.
   Per knot: knot_R[9], knot_t[3], knot_s, knot_n (rows in the window), knot_rms (RMS of T_k(pos_i) - gps_i over them), knot_flags.  An
   invalid knot keeps knot_n and its flags and gets NaN for the rest.  [slots]  Slots k >= n_knots[b] are NaN-FILLED (knot_n = 0,
   knot_flags = 0): every call writes every byte of the B x Kmax knot arrays.
   [neighbours]  of a pose with k = min(floor((ts - t0) / spacing), K_b - 2): L = the nearest valid knot <= k, Rr = the nearest valid
     knot >= k + 1.  Both: w = (ts - tau_L) / (tau_Rr - tau_L), GSF_LP_BRIDGED when Rr - L > 1.  One: that knot alone, GSF_LP_HELD.  None:
     the global transform, GSF_LP_GLOBAL.
   [blend]  T_k(p) = s_k R_k p + t_k in the operation order of gsf_apply_sim3_batch_dev.
     pos' = T_L(p) + w (T_Rr(p) - T_L(p)) -- this form, so equal knots return T_L(p) to the bit;
     quat' = quaternion_nlerp(R_L (x) q, R_Rr (x) q, w) (:94-105), R (x) q as gsf_apply_sim3_batch_dev forms it; where the two products
     are the same numbers the result is that product itself.  A quaternion whose norm is 0 / NaN / inf gives a NaN quaternion and
     GSF_LP_BAD_QUAT.  scale_at = s_L + w (s_Rr - s_L).
   A pose of a track whose track_status is not 0 gets NaN rows and GSF_LP_TRACK.
   gsf_sim3_local_apply_dev takes knots from anywhere -- a caller may edit them or feed its own -- and reads exactly the fields the fit
   writes: knot_R, knot_t, knot_s, knot_flags (the validity bits), n_knots, track_status.  With every knot of a track equal to its global
   transform, pos_out / quat_out are the bytes of gsf_apply_sim3_batch_dev and scale_at is s.
   Nothing outside rows offsets[b] .. offsets[b + 1] of a per-pose array is written.  One wave per (track, knot) for the fit, no LDS, no
   atomics; one thread per pose for the blend; 2 x B x Kmax words of the context's kernel workspace (the neighbour tables).  Device
   pointers, asynchronous on the context's stream.  There is no host-pointer form: the Python binding uploads host arrays itself. */
typedef struct gsf_local_config {
    int32_t mode;          /* GSF_LOC_SCALE / GSF_LOC_SIM3                                  [fit] */
    int32_t min_rows;      /* fewest usable rows of a window: >= 2 (mode 0), >= 3 (mode 1)  [fit] */
    double spacing;        /* seconds between knots, > 0                                    [grid] */
    double half_window;    /* seconds on either side of a knot, >= 0                        [window] */
    double rot_open;       /* mode 1: rotation-open threshold, default 1e-3                 [fit] */
    double ratio_max;      /* largest s_k / s and s / s_k of a valid knot, >= 1, default 2  [validity] */
} gsf_local_config;
#define GSF_LOC_SCALE 0           /* gsf_local_config.mode: scale and translation per knot under the global rotation   [fit] */
#define GSF_LOC_SIM3 1            /* ... the full closed form per knot, mode 0 where the window is rotation-open       [fit] */
#define GSF_LOC_EMPTY 1           /* track_status: the track has no pose                                               [grid] */
#define GSF_LOC_UNSORTED 2        /* ... its stamps are not non-decreasing, or one is NaN                              [grid] */
#define GSF_LOC_TOO_MANY 4        /* ... K_b > Kmax                                                                    [grid] */
#define GSF_LOC_SKIPPED 8         /* ... set by a caller for a track it wants passed through as NaN rows (the Python binding: run_status != 0) */
#define GSF_KNOT_FEW 1            /* knot_flags: fewer than min_rows usable rows in the window                         [validity] */
#define GSF_KNOT_VAR0 2           /* ... sum |a_i|^2 / n < 1e-12                                                       [validity] */
#define GSF_KNOT_SCALE 4          /* ... s_k <= 1e-6 or s_k / s outside [1 / ratio_max, ratio_max]                     [validity] */
#define GSF_KNOT_ROT_FALLBACK 8   /* ... mode 1, rotation-open window: fitted in the mode-0 form (the knot is valid)   [fit] */
#define GSF_LP_BRIDGED 1          /* pose_flags: the two knots are not adjacent (Rr - L > 1)                           [neighbours] */
#define GSF_LP_HELD 2             /* ... one valid knot on one side only: that knot alone                              [neighbours] */
#define GSF_LP_GLOBAL 4           /* ... no valid knot on either side: the global transform                            [neighbours] */
#define GSF_LP_BAD_QUAT 8         /* ... the pose's quaternion could not be normalised: NaN quaternion                 [blend] */
#define GSF_LP_TRACK 16           /* ... the track's status is not 0: NaN row */
GSF_API int gsf_sim3_local_fit_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *gps, const uint8_t *valid,
                                   const int64_t *offsets, int64_t B, const double *R, const double *t, const double *s,
                                   const gsf_local_config *cfg, int32_t Kmax, double *knot_R, double *knot_t, double *knot_s,
                                   int32_t *knot_n, double *knot_rms, int32_t *knot_flags, int32_t *n_knots, int32_t *track_status);
GSF_API int gsf_sim3_local_apply_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *offsets,
                                     int64_t B, const double *R, const double *t, const double *s, double spacing, int32_t Kmax,
                                     const double *knot_R, const double *knot_t, const double *knot_s, const int32_t *knot_flags,
                                     const int32_t *n_knots, const int32_t *track_status, double *pos_out, double *quat_out,
                                     double *scale_at, int32_t *pose_flags);

/* ---- antenna lever arm: fit the GNSS offset per track, take it out of fixes ---------------------------------------------------------------
   Every other entry treats a fix as a measurement of the pose itself.  On a vehicle the antenna is not at the camera, and a fix measures
       gps_i = s R pos_i + t + R M(q_i) l + noise
   with l the antenna offset in the sensor frame (metres) and M(q) the rotation matrix of the normalised SLAM quaternion (SciPy's
   convention); R M(q_i) is the orientation gsf_apply_sim3_batch_dev writes.  GNSS never touches the quaternion, so the world orientation
   of every pose is known before the filter runs and a fix can be moved from the antenna to the camera in a pre-pass,
   gps'_i = gps_i - R M(q_i) l; every existing entry is then fed those fixes unchanged.  The reference has no such step.
   In, per track b = rows offsets[b] .. offsets[b + 1]: pos[.][3], quat[.][4] of the original SLAM track; gps[.][3] / valid as
   dynamic_time_alignment returns them (NaN allowed); the starting values R[9], t[3], s (the track's global Sim3) and l0[3]; run_status
   (may be NULL).  Stamps are not read.
   [rows]  a row is USABLE when valid != 0, its fix and its position are finite and its quaternion can be normalised (|q| > 1e-9, the
     rule of ExtendedKalmanFilter.normalize_quaternion; a NaN fails every comparison).  n_rows counts them; n_bad_quat counts the rows whose
     only defect is the quaternion.
   [shift]  by the first usable row f:  v_i = pos_i - pos_f,  u_i = R^T (gps_i - gps_f): no UTM-sized number enters a sum.
   [unknowns]  ten: s, c[3] with t = R (c - s pos_f) + gps_f, l[3], a rotation increment dtheta[3].
   [iteration]  from (R, t, s, l0) with phi = 0, for `iters` rounds (1 .. 8; a fixed count, no convergence exit):
     w_i = s v_i + c + M_i l,  r_i = u_i - w_i,  J_i = [ v_i | I | M_i | -[w_i]x ];  N = sum J^T J + priors,  g = sum J^T r + priors;
     priors: weight (sigma_fix / sigma_prior[j])^2 on l_j towards l0_j, (sigma_fix / sigma_rot)^2 on phi + dtheta towards 0, an infinite
     sigma is weight 0;  N d = g by Cholesky on D N D, D = diag(N)^(-1/2);
     s += d_s, c += d_c, l += d_l, phi += d_theta, R <- R exp([d_theta]x) (Rodrigues).
   [switches]  fit_scale = 0 / fit_rotation = 0 pin s / dtheta: the unknown's row and column of N become the identity's, its g entry 0.
   Out, per track: R[9], t[3], s, l[3]; l_cov[9] = the l block of sigma_fix^2 N^-1 of the last round; n_rows, n_bad_quat; rms_before /
   rms_after = the RMS of r_i over the usable rows at the starting / final values (NaN without a usable row); last_step = the largest
   |d_l| component of the last round; flags.
   [flags]  GSF_LEVER_FEW (n_rows < min_rows), GSF_LEVER_VAR0 (sum |v_i - mean v|^2 / n < 1e-12), GSF_LEVER_SINGULAR (in any round a
     pivot of the scaled Cholesky -- the value under its square root -- is <= pivot_min or not finite, or a step is not finite),
     GSF_LEVER_SCALE (after any round s <= 1e-6 or s / s_start outside [1 / ratio_max, ratio_max]) and GSF_LEVER_TRACK (run_status != 0:
     the rows are not read, n_rows = 0): the track keeps its starting R, t, s, l0 BYTE FOR BYTE, l_cov is diag(sigma_prior^2), rms_after =
     rms_before and last_step is NaN.  GSF_LEVER_WEAK_X/Y/Z: l_cov[jj] > weak_ratio sigma_prior[j]^2 (the data did not observe that
     axis; a ground vehicle never observes the one along its yaw axis).  GSF_LEVER_NOT_CONVERGED: last_step > conv_tol.
   Every call writes every output byte.  One wave per track, no LDS, no atomics, no workspace.
   gsf_lever_apply_dev:  xyz_out_i = xyz_i + sign R (M(q_i) l), R[9] and l[3] per track; sign = -1 moves antenna to camera, +1 camera to
   antenna; pass the identity as R when quat is already a world quaternion (a fused one).  A component whose shift is exactly 0 returns
   the input's bytes (so l = 0 returns xyz), a NaN fix stays NaN, a quaternion that cannot be normalised gives a NaN row and
   GSF_LVP_BAD_QUAT (the filter then treats the pose as having no fix).  Nothing outside a track's rows is written.  One thread per pose.
   Device pointers, asynchronous on the context's stream.  There is no host-pointer form: the Python binding uploads host arrays itself. */
typedef struct gsf_lever_config {
    double sigma_fix;       /* noise of a fix, metres (> 0)                                  [iteration] */
    double sigma_prior[3];  /* prior sigma of l about l0 per sensor axis, metres (inf: none) [iteration] */
    double sigma_rot;       /* prior sigma of the accumulated rotation, radians (inf: none)  [iteration] */
    double ratio_max;       /* largest s / s_start and s_start / s, >= 1, default 2          [flags] */
    double pivot_min;       /* smallest pivot of the scaled Cholesky, default 1e-10          [flags] */
    double weak_ratio;      /* l_cov[jj] / sigma_prior[j]^2 above which an axis is weak, default 0.5 */
    double conv_tol;        /* last_step above which a fit is not converged, default 1e-6 m  [flags] */
    int32_t min_rows;       /* fewest usable rows, >= 1, default 8                           [flags] */
    int32_t iters;          /* rounds, 1 .. 8, default 4                                     [iteration] */
    int32_t fit_scale;      /* 0: s stays at its starting value                              [switches] */
    int32_t fit_rotation;   /* 0: R stays at its starting value                              [switches] */
} gsf_lever_config;
#define GSF_LEVER_FEW 1             /* flags: fewer than min_rows usable rows */
#define GSF_LEVER_VAR0 2            /* ... the usable SLAM positions do not move */
#define GSF_LEVER_SINGULAR 4        /* ... a pivot <= pivot_min or not finite */
#define GSF_LEVER_SCALE 8           /* ... s <= 1e-6 or s / s_start outside [1 / ratio_max, ratio_max] */
#define GSF_LEVER_WEAK_X 16         /* ... l_cov[0] > weak_ratio sigma_prior[0]^2 */
#define GSF_LEVER_WEAK_Y 32         /* ... l_cov[4] > weak_ratio sigma_prior[1]^2 */
#define GSF_LEVER_WEAK_Z 64         /* ... l_cov[8] > weak_ratio sigma_prior[2]^2 */
#define GSF_LEVER_NOT_CONVERGED 128 /* ... last_step > conv_tol */
#define GSF_LEVER_TRACK 256         /* ... run_status != 0 */
#define GSF_LVP_BAD_QUAT 1          /* pose_flags of gsf_lever_apply_dev: the quaternion could not be normalised, NaN row */
GSF_API int gsf_lever_fit_dev(gsf_ctx *ctx, const double *pos, const double *quat, const double *gps, const uint8_t *valid,
                              const int64_t *offsets, int64_t B, const double *R, const double *t, const double *s, const double *l0,
                              const int32_t *run_status, const gsf_lever_config *cfg, double *R_out, double *t_out, double *s_out,
                              double *l_out, double *l_cov, int32_t *n_rows, int32_t *n_bad_quat, double *rms_before, double *rms_after,
                              double *last_step, int32_t *flags);
GSF_API int gsf_lever_apply_dev(gsf_ctx *ctx, const double *quat, const double *xyz, const int64_t *offsets, int64_t B, const double *R,
                                const double *l, double sign, double *xyz_out, int32_t *pose_flags);

/* ---- pose queries: the fused track at any stamp, sensor points into the track's frame ----------------------------------------------------
   The fused track exists at the SLAM stamps; LiDAR returns, other exposures, map points and a second receiver have stamps of their own.
   These entries evaluate the track between its poses with the rule the filter itself uses for orientations (quaternion_nlerp,
   EKFGPSSLAM.py:94-105) and, for points, carry a sensor-frame point through its extrinsics and the interpolated pose.
   Tracks are given as the ragged entries give them: ts[P], pos[P][3], quat[P][4], offsets int64[B+1].  Queries are ragged per track:
   q_t[M], q_offsets int64[B+1] (query m belongs to track b with q_offsets[b] <= m < q_offsets[b+1]); they need not be sorted.  M is
   passed by the host.  All indexing is int64.
   Per track, track_state[B] (required output) holds GSF_QT_* bits; 0 = usable:
   - GSF_QT_SKIPPED: run_status != NULL && run_status[b] != 0.  The track's rows are not read and no other bit is set.
   - GSF_QT_EMPTY: the track has 0 poses.
   - GSF_QT_UNSORTED: ts[0] is NaN, or !(ts[i] >= ts[i-1]) for some i inside the track (a NaN stamp counts).
   - GSF_QT_BAD_EXTRINSIC (points entry only): ext_q[b] has a norm that is 0, NaN or infinite (Rotation.from_quat raises).
   Per query tau of track b (n poses, stamps t[0..n-1]), q_flags[M] holds GSF_Q_* bits and the outputs are:
   - track_state[b] != 0: NaN, GSF_Q_TRACK (also a query that q_offsets assigns to no track).
   - tau is NaN: NaN, GSF_Q_NAN.   tau < t[0]: NaN, GSF_Q_BEFORE.   tau > t[n-1]: NaN, GSF_Q_AFTER.  There is no extrapolation.
   - otherwise i = #{k : t[k] <= tau} - 1 = np.searchsorted(t, tau, side='right') - 1 (among equal stamps: the last one), and
     - t[i] == tau: pose i copied bit for bit, GSF_Q_EXACT; pose i + 1 is not read, so a NaN neighbour cannot leak in;
     - else j = i + 1 (it exists and t[j] > t[i]), gap = t[j] - t[i]:
       - max_gap > 0 && gap > max_gap: NaN, GSF_Q_GAP (nobody interpolates across a tracking loss);
       - else w = (tau - t[i]) / gap (two subtractions and one IEEE division), pos_c = fma(w, p_j,c - p_i,c, p_i,c),
         quat = quaternion_nlerp(q_i, q_j, w) (:94-105: sign flip on a negative dot product, clip of w, and q_i / q_j by w < 0.5 where the
         blend's norm is below 1e-9); flags 0.
   Optional outputs (may be NULL): q_index[M] = i relative to the track's first pose, -1 where the query has no bracket (GSF_Q_GAP keeps
   its i); q_pose_flags[M] = pose_flags[i] | pose_flags[j] (exact hit: pose_flags[i]; no bracket: 0) when the GSF_POSE_* flags of
   gsf_ekf_cov_ragged_dev are passed as pose_flags[P] (may be NULL): "was this point georeferenced through a dead-reckoned stretch".
   A query's result does not depend on the other queries of the call, nor on their order.  B == 0 or M == 0: nothing is done, GSF_OK.
   Two launches on the context's stream (track_state, then the queries); no workspace. */
#define GSF_QT_EMPTY 1
#define GSF_QT_UNSORTED 2
#define GSF_QT_SKIPPED 4
#define GSF_QT_BAD_EXTRINSIC 8
#define GSF_Q_EXACT 1      /* the query hit a pose's stamp: that pose, bit for bit */
#define GSF_Q_BEFORE 2
#define GSF_Q_AFTER 4
#define GSF_Q_GAP 8
#define GSF_Q_NAN 16
#define GSF_Q_TRACK 32
#define GSF_Q_BAD_QUAT 64  /* points entry only: the pose's quaternion at tau cannot be normalised (norm 0, NaN or infinite): NaN row */
/* Out: out_pos[M][3], out_quat[M][4] (the blend is normalised by quaternion_nlerp; an exact hit returns the stored quaternion as it is). */
GSF_API int gsf_pose_query_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *offsets,
                               const int32_t *run_status, const uint8_t *pose_flags, int64_t B, const double *q_t, const int64_t *q_offsets,
                               int64_t M, double max_gap, double *out_pos, double *out_quat, uint8_t *q_flags, int32_t *q_index,
                               uint8_t *q_pose_flags, int32_t *track_state);
/* Points: x[M][3] in the sensor frame, stamped by q_t.  ext_q[B][4] / ext_t[B][3] = sensor -> body per track (NULL: identity / zero);
   scale[B] (NULL: 1): map points in SLAM units pass the run's s, a metric sensor passes nothing.  With p(tau), q(tau) as above:
     y = scale * (R(ext_q / |ext_q|) x + ext_t);   qh = q(tau) / |q(tau)| (fails: NaN row, GSF_Q_BAD_QUAT or'ed in);   out_xyz = p(tau) + R(qh) y.
   R(.) x is Rotation.apply of the unit quaternion.  Rows without a pose (the NaN cases above) are NaN with the same flags. */
GSF_API int gsf_georef_points_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *offsets,
                                  const int32_t *run_status, const uint8_t *pose_flags, int64_t B, const double *q_t, const int64_t *q_offsets,
                                  int64_t M, double max_gap, const double *x, const double *ext_q, const double *ext_t, const double *scale,
                                  double *out_xyz, uint8_t *q_flags, int32_t *q_index, uint8_t *q_pose_flags, int32_t *track_state);
/* the same with host arrays: staged upload, the two launches, download */
GSF_API int gsf_pose_query(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *offsets,
                           const int32_t *run_status, const uint8_t *pose_flags, int64_t B, const double *q_t, const int64_t *q_offsets,
                           int64_t M, double max_gap, double *out_pos, double *out_quat, uint8_t *q_flags, int32_t *q_index,
                           uint8_t *q_pose_flags, int32_t *track_state);
GSF_API int gsf_georef_points(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *offsets,
                              const int32_t *run_status, const uint8_t *pose_flags, int64_t B, const double *q_t, const int64_t *q_offsets,
                              int64_t M, double max_gap, const double *x, const double *ext_q, const double *ext_t, const double *scale,
                              double *out_xyz, uint8_t *q_flags, int32_t *q_index, uint8_t *q_pose_flags, int32_t *track_state);

/* ---- trajectory evaluation: absolute / relative pose error and KITTI's segment errors against 6-DoF truth ---------------------------------
   gsf_eval_errors_batch_dev (step 6) grades positions against the GNSS fixes the filter was fed.  This entry grades whole poses against a
   truth trajectory of its own (KITTI ground truth, a survey, a simulator), after an alignment, as evo and the KITTI devkit do.
   Estimate: ts[P], pos[P][3], quat[P][4], offsets int64[B+1] as every ragged entry takes them; P (the rows of the per-pose arrays) is
   passed by the host.  Truth per track: ref_ts[G], ref_pos[G][3], ref_quat[G][4], ref_offsets int64[B+1].  All indexing is int64; all
   pointers are device pointers; the call is asynchronous on the context's stream.  Quaternions are [x, y, z, w].
   Track state, track_state[B], GSF_TE_TRACK_* bits, 0 = evaluated:
   - SKIPPED: run_status != NULL && run_status[b] != 0.  Neither the track's rows nor its truth are read; no other bit is set.
   - EMPTY: the track has no poses or no truth poses.
   - UNSORTED: ts[0] or ref_ts[0] of the track is NaN, or !(x[i] >= x[i-1]) inside either stamp array (a NaN stamp counts, as in
     GSF_QT_UNSORTED).  Decided before anything is searched.
   - FEW: align_mode is _SE3 / _SIM3 and fewer than 3 poses are matched.   - DEGENERATE: the closed form returns GSF_SIM3_NONE.
   Any bit: R, t, s of the track are NaN, ape_t / ape_r of its poses are NaN, ape_stats holds n = 0 and NaN, rpe_n = 0 with zero sums.
   Under SKIPPED / EMPTY / UNSORTED every pose has pose_flags GSF_TE_TRACK and match_index -1; under FEW / DEGENERATE pose_flags and
   match_index keep what the association found.
   Association, per estimate pose i of a usable track (checked in this order; the first failure is the flag, the per-pose outputs are NaN
   and match_index is -1):
   - the position holds a NaN or an infinity: GSF_TE_NAN;   - the quaternion's norm is 0, NaN or infinite: GSF_TE_BAD_QUAT;
   - GSF_TE_NEAREST: the truth pose j with the smallest |ref_ts[j] - ts[i]|, on a tie the earlier j, among equal truth stamps the first;
     matched when that difference is <= max_diff, else GSF_TE_NO_TRUTH.  Two estimate poses may match the same truth pose; both are kept.
     match_index = j, relative to the track's first truth pose.
   - GSF_TE_INTERP: the truth pose at ts[i] by the rule of gsf_pose_query_dev with max_gap = max_diff (position linear, orientation
     quaternion_nlerp, an exact stamp is that pose bit for bit); before the first / after the last truth stamp or across a bracket wider
     than max_diff (> 0): GSF_TE_NO_TRUTH.  match_index = the bracket's i.
   - the truth position holds a NaN or an infinity: GSF_TE_NAN;   the truth quaternion cannot be normalised: GSF_TE_BAD_QUAT;
   - else GSF_TE_MATCHED.  Both quaternions of the pair are normalised once.
   Alignment over the matched pairs (src = estimate, dst = truth): GSF_TE_ALIGN_NONE: identity, s = 1.  _SIM3: centroids, centred moments,
   the Umeyama closed form by its SVD route (compute_sim3_transform, EKFGPSSLAM.py:436-451, scale rules included).  _SE3: that rotation,
   s = 1, t = dc - R sc.  The aligned estimate is p' = s R p + t, q' = q_R (x) q (transform_trajectory, :461-468).
   Absolute errors per matched pose: ape_t = |p' - g|; ape_r = the angle of conj(q_g) (x) q' as 2 atan2(|v|, |w|), radians in [0, pi].
   ape_stats[B][2][8] (0: translation, 1: rotation) = {n, mean, median, rmse, std, min, max, sse} of the track's matched poses, evo's
   statistics: std is np.std (ddof 0) in two passes; median (the mean of the two middle values for an even n), min and max are exact order
   statistics of the per-pose values returned.
   Relative errors: K >= 0 scenarios (rpe_kind[K], rpe_value[K], rpe_stride int64[K]) over the matched poses m = 0 .. M-1 of a track, in
   order; d[m] = the truth path length over matched poses.  First frames f = 0, stride, 2 stride, ... (stride < 1: no pair); last frame:
   - GSF_TE_FRAMES: l = f + (int64) value (value < 1: no pair);
   - GSF_TE_METRES: the smallest l > f with d[l] > d[f] + value (KITTI's lastFrameFromSegmentLength);
   - GSF_TE_SECONDS: the smallest l > f with ts[l] >= ts[f] + value;   no such l < M: no pair.
   Pair error E = (g_f^-1 g_l)^-1 (e'_f^-1 e'_l): et = |E.t|, er = the angle of E.R (the same atan2 form).
   rpe_n int64[B][K] = pairs; rpe_sums[B][K][8] = {sum et, sum et^2, max et, sum er, sum er^2, max er, sum et / value, sum er / value}; the
   last two for GSF_TE_METRES only, NaN otherwise; no pair: zeros.  Sums are reduced in a fixed order: a track's results do not depend on
   the other tracks or scenarios of the call.  With 0 <= trace_k < K the optional outputs (each may be NULL; rpe_t / rpe_r are written only
   with rpe_last) hold, at the estimate row of every first frame of scenario trace_k that has a pair, rpe_last = the estimate row of l
   relative to the track's first pose, rpe_t = et, rpe_r = er; every other row is -1 / NaN.
   K == 0: the scenario arrays may be NULL.  B == 0: nothing is done, GSF_OK.  Three launches (association; alignment, absolute errors and
   statistics; scenarios -- not launched for K == 0); scratch (16 doubles and one int32 a pose = 132 bytes, 8 bytes a
   track, 8 bytes) from the context's kernel workspace.
   Input range: positions whose differences, and whose products with s R, stay below 1e150 in magnitude, so that no square overflows.
   Beyond it a matched pose's error can come out infinite or NaN; a NaN error is left out of the sums, min, max and median of ape_stats
   while n still counts the pose, and moments that overflow give GSF_TE_TRACK_DEGENERATE -- in range the closed form's SVD route
   always returns a fit (a collinear or a single-point cloud included), so DEGENERATE marks exactly that overflow. */
#define GSF_TE_NEAREST 0
#define GSF_TE_INTERP 1
#define GSF_TE_ALIGN_NONE 0
#define GSF_TE_ALIGN_SE3 1
#define GSF_TE_ALIGN_SIM3 2
#define GSF_TE_FRAMES 0
#define GSF_TE_METRES 1
#define GSF_TE_SECONDS 2
#define GSF_TE_MATCHED 1
#define GSF_TE_NO_TRUTH 2
#define GSF_TE_NAN 4
#define GSF_TE_BAD_QUAT 8
#define GSF_TE_TRACK 16
#define GSF_TE_TRACK_SKIPPED 1
#define GSF_TE_TRACK_EMPTY 2
#define GSF_TE_TRACK_UNSORTED 4
#define GSF_TE_TRACK_FEW 8
#define GSF_TE_TRACK_DEGENERATE 16
/* Out: R[B][9] row-major, t[B][3], s[B], track_state[B], pose_flags uint8[P], match_index int32[P], ape_t[P], ape_r[P],
   ape_stats[B][2][8], rpe_n int64[B][K], rpe_sums[B][K][8]; optional rpe_last int32[P], rpe_t[P], rpe_r[P]. */
GSF_API int gsf_traj_eval_dev(gsf_ctx *ctx, const double *ts, const double *pos, const double *quat, const int64_t *offsets, int64_t P,
                              const double *ref_ts, const double *ref_pos, const double *ref_quat, const int64_t *ref_offsets,
                              const int32_t *run_status, int64_t B, int32_t assoc_mode, double max_diff, int32_t align_mode, int32_t K,
                              const int32_t *rpe_kind, const double *rpe_value, const int64_t *rpe_stride, int32_t trace_k, double *R,
                              double *t, double *s, int32_t *track_state, uint8_t *pose_flags, int32_t *match_index, double *ape_t,
                              double *ape_r, double *ape_stats, int64_t *rpe_n, double *rpe_sums, int32_t *rpe_last, double *rpe_t,
                              double *rpe_r);

/* ---- step 7 of main_process_gui (EKFGPSSLAM.py:1085-1104): the corrected track as WGS84 rows and as the bytes of its TUM files ------------
   Rows are flat over P poses with offsets int64[B+1], as in gsf_run_fusion_ragged_dev; any offsets work (a dense batch: b * N). */
/* Rows [E, N, alt] (pos[P][3]) -> rows [lon deg, lat deg, alt] (lonlatalt[P][3]): utm_to_wgs84(corrected_pos, projector) (:1097, :291-296),
   with projector = the primary log's zone / hemisphere (zone[B], south[B]; :266-283).  lon / lat are bit for bit what
   gsf_utm_inverse_batch_dev (and the host form gsf_utm_inverse) returns for the same E, N -- the same kernel runs; alt is copied (:296).
   run_status (may be NULL): a track with run_status[b] != 0 gets NaN rows and its zone / south are not read. */
GSF_API int gsf_utm_to_wgs84_rows_dev(gsf_ctx *ctx, const double *pos, const int64_t *offsets, const int32_t *zone, const int32_t *south,
                                      const int32_t *run_status, int64_t B, double *lonlatalt);
/* the two np.savetxt formats of step 7 (comments='', fields joined by ' ', every line ends in '\n') */
#define GSF_TUM_UTM 0      /* *_corrected_utm.txt (:1091-1092): fmt ['%.6f'] + ['%.6f']*3 + ['%.8f']*4, header "timestamp x y z qx qy qz qw (UTM)" */
#define GSF_TUM_WGS84 1    /* *_corrected_wgs84.txt (:1098-1101): fmt ['%.6f'] + ['%.8f','%.8f','%.3f'] + ['%.8f']*4,
                              header "timestamp lon lat alt qx qy qz qw (WGS84)" */
#define GSF_TEXT_DEVICE 0  /* track_state: the track's file image was formatted on the device */
#define GSF_TEXT_SKIPPED 1 /* run_status[b] != 0: no file (the reference raised before step 7), 0 bytes */
#define GSF_TEXT_HOST 2    /* a finite value with |x| >= 2^63: 0 bytes here, the caller writes this track with np.savetxt */
/* Byte-exact TUM files of tracks [0, B) of `offsets` (pass offsets + b0 to work in chunks): rows ts[P], xyz[P][3], quat[P][4] (for
   GSF_TUM_WGS84, xyz = the rows of gsf_utm_to_wgs84_rows_dev).  Every field equals Python's '%.{p}f' of the float64 value (what np.savetxt
   writes): the exact binary value rounded half to even, '-0.000000' for -0.0 and negatives that round to zero, 'nan' for a NaN of either
   sign, 'inf' / '-inf'.  Two calls:
   - SIZE (text == NULL): writes text_offsets[B+1] (byte ranges of each track's whole file image: header line, then one line per row; a 0-row
     track gets the header alone) and track_state[B] (GSF_TEXT_*).  run_status may be NULL.
   - WRITE (text != NULL, text_offsets[B] bytes, text_offsets / track_state of the size call with the same rows): writes every byte of those
     ranges and nothing outside [0, text_offsets[B]).
   Both calls derive a row's length from the same routine; the write pass places rows with a wave-wide scan recomputed per 64 rows (no
   workspace).  Offsets must be non-decreasing within [0, P]; reads are clamped into [0, P) whatever they hold. */
GSF_API int gsf_tum_text_dev(gsf_ctx *ctx, int32_t format, const double *ts, const double *xyz, const double *quat, const int64_t *offsets,
                             const int32_t *run_status, int64_t B, int64_t P, int64_t *text_offsets, int32_t *track_state, uint8_t *text);

/* ---- time alignment (dynamic_time_alignment, EKFGPSSLAM.py:325-387) ------------------------------ */
/* B trajectories: SLAM stamps slam_t[slam_offsets[b]..), GNSS fixes gps_t / gps_p[.][3] at gps_offsets (any order, duplicates
   allowed: stable sort + first-of-equal-stamps).  Per gap-free segment (gap > max_gps_gap_threshold splits): not-a-knot cubic
   spline (>= 4 fixes) or linear (2-3 fixes) evaluated at the SLAM stamps inside the segment; aligned[total_slam][3] gets NaN
   elsewhere, valid[total_slam] = 1 where all three components are finite.  max_gps_per_trajectory sizes the per-trajectory staging
   (LDS up to 2560 fixes, a global scratch slab beyond); status[b] (may be NULL) = 1 if trajectory b has more fixes than that and
   was left unaligned. */
GSF_API int gsf_time_align_batch_dev(gsf_ctx *ctx, const double *slam_t, const int64_t *slam_offsets, const double *gps_t,
                                     const double *gps_p, const int64_t *gps_offsets, int64_t B, int32_t max_gps_per_trajectory,
                                     double max_gps_gap_threshold, double *aligned, uint8_t *valid, int32_t *status);
GSF_API int gsf_time_align_batch(gsf_ctx *ctx, const double *slam_t, const int64_t *slam_offsets, const double *gps_t, const double *gps_p,
                                 const int64_t *gps_offsets, int64_t B, double max_gps_gap_threshold, double *aligned, uint8_t *valid,
                                 int32_t *status);
/* The same for a GNSS log that comes straight from gsf_gps_rows_to_utm_batch_dev: rows whose easting AND northing are NaN are the
   rows load_gps_data removes before the projection (EKFGPSSLAM.py:259-264: lat/lon zero or out of range); they are dropped when the
   log is staged, so the alignment sees exactly the fixes the reference's loader hands to dynamic_time_alignment. */
GSF_API int gsf_time_align_loaded_rows_batch_dev(gsf_ctx *ctx, const double *slam_t, const int64_t *slam_offsets, const double *gps_t,
                                                 const double *gps_p, const int64_t *gps_offsets, int64_t B,
                                                 int32_t max_gps_per_trajectory, double max_gps_gap_threshold, double *aligned,
                                                 uint8_t *valid, int32_t *status);

/* ---- clock-offset search: the offset between the SLAM clock and the GNSS clock ----------------------------------------------------------
   The reference's estimate_time_offset (EKFGPSSLAM.py:301-323) correlates two linspace ramps and always returns 0; its workflow takes the
   offset from the keyboard (GPSmerge.py:73-80) and dynamic_time_alignment adds it to the GNSS stamps (:337-338).  This entry sweeps that
   number: for track b (rows slam_offsets[b]..slam_offsets[b+1] of ts[P], pos[P][3]) and candidate k < K,
     tau[b][k] = tau0[b] + (double)k * dtau  (a product and a sum, each rounded once: numpy's tau0 + k * dtau bit for bit; tau0 == NULL: 0);
     fixes used: fix i of log b (gps_offsets, gps_t[G], gps_utm[G][3] = (E, N, alt)) with gps_keep == NULL || gps_keep[i], and not the
       loader's drop mark (easting AND northing NaN, as in gsf_time_align_loaded_rows_batch_dev);
     alignment: dynamic_time_alignment (:325-387) with adjusted_gps_times = gps_t + tau[b][k] (:338), otherwise as gsf_time_align_batch_dev
       (sort, first of equal stamps, gap split at max_gps_gap_threshold, cubic >= 4 fixes, linear 2-3, NaN outside); the splines are
       rebuilt per candidate from the shifted stamps;
     fit rows: the context's row rule (gsf_set_sim3_rows; :973-998 in mode 1), as gsf_fuse_pipeline_ragged_dev applies it;
     fit: compute_sim3_transform (:428-459), src = SLAM positions, dst = aligned fixes;
     J[b][k] = sqrt(mean ||dst_i - (s R src_i + t)||^2) over the fit rows, in metres; n_rows[b][k] (may be NULL) = their number (where the
       row rule raises, :975 / :997: the number of valid rows it found too few).  J = NaN where the reference would raise or return None
       (GSF_SIM3_NONE, GSF_SIM3_FLAG_FEW_ROWS), and where n_rows < min_rows (min_rows <= 0: the row rule's min_samples).
   Per track: best_k[b] = the first k with the smallest non-NaN J (-1: none); tau_best[b] = tau[b][best_k]; tau_refined[b] = the vertex of the
   parabola through (tau, J^2) at best_k - 1, best_k, best_k + 1, tau_best + 0.5 dtau (a - c) / (a - 2m + c), when best_k is interior, both
   neighbours are finite and a - 2m + c > 0, else tau_best (both NaN without a best_k); R[B][9], t[B][3], s[B] (all three may be NULL) = the
   fit of best_k (NaN without one); clk_status[b] = GSF_CLK_* bits.  An empty track gets a NaN row and GSF_CLK_NONE.
   1 <= K <= 4096, any track length; max_fixes >= the longest log sizes the staging (LDS up to 2 560 fixes, beyond that a scratch slab with
   one row per resident workgroup); a longer log is left unaligned (NaN row).  One 64-lane workgroup per (b, k) and one per track for the
   pick; nothing per candidate is written but J and n_rows.  Device pointers, asynchronous. */
#define GSF_CLK_NONE 1     /* no candidate has a fit */
#define GSF_CLK_AT_EDGE 2  /* best_k is 0 or K - 1 with K > 1: the minimum may lie outside the grid, widen it */
#define GSF_CLK_FLAT 4     /* max finite J - min J < flat_threshold: the offset is not observable on this track (a straight constant-velocity
                              run); flat_threshold <= 0 never sets it */
GSF_API int gsf_clock_offset_search_dev(gsf_ctx *ctx, const double *ts, const double *pos, const int64_t *slam_offsets, const double *gps_t,
                                        const double *gps_utm, const uint8_t *gps_keep, const int64_t *gps_offsets, int64_t B, int32_t max_fixes,
                                        const double *tau0, double dtau, int32_t K, double max_gps_gap_threshold, int32_t min_rows,
                                        double flat_threshold, double *J, int32_t *n_rows, int32_t *best_k, double *tau_best, double *tau_refined,
                                        double *R, double *t, double *s, int32_t *clk_status);
/* the same with host arrays (max_fixes is read from gps_offsets): staged upload, the two launches, download */
GSF_API int gsf_clock_offset_search(gsf_ctx *ctx, const double *ts, const double *pos, const int64_t *slam_offsets, const double *gps_t,
                                    const double *gps_utm, const uint8_t *gps_keep, const int64_t *gps_offsets, int64_t B, const double *tau0,
                                    double dtau, int32_t K, double max_gps_gap_threshold, int32_t min_rows, double flat_threshold, double *J,
                                    int32_t *n_rows, int32_t *best_k, double *tau_best, double *tau_refined, double *R, double *t, double *s,
                                    int32_t *clk_status);

/* ---- error evaluation (main_process_gui step 6, EKFGPSSLAM.py:1013-1033) -------------------- */
/* B trajectories x N poses, trajectory-major.  For every index with valid finite aligned GNSS and ts > ts[0] + skip_seconds:
   error = min over all such candidate fixes of |traj_pos[i] - gps[j]| (cdist + min, :1030-1031).
   stats[B][4] = {count, mean, median, rmse} (:1033); errors[B][N] = per-pose error, NaN where not evaluated. */
GSF_API int gsf_eval_errors_batch_dev(gsf_ctx *ctx, const double *ts, const double *traj_pos, const double *aligned_gps,
                                      const uint8_t *valid, int64_t B, int64_t N, double skip_seconds, double *stats, double *errors);
GSF_API int gsf_eval_errors_batch(gsf_ctx *ctx, const double *ts, const double *traj_pos, const double *aligned_gps, const uint8_t *valid,
                                  int64_t B, int64_t N, double skip_seconds, double *stats, double *errors);

/* ---- helper functions of the reference's EKF surface (API completeness; host pointers, synchronous) ------------ */
/* calculate_relative_pose (EKFGPSSLAM.py:77-92) for n pose pairs; bad[i]=1 where the zero-motion branch (:84-86) was taken */
GSF_API int gsf_relative_pose_batch(gsf_ctx *ctx, const double *p1, const double *q1, const double *p2, const double *q2, int64_t n,
                                    double *delta_pos_local, double *delta_quat, int32_t *bad);
/* quaternion_nlerp (EKFGPSSLAM.py:94-105) for n pairs */
GSF_API int gsf_quaternion_nlerp_batch(gsf_ctx *ctx, const double *q1, const double *q2, const double *weight_q2, int64_t n, double *out);
/* is_sharp_turn_in_segment (EKFGPSSLAM.py:808-826) for B ragged segments: result[b] in {0,1}, max_rate[b] rad/s (may be NULL) */
GSF_API int gsf_is_sharp_turn_batch(gsf_ctx *ctx, const double *quats, const double *stamps, const int64_t *offsets, int64_t B,
                                    double yaw_rate_threshold_rad_per_sec, int32_t *result, double *max_rate);
/* one ExtendedKalmanFilter.process_step (EKFGPSSLAM.py:736-772) in the reference's general dense form: state[7], cov[49],
   Q_per_sec[49], R[9]; gnss_available_prev in {-1 None, 0, 1}; gps_meas NULL = None; override_transition_steps < 0 = None */
GSF_API int gsf_ekf_process_step(gsf_ctx *ctx, double *state, double *cov, const double *process_noise_per_sec, const double *meas_noise,
                                 int32_t *gnss_available_prev, double *gnss_update_weight, int32_t current_transition_steps,
                                 const double *delta_pos_local, const double *delta_quat, const double *gps_meas,
                                 int32_t gnss_is_available, double delta_time, int32_t override_transition_steps, double *pred_state,
                                 double *pred_cov);
/* rts_smoother_segment (EKFGPSSLAM.py:777-803), dense 7x7, for B ragged segments (rows offsets[b]..offsets[b+1]) */
GSF_API int gsf_rts_smoother_segment_batch(gsf_ctx *ctx, const double *states_filt, const double *covs_filt, const double *states_pred,
                                           const double *covs_pred, const int64_t *offsets, int64_t B, double *states_smooth,
                                           double *covs_smooth);

/* ---- multi-GPU collect: RCCL all-gather of the fused poses over xGMI ------------------------------- */
/* The reference is single-process (no collective exists in it: filter state is per ExtendedKalmanFilter instance,
   EKFGPSSLAM.py:842); trajectories shard by contiguous id blocks, one process per GPU, and this is the one exchange: every rank
   receives every rank's fused poses.  RCCL is resolved at run time (dlopen).
   gsf_comm_unique_id: 128-byte ncclUniqueId (rank 0 creates it, the host ships it to the other ranks by any side channel);
   gsf_comm_init_rank: collective over all `world` processes, device = the context's; gsf_comm_destroy frees the communicator. */
/* ncclGetVersion of the librccl.so the library resolved (MAJOR*10000 + MINOR*100 + PATCH; 0 = the symbol is missing) */
GSF_API int gsf_comm_rccl_version(int32_t *version);
GSF_API int gsf_comm_unique_id(uint8_t *id128);
GSF_API int gsf_comm_init_rank(gsf_ctx *ctx, const uint8_t *id128, int32_t world, int32_t rank, void **comm);
GSF_API int gsf_comm_destroy(void *comm);
/* All-gather `count` doubles per rank into recv[world][count], asynchronously on the context's stream, on a communicator from
   gsf_comm_init_rank (or any caller-provided ncclComm_t).  mode 0 = one ncclAllGather; mode 1 = direct exchange (grouped
   ncclSend/ncclRecv with every peer, `chunk_count` doubles at a time; 0 = all at once) so all seven point-to-point xGMI links of
   a GPU carry traffic at once. */
GSF_API int gsf_allgather_poses(gsf_ctx *ctx, void *nccl_comm, const double *send, double *recv, int64_t count, int32_t mode,
                                int64_t chunk_count);

/* ---- layout helpers + synthetic workload (bench / tests) ------------------------------------------ */
/* [B][N][C] <-> [N][C][B] transposes of float64 (C = 1,3,4) and uint8 (C = 1) arrays, on device */
GSF_API int gsf_transpose_to_time_major_dev(gsf_ctx *ctx, const void *src, void *dst, int64_t B, int64_t N, int32_t C, int32_t elem_bytes);
GSF_API int gsf_transpose_to_traj_major_dev(gsf_ctx *ctx, const void *src, void *dst, int64_t B, int64_t N, int32_t C, int32_t elem_bytes);
/* deterministic KITTI-04-shaped synthetic batch, generated on device straight into `layout`;
   trajectory ids [traj0, traj0+B).  Integer counter-based RNG + polynomial / rational curves only (no libm call), so the values do
   not depend on a math library and a shard generated with traj0 = k equals rows k.. of the full batch bit for bit. */
/* the same trajectories with the GNSS side as a ragged GEODETIC log (fixes at their own stamps, rows (lat, lon, alt) about
   49.0336 N 8.3950 E, outages = missing fixes): the input of the device chain K1 -> time alignment -> fit -> EKF.  Two passes:
   counts != NULL sizes (counts[B] int64 fixes per trajectory), gps_offsets != NULL writes rows at gps_offsets[b]. */
GSF_API int gsf_synth_geodetic_batch_dev(gsf_ctx *ctx, uint64_t seed, int64_t traj0, int64_t B, int64_t N, double *ts, double *pos,
                                         double *quat, int64_t *counts, const int64_t *gps_offsets, double *gps_t, double *gps_llh);
GSF_API int gsf_synth_batch_dev(gsf_ctx *ctx, int32_t layout, uint64_t seed, int64_t traj0, int64_t B, int64_t N, double *ts,
                        double *pos, double *quat, double *gps, uint8_t *valid, double *init_pos, double *init_quat);

#ifdef __cplusplus
}
#endif
#endif /* GSF_H */
