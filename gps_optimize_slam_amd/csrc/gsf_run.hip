// gsf_run.hip -- steps 1-6 of main_process_gui (EKFGPSSLAM.py:959-1033) for B trajectories as ONE device chain, no host round trip:
//   geodesy slice    lat/lon range mask, zone pick, UTM forward, [E, N, alt] rows                (ref :258-271;  gsf_utm.hip)
//   loaded rows      the fixes the loader keeps, compacted per log                                (ref :259-264)
//   pre-filter       sliding-window polynomial RANSAC, windows walked on the device               (ref :275, :136-247;  gsf_gpsfilter.hip)
//   filtered log     rows the pre-filter drops blanked; "fewer than 2 fixes" flagged               (ref :283, :967)
//   alignment        dynamic_time_alignment to the SLAM stamps                                     (ref :971;  gsf_align.hip)
//   steps 3-5        row choice, robust fit, Sim3 of pose 0, EKF + RTS                             (ref :973-1010;  gsf_robust.hip)
//   step 4 in full   transform_trajectory of every pose (the metric's "Sim3" row)                  (ref :1006;  gsf_sim3.hip)
//   step 6           nearest-fix error of raw SLAM / Sim3 / EKF against the primary GPS            (ref :1013-1033;  gsf_eval.hip)
//   outcome          run_status per trajectory, NaN outputs where the reference raises
// Each trajectory's legacy MT19937 stream is used by the pre-filter first and the robust fit second, in the reference's order.
// The ragged entry (gsf_run_fusion_ragged_dev) runs the same chain on tracks of different lengths, with the optional ground-truth log of
// main_process_gui (:962-966, :1035-1075): its own geodesy slice and pre-filter between the primary pre-filter and the fit, and three more
// step-6 rows against it.
#include "gsf_wave_common.hpp"

using namespace gsf;

namespace {

// one wave per log: stable compaction of the fixes the loader keeps (ref :259-264: the geodesy slice marks a dropped fix by NaN easting AND
// northing) into slot [gps_offsets[b], +counts[b]); rowmap = the row of the log each slot came from
// (gate, may be NULL: a log whose gate[b] != 0 counts 0 fixes -- the ground-truth log of a run that already stopped: its pre-filter draws nothing)
__global__ __launch_bounds__(64) void run_compact_rows_kernel(const double* __restrict__ gps_t, const double* __restrict__ utm, const int64_t* __restrict__ offsets,
                                                              double* __restrict__ ct, double* __restrict__ cp, int32_t* __restrict__ rowmap,
                                                              int32_t* __restrict__ counts, const int32_t* __restrict__ gate)
{
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x, base = offsets[b], n_log = (gate && gate[b] != 0) ? 0 : offsets[b + 1] - base;
    int n = 0;
    for (int64_t c0 = 0; c0 < n_log; c0 += 64) {
        const int64_t i = c0 + lane;
        double e = NAN, nn = NAN, a = NAN, tt = 0.0;
        if (i < n_log) { e = utm[(base + i) * 3]; nn = utm[(base + i) * 3 + 1]; a = utm[(base + i) * 3 + 2]; tt = gps_t[base + i]; }
        const bool ok = i < n_log && !(isnan(e) && isnan(nn));
        const u64 m = __ballot(ok);
        if (ok) {
            const int64_t o = base + n + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
            ct[o] = tt; cp[o * 3] = e; cp[o * 3 + 1] = nn; cp[o * 3 + 2] = a; rowmap[o] = (int32_t)i;
        }
        n += __popcll(m);
    }
    if (lane == 0) counts[b] = n;
}

// one wave per log: what load_gps_data returns (ref :275-287) as a mask over the ORIGINAL rows and as a copy of the UTM rows in which every
// other row is blanked (NaN easting and northing: the alignment drops such rows when it stages a log); flags GPS_EMPTY / GPS_FEW /
// PREFILTER_UNHANDLED
__global__ __launch_bounds__(64) void run_filtered_rows_kernel(const double* __restrict__ utm, const int64_t* __restrict__ offsets, const int32_t* __restrict__ counts,
                                                               const int32_t* __restrict__ rowmap, const uint8_t* __restrict__ ckeep,
                                                               const int32_t* __restrict__ log_status, double* __restrict__ fut,
                                                               uint8_t* __restrict__ gps_keep, int32_t* __restrict__ run_status,
                                                               int64_t* __restrict__ slam_off, int32_t* __restrict__ bad_quat, int64_t B, int64_t N)
{
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x, base = offsets[b], n_log = offsets[b + 1] - base;
    // (two chores of the later steps ride along: the fixed-stride offsets of the SLAM tracks, and the zeroed flag K3 ORs into; either may be NULL)
    if (lane == 0) { if (slam_off) { slam_off[b] = b * N; if (b == B - 1) slam_off[B] = B * N; } if (bad_quat) bad_quat[b] = 0; }
    const int n = counts[b];
    const bool unhandled = log_status[b] != 0;
    for (int64_t i = lane; i < n_log; i += 64) {
        gps_keep[base + i] = 0;
        fut[(base + i) * 3] = NAN; fut[(base + i) * 3 + 1] = NAN; fut[(base + i) * 3 + 2] = utm[(base + i) * 3 + 2];
    }
    __syncthreads();
    int kept = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool keep = k < n && !unhandled && ckeep[base + k] != 0;
        if (keep) {
            const int64_t r = base + rowmap[base + k];
            gps_keep[r] = 1;
            fut[r * 3] = utm[r * 3]; fut[r * 3 + 1] = utm[r * 3 + 1];
        }
        kept += __popcll(__ballot(keep));
    }
    if (lane == 0) run_status[b] = (n == 0 ? GSF_RUN_GPS_EMPTY : 0) | (unhandled ? GSF_RUN_PREFILTER_UNHANDLED : ((n > 0 && kept < 2) ? GSF_RUN_GPS_FEW : 0));
}

// the runs that raised before the fit: step 1 (either log) or the empty SLAM track (only the ragged entry sets the last four)
constexpr int32_t RUN_BEFORE_FIT = GSF_RUN_GPS_EMPTY | GSF_RUN_GPS_FEW | GSF_RUN_PREFILTER_UNHANDLED | GSF_RUN_GT_EMPTY | GSF_RUN_GT_FEW | GSF_RUN_GT_UNHANDLED |
                                   GSF_RUN_SLAM_EMPTY;
constexpr int32_t RUN_GT_BITS = GSF_RUN_GT_EMPTY | GSF_RUN_GT_FEW | GSF_RUN_GT_UNHANDLED;

// (ragged entry) one wave per trajectory, after both logs were loaded: the ground-truth log's outcome (gt_rs, run_filtered_rows_kernel's bits)
// on runs whose primary log went through (ref :964: load_gps_data raises for it too -- and :966 is never reached), then the empty SLAM track
// (ref :967).  A run stopped here draws nothing more: its primary fixes are blanked, so the alignment finds no row and the fit does not draw.
__global__ __launch_bounds__(64) void run_gt_status_kernel(const int64_t* __restrict__ slam_offsets, const int64_t* __restrict__ gps_offsets,
                                                           const int64_t* __restrict__ gt_offsets, const int32_t* __restrict__ gt_rs,
                                                           int32_t* __restrict__ run_status, double* __restrict__ fut)
{
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    int32_t rs = run_status[b];
    if (rs == 0 && gt_offsets && gt_offsets[b + 1] > gt_offsets[b]) {
        const int32_t g = gt_rs[b];
        rs |= ((g & GSF_RUN_GPS_EMPTY) ? GSF_RUN_GT_EMPTY : 0) | ((g & GSF_RUN_GPS_FEW) ? GSF_RUN_GT_FEW : 0) |
              ((g & GSF_RUN_PREFILTER_UNHANDLED) ? GSF_RUN_GT_UNHANDLED : 0);
    }
    if (rs == 0 && slam_offsets[b + 1] == slam_offsets[b]) rs = GSF_RUN_SLAM_EMPTY;
    if ((rs & RUN_GT_BITS) != 0) {
        const int64_t base = gps_offsets[b], n_log = gps_offsets[b + 1] - base;
        for (int64_t i = lane; i < n_log; i += 64) { fut[(base + i) * 3] = NAN; fut[(base + i) * 3 + 1] = NAN; }
    }
    if (lane == 0) run_status[b] = rs;
}

// one wave per trajectory: the reference stopped before (or at) the fit -> every output of the later steps is NaN; Sim3 failures are flagged.
// Ragged entry: slam_offsets gives the track's rows; err_gt (may be NULL) = the ground-truth block of the step-6 rows, gt_none: no ground-truth
// leg ran (every track's block is count 0, NaN); plot_ref (may be NULL) = which reference the reference's plot takes (ref :1064-1075)
__global__ __launch_bounds__(64) void run_outcome_kernel(int64_t B, int64_t N, const int32_t* __restrict__ status, int32_t* __restrict__ run_status,
                                                         double* __restrict__ R, double* __restrict__ t, double* __restrict__ s,
                                                         double* __restrict__ pos_out, double* __restrict__ quat_out, double* __restrict__ sim3_pos,
                                                         double* __restrict__ err_stats, int32_t* __restrict__ n_inliers, const int32_t* __restrict__ bad_quat,
                                                         const int64_t* __restrict__ slam_offsets, double* __restrict__ err_gt, int gt_none,
                                                         int32_t* __restrict__ plot_ref)
{
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    int64_t base = b * N;
    if (slam_offsets) { base = uniform64(slam_offsets[b]); N = uniform64(slam_offsets[b + 1]) - base; }
    int32_t rs = run_status[b];
    // a SLAM quaternion that cannot be normalised: SciPy raises in transform_trajectory (ref :466), the run ends in step 4
    if (bad_quat[b] != 0 && (rs & RUN_BEFORE_FIT) == 0 && ((status[b] >> 8) & SIM3_NONE) == 0) rs |= GSF_RUN_BAD_QUAT;
    if (((status[b] >> 8) & SIM3_NONE) != 0 && (rs & RUN_BEFORE_FIT) == 0) rs |= GSF_RUN_SIM3_FAILED;
    if (err_gt && (gt_none || rs != 0) && lane < 12) err_gt[((int64_t)(lane / 4) * B + b) * 4 + (lane & 3)] = (lane & 3) == 0 ? 0.0 : NAN;
    if (rs != 0) {
        for (int64_t i = lane; i < N; i += 64) {
            for (int c = 0; c < 3; ++c) { pos_out[(base + i) * 3 + c] = NAN; if (sim3_pos) sim3_pos[(base + i) * 3 + c] = NAN; }
            for (int c = 0; c < 4; ++c) quat_out[(base + i) * 4 + c] = NAN;
        }
        if (lane < 9) R[b * 9 + lane] = NAN;
        if (lane < 3) t[b * 3 + lane] = NAN;
        if (lane == 0) s[b] = NAN;
        // the metric of a run that raised was never printed: count 0 and NaN rows (the raw-SLAM row too: the reference never got to step 6)
        if (lane < 12) err_stats[((int64_t)(lane / 4) * B + b) * 4 + (lane & 3)] = (lane & 3) == 0 ? 0.0 : NAN;
        if (lane == 0 && (rs & RUN_BEFORE_FIT) != 0) n_inliers[b] = -1;
    }
    if (lane == 0) {
        run_status[b] = rs;
        // the ground truth's EKF row if it has points past the first seconds, else the primary's, else none (ref :1064-1075)
        if (plot_ref) plot_ref[b] = rs != 0 ? 0 : ((err_gt && !gt_none && err_gt[(2 * B + b) * 4] > 0.0) ? 2 : (err_stats[(2 * B + b) * 4] > 0.0 ? 1 : 0));
    }
}

// ---------------------------------------------------------------------------------------------------------------- the chain, host side
// one GNSS log per track (the primary logs, or the ground truth): inputs, then what step 1 leaves behind.  NULL means what it means in include/gsf.h
struct RunLog {
    const double* t; const double* llh /* NULL: utm holds the projected rows already */; const int64_t* offsets; int64_t total; int32_t max_fixes;
    const gsf_prefilter_config* filter; int32_t* zone; int32_t* south; double* utm; uint8_t* keep;
};

// every pointer and size of a run: what the two device entries fill in from their arguments (device pointers) and the two host entries from
// theirs (host pointers, staged by run_staged).  NULL means what it means in include/gsf.h
struct RunIO {
    const double* ts; const double* pos; const double* quat;
    const int64_t* slam_offsets;     // NULL: the dense entry, B tracks of N poses each
    int64_t B, N, total_poses;       // N: poses per track (dense) / the longest track (ragged); total_poses: rows of ts, pos, quat
    RunLog gps, gt;                  // gt.offsets == NULL: no ground-truth leg (the dense entry has none)
    const gsf_run_config* cfg; uint32_t* mt_state;
    double* R; double* t; double* s; double* pos_out; double* quat_out; int32_t* status; int32_t* n_inliers; double* aligned; uint8_t* valid;
    double* sim3_pos; double* gt_aligned; uint8_t* gt_valid;
    double* err_stats;               // dense: [3][B][4]; ragged: [2][3][B][4], the second block against the ground truth
    int32_t* plot_ref; int32_t* run_status; uint8_t* inlier_mask; int32_t* trial_info;
};

// temporaries of the chain in the run workspace (byte offsets, 256-byte aligned); used by run_chain and by nothing else
struct RunLayout {
    struct Log { size_t ct, cp, map, ck, cnt, ls, fut; } gps, gt;             // per log: compacted stamps / rows, row map, keep marks, counts, status, filtered rows
    size_t li, so, as, sp, sq, bq, err, grs, bytes;
};

RunLayout run_layout(const RunIO& io)
{
    const bool ragged = io.slam_offsets != nullptr;
    const size_t nb = (size_t)io.B, P = (size_t)io.total_poses;
    RunLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; };
    auto log = [&](RunLayout::Log& l, size_t T, size_t per_track) {
        l.ct = take(T * 8); l.cp = take(T * 24); l.map = take(T * 4); l.ck = take(T); l.cnt = take(per_track); l.ls = take(per_track); l.fut = take(T * 24);
    };
    log(L.gps, (size_t)(io.gps.total > 0 ? io.gps.total : 1), nb * 4);
    L.li = take(nb * 8);
    L.so = take(ragged ? 0 : (nb + 1) * 8);                                      // the dense entry's fixed-stride offsets
    L.as = take(nb * 4);
    L.sp = take(io.sim3_pos ? 0 : P * 24); L.sq = take(P * 32); L.bq = take(nb * 4); L.err = take(P * 24);
    log(L.gt, io.gt.offsets ? (size_t)(io.gt.total > 0 ? io.gt.total : 1) : 0, ragged ? nb * 4 : 0);
    L.grs = take(ragged ? nb * 4 : 0);
    L.bytes = off;
    return L;
}

// step 1 of one log (load_gps_data, ref :258-287): mask, zone, UTM; the loaded rows compacted; the pre-filter -- the next draws of each track's
// generator --; the filtered log w.fut and its flags rs.  gate (may be NULL): tracks with gate[b] != 0 count no fix and draw nothing.
// slam_off / badq (may be NULL) and N: the two chores run_filtered_rows_kernel carries for the later steps
int load_log(gsf_ctx* ctx, const RunLog& g, char* ws, const RunLayout::Log& w, int32_t* log_info, int64_t B, uint32_t* mt_state, const int32_t* gate, int32_t* rs,
             int64_t* slam_off, int32_t* badq, int64_t N)
{
    double* ct = (double*)(ws + w.ct); double* cp = (double*)(ws + w.cp); int32_t* rowmap = (int32_t*)(ws + w.map); uint8_t* ckeep = (uint8_t*)(ws + w.ck);
    int32_t* counts = (int32_t*)(ws + w.cnt); int32_t* log_status = (int32_t*)(ws + w.ls); double* fut = (double*)(ws + w.fut);
    int rc;
    // (llh == NULL: the caller's utm rows are the projected log already)
    if (g.llh && (rc = gsf_gps_rows_to_utm_batch_dev(ctx, g.llh, g.offsets, B, g.utm, g.zone, g.south))) return rc;
    hipLaunchKernelGGL(run_compact_rows_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, g.t, (const double*)g.utm, g.offsets, ct, cp, rowmap, counts, gate);
    GSF_HIP(hipGetLastError());
    if ((rc = launch_gps_prefilter_auto(ctx, ct, cp, g.offsets, counts, B, g.max_fixes > 0 ? g.max_fixes : 1, g.filter, mt_state, ckeep, log_status, log_info))) return rc;
    hipLaunchKernelGGL(run_filtered_rows_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, (const double*)g.utm, g.offsets, (const int32_t*)counts,
                       (const int32_t*)rowmap, (const uint8_t*)ckeep, (const int32_t*)log_status, fut, g.keep, rs, slam_off, badq, B, N);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

// the chain of both device entries; the arguments were checked by the entry.  What differs between the two is said where it differs.
int run_chain(gsf_ctx* ctx, const RunIO& io)
{
    const bool ragged = io.slam_offsets != nullptr, gt = io.gt.offsets != nullptr;
    const gsf_run_config* cfg = io.cfg;
    const int64_t B = io.B, nmax = io.N > 0 ? io.N : 1;                          // (only a ragged batch can have N == 0: every track empty)
    int rc;
    // both pre-filters' configurations and log lengths before the first one draws: a failing call leaves every generator where it was
    // (the dense entry used to meet this check inside launch_gps_prefilter_auto: the same code and message, now earlier)
    if ((rc = check_gps_prefilter(io.gps.filter, io.gps.max_fixes > 0 ? io.gps.max_fixes : 1, B))) return rc;
    if (gt && (rc = check_gps_prefilter(io.gt.filter, io.gt.max_fixes > 0 ? io.gt.max_fixes : 1, B))) return rc;
    GSF_HIP(hipSetDevice(ctx->device));
    const RunLayout L = run_layout(io);
    if ((rc = ensure_workspace(ctx, GSF_WS_RUN, L.bytes))) return rc;
    char* w = workspace(ctx, GSF_WS_RUN);
    int32_t* log_info = (int32_t*)(w + L.li); int32_t* align_status = (int32_t*)(w + L.as);     // (both logs' launches reuse these two)
    double* fut = (double*)(w + L.gps.fut); double* gfut = (double*)(w + L.gt.fut); int32_t* grs = (int32_t*)(w + L.grs);
    double* sp = io.sim3_pos ? io.sim3_pos : (double*)(w + L.sp); double* sq = (double*)(w + L.sq); int32_t* badq = (int32_t*)(w + L.bq);
    double* errs = (double*)(w + L.err);
    // the tracks' row offsets for the alignment and step 4.  Dense: fixed-stride offsets written on the device by run_filtered_rows_kernel (which
    // gets N for that); ragged: the caller's, and the kernel gets no array and N = 0
    const int64_t* track_off = ragged ? io.slam_offsets : (const int64_t*)(w + L.so);
    // ---- step 1, primary log (ref :961) -- the first draws of each track's generator
    if ((rc = load_log(ctx, io.gps, w, L.gps, log_info, B, io.mt_state, nullptr, io.run_status, ragged ? nullptr : (int64_t*)(w + L.so), badq, ragged ? 0 : io.N))) return rc;
    // ---- step 1, ground-truth log (ref :962-966): its own zone, its own pre-filter (CONFIG['ground_truth_gps_filtering']) -- the next draws, and
    // none for a track whose primary log already stopped the run (gated to 0 fixes) or that has no ground truth (an empty range)
    if (gt && (rc = load_log(ctx, io.gt, w, L.gt, log_info, B, io.mt_state, io.run_status, grs, nullptr, nullptr, 0))) return rc;
    // ---- ragged only: the ground truth's outcome and the empty SLAM track (ref :964, :967); a dense batch has neither
    if (ragged) {
        hipLaunchKernelGGL(run_gt_status_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, io.slam_offsets, io.gps.offsets, io.gt.offsets, (const int32_t*)grs,
                           io.run_status, fut);
        GSF_HIP(hipGetLastError());
    }
    // ---- step 2
    if ((rc = gsf_time_align_loaded_rows_batch_dev(ctx, io.ts, track_off, io.gps.t, fut, io.gps.offsets, B, io.gps.max_fixes > 2 ? io.gps.max_fixes : 2,
                                                   cfg->max_gps_gap_threshold, io.aligned, io.valid, align_status))) return rc;
    // ---- steps 3-5 on the rows main_process_gui picks (ref :973-998), whatever the context's own row rule is: restored on every path below.
    // Dense passes offsets = NULL here and to step 6: that selects the equal-length kernel builds (sized tail scans, the workgroup kernel, early
    // variances, the LDS metric kernel); the offsets in the workspace would give the same results, slower
    const FitRows saved = ctx->fit_rows;
    ctx->fit_rows = FitRows{ 1, cfg->sim3_min_samples, cfg->max_gps_gap_threshold, cfg->sim3_max_initial_duration };
    rc = robust_chain(ctx, io.ts, io.pos, io.quat, io.aligned, io.valid, &cfg->ekf, B, nmax, io.slam_offsets, ragged ? io.total_poses : 0, cfg->sim3_min_samples,
                      cfg->sim3_residual_threshold, cfg->sim3_max_trials, cfg->sim3_min_inliers_needed, io.mt_state, io.R, io.t, io.s, io.pos_out, io.quat_out,
                      io.status, io.n_inliers, io.inlier_mask, io.trial_info);
    ctx->fit_rows = saved;
    if (rc) return rc;
    // ---- step 4 for every pose, step 6 against the primary fixes and (ref :1035-1062) against the ground truth, aligned with the same values
    if ((rc = launch_apply_sim3(ctx, io.pos, io.quat, track_off, B, io.R, io.t, io.s, sp, sq, badq, true))) return rc;
    if ((rc = launch_eval_errors3(ctx, io.ts, io.pos, sp, io.pos_out, io.aligned, io.valid, B, nmax, cfg->eval_skip_seconds, io.err_stats, errs, io.slam_offsets,
                                  ragged ? io.total_poses : 0))) return rc;
    // err_stats: 12 doubles per track in the dense entry; 24 in the ragged one, whose second block the outcome kernel fills itself (count 0, NaN)
    // when no ground-truth leg ran (gt_none)
    double* err_gt = ragged ? io.err_stats + (size_t)B * 12 : nullptr;
    if (gt) {
        if ((rc = gsf_time_align_loaded_rows_batch_dev(ctx, io.ts, track_off, io.gt.t, gfut, io.gt.offsets, B, io.gt.max_fixes > 2 ? io.gt.max_fixes : 2,
                                                       cfg->max_gps_gap_threshold, io.gt_aligned, io.gt_valid, align_status))) return rc;
        if ((rc = launch_eval_errors3(ctx, io.ts, io.pos, sp, io.pos_out, io.gt_aligned, io.gt_valid, B, nmax, cfg->eval_skip_seconds, err_gt, errs, io.slam_offsets,
                                      io.total_poses))) return rc;
    }
    hipLaunchKernelGGL(run_outcome_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, B, ragged ? (int64_t)0 : io.N, (const int32_t*)io.status, io.run_status, io.R,
                       io.t, io.s, io.pos_out, io.quat_out, io.sim3_pos, io.err_stats, io.n_inliers, (const int32_t*)badq, io.slam_offsets, err_gt,
                       (ragged && !gt) ? 1 : 0, io.plot_ref);
    GSF_HIP(hipGetLastError());
    return GSF_OK;
}

// the dense device entry on a RunIO: its argument checks (before the context is touched), then the chain
int run_fusion_batch_dev(gsf_ctx* ctx, const RunIO& io)
{
    GSF_REQUIRE(ctx && io.cfg, "ctx/cfg is NULL");
    GSF_REQUIRE(io.B >= 0 && io.N >= 0 && io.B <= 0x7fffffff && io.gps.total >= 0 && io.gps.max_fixes >= 0, "bad B, N, total_fixes or max_fixes");
    if (io.B == 0 || io.N == 0) return GSF_OK;                                   // nothing written
    GSF_REQUIRE(io.ts && io.pos && io.quat && io.gps.offsets && io.mt_state && io.R && io.t && io.s && io.pos_out && io.quat_out && io.status && io.n_inliers &&
                io.aligned && io.valid && io.err_stats && io.run_status && (!io.gps.llh || (io.gps.zone && io.gps.south)), "NULL array");
    GSF_REQUIRE(io.gps.total == 0 || (io.gps.t && io.gps.utm && io.gps.keep), "NULL GNSS array");
    GSF_REQUIRE(io.N <= 28000, "N too large for the device-side draws (<= 28000 poses per trajectory)");
    return run_chain(ctx, io);
}

// the ragged device entry on a RunIO.  Unlike the dense one it returns early only for B == 0: a batch whose tracks are all empty runs (SLAM_EMPTY)
int run_fusion_ragged_dev(gsf_ctx* ctx, const RunIO& io)
{
    const RunLog& g = io.gt;
    GSF_REQUIRE(ctx && io.cfg, "ctx/cfg is NULL");
    GSF_REQUIRE(io.B >= 0 && io.B <= 0x7fffffff && io.total_poses >= 0 && io.N >= 0 && io.gps.total >= 0 && io.gps.max_fixes >= 0 && g.total >= 0 && g.max_fixes >= 0,
                "bad B, total_poses, max_poses, total_fixes, max_fixes, gt_total or gt_max_fixes");
    if (io.B == 0) return GSF_OK;                                                // nothing written
    GSF_REQUIRE(io.N <= 28000, "a track is too long for the device-side draws (<= 28000 poses per trajectory)");
    GSF_REQUIRE(io.slam_offsets && io.gps.offsets && io.mt_state && io.R && io.t && io.s && io.status && io.n_inliers && io.err_stats && io.run_status &&
                (!io.gps.llh || (io.gps.zone && io.gps.south)), "NULL array");
    GSF_REQUIRE(io.total_poses == 0 || (io.ts && io.pos && io.quat && io.pos_out && io.quat_out && io.aligned && io.valid), "NULL SLAM array");
    GSF_REQUIRE(io.gps.total == 0 || (io.gps.t && io.gps.utm && io.gps.keep), "NULL GNSS array");
    GSF_REQUIRE(!g.offsets || (g.filter && (!g.llh || (g.zone && g.south)) && (io.total_poses == 0 || (io.gt_aligned && io.gt_valid)) &&
                               (g.total == 0 || (g.t && g.utm && g.keep))), "NULL ground-truth array");
    return run_chain(ctx, io);
}

// the host-pointer entries: h holds host pointers (checked by the entry); one staged upload, `dev` on the device copies, one download.
// d starts as a copy of h; every array in the list below is declared to the staging and its field of d bound to the device copy
int run_staged(gsf_ctx* ctx, const RunIO& h, int (*dev)(gsf_ctx*, const RunIO&))
{
    const bool ragged = h.slam_offsets != nullptr, gt = h.gt.offsets != nullptr;
    const size_t nb = (size_t)h.B, P = (size_t)h.total_poses, T = (size_t)h.gps.total, Tg = (size_t)h.gt.total;
    Staging st(ctx);
    RunIO d = h;
    auto in = [&](auto*& p, size_t count, bool want = true) { if (want) st.bind(p, st.in(p, count)); else p = nullptr; };
    auto out = [&](auto*& p, size_t count, bool want = true) { if (want) st.bind(p, st.out(p, count)); else p = nullptr; };
    in(d.ts, P); in(d.pos, P * 3); in(d.quat, P * 4); in(d.slam_offsets, nb + 1, ragged);
    in(d.gps.t, T); in(d.gps.llh, T * 3); in(d.gps.offsets, nb + 1);
    in(d.gt.t, Tg, gt); in(d.gt.llh, Tg * 3, gt); in(d.gt.offsets, nb + 1, gt);
    st.bind(d.mt_state, st.inout(d.mt_state, nb * 625));
    out(d.R, nb * 9); out(d.t, nb * 3); out(d.s, nb); out(d.pos_out, P * 3); out(d.quat_out, P * 4);
    out(d.status, nb); out(d.n_inliers, nb); out(d.gps.zone, nb); out(d.gps.south, nb);
    out(d.gps.utm, T * 3); out(d.gps.keep, T); out(d.aligned, P * 3); out(d.valid, P);
    out(d.sim3_pos, P * 3, h.sim3_pos != nullptr);
    out(d.gt.zone, nb, gt); out(d.gt.south, nb, gt); out(d.gt.utm, Tg * 3, gt); out(d.gt.keep, Tg, gt);
    out(d.gt_aligned, P * 3, gt); out(d.gt_valid, P, gt);
    out(d.err_stats, nb * (ragged ? 24 : 12)); out(d.plot_ref, nb, h.plot_ref != nullptr); out(d.run_status, nb);
    out(d.inlier_mask, P, h.inlier_mask != nullptr); out(d.trial_info, nb * 2, h.trial_info != nullptr);
    ST_RUN(dev(ctx, d));
}

}  // namespace

extern "C" int gsf_run_fusion_batch_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, int64_t B, int64_t N,
                                        const double* gps_t, const double* gps_llh, const int64_t* gps_offsets, int64_t total_fixes,
                                        int32_t max_fixes, const gsf_run_config* cfg, uint32_t* mt_state, double* R, double* t, double* s,
                                        double* pos_out, double* quat_out, int32_t* status, int32_t* n_inliers, int32_t* zone, int32_t* south,
                                        double* gps_utm, uint8_t* gps_keep, double* aligned, uint8_t* valid, double* sim3_pos,
                                        double* err_stats, int32_t* run_status, uint8_t* inlier_mask, int32_t* trial_info)
{
    const RunIO io = { ts, pos, quat, nullptr, B, N, B * N,
                       { gps_t, gps_llh, gps_offsets, total_fixes, max_fixes, cfg ? &cfg->gps_filter : nullptr, zone, south, gps_utm, gps_keep }, {},
                       cfg, mt_state, R, t, s, pos_out, quat_out, status, n_inliers, aligned, valid, sim3_pos, nullptr, nullptr,
                       err_stats, nullptr, run_status, inlier_mask, trial_info };
    return run_fusion_batch_dev(ctx, io);
}

// the same with host arrays (what a cgo / JNI / ctypes caller with its data in host memory calls): one staged upload, the chain, one download
extern "C" int gsf_run_fusion_batch(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, int64_t B, int64_t N, const double* gps_t,
                                    const double* gps_llh, const int64_t* gps_offsets, const gsf_run_config* cfg, uint32_t* mt_state, double* R,
                                    double* t, double* s, double* pos_out, double* quat_out, int32_t* status, int32_t* n_inliers, int32_t* zone,
                                    int32_t* south, double* gps_utm, uint8_t* gps_keep, double* aligned, uint8_t* valid, double* sim3_pos,
                                    double* err_stats, int32_t* run_status, uint8_t* inlier_mask, int32_t* trial_info)
{
    GSF_REQUIRE(ctx && cfg && B >= 0 && N >= 0 && gps_offsets && mt_state, "bad arguments");
    if (B == 0 || N == 0) return GSF_OK;
    GSF_REQUIRE(ts && pos && quat && R && t && s && pos_out && quat_out && status && n_inliers && zone && south && aligned && valid && err_stats && run_status,
                "NULL array");
    const int64_t total = gps_offsets[B];
    GSF_REQUIRE(total >= 0 && (total == 0 || (gps_t && gps_llh && gps_utm && gps_keep)), "bad gps_offsets / NULL GNSS array");
    int64_t max_fixes = 0;
    for (int64_t b = 0; b < B; ++b) { const int64_t g = gps_offsets[b + 1] - gps_offsets[b]; GSF_REQUIRE(g >= 0, "gps_offsets must not decrease"); if (g > max_fixes) max_fixes = g; }
    GSF_REQUIRE(max_fixes <= 0x7fffffff, "a log is too long");
    const RunIO io = { ts, pos, quat, nullptr, B, N, B * N,
                       { gps_t, gps_llh, gps_offsets, total, (int32_t)max_fixes, &cfg->gps_filter, zone, south, gps_utm, gps_keep }, {},
                       cfg, mt_state, R, t, s, pos_out, quat_out, status, n_inliers, aligned, valid, sim3_pos, nullptr, nullptr,
                       err_stats, nullptr, run_status, inlier_mask, trial_info };
    return run_staged(ctx, io, run_fusion_batch_dev);
}

// ---- the ragged entry: tracks of different lengths, optional ground-truth log (include/gsf.h)
extern "C" int gsf_run_fusion_ragged_dev(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* slam_offsets, int64_t B,
                                         int64_t total_poses, int32_t max_poses, const double* gps_t, const double* gps_llh, const int64_t* gps_offsets,
                                         int64_t total_fixes, int32_t max_fixes, const double* gt_t, const double* gt_llh, const int64_t* gt_offsets,
                                         int64_t gt_total, int32_t gt_max_fixes, const gsf_run_config* cfg, const gsf_prefilter_config* gt_filter,
                                         uint32_t* mt_state, double* R, double* t, double* s, double* pos_out, double* quat_out, int32_t* status,
                                         int32_t* n_inliers, int32_t* zone, int32_t* south, double* gps_utm, uint8_t* gps_keep, double* aligned,
                                         uint8_t* valid, double* sim3_pos, int32_t* gt_zone, int32_t* gt_south, double* gt_utm, uint8_t* gt_keep,
                                         double* gt_aligned, uint8_t* gt_valid, double* err_stats, int32_t* plot_ref, int32_t* run_status,
                                         uint8_t* inlier_mask, int32_t* trial_info)
{
    const RunIO io = { ts, pos, quat, slam_offsets, B, max_poses, total_poses,
                       { gps_t, gps_llh, gps_offsets, total_fixes, max_fixes, cfg ? &cfg->gps_filter : nullptr, zone, south, gps_utm, gps_keep },
                       { gt_t, gt_llh, gt_offsets, gt_total, gt_max_fixes, gt_filter, gt_zone, gt_south, gt_utm, gt_keep },
                       cfg, mt_state, R, t, s, pos_out, quat_out, status, n_inliers, aligned, valid, sim3_pos, gt_aligned, gt_valid,
                       err_stats, plot_ref, run_status, inlier_mask, trial_info };
    return run_fusion_ragged_dev(ctx, io);
}

// host arrays: the offsets are read here (sizes, limits), then one staged upload, the chain, one download
extern "C" int gsf_run_fusion_ragged(gsf_ctx* ctx, const double* ts, const double* pos, const double* quat, const int64_t* slam_offsets, int64_t B,
                                     const double* gps_t, const double* gps_llh, const int64_t* gps_offsets, const double* gt_t, const double* gt_llh,
                                     const int64_t* gt_offsets, const gsf_run_config* cfg, const gsf_prefilter_config* gt_filter, uint32_t* mt_state,
                                     double* R, double* t, double* s, double* pos_out, double* quat_out, int32_t* status, int32_t* n_inliers, int32_t* zone,
                                     int32_t* south, double* gps_utm, uint8_t* gps_keep, double* aligned, uint8_t* valid, double* sim3_pos,
                                     int32_t* gt_zone, int32_t* gt_south, double* gt_utm, uint8_t* gt_keep, double* gt_aligned, uint8_t* gt_valid,
                                     double* err_stats, int32_t* plot_ref, int32_t* run_status, uint8_t* inlier_mask, int32_t* trial_info)
{
    GSF_REQUIRE(ctx && cfg && B >= 0 && B <= 0x7fffffff, "bad arguments");
    if (B == 0) return GSF_OK;
    GSF_REQUIRE(slam_offsets && gps_offsets && mt_state && R && t && s && status && n_inliers && zone && south && err_stats && run_status, "NULL array");
    // sizes and limits from the offsets, before any device work
    auto scan = [](const int64_t* o, int64_t B_, int64_t& total, int64_t& longest) {
        longest = 0;
        if (o[0] < 0) return false;
        for (int64_t b = 0; b < B_; ++b) { const int64_t n = o[b + 1] - o[b]; if (n < 0) return false; if (n > longest) longest = n; }
        total = o[B_];
        return true;
    };
    int64_t P = 0, max_poses = 0, total = 0, max_fixes = 0, gtot = 0, gmax = 0;
    GSF_REQUIRE(scan(slam_offsets, B, P, max_poses), "slam_offsets must start at >= 0 and not decrease");
    GSF_REQUIRE(scan(gps_offsets, B, total, max_fixes), "gps_offsets must start at >= 0 and not decrease");
    GSF_REQUIRE(!gt_offsets || scan(gt_offsets, B, gtot, gmax), "gt_offsets must start at >= 0 and not decrease");
    GSF_REQUIRE(max_poses <= 28000, "a track is too long for the device-side draws (<= 28000 poses per trajectory)");
    GSF_REQUIRE(max_fixes <= 14000 && gmax <= 14000, "a log is too long for the device pre-filter (<= 14000 fixes)");
    GSF_REQUIRE(P == 0 || (ts && pos && quat && pos_out && quat_out && aligned && valid), "NULL SLAM array");
    GSF_REQUIRE(total == 0 || (gps_t && gps_llh && gps_utm && gps_keep), "NULL GNSS array");
    const bool gt = gt_offsets != nullptr;
    GSF_REQUIRE(!gt || (gt_filter && gt_zone && gt_south && (P == 0 || (gt_aligned && gt_valid)) && (gtot == 0 || (gt_t && gt_llh && gt_utm && gt_keep))),
                "NULL ground-truth array");
    // both pre-filters' configurations before the context is touched
    int rc0 = check_gps_prefilter(&cfg->gps_filter, max_fixes > 0 ? (int32_t)max_fixes : 1, B);
    if (rc0 || (gt && (rc0 = check_gps_prefilter(gt_filter, gmax > 0 ? (int32_t)gmax : 1, B)))) return rc0;
    const RunIO io = { ts, pos, quat, slam_offsets, B, max_poses, P,
                       { gps_t, gps_llh, gps_offsets, total, (int32_t)max_fixes, &cfg->gps_filter, zone, south, gps_utm, gps_keep },
                       { gt_t, gt_llh, gt_offsets, gtot, (int32_t)gmax, gt_filter, gt_zone, gt_south, gt_utm, gt_keep },
                       cfg, mt_state, R, t, s, pos_out, quat_out, status, n_inliers, aligned, valid, sim3_pos, gt_aligned, gt_valid,
                       err_stats, plot_ref, run_status, inlier_mask, trial_info };
    return run_staged(ctx, io, run_fusion_ragged_dev);
}
