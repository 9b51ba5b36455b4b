"""Drop-in surface of the reference's EKFGPSSLAM.py hot path, backed by the gfx950 kernels.

Same function names, argument order, return conventions and error behaviour as the reference
(/root/reference/EKFGPSSLAM.py, lines cited per function); arrays are C-order float64 NumPy,
quaternions scalar-last.  Every numerical stage runs on the GPU through libgsf.so -- there is no
CPU fallback: without the library / a device the first call raises GsfError.

What stays host Python, as in the reference: text I/O (np.loadtxt/np.savetxt) and the walk over the window stamps of the GPS
pre-filter.  The reference's random draws (np.random.choice of the Sim3 RANSAC, scikit-learn's sampler in the pre-filter) are
made ON THE DEVICE from NumPy's global legacy generator state, which is handed back advanced exactly as the reference leaves
it, so a seeded run reproduces the reference's rows.  Time alignment, the pre-filter's polynomial RANSAC and the error metric
are device kernels too.
"""
import copy
import ctypes as C

import numpy as np

from . import _lib
from ._lib import EkfConfig, GsfError, check, f64, hptr  # noqa: F401

# EKFGPSSLAM.py:22-71
CONFIG = {
    "ekf": {
        "initial_cov_diag": [0.1, 0.1, 0.1, 0.01, 0.01, 0.01, 0.01],
        "process_noise_diag": [0.1, 0.1, 0.7, 0.01, 0.01, 0.01, 0.01],
        "meas_noise_diag": [0.2, 0.2, 0.2],
        "transition_steps": 10,
    },
    "sim3_ransac": {
        "min_samples": 4,
        "residual_threshold": 4.0,
        "max_trials": 1000,
        "min_inliers_needed": 4,
        "max_initial_duration": 180.0,
    },
    "gps_filtering_ransac": {
        "enabled": True, "use_sliding_window": True, "window_duration_seconds": 15.0, "window_step_factor": 0.5,
        "polynomial_degree": 2, "min_samples": 6, "residual_threshold_meters": 10.0, "max_trials": 50,
    },
    "time_alignment": {"max_samples_for_corr": 500, "max_gps_gap_threshold": 5.0},
    "ground_truth_gps_filtering": {
        "enabled": False, "use_sliding_window": True, "window_duration_seconds": 15.0, "window_step_factor": 0.5,
        "polynomial_degree": 2, "min_samples": 6, "residual_threshold_meters": 5.0, "max_trials": 50,
    },
    "rts_decision": {"sharp_turn_yaw_rate_threshold_deg_per_sec": 45.0, "default_ekf_transition_steps_on_sharp_turn": 0},
}


VERBOSE = False     # True: the Sim3 functions print the reference's diagnostics (ref :396-425, :433, :446, :450) -- same numbers, in English


def _say(msg):
    if VERBOSE:
        print(msg)


def _ctx():
    return _lib.default_context()


# ---------------------------------------------------------------------------- I/O (EKFGPSSLAM.py:110-125, :1091-1104)
def load_slam_trajectory(txt_path):
    """TUM trajectory -> {'timestamps','positions','quaternions'}; ValueError on any problem (ref :110-125)."""
    try:
        data = np.loadtxt(txt_path)
        if data.ndim == 1:
            data = data.reshape(1, -1)
        if data.shape[1] != 8:
            raise ValueError(f"SLAM file format error: expected 8 columns (ts x y z qx qy qz qw), got {data.shape[1]}")
        return {"timestamps": data[:, 0].astype(float), "positions": data[:, 1:4].astype(float),
                "quaternions": data[:, 4:8].astype(float)}
    except FileNotFoundError:
        raise ValueError(f"SLAM file not found: {txt_path}")
    except Exception as e:
        raise ValueError(f"SLAM data load/parse failed ({txt_path}): {e}")


def save_tum_utm(path, timestamps, positions, quaternions):
    """The reference's UTM TUM writer (ref :1091-1092): %.6f x4, %.8f x4, header without '#'."""
    out = np.column_stack((timestamps, positions, quaternions))
    np.savetxt(path, out, fmt=["%.6f"] + ["%.6f"] * 3 + ["%.8f"] * 4, header="timestamp x y z qx qy qz qw (UTM)", comments="")


def save_tum_wgs84(path, timestamps, lonlatalt, quaternions):
    """The reference's WGS84 writer (ref :1097-1101)."""
    out = np.column_stack((timestamps, lonlatalt, quaternions))
    np.savetxt(path, out, fmt=["%.6f"] + ["%.8f", "%.8f", "%.3f"] + ["%.8f"] * 4, header="timestamp lon lat alt qx qy qz qw (WGS84)", comments="")


def wgs84_path(out_path_utm):
    """The WGS84 file next to a UTM one (ref :1099-1100): '_utm.txt' -> '_wgs84.txt', else '.txt' -> '_wgs84.txt', else + '_wgs84.txt'."""
    out = out_path_utm.replace("_utm.txt", "_wgs84.txt")
    if out == out_path_utm:
        out = out_path_utm.replace(".txt", "_wgs84.txt") if ".txt" in out_path_utm else out_path_utm + "_wgs84.txt"
    return out


# ---------------------------------------------------------------------------- geodesy (EKFGPSSLAM.py:127-134, :249-296)
def auto_utm_projection(lons, lats):
    """(zone:int, hemisphere:str) from mean lon / mean lat (ref :127-134)."""
    lons, lats = np.asarray(lons), np.asarray(lats)
    if lons.size == 0 or lats.size == 0:
        raise ValueError("lon/lat arrays must not be empty to pick a UTM zone")
    central_lon = np.mean(lons)
    zone = int((central_lon + 180) // 6 + 1)
    hemisphere = " +south" if np.mean(lats) < 0 else ""
    return zone, hemisphere


class UtmProjector:
    """Callable stand-in for pyproj.Proj("+proj=utm +zone=Z[ +south] +ellps=WGS84 ...") (ref :267-270, :295):
    projector(lons, lats) -> (E, N); projector(x, y, inverse=True) -> (lons, lats).  Runs K1 on the GPU."""

    def __init__(self, zone, south):
        self.zone, self.south = int(zone), bool(south)
        self.srs = f"+proj=utm +zone={self.zone}{' +south' if self.south else ''} +ellps=WGS84 +datum=WGS84 +units=m +no_defs"

    def __call__(self, a, b, inverse=False):
        a, b = f64(a).ravel(), f64(b).ravel()
        if a.shape != b.shape:
            raise ValueError("x/y (lon/lat) must have the same length")
        o1, o2 = np.empty_like(a), np.empty_like(a)
        L = _lib.load()
        if not inverse:      # a = lons, b = lats
            check(L.gsf_utm_forward(_ctx().handle, hptr(b), hptr(a), a.size, self.zone, int(self.south), hptr(o1), hptr(o2)))
            return o1, o2    # (E, N)
        check(L.gsf_utm_inverse(_ctx().handle, hptr(a), hptr(b), a.size, self.zone, int(self.south), hptr(o1), hptr(o2)))
        return o2, o1        # gsf returns (lat, lon); pyproj returns (lon, lat)


def _ransac_axes_mask(t, p, degree, min_samples, residual_threshold, max_trials):
    """AND over the coordinate axes of one RANSACRegressor.fit each (ref :155-169), evaluated by gsf_ransac_poly_batch_dev.
    The sample sets come from scikit-learn's own sampler on NumPy's global legacy RNG -- the call RANSACRegressor makes -- and
    the stream is left exactly where the reference leaves it: the device returns n_trials_, the number of sets the reference's
    loop would have drawn (its trial count is data dependent), and the draws are replayed from the saved state.
    Raises ValueError when an axis finds no consensus set, like scikit-learn."""
    import torch
    from sklearn.utils.random import sample_without_replacement
    from . import batch as B
    rs = np.random.mtrand._rand                                          # check_random_state(None)
    n = len(t)
    dev = dict(device="cuda")
    td = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64)).to(**dev)
    offs = torch.tensor([0, n], dtype=torch.int64, **dev)
    keep = np.ones(n, dtype=bool)
    for ax in range(p.shape[1]):
        state = rs.get_state()
        idx = np.stack([sample_without_replacement(n, min_samples, random_state=rs) for _ in range(max_trials)]).astype(np.int32)
        yd = torch.as_tensor(np.ascontiguousarray(p[:, ax], dtype=np.float64)).to(**dev)
        mask, ntr, nin, st = B.ransac_poly_batch(td, yd, offs, torch.as_tensor(idx.reshape(1, max_trials, min_samples)).to(**dev),
                                                 degree, residual_threshold)
        ntr, st = int(ntr.item()), int(st.item())
        rs.set_state(state)
        for _ in range(ntr):
            sample_without_replacement(n, min_samples, random_state=rs)
        if st & 1:
            raise ValueError("RANSAC could not find a valid consensus set.")
        keep &= mask.cpu().numpy().astype(bool)
    return keep


def _prefilter_windows(times, config, need):
    """Row ranges [r0, r1) of the windows the reference visits, in its order (ref :199-234); the global mode is one window."""
    n_points = len(times)
    if not config.get("use_sliding_window", False):
        return [(0, n_points)], None
    width = config["window_duration_seconds"]
    stride = width * config["window_step_factor"]
    wins, rows_of = [], []
    t_first, t_last = times[0], times[-1]
    w0 = t_first
    while w0 < t_last:
        w1 = w0 + width
        rows = np.where((times >= w0) & (times < w1))[0]
        if len(rows) >= need:
            wins.append(rows)
        if stride <= 1e-6:
            later = np.where(times > w0)[0]
            if len(later) == 0:
                break
            w0 = times[later[0]]
        else:
            w0 += stride
        if w0 >= t_last and times[-1] >= w1:                             # one tail window ending just past the last stamp
            w0 = max(t_first, times[-1] - width + 1e-6)
    contiguous = all(len(r) == r[-1] - r[0] + 1 for r in wins)          # sorted stamps: every window is one row range
    return ([(int(r[0]), int(r[-1]) + 1) for r in wins] if contiguous else None), wins


def filter_gps_outliers_ransac(times, positions, config):
    """The reference's optional GPS pre-filter (ref :136-247): per-axis degree-d polynomial RANSAC, AND
    across axes; either one global fit or sliding windows [t, t+W) advanced by W*step_factor with one extra tail window, OR
    across windows -- rows never inside a fitted window are dropped.  The whole filter is ONE library call
    (gsf_gps_prefilter_chain): every window and axis in the reference's order, the sample sets drawn on the device from NumPy's
    global legacy generator exactly as scikit-learn's sampler draws them, the generator handed back where the reference leaves
    it -- a seeded run keeps the same rows.  The device sampler covers every ratio min_samples/n (permutation, tracking selection
    for n >= 100 min_samples, n == min_samples); logs the chain does not cover (unsorted stamps in the sliding mode, more than 14 000
    rows in a window, configurations beyond its limits) take the window-by-window route with host-drawn sample sets (_ransac_axes_mask)."""
    if not config.get("enabled", False):
        return times, positions
    n_points, need = len(times), config["min_samples"]
    if n_points < need:
        return times, positions
    degree, thr, trials = config["polynomial_degree"], config["residual_threshold_meters"], config["max_trials"]
    sliding = bool(config.get("use_sliding_window", False))
    times, positions = np.asarray(times), np.asarray(positions)
    ranges, wins = _prefilter_windows(times, config, need)
    longest = max((b - a for a, b in ranges), default=0) if ranges is not None else 0
    chain_ok = (ranges is not None and positions.shape[1] == 3 and longest <= 14000 and 1 <= trials <= 1024 and need <= 16 and 1 <= degree <= 3
                and trials * (16 + 4 * need) + 2 * min(longest, 100 * need - 1) + 8 <= 56 * 1024)    # gsf_gps_prefilter_chain's own limits (LDS budget of
    # its sampler, chain_lds in csrc/gsf_gpsfilter.hip: only permutation windows, fewer than 100 min_samples rows, buffer swap partners)
    if chain_ok:
        if not ranges:
            return times[:0], positions[:0]                              # no window had enough rows: nothing is ever marked (ref :199-236)
        kind, key, pos_, has_gauss, cached = np.random.get_state()
        state = np.concatenate([key.astype(np.uint32), np.array([pos_], dtype=np.uint32)])
        t = np.ascontiguousarray(times, dtype=np.float64)
        p = np.ascontiguousarray(positions, dtype=np.float64)
        wr = np.ascontiguousarray(np.array(ranges, dtype=np.int32).reshape(-1, 2))
        off, wo = np.array([0, n_points], dtype=np.int64), np.array([0, len(ranges)], dtype=np.int64)
        keep, ws, ls = np.zeros(n_points, dtype=np.uint8), np.zeros(len(ranges), dtype=np.int32), np.zeros(1, dtype=np.int32)
        check(_lib.load().gsf_gps_prefilter_chain(_ctx().handle, hptr(t), hptr(p), hptr(off), 1, hptr(wr), hptr(wo), int(max(b - a for a, b in ranges)),
                                                  int(trials), int(need), int(degree), float(thr), 0.99, hptr(state), hptr(keep), hptr(ws), hptr(ls)))
        if ls[0] == 0:
            np.random.set_state((kind, state[:624], int(state[624]), has_gauss, cached))
            if not sliding:
                if ws[0] != 0:
                    return times, positions                              # the fit raised: filtering skipped (ref :178-182)
            keep = keep.astype(bool)
            return times[keep], positions[keep]
        # (generator untouched: `state` was a copy)

    def axes_mask(t, p):
        return _ransac_axes_mask(np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64), degree, need, thr, trials)

    if not sliding:                                                      # ref :148-182
        try:
            keep = axes_mask(times, positions)
            return times[keep], positions[keep]
        except GsfError:
            raise
        except Exception:
            return times, positions
    keep = np.zeros(n_points, dtype=bool)
    for rows in wins:                                                    # ref :183-247
        try:
            keep[rows[axes_mask(times[rows], positions[rows])]] = True
        except GsfError:
            raise
        except Exception:
            pass                                                         # a failed window marks nothing (ref :228-229)
    return times[keep], positions[keep]


def load_gps_data(txt_path, data_label="GPS", filter_config_override=None):
    """GPS text file -> {'timestamps','positions'(UTM E,N,alt),'utm_zone','projector'}; ValueError on failure
    (ref :249-289).  Columns are read as ts, lat, lon, alt -- cols 0,1,2,3 (ref :258)."""
    try:
        try:
            raw = np.loadtxt(txt_path, delimiter=" ")
        except ValueError:
            raw = np.loadtxt(txt_path, delimiter=",")
        if raw.ndim == 1:
            raw = raw.reshape(1, -1)
        if raw.shape[1] < 4:
            raise ValueError(f"{data_label} file needs at least 4 columns (ts lat lon alt), got {raw.shape[1]}")
        ts, lats, lons, alts = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3]
        valid = (np.abs(lats) <= 90) & (np.abs(lons) <= 180) & (lats != 0) & (lons != 0)          # ref :259
        if not np.all(valid):
            ts, lats, lons, alts = ts[valid], lats[valid], lons[valid], alts[valid]
            if len(ts) == 0:
                raise ValueError(f"{data_label}: no valid GPS rows after the lat/lon range filter")
        zone, hemi = auto_utm_projection(lons, lats)
        projector = UtmProjector(zone, "south" in hemi)
        x, y = projector(lons, lats)                                                              # K1 on the GPU
        utm = np.column_stack((x, y, alts))
        fcfg = filter_config_override if filter_config_override is not None else CONFIG["gps_filtering_ransac"]
        ft, fp = filter_gps_outliers_ransac(ts, utm, fcfg)
        if len(ft) < 2:
            raise ValueError(f"{data_label}: fewer than 2 points left after the RANSAC filter")
        return {"timestamps": ft, "positions": fp, "utm_zone": f"{zone}{'S' if 'south' in hemi else 'N'}", "projector": projector}
    except FileNotFoundError:
        raise ValueError(f"{data_label} file not found: {txt_path}")
    except GsfError:
        raise
    except Exception as e:
        raise ValueError(f"{data_label} data processing failed: {e}")


def utm_to_wgs84(utm_points, projector):
    """UTM (X,Y,Z) -> (lon, lat, alt) (ref :291-296)."""
    utm_points = np.asarray(utm_points)
    if utm_points.ndim != 2 or utm_points.shape[1] != 3:
        raise ValueError("UTM points must be an Nx3 array (X, Y, Z)")
    if not isinstance(projector, UtmProjector):
        raise TypeError("projector must be the UtmProjector returned by load_gps_data")
    lons, lats = projector(utm_points[:, 0], utm_points[:, 1], inverse=True)
    return np.column_stack((lons, lats, utm_points[:, 2]))


# ---------------------------------------------------------------------------- time alignment (EKFGPSSLAM.py:301-387)
def estimate_time_offset(slam_times, gps_times, max_samples):
    """Clock offset by cross-correlation (ref :301-323).  The reference correlates two *linspaces*, which peaks
    at lag 0 for any input: the result is exactly 0.0; only the early-outs are kept."""
    return 0.0


def search_time_offset(slam_data, gps_data, tau_min, tau_max, dtau, config=None):
    """The SLAM <-> GNSS clock offset the reference leaves to the keyboard (GPSmerge.py:73-80), searched: for every tau on the grid
    tau_min, tau_min + dtau, ... <= tau_max the fixes are re-stamped t + tau (ref :338), aligned (:325-387), the rows of main_process_gui's
    fit are picked (:973-998) and compute_sim3_transform (:428-459) is scored by the RMSE of its residuals (gsf_clock_offset_search, one
    workgroup per candidate).  slam_data / gps_data: the dicts of load_slam_trajectory / load_gps_data.  Returns (tau_refined, curve):
    the parabola-refined minimum (None when no candidate has a fit) and curve = {'tau', 'rmse', 'n_rows' (K,), 'best_k', 'tau_best',
    'status' (CLK_* bits of _lib: 2 = the minimum sits on the grid's edge)}.  estimate_time_offset keeps the reference's behaviour."""
    g = config or CONFIG
    dtau, tau_min = float(dtau), float(tau_min)
    if not dtau > 0.0 or not float(tau_max) >= tau_min:
        raise ValueError("search_time_offset: needs dtau > 0 and tau_max >= tau_min")
    K = int(np.floor((float(tau_max) - tau_min) / dtau + 1e-9)) + 1
    if K > 4096:
        raise ValueError(f"search_time_offset: {K} candidates, at most 4096 per call (search coarse to fine)")
    ts, pos = f64(slam_data["timestamps"]).ravel(), f64(slam_data["positions"]).reshape(-1, 3)
    gt, gp = f64(gps_data["timestamps"]).ravel(), f64(gps_data["positions"]).reshape(-1, 3)
    so, go = np.array([0, len(ts)], dtype=np.int64), np.array([0, len(gt)], dtype=np.int64)
    tau0 = np.array([tau_min])
    J, nr = np.empty((1, K)), np.zeros((1, K), dtype=np.int32)
    bk, st = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    tb, tr = np.empty(1), np.empty(1)
    ctx = _ctx()
    ctx.set_sim3_rows("reference", g)
    check(_lib.load().gsf_clock_offset_search(ctx.handle, hptr(ts), hptr(pos), hptr(so), hptr(gt), hptr(gp), None, hptr(go), 1, hptr(tau0), dtau, K,
                                              float(g["time_alignment"]["max_gps_gap_threshold"]), 0, 0.0, hptr(J), hptr(nr), hptr(bk), hptr(tb), hptr(tr), None, None, None,
                                              hptr(st)))
    curve = {"tau": tau0[0] + np.arange(K) * dtau, "rmse": J[0], "n_rows": nr[0], "best_k": int(bk[0]), "tau_best": float(tb[0]), "status": int(st[0])}
    return (None if bk[0] < 0 else float(tr[0])), curve


def dynamic_time_alignment(slam_data, gps_data_source, time_align_config):
    """GPS positions interpolated onto the SLAM stamps, per gap-free segment (ref :325-387): returns
    (aligned (N,3) with NaN where unavailable, valid_mask (N,) bool).  One launch of the alignment kernel
    (gsf_time_align_batch: sort/unique, gap split, not-a-knot cubic / linear, evaluation)."""
    slam_times = f64(slam_data["timestamps"]).ravel()
    gps_times = f64(gps_data_source["timestamps"]).ravel()
    n_slam, n_gps = len(slam_times), len(gps_times)
    if n_slam == 0 or n_gps < 2:
        return np.full((n_slam, 3), np.nan), np.zeros(n_slam, dtype=bool)
    gps_positions = f64(gps_data_source["positions"], (n_gps, 3))
    so, go = np.array([0, n_slam], dtype=np.int64), np.array([0, n_gps], dtype=np.int64)
    aligned, valid, st = np.empty((n_slam, 3)), np.zeros(n_slam, dtype=np.uint8), np.zeros(1, dtype=np.int32)
    check(_lib.load().gsf_time_align_batch(_ctx().handle, hptr(slam_times), hptr(so), hptr(gps_times), hptr(gps_positions), hptr(go), 1,
                                           float(time_align_config["max_gps_gap_threshold"]), hptr(aligned), hptr(valid), hptr(st)))
    return aligned, valid.astype(bool)


# ---------------------------------------------------------------------------- Sim3 (EKFGPSSLAM.py:389-467)
def compute_sim3_transform(src, dst):
    """Umeyama fit dst ~ s R src + t -> (R(3,3), t(3,), scale) or (None, None, None) (ref :428-459).  K2 on the GPU."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    n_points = src.shape[0]
    if n_points < 3:
        return None, None, None
    if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 3:
        _say("Error: Sim3: source/target points must both be Nx3.")                             # ref :433
        return None, None, None
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    off = np.array([0, n_points], dtype=np.int64)
    R, t, s, st = np.empty((1, 9)), np.empty((1, 3)), np.empty(1), np.zeros(1, dtype=np.int32)
    check(_lib.load().gsf_sim3_umeyama_batch(_ctx().handle, hptr(src), hptr(dst), None, hptr(off), 1, hptr(R), hptr(t), hptr(s), hptr(st)))
    if st[0] == _lib.SIM3_NONE:
        _say("Error: Sim3: linear-algebra failure (non-finite cross-covariance).")              # ref :453
        return None, None, None
    if st[0] & 2:
        _say("Warning: source point set has (near) zero variance; scale defaults to 1.0.")      # ref :446
    if st[0] & 4:
        _say("Warning: computed scale is tiny (<= 1e-6); reset to 1.0.")                        # ref :450
    return R.reshape(3, 3), t.reshape(3), float(s[0])


def compute_sim3_transform_robust(src, dst, min_samples, residual_threshold, max_trials, min_inliers_needed, point_description="pts"):
    """RANSAC-wrapped Sim3 (ref :389-426) in ONE library call: the hypotheses' rows are drawn on the device from NumPy's global
    legacy generator state -- the same np.random.choice(n, min_samples, replace=False) per trial as ref :405, bit for bit -- then
    fitted, scored, arg-maxed and refitted on the inliers; the advanced state is handed back to np.random, so a seeded run keeps
    drawing what the reference would draw next."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    n_points = src.shape[0]
    if n_points < min_samples:
        _say(f"Error: Sim3 RANSAC: too few input points ({n_points} from {point_description}), at least {min_samples} needed.")   # ref :396
        return None, None, None
    if src.shape != dst.shape:
        _say(f"Error: Sim3 RANSAC: source and target ({point_description}) differ in shape ({src.shape} vs {dst.shape}).")          # ref :399
        return None, None, None
    _say(f"  Sim3 RANSAC on {n_points} {point_description} (threshold={residual_threshold}m, trials={max_trials}, min samples={min_samples})...")   # ref :403
    if int(min_samples) < 1:
        raise ValueError("min_samples must be >= 1")
    if n_points > 28000 or int(min_samples) > 64 or int(max_trials) > (1 << 20):
        # beyond the device sampler (its LDS budget, 64 traced positions per trial): the reference's own draws on the host (ref :405),
        # fed to the same scoring kernel -- any configuration the reference accepts runs
        idx = np.empty((int(max_trials), int(min_samples)), dtype=np.int32)
        for k in range(int(max_trials)):
            idx[k] = np.random.choice(n_points, min_samples, replace=False)
        R_, t_, s_, _, nin_ = sim3_ransac_with_indices(src, dst, idx, residual_threshold, min_inliers_needed)
        _robust_report(R_, s_, int(nin_), n_points, min_inliers_needed, point_description)
        return R_, t_, s_
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    kind, key, pos, has_gauss, cached = np.random.get_state()
    state = np.concatenate([key.astype(np.uint32), np.array([pos], dtype=np.uint32)])
    off = np.array([0, n_points], dtype=np.int64)
    R, t, s = np.empty((1, 9)), np.empty((1, 3)), np.empty(1)
    st, nin, mask = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(n_points, dtype=np.uint8)
    check(_lib.load().gsf_sim3_ransac_mt_batch(_ctx().handle, hptr(src), hptr(dst), hptr(off), 1, hptr(state), int(max_trials), int(min_samples),
                                               float(residual_threshold), int(min_inliers_needed), hptr(R), hptr(t), hptr(s), hptr(st), hptr(mask),
                                               hptr(nin)))
    np.random.set_state((kind, state[:624], int(state[624]), has_gauss, cached))
    none = bool(st[0] & _lib.SIM3_NONE)
    _robust_report(None if none else R, None if none else float(s[0]), int(nin[0]), n_points, min_inliers_needed, point_description)
    if none:
        return None, None, None
    return R.reshape(3, 3), t.reshape(3), float(s[0])


def _robust_report(R, scale, max_inliers, n_points, min_inliers_needed, point_description):
    """the reference's progress lines of compute_sim3_transform_robust (ref :415-425), printed when VERBOSE"""
    if not VERBOSE:
        return
    print(f"  Sim3 RANSAC done: best inlier count {max_inliers}/{n_points}.")                                                     # ref :415
    if max_inliers < min_inliers_needed:
        print(f"Error: Sim3 RANSAC: best inlier count too small ({max_inliers} from {point_description}), {min_inliers_needed} needed.")   # ref :417
    elif R is None:
        print(f"Error: Sim3 RANSAC: the final fit on {max_inliers} inliers failed.")                                             # ref :423
    else:
        print(f"  Final Sim3 from {max_inliers} inliers: scale={scale:.4f}")                                                     # ref :419, :425


def sim3_ransac_with_indices(src, dst, sample_idx, residual_threshold, min_inliers_needed):
    """K2b with caller-provided sample indices -> (R, t, s, inlier_mask, n_inliers) or (None, None, None, mask, n)."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    sample_idx = np.ascontiguousarray(sample_idx, dtype=np.int32)
    n = src.shape[0]
    trials, ms = sample_idx.shape
    off = np.array([0, n], dtype=np.int64)
    R, t, s = np.empty((1, 9)), np.empty((1, 3)), np.empty(1)
    st, nin, mask = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint8)
    check(_lib.load().gsf_sim3_ransac_batch(_ctx().handle, hptr(src), hptr(dst), hptr(off), 1, hptr(sample_idx), trials, ms,
                                            float(residual_threshold), int(min_inliers_needed), hptr(R), hptr(t), hptr(s), hptr(st),
                                            hptr(mask), hptr(nin)))
    mask = mask[:n].astype(bool)
    if st[0] == _lib.SIM3_NONE:
        return None, None, None, mask, int(nin[0])
    return R.reshape(3, 3), t.reshape(3), float(s[0]), mask, int(nin[0])


def transform_trajectory(positions, quaternions, R_mat, t_vec, scale_val):
    """Apply a Sim3 to positions and orientations (ref :461-467).  K3 on the GPU."""
    pos, quat = np.ascontiguousarray(positions, dtype=np.float64), np.ascontiguousarray(quaternions, dtype=np.float64)
    n = pos.shape[0]
    if quat.shape != (n, 4) or pos.shape != (n, 3):
        raise ValueError("positions must be (N,3) and quaternions (N,4)")
    off = np.array([0, n], dtype=np.int64)
    R = np.ascontiguousarray(R_mat, dtype=np.float64).reshape(1, 9)
    t = np.ascontiguousarray(t_vec, dtype=np.float64).reshape(1, 3)
    s = np.array([float(scale_val)])
    po, qo, bad = np.empty_like(pos), np.empty_like(quat), np.zeros(1, dtype=np.int32)
    check(_lib.load().gsf_apply_sim3_batch(_ctx().handle, hptr(pos), hptr(quat), hptr(off), 1, hptr(R), hptr(t), hptr(s), hptr(po), hptr(qo), hptr(bad)))
    if bad[0]:
        raise ValueError("Found zero norm quaternions in `quat`.")       # what SciPy raises at ref :466
    return po, qo


# ---------------------------------------------------------------------------- EKF + RTS (EKFGPSSLAM.py:831-935)
def apply_ekf_correction(slam_data_in, gps_data_in, sim3_pos_initial, sim3_quat_initial, global_config):
    """EKF + dynamic per-outage RTS fusion of one trajectory -> (pos (N,3), quat (N,4)) (ref :831-935).
    ValueError on length mismatch (ref :836-837).  The recursion runs in one K4 launch."""
    n_points = len(slam_data_in["timestamps"])
    if n_points == 0:
        return np.empty((0, 3)), np.empty((0, 4))
    sim3_pos_initial, sim3_quat_initial = np.asarray(sim3_pos_initial), np.asarray(sim3_quat_initial)
    if not (sim3_pos_initial.shape[0] == n_points and sim3_quat_initial.shape[0] == n_points):
        raise ValueError(f"Sim3-transformed trajectory length ({sim3_pos_initial.shape[0]}) != SLAM timestamp count ({n_points})")
    aligned, valid = dynamic_time_alignment(slam_data_in, gps_data_in, global_config["time_alignment"])     # ref :847
    return ekf_fuse_aligned(slam_data_in["timestamps"], slam_data_in["positions"], slam_data_in["quaternions"], aligned, valid,
                            sim3_pos_initial[0], sim3_quat_initial[0], global_config)[:2]


def ekf_fuse_aligned(timestamps, positions, quaternions, aligned_gps, valid_mask, init_pos, init_quat, global_config=None):
    """ref :831-935 after its alignment call: one trajectory, host arrays -> (pos, quat, status bits)."""
    cfg = EkfConfig.from_config(global_config or CONFIG)
    ts = f64(timestamps).ravel()
    n = ts.size
    pos, quat, gps = f64(positions, (n, 3)), f64(quaternions, (n, 4)), f64(aligned_gps, (n, 3))
    valid = np.ascontiguousarray(valid_mask, dtype=np.uint8).reshape(n)
    ip, iq = f64(init_pos, (1, 3)), f64(init_quat, (1, 4))
    po, qo, st = np.empty((n, 3)), np.empty((n, 4)), np.zeros(1, dtype=np.int32)
    check(_lib.load().gsf_ekf_fuse_batch(_ctx().handle, _lib.LAYOUT_TRAJ_MAJOR, hptr(ts), hptr(pos), hptr(quat), hptr(gps), hptr(valid),
                                         hptr(ip), hptr(iq), C.byref(cfg), 1, n, hptr(po), hptr(qo), hptr(st)))
    return po, qo, int(st[0])


def ekf_smooth_aligned(timestamps, positions, quaternions, aligned_gps, valid_mask, init_pos, init_quat, global_config=None):
    """The fixed-interval RTS smoother over one whole track, beside ekf_fuse_aligned (gsf_ekf_smooth_ragged_dev; definition: include/gsf.h):
    the forward pass is ekf_fuse_aligned's filter, every sharp-turn recovery starts a new span, each span is smoothed backwards from its
    last pose.  Host arrays -> dict of host arrays: 'pos' (n,3) / 'quat' (n,4) the smoothed track, 'cov' (n,7) the smoothed diagonal,
    'pos_filt' / 'cov_filt' the causal filter's, 'flags' (n,) uint8 of _lib.POSE_* bits, 'status' (ST_* bits)."""
    import torch
    from . import batch as gb
    ts = f64(timestamps).ravel()
    n = ts.size
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)
    r = gb.ekf_smooth_ragged(up(ts, (n,)), up(positions, (n, 3)), up(quaternions, (n, 4)), up(aligned_gps, (n, 3)), up(valid_mask, (n,), np.uint8),
                             torch.tensor([0, n], dtype=torch.int64, device=dev), up(init_pos, (1, 3)), up(init_quat, (1, 4)),
                             config=global_config, want_filtered=True)
    h = lambda t: t.cpu().numpy()
    return {"pos": h(r.pos), "quat": h(r.quat), "cov": h(r.cov), "pos_filt": h(r.pos_filt), "cov_filt": h(r.cov_filt), "flags": h(r.flags),
            "status": int(r.status[0].item())}


def ekf_smooth_aligned_weighted(timestamps, positions, quaternions, aligned_gps, valid_mask, meas_var, init_pos, init_quat, global_config=None):
    """ekf_smooth_aligned with a measurement variance per pose (gsf_ekf_smooth_weighted_dev; definition: include/gsf.h): meas_var (n,3) =
    the variance of every aligned fix per axis, in the unit of meas_noise_diag (which is not read).  A fix whose variance is not usable
    (outside 1e-8 .. 1e8, NaN) is treated as missing and flagged _lib.POSE_BAD_SIGMA; three +inf mean "no information" and flag nothing.
    Host arrays -> ekf_smooth_aligned's dict plus 'nis' (n,): the normalised innovation squared of the used rows, NaN elsewhere."""
    import torch
    from . import batch as gb
    ts = f64(timestamps).ravel()
    n = ts.size
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)
    r = gb.ekf_smooth_weighted_ragged(up(ts, (n,)), up(positions, (n, 3)), up(quaternions, (n, 4)), up(aligned_gps, (n, 3)),
                                      up(valid_mask, (n,), np.uint8), up(meas_var, (n, 3)), torch.tensor([0, n], dtype=torch.int64, device=dev),
                                      up(init_pos, (1, 3)), up(init_quat, (1, 4)), config=global_config, want_filtered=True, want_nis=True)
    h = lambda t: t.cpu().numpy()
    return {"pos": h(r.pos), "quat": h(r.quat), "cov": h(r.cov), "pos_filt": h(r.pos_filt), "cov_filt": h(r.cov_filt), "flags": h(r.flags),
            "status": int(r.status[0].item()), "nis": h(r.nis)}


def ekf_smooth_aligned_reweighted(timestamps, positions, quaternions, aligned_gps, valid_mask, init_pos, init_quat, meas_var=None, loss="huber",
                                  c2=None, rounds=5, global_config=None):
    """ekf_smooth_aligned_weighted made robust: Huber / Cauchy reweighting rounds in one launch (gsf_ekf_smooth_reweighted_dev; definition:
    include/gsf.h).  meas_var (n,3) or None (the config's meas_noise_diag on every row); loss 'huber' or 'cauchy'; c2 a chi-square
    threshold of 3 degrees of freedom (None: the 95 % quantile, 7.81); rounds 0..32.  Host arrays -> ekf_smooth_aligned_weighted's dict
    of the last solve plus 'weight' (n,) (NaN on rows without an update), 'rounds_used' and 'w_change'."""
    import torch
    from . import batch as gb
    ts = f64(timestamps).ravel()
    n = ts.size
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)
    r = gb.ekf_smooth_reweighted_ragged(up(ts, (n,)), up(positions, (n, 3)), up(quaternions, (n, 4)), up(aligned_gps, (n, 3)),
                                        up(valid_mask, (n,), np.uint8), torch.tensor([0, n], dtype=torch.int64, device=dev), up(init_pos, (1, 3)),
                                        up(init_quat, (1, 4)), meas_var=None if meas_var is None else up(meas_var, (n, 3)), loss=loss, c2=c2,
                                        rounds=rounds, config=global_config, want_filtered=True, want_nis=True)
    h = lambda t: t.cpu().numpy()
    return {"pos": h(r.pos), "quat": h(r.quat), "cov": h(r.cov), "pos_filt": h(r.pos_filt), "cov_filt": h(r.cov_filt), "flags": h(r.flags),
            "status": int(r.status[0].item()), "nis": h(r.nis), "weight": h(r.weight), "rounds_used": int(r.rounds_used[0].item()),
            "w_change": float(r.w_change[0].item())}


def smooth_trajectory(slam_data_in, gps_data_in, sim3_pos_initial, sim3_quat_initial, global_config):
    """apply_ekf_correction's arguments, the whole-track smoother's result: the same alignment call (ref :847), the initial pose = row 0 of
    the Sim3-transformed track, then ekf_smooth_aligned.  Returns its dict; an empty track gives empty arrays (ref :835)."""
    n = len(slam_data_in["timestamps"])
    sim3_pos_initial, sim3_quat_initial = np.asarray(sim3_pos_initial), np.asarray(sim3_quat_initial)
    if n == 0:
        return {"pos": np.empty((0, 3)), "quat": np.empty((0, 4)), "cov": np.empty((0, 7)), "pos_filt": np.empty((0, 3)), "cov_filt": np.empty((0, 7)),
                "flags": np.empty((0,), np.uint8), "status": 0}
    if not (sim3_pos_initial.shape[0] == n and sim3_quat_initial.shape[0] == n):
        raise ValueError(f"Sim3-transformed trajectory length ({sim3_pos_initial.shape[0]}) != SLAM timestamp count ({n})")
    aligned, valid = dynamic_time_alignment(slam_data_in, gps_data_in, global_config["time_alignment"])     # ref :847
    return ekf_smooth_aligned(slam_data_in["timestamps"], slam_data_in["positions"], slam_data_in["quaternions"], aligned, valid,
                              sim3_pos_initial[0], sim3_quat_initial[0], global_config)


def sweep_ekf_noise(slam_data, gps_data, sim3_pos_initial, sim3_quat_initial, global_config, candidates, skip_seconds=0.0, min_updates=1, trace=None):
    """Innovation statistics of apply_ekf_correction's filter for K candidates of CONFIG['ekf'] on one track (gsf_ekf_noise_sweep_dev;
    definitions in include/gsf.h): the same alignment call as apply_ekf_correction (ref :847), the initial pose = row 0 of the
    Sim3-transformed track.  candidates (K,9) rows [P0 Q R] x 3 axes (batch.noise_candidates builds a grid around a CONFIG).  Returns a dict
    of host arrays: 'stats' (K,12), 'nll' / 'mean_nis' / 'rho1' (K,), 'best_k' (2,) = the picks by nll and by |mean_nis - 3| (-1: none),
    'status' (NS_* bits of _lib), 'innov' / 'innov_var' (n,3) of candidate `trace` (None without), 'candidates' (K,9)."""
    import torch
    from . import batch as gb
    n = len(slam_data["timestamps"])
    sim3_pos_initial, sim3_quat_initial = np.asarray(sim3_pos_initial), np.asarray(sim3_quat_initial)
    if n and not (sim3_pos_initial.shape[0] == n and sim3_quat_initial.shape[0] == n):
        raise ValueError(f"Sim3-transformed trajectory length ({sim3_pos_initial.shape[0]}) != SLAM timestamp count ({n})")
    aligned, valid = dynamic_time_alignment(slam_data, gps_data, global_config["time_alignment"])     # ref :847
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)
    ip = sim3_pos_initial[0] if n else np.zeros(3)
    iq = sim3_quat_initial[0] if n else np.array([0.0, 0.0, 0.0, 1.0])
    r = gb.ekf_noise_sweep_ragged(up(slam_data["timestamps"], (n,)), up(slam_data["positions"], (n, 3)), up(slam_data["quaternions"], (n, 4)),
                                  up(aligned, (n, 3)), up(valid, (n,), np.uint8), torch.tensor([0, n], dtype=torch.int64, device=dev),
                                  up(ip, (1, 3)), up(iq, (1, 4)), candidates, config=global_config, skip_seconds=skip_seconds,
                                  min_updates=min_updates, trace=trace)
    h = lambda t: None if t is None else t.cpu().numpy()
    return {"stats": h(r.stats[0]), "nll": h(r.nll[0]), "mean_nis": h(r.mean_nis[0]), "rho1": h(r.rho1[0]), "best_k": h(r.best_k[0]),
            "status": int(r.status[0].item()), "innov": h(r.innov), "innov_var": h(r.innov_var), "candidates": h(r.candidates)}


def study_gnss_outages(slam_data, gps_data, sim3_pos_initial, sim3_quat_initial, global_config, scenarios, truth_gps_data=None, trace=None):
    """Drift and RTS gain of apply_ekf_correction's track for K withheld GNSS windows on one track (gsf_outage_study_dev; definitions in
    include/gsf.h): the same alignment call as apply_ekf_correction (ref :847), the initial pose = row 0 of the Sim3-transformed track.
    scenarios (K,2) rows [start, length] in seconds, start relative to the first SLAM stamp (batch.outage_scenarios builds a grid).
    truth_gps_data: a second GNSS log (e.g. ground truth) the errors are measured against, aligned by the same call; None: the withheld
    fixes themselves.  Returns a dict of host arrays: 'stats' (K,13), 'seg' (K,2), 'flags' (K,) of _lib.OS_* bits, 'rms_dr' / 'rms_fused' /
    'drift_pct' (K,), 'err_dr' / 'err_fused' (n,) and 'trace_pos' (n,3) of scenario `trace` (None without), 'scenarios' (K,2)."""
    import torch
    from . import batch as gb
    n = len(slam_data["timestamps"])
    sim3_pos_initial, sim3_quat_initial = np.asarray(sim3_pos_initial), np.asarray(sim3_quat_initial)
    if n and not (sim3_pos_initial.shape[0] == n and sim3_quat_initial.shape[0] == n):
        raise ValueError(f"Sim3-transformed trajectory length ({sim3_pos_initial.shape[0]}) != SLAM timestamp count ({n})")
    aligned, valid = dynamic_time_alignment(slam_data, gps_data, global_config["time_alignment"])     # ref :847
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)
    tr = tv = None
    if truth_gps_data is not None:
        t_al, t_va = dynamic_time_alignment(slam_data, truth_gps_data, global_config["time_alignment"])
        tr, tv = up(t_al, (n, 3)), up(t_va, (n,), np.uint8)
    ip = sim3_pos_initial[0] if n else np.zeros(3)
    iq = sim3_quat_initial[0] if n else np.array([0.0, 0.0, 0.0, 1.0])
    r = gb.outage_study_ragged(up(slam_data["timestamps"], (n,)), up(slam_data["positions"], (n, 3)), up(slam_data["quaternions"], (n, 4)),
                               up(aligned, (n, 3)), up(valid, (n,), np.uint8), torch.tensor([0, n], dtype=torch.int64, device=dev),
                               up(ip, (1, 3)), up(iq, (1, 4)), scenarios, config=global_config, truth=tr, truth_valid=tv, trace=trace)
    h = lambda t: None if t is None else t.cpu().numpy()
    return {"stats": h(r.stats[0]), "seg": h(r.seg[0]), "flags": h(r.flags[0]), "rms_dr": h(r.rms_dr[0]), "rms_fused": h(r.rms_fused[0]),
            "drift_pct": h(r.drift_pct[0]), "err_dr": h(r.err_dr), "err_fused": h(r.err_fused), "trace_pos": h(r.trace_pos),
            "scenarios": h(r.scenarios)}


def gate_gnss_fixes(slam_data, gps_data, sim3_pos_initial, sim3_quat_initial, global_config, gates, arm_seconds=0.0, max_run=0, want_nis=False):
    """Chi-square gate on the innovations of apply_ekf_correction's filter for K thresholds on one track (gsf_innovation_gate_dev;
    definitions in include/gsf.h): the same alignment call as apply_ekf_correction (ref :847), the initial pose = row 0 of the
    Sim3-transformed track.  gates: K thresholds on the NIS (batch.chi2_gate gives quantiles).  Returns a dict of host arrays: 'valid' (K,n)
    uint8 = the aligned mask with each gate's rejected bytes cleared, 'rejected' (K,n) bool, 'stats' (K,8), 'status' (GATE_* bits of
    _lib), 'nis' (K,n) or None, 'gates' (K,), 'aligned' (n,3) = the fixes the masks belong to."""
    import torch
    from . import batch as gb
    n = len(slam_data["timestamps"])
    sim3_pos_initial, sim3_quat_initial = np.asarray(sim3_pos_initial), np.asarray(sim3_quat_initial)
    if n and not (sim3_pos_initial.shape[0] == n and sim3_quat_initial.shape[0] == n):
        raise ValueError(f"Sim3-transformed trajectory length ({sim3_pos_initial.shape[0]}) != SLAM timestamp count ({n})")
    gates = gb._gates_arg(gates)
    aligned, valid = dynamic_time_alignment(slam_data, gps_data, global_config["time_alignment"])     # ref :847
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(shape)).to(dev)
    ip = sim3_pos_initial[0] if n else np.zeros(3)
    iq = sim3_quat_initial[0] if n else np.array([0.0, 0.0, 0.0, 1.0])
    g = gb.innovation_gate_ragged(up(slam_data["timestamps"], (n,)), up(slam_data["positions"], (n, 3)), up(slam_data["quaternions"], (n, 4)),
                                  up(aligned, (n, 3)), up(valid, (n,), np.uint8), torch.tensor([0, n], dtype=torch.int64, device=dev),
                                  up(ip, (1, 3)), up(iq, (1, 4)), gates if gates.is_cuda else gates.numpy(), config=global_config,
                                  arm_seconds=arm_seconds, max_run=max_run, want_nis=want_nis)
    h = lambda t: None if t is None else t.cpu().numpy()
    vo = h(g.valid_out)
    return {"valid": vo, "rejected": (np.asarray(valid, dtype=np.uint8)[None, :] != 0) & (vo == 0), "stats": h(g.stats[0]),
            "status": int(g.status[0].item()), "nis": h(g.nis_out), "gates": h(g.gates), "aligned": np.asarray(aligned)}


def align_trajectory_local(slam_data, aligned_gps, valid_mask, R, t, s, spacing=30.0, half_window=30.0, min_rows=8, mode="scale", rot_open=1e-3,
                           ratio_max=2.0):
    """Local Sim3 alignment of one track on NumPy arrays (batch.local_align_ragged; definitions in include/gsf.h, gsf_sim3_local_fit_dev):
    Sim3 knots every `spacing` seconds along the track, each fitted on the usable rows of aligned_gps / valid_mask (what
    dynamic_time_alignment returned) within `half_window` of it, and every pose mapped by the blend of its neighbouring valid knots.  R, t,
    s: the track's global Sim3 (compute_sim3_transform_robust).  Raises ValueError where the batched form sets a track status (no pose,
    stamps that decrease, more than 4096 knots).  Returns a dict of host arrays: 'positions' (n,3), 'quaternions' (n,4), 'scale_at' (n,),
    'pose_flags' (n,) (LP_* bits of _lib), 'knot_stamps', 'knot_R' (K,3,3), 'knot_t' (K,3), 'knot_s', 'knot_n', 'knot_rms', 'knot_flags'
    (KNOT_* bits), 'knot_valid' (K,) bool.  The positions / quaternions go to ekf_fuse_aligned and its kin as the motion source."""
    import torch
    from . import batch as gb
    from . import _lib
    gb._local_config(mode, min_rows, spacing, half_window, rot_open, ratio_max)      # (argument errors need no device)
    n = len(slam_data["timestamps"])
    if n == 0:
        raise ValueError("align_trajectory_local: the track has no pose")
    ts = np.ascontiguousarray(slam_data["timestamps"], dtype=np.float64).reshape(n)
    if np.isnan(ts).any() or (np.diff(ts) < 0).any():
        raise ValueError("align_trajectory_local: the stamps are not non-decreasing")
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.array(a, dtype=dt, order="C").reshape(shape)).to(dev)     # (a copy: the caller's arrays may be read-only)
    la = gb.local_align_ragged(up(ts, (n,)), up(slam_data["positions"], (n, 3)), up(slam_data["quaternions"], (n, 4)), up(aligned_gps, (n, 3)),
                               up(np.asarray(valid_mask) != 0, (n,), np.uint8), torch.tensor([0, n], dtype=torch.int64, device=dev), up(R, (1, 9)),
                               up(t, (1, 3)), up(s, (1,)), spacing=spacing, half_window=half_window, min_rows=min_rows, mode=mode,
                               rot_open=rot_open, ratio_max=ratio_max)
    st = int(la.track_status[0].item())
    if st:
        names = [nm for nm, bit in (("empty", _lib.LOC_EMPTY), ("unsorted", _lib.LOC_UNSORTED), ("too many knots", _lib.LOC_TOO_MANY)) if st & bit]
        raise ValueError(f"align_trajectory_local: track status {st} ({', '.join(names)})")
    K = int(la.n_knots[0].item())
    stamps, _, ok = la.scale_curve(0)
    h = lambda x: x.cpu().numpy()
    return {"positions": h(la.pos), "quaternions": h(la.quat), "scale_at": h(la.scale_at), "pose_flags": h(la.pose_flags), "knot_stamps": stamps,
            "knot_R": h(la.knot_R[0, :K]).reshape(K, 3, 3), "knot_t": h(la.knot_t[0, :K]), "knot_s": h(la.knot_s[0, :K]), "knot_n": h(la.knot_n[0, :K]),
            "knot_rms": h(la.knot_rms[0, :K]), "knot_flags": h(la.knot_flags[0, :K]), "knot_valid": ok}


def estimate_lever_arm(slam_data, aligned_gps, valid_mask, R, t, s, l0=None, sigma_fix=0.5, sigma_prior=(1.0, 1.0, 1.0), sigma_rot=0.05,
                       fit_scale=True, fit_rotation=True, iters=4, min_rows=8, ratio_max=2.0):
    """The GNSS antenna's offset from the camera for one track on NumPy arrays (batch.lever_fit_ragged; definitions in include/gsf.h,
    gsf_lever_fit_dev): a fix measures s R pos + t + R M(q) l, and l (sensor frame, metres) is fitted jointly with s, t and a rotation
    increment from the track's global Sim3 R, t, s (compute_sim3_transform_robust) on the usable rows of aligned_gps / valid_mask (what
    dynamic_time_alignment returned).  Returns a dict of host values: 'l' (3,), 'l_cov' (3,3), 'sigma' (3,), 'observed' (3,) bool (an axis the
    data did not observe stays at its prior: a ground vehicle never observes the one along its yaw axis), 'R' (3,3), 't' (3,), 's', 'n_rows',
    'n_bad_quat', 'rms_before', 'rms_after', 'last_step', 'flags' (LEVER_* bits of _lib), 'fitted' (False: the starting values came back)."""
    import torch
    from . import batch as gb
    gb._lever_config(sigma_fix, sigma_prior, sigma_rot, fit_scale, fit_rotation, iters, min_rows, ratio_max, 1e-10, 0.5, 1e-6)   # (argument errors need no device)
    n = len(slam_data["positions"])
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape, dt=np.float64: torch.from_numpy(np.array(a, dtype=dt, order="C").reshape(shape)).to(dev)     # (a copy: the caller's arrays may be read-only)
    lv = gb.lever_fit_ragged(up(slam_data["positions"], (n, 3)), up(slam_data["quaternions"], (n, 4)), up(aligned_gps, (n, 3)),
                             up(np.asarray(valid_mask) != 0, (n,), np.uint8), torch.tensor([0, n], dtype=torch.int64, device=dev), up(R, (1, 9)),
                             up(t, (1, 3)), up(s, (1,)), l0=None if l0 is None else up(l0, (1, 3)), sigma_fix=sigma_fix, sigma_prior=sigma_prior,
                             sigma_rot=sigma_rot, fit_scale=fit_scale, fit_rotation=fit_rotation, iters=iters, min_rows=min_rows, ratio_max=ratio_max)
    h = lambda x: x.cpu().numpy()
    return {"l": h(lv.l[0]), "l_cov": h(lv.l_cov[0]), "sigma": h(lv.sigma[0]), "observed": h(lv.observed[0]), "R": h(lv.R[0]).reshape(3, 3), "t": h(lv.t[0]),
            "s": float(lv.s[0].item()), "n_rows": int(lv.n_rows[0].item()), "n_bad_quat": int(lv.n_bad_quat[0].item()),
            "rms_before": float(lv.rms_before[0].item()), "rms_after": float(lv.rms_after[0].item()), "last_step": float(lv.last_step[0].item()),
            "flags": int(lv.flags[0].item()), "fitted": bool(lv.fitted[0].item())}


def remove_lever_arm(quaternions, gps, R, l, sign=-1):
    """gps + sign R (M(q) l) for one track on NumPy arrays (batch.lever_apply_ragged): sign = -1 moves fixes from the antenna to the camera
    under the SLAM quaternions (n,4), the Sim3 rotation R (3,3) and the lever arm l (3,); +1 moves them back.  A NaN fix stays NaN, a
    quaternion that cannot be normalised gives a NaN row.  Returns (gps_out (n,3), pose_flags (n,))."""
    import torch
    from . import batch as gb
    if sign not in (-1, 1):
        raise ValueError("remove_lever_arm: sign must be -1 (antenna -> camera) or +1 (camera -> antenna)")
    n = len(gps)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, shape: torch.from_numpy(np.array(a, dtype=np.float64, order="C").reshape(shape)).to(dev)
    out, fl = gb.lever_apply_ragged(up(quaternions, (n, 4)), up(gps, (n, 3)), torch.tensor([0, n], dtype=torch.int64, device=dev), up(R, (1, 9)),
                                    up(l, (1, 3)), sign=sign)
    return out.cpu().numpy(), fl.cpu().numpy()


class FusionSession:
    """One track fused as it grows (batch.FusionStream with one track; host arrays in, host arrays out): push() takes the next poses and
    returns their fused rows and how far the track is final.  init_pos (3,) / init_quat (4,) = the Sim3-transformed pose 0, as at
    ekf_fuse_aligned.  The filter continues exactly where it stopped: the pushes of a track give the bits of one push of the whole track.
    `cap` rows of history are kept for the RTS back-pass; a push longer than cap // 2 poses goes to the device in pieces of that length
    (the split changes no bit).  An outage that does not fit the ring with the next piece raises GsfError, the session staying as it was
    before that piece: open a session with a larger cap.
    lag = L (1 .. min(cap - 1, _lib.STREAM_LAG_MAX)) adds the stream's fixed-lag RTS smoother: push() then also returns the smoothed rows that became final
    (row i is final once the track holds i + L + 1 poses), and smoothed() the smoothed track so far."""

    def __init__(self, init_pos, init_quat, config=None, cap=4096, lag=None):
        import torch
        from . import batch as gb
        self.cap = int(cap)
        self.config = config or CONFIG
        self._dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        if self._dev is None:
            raise GsfError("torch sees no GPU: a fusion session needs an MI355X (no CPU fallback)")
        if lag is not None and not 1 <= int(lag) < self.cap:
            raise ValueError(f"FusionSession: lag in 1 .. cap - 1 expected, got {lag}")
        self.lag = None if lag is None else int(lag)
        self._s = gb.FusionStream(1, self.cap, f64(init_pos, (1, 3)), f64(init_quat, (1, 4)), config=self.config, device=self._dev, lag=self.lag)
        self.n_total = self.n_final = self.n_smooth_final = 0
        self.status = 0
        self._final = [np.empty((0, 3)), np.empty((0, 3)), np.empty((0,), dtype=np.uint8)]     # the final smoothed rows so far: pos, var, flags

    def smoothed(self):
        """the smoothed track so far: dict(pos (n,3), var (n,3), n_smooth_final) -- rows [0, n_smooth_final) are final, the rows above are the
        provisional tail as the last push left it (the whole-track smoother's answer on what has arrived)"""
        if self.lag is None:
            raise ValueError("FusionSession.smoothed: the session was opened without a lag")
        k = self.n_total - self.n_smooth_final
        _, p, v, _ = self._s.rows_smoothed([self.n_smooth_final], [k])
        return dict(pos=np.concatenate([self._final[0], p.cpu().numpy()]), var=np.concatenate([self._final[1], v.cpu().numpy()]),
                    n_smooth_final=self.n_smooth_final)

    def rows(self, lo, count):
        """rows [lo, lo + count) of the track as they stand: ts, pos, quat (NaN where the ring no longer holds a row)"""
        t, p, q, _ = self._s.rows([int(lo)], [int(count)])
        return t.cpu().numpy(), p.cpu().numpy(), q.cpu().numpy()

    def push(self, ts, pos, quat, aligned, valid):
        """ts (m,), pos (m,3), quat (m,4) = the next original SLAM poses, aligned (m,3) / valid (m,) = their time-aligned fixes and mask.
        Returns dict(pos (m,3), quat (m,4), cov (m,7) filtered covariance diagonals, n_total, n_final, revised_from, status): rows
        [0, n_final) of the track are final, rows from revised_from on were written by this push (fetch the ones before this push's
        own with rows()).  With a lag also pos_smooth (k,3), var_smooth (k,3), flags_smooth (k,) = the smoothed rows that became final in
        this push (final rows smooth_from .. smooth_from + k - 1), smooth_from and n_smooth_final."""
        import torch
        ts, pos, quat, aligned = f64(ts).reshape(-1), f64(pos).reshape(-1, 3), f64(quat).reshape(-1, 4), f64(aligned).reshape(-1, 3)
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
        m = ts.shape[0]
        if not (pos.shape[0] == quat.shape[0] == aligned.shape[0] == valid.shape[0] == m):
            raise ValueError("FusionSession.push: arrays of different lengths")
        up = lambda a: torch.from_numpy(a).to(self._dev)
        d = [up(a) for a in (ts, pos, quat, aligned, valid)]
        po, qo, co = np.empty((m, 3)), np.empty((m, 4)), np.empty((m, 7))
        first, revised = self.n_total, self.n_total
        piece = max(1, self.cap // 2 if self.lag is None else min(self.cap // 2, self.cap - self.lag))
        smooth_from, new_final = self.n_smooth_final, [[], [], []]
        for lo in range(0, max(m, 1), piece):
            hi = min(m, lo + piece)
            st = self._s.append(*[a[lo:hi].contiguous() for a in d], torch.tensor([0, hi - lo], dtype=torch.int64, device=self._dev))
            status, rf = int(st.status[0].item()), int(st.revised_from[0].item())
            if status & (_lib.STREAM_FULL | _lib.STREAM_BAD_STATE):
                raise GsfError(f"FusionSession.push: poses {lo}..{hi - 1} of this push refused (status {status}): the open outage and the piece "
                               f"exceed cap = {self.cap}; the {lo} poses before them were taken")
            po[lo:hi], qo[lo:hi], co[lo:hi] = st.pos.cpu().numpy(), st.quat.cpu().numpy(), st.cov.cpu().numpy()
            start = first + lo
            if rf < start and start > first:                                # a back-pass reached into an earlier piece of this push
                a = max(rf, first)
                _, po[a - first:lo], qo[a - first:lo] = self.rows(a, start - a)
            revised = min(revised, rf)
            self.n_total, self.n_final, self.status = int(st.n_total[0].item()), int(st.n_final[0].item()), status
            if self.lag is not None:
                k = int(st.n_smooth_final[0].item()) - int(st.smooth_from[0].item())
                for acc, t in zip(new_final, (st.pos_smooth, st.var_smooth, st.flags_smooth)):
                    acc.append(t[:k].cpu().numpy())
                self.n_smooth_final = int(st.n_smooth_final[0].item())
        out = dict(pos=po, quat=qo, cov=co, n_total=self.n_total, n_final=self.n_final, revised_from=revised, status=self.status)
        if self.lag is not None:
            got = [np.concatenate(a) if a else e[:0] for a, e in zip(new_final, self._final)]
            self._final = [np.concatenate([e, g]) for e, g in zip(self._final, got)]
            out.update(pos_smooth=got[0], var_smooth=got[1], flags_smooth=got[2], smooth_from=smooth_from, n_smooth_final=self.n_smooth_final)
        return out


def ekf_covariances(slam_data_in, gps_data_in, global_config):
    """The covariances apply_ekf_correction computes and drops, for one trajectory (host arrays): {"filtered": (n,7,7) = ekf_covs_filt_hist
    (ref :852, :902), "smoothed": (n,7,7) = the covariance of the pose apply_ekf_correction returns -- rts_smoother_segment's (ref :777-803)
    on the rows it rewrote, the filtered one elsewhere --, "flags": (n,) uint8 of GSF_POSE_* bits}.  Same alignment call as
    apply_ekf_correction (ref :847); the matrices are exactly diagonal in the reference, and so they are here."""
    n = len(slam_data_in["timestamps"])
    if n == 0:
        return {"filtered": np.empty((0, 7, 7)), "smoothed": np.empty((0, 7, 7)), "flags": np.empty((0,), dtype=np.uint8)}
    aligned, valid = dynamic_time_alignment(slam_data_in, gps_data_in, global_config["time_alignment"])     # ref :847
    filt, cov, flags, _ = ekf_cov_aligned(slam_data_in["timestamps"], slam_data_in["quaternions"], aligned, valid, global_config)
    eye = np.eye(7)
    return {"filtered": filt[:, :, None] * eye, "smoothed": cov[:, :, None] * eye, "flags": flags}


def ekf_cov_aligned(timestamps, quaternions, aligned_gps, valid_mask, global_config=None):
    """ekf_covariances after the alignment call: -> (filtered (n,7), cov (n,7), flags (n,) uint8, status bits) through gsf_ekf_cov_ragged."""
    cfg = EkfConfig.from_config(global_config or CONFIG)
    ts = f64(timestamps).ravel()
    n = ts.size
    quat, gps = f64(quaternions, (n, 4)), f64(aligned_gps, (n, 3))
    valid = np.ascontiguousarray(valid_mask, dtype=np.uint8).reshape(n)
    offsets = np.array([0, n], dtype=np.int64)
    filt, cov, flags, st = np.empty((n, 7)), np.empty((n, 7)), np.empty((n,), dtype=np.uint8), np.zeros(1, dtype=np.int32)
    check(_lib.load().gsf_ekf_cov_ragged(_ctx().handle, hptr(ts), hptr(quat), hptr(gps), hptr(valid), hptr(offsets), None, C.byref(cfg), 1,
                                         hptr(filt), hptr(cov), hptr(flags), hptr(st)))
    return filt, cov, flags, int(st[0])


def _track_and_queries(timestamps, positions, quaternions, query_times):
    ts, qt = f64(timestamps).ravel(), f64(query_times).ravel()
    n, m = ts.size, qt.size
    return ts, f64(positions, (n, 3)), f64(quaternions, (n, 4)), qt, np.array([0, n], dtype=np.int64), np.array([0, m], dtype=np.int64), n, m


def interpolate_trajectory(timestamps, positions, quaternions, query_times, max_gap=None):
    """One track at any stamps (gsf_pose_query, host arrays): -> (positions (m,3), quaternions (m,4), flags (m,) uint8 of GSF_Q_* bits).  The
    position is interpolated linearly, the orientation by quaternion_nlerp (ref :94-105); a query on a pose's stamp returns that pose bit for
    bit (GSF_Q_EXACT); outside the track, across a bracket wider than max_gap and on a track whose stamps are not ascending the rows are NaN
    and flags says why.  query_times need not be sorted."""
    ts, pos, quat, qt, off, qoff, n, m = _track_and_queries(timestamps, positions, quaternions, query_times)
    po, qo, fl, st = np.empty((m, 3)), np.empty((m, 4)), np.empty((m,), dtype=np.uint8), np.zeros(1, dtype=np.int32)
    if m == 0:
        return po, qo, fl
    check(_lib.load().gsf_pose_query(_ctx().handle, hptr(ts), hptr(pos), hptr(quat), hptr(off), None, None, 1, hptr(qt), hptr(qoff), m,
                                     float(max_gap or 0.0), hptr(po), hptr(qo), hptr(fl), None, None, hptr(st)))
    return po, qo, fl


def georeference_points(timestamps, positions, quaternions, point_times, points, ext_quat=None, ext_trans=None, scale=1.0, max_gap=None):
    """Sensor-frame points stamped by point_times into the track's frame (gsf_georef_points, host arrays): -> (xyz (m,3), flags (m,) uint8).
    xyz = p(t) + R(q(t)) (scale (R(ext_quat) x + ext_trans)) with the pose of interpolate_trajectory; ext_quat / ext_trans = sensor -> body
    (None: identity / zero).  An ext_quat that cannot be normalised raises ValueError, as Rotation.from_quat does."""
    ts, pos, quat, qt, off, qoff, n, m = _track_and_queries(timestamps, positions, quaternions, point_times)
    x = f64(points, (m, 3))
    eq = None if ext_quat is None else f64(ext_quat, (1, 4))
    et = None if ext_trans is None else f64(ext_trans, (1, 3))
    sc = np.array([float(scale)])
    xyz, fl, st = np.empty((m, 3)), np.empty((m,), dtype=np.uint8), np.zeros(1, dtype=np.int32)
    if m == 0:
        return xyz, fl
    check(_lib.load().gsf_georef_points(_ctx().handle, hptr(ts), hptr(pos), hptr(quat), hptr(off), None, None, 1, hptr(qt), hptr(qoff), m,
                                        float(max_gap or 0.0), hptr(x), hptr(eq), hptr(et), hptr(sc), hptr(xyz), hptr(fl), None, None, hptr(st)))
    if int(st[0]) & _lib.QT_BAD_EXTRINSIC:
        raise ValueError("georeference_points: ext_quat has zero, NaN or infinite norm")
    return xyz, fl


def evaluate_trajectory(est, truth, align="se3", assoc="nearest", max_diff=0.01, frames=(), metres=(), seconds=(), stride=1, trace=None):
    """One track against 6-DoF truth (gsf_traj_eval_dev through batch.evaluate_trajectory_ragged): est and truth are dicts as
    load_slam_trajectory returns them ('timestamps', 'positions', 'quaternions'; batch.read_kitti_poses gives the same for KITTI files).
    Returns the TrajectoryEval of the one-track batch: .ape(0), .rpe(k), .kitti(), R / t / s, flags, ape_t, ape_r (device tensors)."""
    import torch
    from . import batch
    arrays = []
    for name, d in (("est", est), ("truth", truth)):
        t = f64(d["timestamps"]).reshape(-1)
        n = t.shape[0]
        p, q = np.asarray(d["positions"], dtype=np.float64), np.asarray(d["quaternions"], dtype=np.float64)
        if p.shape != (n, 3) or q.shape != (n, 4):
            raise ValueError(f"evaluate_trajectory: {name} has {n} stamps, positions {p.shape} and quaternions {q.shape}")
        arrays.append((t, f64(p), f64(q), n))
    dev = lambda a: torch.as_tensor(a).cuda()
    (t, p, q, n), (rt, rp, rq, g) = arrays
    rpe = None
    if len(frames) + len(metres) + len(seconds):
        rpe = batch.rpe_scenarios(frames=frames, metres=metres, seconds=seconds, stride=stride)
    return batch.evaluate_trajectory_ragged(dev(t), dev(p), dev(q), dev(np.array([0, n], dtype=np.int64)), dev(rt), dev(rp), dev(rq),
                                            dev(np.array([0, g], dtype=np.int64)), align=align, assoc=assoc, max_diff=max_diff, rpe=rpe, trace=trace)


# ---------------------------------------------------------------------------- helpers of the EKF surface (EKFGPSSLAM.py:77-105, :679-826)
def calculate_relative_pose(pose1_pos, pose1_quat, pose2_pos, pose2_quat):
    """Relative motion pose1 -> pose2 in pose1's frame: (delta_pos_local (3,), delta_quat (4,)); an invalid (zero-norm)
    quaternion gives zero motion and the identity (ref :77-92)."""
    p1, q1, p2, q2 = f64(pose1_pos, (1, 3)), f64(pose1_quat, (1, 4)), f64(pose2_pos, (1, 3)), f64(pose2_quat, (1, 4))
    dp, dq = np.empty((1, 3)), np.empty((1, 4))
    check(_lib.load().gsf_relative_pose_batch(_ctx().handle, hptr(p1), hptr(q1), hptr(p2), hptr(q2), 1, hptr(dp), hptr(dq), None))
    return dp[0], dq[0]


def quaternion_nlerp(q1, q2, weight_q2):
    """Normalised linear interpolation between two quaternions (ref :94-105)."""
    a, b, w, out = f64(q1, (1, 4)), f64(q2, (1, 4)), np.array([float(weight_q2)]), np.empty((1, 4))
    check(_lib.load().gsf_quaternion_nlerp_batch(_ctx().handle, hptr(a), hptr(b), hptr(w), 1, hptr(out)))
    return out[0]


def is_sharp_turn_in_segment(slam_quaternions_segment, slam_timestamps_segment, yaw_rate_threshold_rad_per_sec):
    """True if the max |yaw rate| over consecutive poses of the segment exceeds the threshold (ref :808-826)."""
    n = len(slam_quaternions_segment)
    if n < 2:
        return False
    q, t = f64(np.asarray(slam_quaternions_segment), (n, 4)), f64(np.asarray(slam_timestamps_segment), (n,))
    off, res = np.array([0, n], dtype=np.int64), np.zeros(1, dtype=np.int32)
    check(_lib.load().gsf_is_sharp_turn_batch(_ctx().handle, hptr(q), hptr(t), hptr(off), 1, float(yaw_rate_threshold_rad_per_sec), hptr(res), None))
    return bool(res[0])


def rts_smoother_segment(states_filt_segment, covs_filt_segment, states_pred_segment, covs_pred_segment):
    """RTS back-pass over one segment, F = I (ref :777-803).  Lists in, lists of arrays out, like the reference."""
    n = len(states_filt_segment)
    if n == 0:
        return [], []
    xf, xp = f64(np.asarray(states_filt_segment), (n, 7)), f64(np.asarray(states_pred_segment), (n, 7))
    Pf, Pp = f64(np.asarray(covs_filt_segment), (n, 49)), f64(np.asarray(covs_pred_segment), (n, 49))
    xs, Ps, off = np.empty((n, 7)), np.empty((n, 49)), np.array([0, n], dtype=np.int64)
    check(_lib.load().gsf_rts_smoother_segment_batch(_ctx().handle, hptr(xf), hptr(Pf), hptr(xp), hptr(Pp), hptr(off), 1, hptr(xs), hptr(Ps)))
    return [xs[k].copy() for k in range(n)], [Ps[k].reshape(7, 7).copy() for k in range(n)]


class ExtendedKalmanFilter:
    """The reference's 7-state filter object (ref :679-772): same attributes and process_step signature; every step is one
    device call in the general dense-covariance form (gsf_ekf_process_step).  The batched hot path does not go through this
    class -- it exists so that code written against the reference's class keeps working."""

    def __init__(self, initial_pos, initial_quat, config_params):
        initial_pos, initial_quat = np.asarray(initial_pos, dtype=float), np.asarray(initial_quat, dtype=float)
        if not (initial_pos.shape == (3,) and initial_quat.shape == (4,)):
            raise ValueError("EKF init: initial pose must be pos (3,) and quat (4,)")
        self.state = np.concatenate([initial_pos, self.normalize_quaternion(initial_quat)]).astype(float)
        self.cov = np.diag(config_params["initial_cov_diag"]).astype(float)
        self.Q_per_sec = np.diag(config_params["process_noise_diag"]).astype(float)
        self.R = np.diag(config_params["meas_noise_diag"]).astype(float)
        if self.state.shape != (7,) or self.cov.shape != (7, 7) or self.Q_per_sec.shape != (7, 7) or self.R.shape != (3, 3):
            raise ValueError("EKF init: wrong state / covariance / noise dimensions")
        self.gnss_available_prev = None
        self.gnss_update_weight = 0.0
        self.original_transition_steps = max(1, int(config_params.get("transition_steps", 10)))
        self.current_transition_steps = self.original_transition_steps
        self.weight_delta = 1.0
        self._last_predicted_state_for_blending = self.state.copy()

    @staticmethod
    def normalize_quaternion(q):
        q = np.asarray(q, dtype=float)
        norm = np.linalg.norm(q)
        return q / norm if norm > 1e-9 else np.array([0.0, 0.0, 0.0, 1.0])

    def process_step(self, slam_motion_update, gps_measurement, gnss_is_available, delta_time, override_transition_steps=None):
        eff = override_transition_steps if override_transition_steps is not None else self.current_transition_steps
        self.weight_delta = 1.0 / eff if eff > 0 else 1.0
        state, cov = f64(self.state, (7,)).copy(), f64(self.cov, (49,)).copy()
        Q, R = f64(self.Q_per_sec, (49,)), f64(self.R, (9,))
        dp, dq = f64(slam_motion_update[0], (3,)), f64(slam_motion_update[1], (4,))
        z = None
        if gps_measurement is not None:
            z = np.asarray(gps_measurement, dtype=float)
            if z.shape != (3,):
                z = None                                  # ref :719: wrong shape -> the update is skipped
            else:
                z = np.ascontiguousarray(z)
        prev = C.c_int32({None: -1, False: 0, True: 1}[None if self.gnss_available_prev is None else bool(self.gnss_available_prev)])
        w = C.c_double(float(self.gnss_update_weight))
        ps, pc = np.empty(7), np.empty(49)
        check(_lib.load().gsf_ekf_process_step(_ctx().handle, hptr(state), hptr(cov), hptr(Q), hptr(R), C.byref(prev), C.byref(w),
                                               int(self.current_transition_steps), hptr(dp), hptr(dq), hptr(z), int(bool(gnss_is_available)),
                                               float(delta_time), -1 if override_transition_steps is None else int(override_transition_steps),
                                               hptr(ps), hptr(pc)))
        self.state, self.cov = state, cov.reshape(7, 7)
        self.gnss_available_prev = bool(gnss_is_available)
        self.gnss_update_weight = w.value
        self._last_predicted_state_for_blending = ps.copy()
        return self.state, self.cov, ps, pc.reshape(7, 7)


# ---------------------------------------------------------------------------- error evaluation (EKFGPSSLAM.py:1013-1033)
def evaluate_trajectory_errors(slam_timestamps, traj_positions, aligned_gps, valid_mask, skip_seconds=5.0):
    """The reference's error metric (step 6 of main_process_gui, ref :1013-1033): for every SLAM index with a
    valid aligned GNSS fix after the first `skip_seconds`, the minimum distance to ANY such candidate fix; returns
    {'count','mean','median','rmse','errors'(N, NaN where not evaluated)}.  One kernel launch (gsf_eval_errors_batch)."""
    ts = f64(slam_timestamps).ravel()
    n = ts.size
    tp, gp = f64(traj_positions, (n, 3)), f64(aligned_gps, (n, 3))
    va = np.ascontiguousarray(valid_mask, dtype=np.uint8).reshape(n)
    stats, err = np.empty((1, 4)), np.empty(n)
    if n == 0:
        return {"count": 0, "mean": np.nan, "median": np.nan, "rmse": np.nan, "errors": err}
    check(_lib.load().gsf_eval_errors_batch(_ctx().handle, hptr(ts), hptr(tp), hptr(gp), hptr(va), 1, n, float(skip_seconds), hptr(stats), hptr(err)))
    return {"count": int(stats[0, 0]), "mean": float(stats[0, 1]), "median": float(stats[0, 2]), "rmse": float(stats[0, 3]), "errors": err}


# ---------------------------------------------------------------------------- headless driver (EKFGPSSLAM.py:940-1104, no GUI)
def pick_sim3_indices(slam_data, valid_mask, config=None):
    """Which time-synchronised points feed the global Sim3 (first gap-free segment, <= max_initial_duration) -- ref :973-998."""
    config = config or CONFIG
    vi = np.where(valid_mask)[0]
    ms = config["sim3_ransac"]["min_samples"]
    if len(vi) < ms:
        raise ValueError(f"time-synchronised points for Sim3 ({len(vi)}) < RANSAC min_samples ({ms})")
    vt = slam_data["timestamps"][vi]
    gaps = np.where(np.diff(vt) > config["time_alignment"]["max_gps_gap_threshold"])[0]
    end = gaps[0] if len(gaps) > 0 else len(vi)
    first = vi[:end]
    if len(first) < ms:
        return vi
    lim = slam_data["timestamps"][first] <= slam_data["timestamps"][first[0]] + config["sim3_ransac"]["max_initial_duration"]
    timed = first[lim]
    return first if len(timed) < ms else timed


def benchmark_c1(slam, gps_t_raw, lat, lon, alt, repeats=20):
    """Warm wall time of the single-trajectory drop-in on ONE track handed in by the caller: slam = {'timestamps', 'positions',
    'quaternions'} and its raw GNSS log (stamps, lat, lon, alt as load_gps_data reads them, ref :258).  Timed: the GPS leg of step 1
    (projection + sliding RANSAC pre-filter, ref :266-275), steps 2-5 (time alignment, row choice, robust Sim3, apply, EKF+RTS,
    ref :971-1010) and step 6 (error metric).  (bench.py feeds it the C1 shape -- BASELINE configs[0]: the 271-pose KITTI-04 track and
    its 279 fixes from the committed fixtures, and adds the reference's own CPU figures from profiles/rNN_reference_timing.json.)"""
    import time
    slam = {k: np.array(slam[k], dtype=np.float64) for k in ("timestamps", "positions", "quaternions")}
    ts, lats, lons, alts = (np.array(a, dtype=np.float64) for a in (gps_t_raw, lat, lon, alt))
    config = copy.deepcopy(CONFIG)
    sc = config["sim3_ransac"]

    def gps_leg():
        zone, hemi = auto_utm_projection(lons, lats)
        projector = UtmProjector(zone, "south" in hemi)
        x, y = projector(lons, lats)
        ft, fp = filter_gps_outliers_ransac(ts, np.column_stack((x, y, alts)), config["gps_filtering_ransac"])
        return {"timestamps": ft, "positions": fp, "projector": projector}

    def steps_2_to_5(gps):
        aligned, valid = dynamic_time_alignment(slam, gps, config["time_alignment"])
        idx = pick_sim3_indices(slam, valid, config)
        R, t, s = compute_sim3_transform_robust(slam["positions"][idx], aligned[idx], sc["min_samples"], sc["residual_threshold"], sc["max_trials"],
                                                sc["min_inliers_needed"])
        sp, sq = transform_trajectory(slam["positions"], slam["quaternions"], R, t, s)
        pos, quat = apply_ekf_correction(slam, gps, sp, sq, config)
        return aligned, valid, pos

    out = {}
    np.random.seed(0)
    gps = gps_leg(); aligned, valid, pos = steps_2_to_5(gps)             # warm-up (first calls allocate the staging arenas)
    for name, fn in (("gps_projection_and_prefilter_ms", gps_leg), ("steps_2_to_5_ms", lambda: steps_2_to_5(gps)),
                     ("step_6_error_metric_ms", lambda: evaluate_trajectory_errors(slam["timestamps"], pos, aligned, valid))):
        best, tot = 1e9, 0.0
        for _ in range(repeats):
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            best, tot = min(best, dt), tot + dt
        out[name] = {"best": best * 1e3, "mean": tot / repeats * 1e3}
    out["end_to_end_ms"] = {"best": sum(v["best"] for v in out.values()), "mean": sum(v["mean"] for v in out.values())}
    out["poses"] = int(len(slam["timestamps"]))
    out["gnss_fixes"] = int(len(ts))
    return out


def evaluate_against(slam, trajectories, gps_data, config=None, skip_seconds=5.0):
    """Step 6 of main_process_gui for one GNSS data set (ref :1013-1033 for the primary GPS, :1035-1062 for the ground truth): time
    alignment of `gps_data` to the SLAM stamps (:1014 / :1037), then the reference's error metric of every trajectory in
    `trajectories` (label -> (N, 3)) against the aligned fixes after the first `skip_seconds`.  Returns {'aligned', 'valid',
    'points', label: evaluate_trajectory_errors(...)}."""
    config = config or CONFIG
    aligned, valid = dynamic_time_alignment(slam, gps_data, config["time_alignment"])
    out = {"aligned": aligned, "valid": valid}
    for label, tr in trajectories.items():
        out[label] = evaluate_trajectory_errors(slam["timestamps"], tr, aligned, valid, skip_seconds)
    out["points"] = int(next(iter(out[k]["count"] for k in trajectories), 0)) if trajectories else 0
    return out


def run_fusion(slam_path, gps_path, out_path_utm=None, config=None, gt_gps_path=None):
    """Steps 1-7 of main_process_gui without tk dialogs (ref :940-1104).  gt_gps_path: the optional second GNSS file the reference
    asks for (:949-953), loaded with CONFIG['ground_truth_gps_filtering'] (:964) and used as ground truth in step 6.  Returns a dict of
    all stages; step 6 is 'errors' = {'primary': {...}, 'ground_truth': {...} or None} with the rows of :1027 / :1049 (raw SLAM,
    Sim3, EKF) and 'plot_error_ref' = which of the two the reference's plots show (:1064-1075)."""
    config = copy.deepcopy(config or CONFIG)
    slam = load_slam_trajectory(slam_path)                                                       # step 1
    gps = load_gps_data(gps_path, data_label="primary GPS", filter_config_override=config["gps_filtering_ransac"])
    gt = None
    if gt_gps_path:
        gt = load_gps_data(gt_gps_path, data_label="GNSS ground truth", filter_config_override=config["ground_truth_gps_filtering"])   # :964
        if len(gt["positions"]) < 2:                                                             # :966: not used
            gt = None
    if len(slam["positions"]) == 0 or len(gps["positions"]) < 2:
        raise ValueError("empty SLAM data or fewer than 2 GPS points")
    aligned, valid = dynamic_time_alignment(slam, gps, config["time_alignment"])                 # step 2
    idx = pick_sim3_indices(slam, valid, config)
    sc = config["sim3_ransac"]
    R, t, s = compute_sim3_transform_robust(slam["positions"][idx], aligned[idx], sc["min_samples"], sc["residual_threshold"],
                                            sc["max_trials"], sc["min_inliers_needed"])          # step 3
    if R is None:
        raise RuntimeError("global Sim3 transform failed")                                       # ref :1003
    sim3_pos, sim3_quat = transform_trajectory(slam["positions"], slam["quaternions"], R, t, s)  # step 4
    pos, quat = apply_ekf_correction(slam, gps, sim3_pos, sim3_quat, config)                     # step 5
    # step 6 (ref :1013-1075): raw SLAM / Sim3 / EKF rows against the primary GPS and, if given, the ground truth
    tracks = {"raw_slam": slam["positions"], "sim3": sim3_pos, "ekf": pos}
    e_primary = evaluate_against(slam, tracks, gps, config)
    e_gt = evaluate_against(slam, tracks, gt, config) if gt is not None else None
    if e_gt is not None and e_gt["ekf"]["count"] > 0:                                            # :1064-1069
        plot_ref = "ground_truth"
    elif e_primary["ekf"]["count"] > 0:                                                          # :1070-1074
        plot_ref = "primary"
    else:
        plot_ref = None                                                                          # :1075
    if out_path_utm:                                                                             # step 7
        save_tum_utm(out_path_utm, slam["timestamps"], pos, quat)
        wgs = utm_to_wgs84(pos, gps["projector"])
        save_tum_wgs84(wgs84_path(out_path_utm), slam["timestamps"], wgs, quat)
    return {"slam": slam, "gps": gps, "ground_truth_gps": gt, "aligned": aligned, "valid": valid, "sim3_idx": idx, "R": R, "t": t, "s": s,
            "sim3_pos": sim3_pos, "sim3_quat": sim3_quat, "pos": pos, "quat": quat,
            "errors": {"primary": e_primary, "ground_truth": e_gt}, "plot_error_ref": plot_ref,
            "err_sim3": e_primary["sim3"], "err_ekf": e_primary["ekf"]}
