"""Yardstick of tests/test_clock_offset*.py: the clock-offset search as a composition of the CPU oracle's restatements of the reference.

For track b and candidate k the score is what the reference's own functions give when the GNSS stamps are shifted by tau (EKFGPSSLAM.py:338):
dynamic_time_alignment (:325-387) on gps_t + tau, the row choice of main_process_gui (:973-998; oracle.pick_sim3_rows), compute_sim3_transform
(:428-459) and the RMSE of its residuals in NumPy.  The arg-min, the parabola and the status bits are the formulas of include/gsf.h in NumPy.
Also the generator of the planted-offset tracks.  Plain NumPy + the oracle: importable on the CPU tier."""
import numpy as np

CLK_NONE, CLK_AT_EDGE, CLK_FLAT = 1, 2, 4
UTM_ORIGIN = np.array([4.5e5, 5.4e6, 100.0])
TAU_TRUE = 0.30
PLANTED_SHAPES = ((130, 65), (65, 130), (271, 90))            # (poses, fixes)


def curve(u, straight=False):
    """the true path at time u: curved with varying speed (well-conditioned fits, no collinear rows), or a straight constant-velocity run"""
    u = np.asarray(u, dtype=np.float64)
    if straight:
        return np.column_stack((8.0 * u, 6.0 * u, 0.0 * u))
    return np.column_stack((1.5 * u + 6.0 * np.sin(0.31 * u), 8.0 * np.sin(0.17 * u + 0.4) + 0.02 * u * u, 0.3 * np.sin(0.11 * u)))


def make_track(n_poses, n_fixes, tau_true=TAU_TRUE, straight=False, origin=UTM_ORIGIN):
    """SLAM: a rotated, scaled, shifted copy of the path at 10 Hz.  Fixes: the path plus a UTM-sized origin from 3 s before to 3 s after the
    track, stamped u - tau_true: the GNSS clock reads tau_true less than the SLAM clock, so gps_t + tau_true is the SLAM time of a fix."""
    ts = 0.1 * np.arange(n_poses)
    a = 0.7
    R0 = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    pos = (curve(ts, straight) @ R0.T) * 0.8 + np.array([3.0, -2.0, 0.5])
    end = ts[-1] if n_poses else 0.0
    u = np.linspace(-3.0, end + 3.0, n_fixes) if n_fixes > 1 else np.full(n_fixes, 0.5 * end)
    return {"ts": ts, "pos": pos, "gps_t": u - tau_true, "gps_p": curve(u, straight) + np.asarray(origin)}


def used_fixes(gps_t, gps_p, keep=None):
    """definition step 2: keep mask, and never a fix whose easting AND northing are NaN (the loader's drop mark)"""
    gps_t, gps_p = np.asarray(gps_t, dtype=np.float64), np.asarray(gps_p, dtype=np.float64).reshape(-1, 3)
    use = ~(np.isnan(gps_p[:, 0]) & np.isnan(gps_p[:, 1]))
    if keep is not None:
        use &= np.asarray(keep).astype(bool)
    return gps_t[use], gps_p[use]


def score(orc, ts, pos, gps_t, gps_p, tau, max_gap=5.0, mode=1, min_samples=4, max_dur=180.0, min_rows=0, return_fit=False):
    """(J, n_rows) of ONE candidate on the fixes used (already filtered)"""
    ts, pos = np.asarray(ts, dtype=np.float64), np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    none = (np.nan, 0, None) if return_fit else (np.nan, 0)
    if ts.size == 0 or gps_t.size < 2:
        return none
    al, va = orc.dynamic_time_alignment(ts, gps_t + tau, gps_p, max_gap=max_gap)
    ok = va & ~np.isnan(al).any(axis=1)
    if mode == 1:
        rows = orc.pick_sim3_rows(ts, ok, min_samples, max_gap, max_dur)
        if rows is None:                                                  # ValueError of :975 / :997
            return (np.nan, int(ok.sum()), None) if return_fit else (np.nan, int(ok.sum()))
    else:
        rows = np.where(ok)[0]
    n = int(len(rows))
    need = min_rows if min_rows > 0 else min_samples
    if n < need:
        return (np.nan, n, None) if return_fit else (np.nan, n)
    R, t, s = orc.compute_sim3_transform(pos[rows], al[rows])
    if R is None:
        return (np.nan, n, None) if return_fit else (np.nan, n)
    res = al[rows] - (s * pos[rows] @ R.T + t)
    J = float(np.sqrt(np.mean(np.sum(res * res, axis=1))))
    return (J, n, (R, t, s)) if return_fit else (J, n)


def sweep(orc, ts, pos, gps_t, gps_p, keep, tau0, dtau, K, **kw):
    """J (K,), n_rows (K,), tau (K,) of one track; tau = tau0 + k * dtau in NumPy's float64 (a product, then a sum)"""
    gt, gp = used_fixes(gps_t, gps_p, keep)
    tau = tau0 + np.arange(K) * dtau
    J, nr = np.full(K, np.nan), np.zeros(K, dtype=np.int32)
    for k in range(K):
        J[k], nr[k] = score(orc, ts, pos, gt, gp, tau[k], **kw)
    return J, nr, tau


def parabola(J, tau, dtau, k):
    """tau_refined of definition step 8 on a J row"""
    if k < 0:
        return np.nan
    if 0 < k < len(J) - 1 and np.isfinite(J[k - 1]) and np.isfinite(J[k + 1]):
        a, m, c = J[k - 1] ** 2, J[k] ** 2, J[k + 1] ** 2
        if a - 2.0 * m + c > 0.0:
            return tau[k] + 0.5 * dtau * (a - c) / (a - 2.0 * m + c)
    return tau[k]


def pick(J, tau, dtau, flat_threshold=0.0):
    """best_k, tau_best, tau_refined, status of one J row (definition steps 7-9)"""
    K = len(J)
    if np.isnan(J).all():
        return -1, np.nan, np.nan, CLK_NONE
    k = int(np.nanargmin(J))                                              # the first of equal minima
    st = 0
    if K > 1 and k in (0, K - 1):
        st |= CLK_AT_EDGE
    if flat_threshold > 0.0 and np.nanmax(J) - J[k] < flat_threshold:
        st |= CLK_FLAT
    return k, tau[k], parabola(J, tau, dtau, k), st


def margin(J):
    """second-smallest minus smallest finite J (inf with fewer than two)"""
    f = np.sort(J[np.isfinite(J)])
    return np.inf if f.size < 2 else float(f[1] - f[0])
