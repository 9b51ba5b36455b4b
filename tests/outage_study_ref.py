"""Per-pose NumPy restatement of the GNSS outage study (include/gsf.h, gsf_outage_study_dev): the specification the kernels are tested against.

Nothing here uses the closed form.  A scenario is evaluated the long way round: the mask bytes of its window are cleared, the position
filter of apply_ekf_correction is run pose by pose over the whole track (prediction, update, outage bookkeeping, the sharp-turn decision,
the one-step blend), and every outage that recovers without a sharp turn goes through rts_smoother_segment as the reference writes it, a
backward recurrence over the segment [a..b] (ref :777-803) restricted to the position axes (every covariance is diagonal, F = I).  The
study's row is then read off that run.  tests/test_outage_study_host.py pins the fused positions to the oracle's apply_ekf_correction on the
same cleared bytes; tests/test_outage_study.py compares the kernels with this file.  Also here: the first-order bounds of the row's sums."""
import numpy as np

from noise_sweep_ref import _conj, _ekf_normalize, _max_yaw_rate, _mul, _rot, _unit, default_candidate

EPS_P, EPS_V = 1e-6, 1e-10             # the project's gates: positions in metres per axis, variances relative
OS_EMPTY, OS_NO_RECOVERY, OS_SMOOTHED, OS_SHARP_TURN, OS_MERGED, OS_FROM_START, OS_UNSORTED, OS_SKIPPED = 1, 2, 4, 8, 16, 32, 64, 128
NSTAT = 13


def availability(aligned, valid):
    """avail[i] of gsf_ekf_cov_ragged_dev: pose 0 the raw mask byte (:848), every other pose the byte set and a fix free of NaN (:867-869)"""
    av = np.asarray(valid).astype(bool) & ~np.isnan(np.asarray(aligned, float)).any(axis=1)
    if len(av):
        av[0] = bool(valid[0])
    return av


def window(ts, s, L):
    """W = [#{t < lo}, #{t < hi}), lo = t[0] + s, hi = lo + L; (0, 0) for an empty one"""
    if np.isnan(s) or np.isnan(L) or not L > 0:
        return 0, 0
    lo = ts[0] + s
    hi = lo + L
    w0, w1 = int(np.sum(ts < lo)), int(np.sum(ts < hi))
    return (w0, w1) if w1 > w0 else (0, 0)


def motion(ts, pos, quat, init_quat):
    """d[i] = R(q_state[i-1]) dp_local[i] (ref :707) for every pose: calculate_relative_pose (:77-92) and the state quaternion chain
    (:708-709).  GNSS never touches the state quaternion, so a track's increments are the same whatever its mask holds."""
    pos, quat = np.asarray(pos, float), np.asarray(quat, float)
    n = len(ts)
    d = np.zeros((n, 3))
    q_state = _ekf_normalize(np.asarray(init_quat, float))              # ref :842, :683
    for i in range(1, n):
        r1, r2 = _unit(quat[i - 1]), _unit(quat[i])
        if r1 is None or r2 is None:                                    # calculate_relative_pose's except branch (:84-86)
            dpl, dq = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
        else:
            dpl, dq = _rot(_conj(r1), pos[i] - pos[i - 1]), _mul(_conj(r1), r2)
        d[i] = _rot(q_state, dpl)                                       # :707
        q_state = _ekf_normalize(_mul(q_state, dq))                     # :708-709
    return d


def run_filter(ts, pos, quat, aligned, valid, init_pos, init_quat, cfg, d=None):
    """The position filter of apply_ekf_correction with per-outage RTS, pose by pose.  valid is taken as it is (the caller clears bytes).
    d: motion() of the track, if the caller has it already.
    -> dict: filt (n,3) the filter's own positions, fused (n,3) what apply_ekf_correction returns, Pf / Pp (n,3), pred (n,3), d (n,3),
    outages [(a, b, sharp)] with b = n for one still open at the end, y / S (n,3) of the updates."""
    ts, pos, quat, aligned = (np.asarray(a, float) for a in (ts, pos, quat, aligned))
    n = len(ts)
    c = default_candidate(cfg)
    P0, Q, R = c[0:3], c[3:6], c[6:9]
    thr = np.deg2rad(cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"])
    steps = int(cfg["rts_decision"]["default_ekf_transition_steps_on_sharp_turn"])
    filt, Pf, Pp, pred = (np.zeros((n, 3)) for _ in range(4))
    y, S = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    filt[0], Pf[0], Pp[0], pred[0] = np.asarray(init_pos, float), P0, P0, np.asarray(init_pos, float)
    fused = filt.copy()
    d = motion(ts, pos, quat, init_quat) if d is None else d
    in_outage, start = (not bool(valid[0])), 0                          # :848, :861 -- the raw mask
    outages = []
    for i in range(1, n):
        dt = max(1e-6, ts[i] - ts[i - 1])                               # :865
        av = bool(valid[i]) and not np.isnan(aligned[i]).any()          # :867-869
        pred[i] = filt[i - 1] + d[i]
        Pp[i] = Pf[i - 1] + Q * dt                                      # :712-714
        wi, closes = 1.0, None
        if not av and not in_outage:                                    # :875-877
            in_outage, start = True, i
        elif av and in_outage:                                          # :879-894
            sharp = i - start >= 2 and _max_yaw_rate(ts, quat, start, i) > thr
            if sharp and steps > 1:
                wi = 1.0 / steps                                        # :889, :742, :755
            closes, in_outage = (start, i, sharp), False
        if av:
            y[i], S[i] = aligned[i] - pred[i], Pp[i] + R                # :722-723
            g = Pp[i] / S[i]
            Pf[i] = (1 - g) ** 2 * Pp[i] + g ** 2 * R                   # :731
            filt[i] = pred[i] + wi * g * y[i]                           # :727, :764
        else:
            Pf[i], filt[i] = Pp[i], pred[i]
        fused[i] = filt[i]
        if closes is not None:
            a, b, sharp = closes
            outages.append(closes)
            if not sharp:                                               # rts_smoother_segment over [a..b] (:777-803), position axes
                xs, Ps = filt[b].copy(), Pf[b].copy()
                for k in range(b - 1, a - 1, -1):
                    A = Pf[k] / Pp[k + 1]                               # :790, F = I
                    xs = filt[k] + A * (xs - pred[k + 1])               # :795
                    Ps = Pf[k] + A * A * (Ps - Pp[k + 1])               # :797
                    fused[k] = xs
    if in_outage and n:
        outages.append((start, n, False))
    return dict(filt=filt, fused=fused, Pf=Pf, Pp=Pp, pred=pred, d=d, outages=outages, y=y, S=S)


def sorted_stamps(ts):
    ts = np.asarray(ts, float)
    return not (np.isnan(ts).any() or (np.diff(ts) < 0).any())


def scenario(ts, pos, quat, aligned, valid, init_pos, init_quat, cfg, s, L, truth=None, truth_valid=None, base=None):
    """One track, one scenario -> dict(row (13,), seg (2,), flags, p_dr / p_fu (n,3) NaN outside [a, b), e_dr / e_fu (n,) NaN outside E,
    bound (13,) = the first-order bounds of the row, W).  base: run_filter of the unmodified track (made once per track by the caller)."""
    ts, aligned = np.asarray(ts, float), np.asarray(aligned, float)
    n = len(ts)
    nanrow = dict(row=np.full(NSTAT, np.nan), seg=np.array([-1, -1]), p_dr=np.full((n, 3), np.nan), p_fu=np.full((n, 3), np.nan),
                  e_dr=np.full(n, np.nan), e_fu=np.full(n, np.nan), bound=np.zeros(NSTAT), W=(0, 0))
    if n == 0:
        return dict(nanrow, row=np.zeros(NSTAT), flags=OS_EMPTY)
    if not sorted_stamps(ts):
        return dict(nanrow, flags=OS_UNSORTED)
    w0, w1 = window(ts, s, L)
    if w1 <= w0:
        return dict(nanrow, row=np.zeros(NSTAT), flags=OS_EMPTY)
    truth = aligned if truth is None else np.asarray(truth, float)
    truth_valid = np.asarray(valid if truth_valid is None else truth_valid).astype(bool)
    avail = availability(aligned, valid)
    cleared = np.asarray(valid).astype(bool).copy()
    cleared[w0:w1] = False
    run = run_filter(ts, pos, quat, aligned, cleared, init_pos, init_quat, cfg, d=None if base is None else base["d"])
    seg = [o for o in run["outages"] if o[0] <= w0 < o[1]]
    assert len(seg) == 1, (run["outages"], w0, w1)
    a, b, sharp = seg[0]
    assert b >= w1
    rec = b < n
    flags = (OS_NO_RECOVERY if not rec else (OS_SHARP_TURN if sharp else OS_SMOOTHED)) | (OS_MERGED if (a < w0 or b > w1) else 0) \
        | (OS_FROM_START if a == 0 else 0)
    c, be = max(a - 1, 0), min(b, n - 1)
    if base is not None:                                                # nothing before the outage changes
        assert np.array_equal(base["filt"][:a], run["filt"][:a]) and np.array_equal(base["Pf"][:a], run["Pf"][:a])
    p_dr, p_fu = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    p_dr[a:b], p_fu[a:b] = run["filt"][a:b], run["fused"][a:b]
    E = np.zeros(n, bool)
    E[a:b] = truth_valid[a:b] & ~np.isnan(truth[a:b]).any(axis=1)
    H = [i for i in range(w0, w1) if i >= 1 and avail[i]]
    v_dr, v_fu = p_dr[E] - truth[E], p_fu[E] - truth[E]
    e_dr, e_fu = np.full(n, np.nan), np.full(n, np.nan)
    e_dr[E], e_fu[E] = np.sqrt((v_dr ** 2).sum(axis=1)), np.sqrt((v_fu ** 2).sum(axis=1))
    row, bound = np.zeros(NSTAT), np.zeros(NSTAT)
    dl = np.sqrt((run["d"][c + 1:be + 1] ** 2).sum(axis=1))
    row[0:5] = E.sum(), len(H), b - a, ts[be] - ts[c], dl.sum()
    row[5], row[7] = (e_dr[E] ** 2).sum(), (e_fu[E] ** 2).sum()
    row[6], row[8] = (e_dr[E].max(), e_fu[E].max()) if E.any() else (0.0, 0.0)
    row[9], row[10] = (v_dr[:, :2] ** 2).sum(), (v_fu[:, :2] ** 2).sum()
    # ---- bounds.  A kernel position within EPS_P per axis moves an error norm by at most sqrt(3) EPS_P (sqrt(2) horizontally) and a
    # squared error by 2 e sqrt(3) EPS_P to first order.  dist is a difference of two prefix sums of |d| over the track: a sum of m <= 4096
    # terms carries at most m 2^-53 < 5e-13 of itself, so 1e-12 of the distance travelled up to each end, plus 1e-12 of the sum itself.
    r3, r2 = np.sqrt(3.0) * EPS_P, np.sqrt(2.0) * EPS_P
    assert n <= 4096
    bound[4] = 2e-12 * np.sqrt((run["d"][1:be + 1] ** 2).sum(axis=1)).sum() + 1e-12 * dl.sum()
    bound[5] = (2 * e_dr[E] * r3).sum() + 1e-12 * row[5]
    bound[7] = (2 * e_fu[E] * r3).sum() + 1e-12 * row[7]
    bound[6] = bound[8] = r3
    bound[9] = (2 * np.sqrt((v_dr[:, :2] ** 2).sum(axis=1)) * r2).sum() + 1e-12 * row[9]
    bound[10] = (2 * np.sqrt((v_fu[:, :2] ** 2).sum(axis=1)) * r2).sum() + 1e-12 * row[10]
    if rec:
        y, S = run["y"][b], run["S"][b]
        row[11], row[12] = np.sqrt((y ** 2).sum()), (y ** 2 / S).sum()
        bound[11] = r3
        bound[12] = ((2 * np.abs(y) * EPS_P + y ** 2 * EPS_V) / S).sum() + 1e-12 * row[12]
    else:
        row[11] = row[12] = np.nan
    return dict(row=row, seg=np.array([a, b]), flags=flags, p_dr=p_dr, p_fu=p_fu, e_dr=e_dr, e_fu=e_fu, bound=bound, W=(w0, w1), run=run)


def study(track, scen, cfg, truth=None, truth_valid=None):
    """track = (ts, pos, quat, aligned, valid, init_pos, init_quat); scen (K,2) -> list of scenario() results"""
    base = run_filter(*track, cfg) if len(track[0]) and sorted_stamps(track[0]) else None
    return [scenario(*track, cfg, float(s), float(L), truth=truth, truth_valid=truth_valid, base=base) for s, L in np.asarray(scen, float).reshape(-1, 2)]


def pose_window(ts, i0, count):
    """(start, length) of a scenario whose window is exactly the poses i0 .. i0+count-1 of a track with strictly increasing stamps there:
    it starts half a step before t[i0] (at pose 0: before the track) and ends half a step before t[i0+count] (past the end: after it)"""
    ts = np.asarray(ts, float)
    n = len(ts)
    lo = ts[i0] - (0.5 * (ts[i0] - ts[i0 - 1]) if i0 > 0 else 1.0)
    j = i0 + count
    hi = ts[j] - 0.5 * (ts[j] - ts[j - 1]) if j < n else ts[n - 1] + 1.0
    return lo - ts[0], hi - lo


def scenario_list(ts, aligned, valid):
    """The fixed scenarios of one track, as (K,2) rows [start, length] and a tag per row: windows of 1 and 2 poses, over pose 0, to the
    track's end, abutting the track's natural outages on the left, on the right and on both sides, wholly inside one, across poses
    63/64/65 and 127/128, at the quarter points of the track's duration, and the empty ones (between two stamps, beyond the end, L = 0,
    L < 0, NaN start, NaN length).  What does not fit a short track is left out."""
    ts = np.asarray(ts, float)
    n = len(ts)
    out = []
    add = lambda i0, count, tag: out.append((*pose_window(ts, i0, count), tag)) if (0 <= i0 and count >= 1 and i0 + count <= n) else None
    if n == 0:
        return np.array([[0.0, 1.0]]), ["empty track"]
    mid = n // 2
    add(mid, 1, "one pose"); add(mid, 2, "two poses"); add(0, min(3, n), "over pose 0"); add(n - min(4, n), min(4, n), "to the end")
    add(0, n, "the whole track")
    av = availability(aligned, valid)
    runs, i = [], 0
    while i < n:                                                        # natural outages [ra, rb)
        if not av[i]:
            j = i
            while j < n and not av[j]:
                j += 1
            runs.append((i, j)); i = j
        else:
            i += 1
    for ra, rb in runs[:3]:
        add(ra - 2, 2, "abuts a natural outage on its right"); add(rb, 2, "abuts a natural outage on its left")
        add(ra, min(2, rb - ra), "inside a natural outage"); add(ra - 1, rb - ra + 2, "covers a natural outage")
    for (_, rb), (ra2, _) in zip(runs[:-1], runs[1:]):
        if ra2 - rb <= 40:
            add(rb, ra2 - rb, "between two natural outages"); break
    add(62, 4, "across 63/64/65"); add(60, 70, "across two chunk boundaries"); add(127, 2, "across 127/128")
    span = ts[-1] - ts[0] if sorted_stamps(ts) else 1.0
    for q in (0.25, 0.5, 0.75):
        out.append((q * span, 0.1 * span + 0.05, f"quarter point {q}"))
    step = ts[mid] - ts[mid - 1] if mid >= 1 else 0.0
    if step > 0:
        out.append((ts[mid - 1] - ts[0] + 0.25 * step, 0.25 * step, "empty: between two stamps"))
    out += [(span + 5.0, 3.0, "empty: beyond the end"), (0.3 * span, 0.0, "empty: L = 0"), (0.3 * span, -1.0, "empty: L < 0"),
            (np.nan, 1.0, "empty: NaN start"), (0.3 * span, np.nan, "empty: NaN length")]
    return np.array([[s, L] for s, L, _ in out]), [t for _, _, t in out]
