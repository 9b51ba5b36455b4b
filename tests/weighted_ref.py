"""Per-fix GNSS noise (gsf_ekf_smooth_weighted_dev, gsf_fix_var_at_poses_dev): every rule of include/gsf.h restated per pose.

weighted_restate() is tests/test_smooth_host.restate with R a per-row array: the same statements in the same order, so that with
meas_var[i] = meas_noise_diag on every row it returns restate's bytes (tests/test_weighted_host.py holds it to that on every golden track,
which ties it to the goldens generated from the reference).  What it adds: the usable-variance rule, the row kinds (usable / bad / "no
information"), GSF_POSE_BAD_SIGMA, the normalised innovation squared -- formed relative to init_pos, as the kernel forms it -- and the
pieces a yardstick needs (the displacements, the blend weights, dt).  yardstick() runs the same recurrences in 50 digits (mpmath) on the
decisions and displacements of the restatement and rounds once.  fix_var_at_poses_ref() is the bracket rule as a linear search."""
import numpy as np
from scipy.spatial.transform import Rotation

from test_smooth_host import (BAD_QUAT, ENDED_IN_OUTAGE, GNSS_USED, HAD_OUTAGE, IN_OUTAGE, RTS_APPLIED, SHARP_TURN, SMOOTHED, SPAN_START, ST_SHARP,
                              max_yaw_rate, quat_ok)

BAD_SIGMA = 32                                                          # GSF_POSE_BAD_SIGMA
VAR_MIN, VAR_MAX = 1e-8, 1e8                                            # the stated range of a per-fix variance, both ends included
USABLE, BAD, NO_INFO = 0, 1, 2


def usable(v):
    """finite and inside the range (False for NaN, both infinities, 0, negative values)"""
    return bool(VAR_MIN <= v <= VAR_MAX)


def row_kind(v3):
    if all(usable(v) for v in v3):
        return USABLE
    if all(v == np.inf for v in v3):
        return NO_INFO
    return BAD


def weighted_restate(ts, pos, quat, aligned, valid, meas_var, ip, iq, cfg):
    """restate's dict, plus: bad (n,) bool; nis (n,) (NaN off the used rows); xr (n,3) the filtered position relative to init_pos;
    disp (n,3) the predicted displacement; w (n,) the blend weight; dt (n,)"""
    n = len(ts)
    P0, Q = (np.array(cfg["ekf"][k], float) for k in ("initial_cov_diag", "process_noise_diag"))
    thr = np.deg2rad(cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"])
    steps = int(cfg["rts_decision"]["default_ekf_transition_steps_on_sharp_turn"])
    xf, g, qf = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 4))
    Pf, Pp, avail, flags = np.zeros((n, 7)), np.zeros((n, 7)), np.zeros(n, bool), np.zeros(n, np.uint8)
    bad, nis, xr, disp, wts, dts = np.zeros(n, bool), np.full(n, np.nan), np.zeros((n, 3)), np.zeros((n, 3)), np.ones(n), np.zeros(n)
    nq = np.linalg.norm(iq)
    q = np.asarray(iq, float) / nq if nq > 1e-9 else np.array([0.0, 0.0, 0.0, 1.0])      # :683, :697-700
    xf[0], qf[0], Pf[0], Pp[0] = ip, q, P0, P0
    in_outage = not bool(valid[0])                                      # :848, :861 -- the raw mask, not NaN-gated; meas_var[0] is not read
    start, status = 0, (HAD_OUTAGE if in_outage else 0)
    flags[0] = (IN_OUTAGE if in_outage else 0) | SPAN_START
    starts, rates = [0], []
    for i in range(1, n):
        dt = max(1e-6, ts[i] - ts[i - 1])                               # :865
        if quat_ok(quat[i - 1]) and quat_ok(quat[i]):                   # calculate_relative_pose, :77-92
            r1 = Rotation.from_quat(quat[i - 1])
            dpl, dq = r1.inv().apply(pos[i] - pos[i - 1]), r1.inv() * Rotation.from_quat(quat[i])
        else:
            dpl, dq = np.zeros(3), Rotation.identity(); status |= BAD_QUAT
        rq = Rotation.from_quat(q)
        step = rq.apply(dpl)
        xp = xf[i - 1] + step                                           # :708
        q = (rq * dq).as_quat(); q = q / np.linalg.norm(q)              # :709-710
        Pp[i] = Pf[i - 1] + Q * dt                                      # :712-714
        av = bool(valid[i]) and not np.isnan(aligned[i]).any()          # :867-869
        if av:                                                          # ... and three usable variances; meas_var is read on these rows only
            kind = row_kind(meas_var[i])
            av, bad[i] = kind == USABLE, kind == BAD
        w = 1.0
        if not av and not in_outage:                                    # :875-877
            in_outage, start = True, i
            status |= HAD_OUTAGE
        elif av and in_outage:                                          # :879-894
            is_sharp = False
            if i - start >= 2:
                rate = max_yaw_rate(ts, quat, start, i)
                rates.append((rate, thr))
                is_sharp = rate > thr
            if is_sharp:                                                # a new span starts at the recovery; the one-step blend of :752-768, :889
                status |= ST_SHARP
                flags[start:i] |= SHARP_TURN
                starts.append(i)
                w = 1.0 / steps if steps > 1 else 1.0
            in_outage = False
        Pf[i] = Pp[i]
        xf[i] = xp
        xpr = xr[i - 1] + step                                          # the same prediction relative to init_pos
        xr[i] = xpr
        if av:
            R = np.array(meas_var[i], float)                            # the row's own
            k = Pp[i, :3] / (Pp[i, :3] + R)                             # :723-727
            g[i] = w * k * (aligned[i] - xp)                            # :728, :764
            xf[i] = xp + g[i]
            Pf[i, :3] = (1 - k) * Pp[i, :3] * (1 - k) + k * R * k       # :731 (the blend keeps the updated covariance, :767)
            y = (aligned[i] - ip) - xpr                                 # the innovation before any blend, relative to init_pos
            xr[i] = xpr + w * k * y
            nis[i] = float(np.sum(y * y / (Pp[i, :3] + R)))
            flags[i] = GNSS_USED
        else:
            flags[i] = IN_OUTAGE | (flags[i] & SHARP_TURN) | (BAD_SIGMA if bad[i] else 0)
        avail[i], qf[i], disp[i], wts[i], dts[i] = av, q, step, w, dt
    for s in starts:
        flags[s] |= SPAN_START
    if in_outage:
        status |= ENDED_IN_OUTAGE                                       # :932
    # ---- the backward pass, span by span (rts_smoother_segment, :777-803, in correction coordinates): R does not enter it
    e, d, reached = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, bool)
    for s, end in zip(starts, starts[1:] + [n]):
        for k in range(end - 2, s - 1, -1):
            Ppn = Pp[k + 1, :3]
            A = np.where(Ppn > 0, Pf[k, :3] / np.where(Ppn > 0, Ppn, 1.0), 0.0)      # pinv of a zero variance is 0
            e[k] = A * (e[k + 1] + g[k + 1])
            d[k] = A * A * (d[k + 1] + (Pf[k + 1, :3] - Pp[k + 1, :3]))
            reached[k] = avail[k + 1] or reached[k + 1]
    e[~reached], d[~reached] = 0.0, 0.0                                 # (structurally zero already)
    Ps = Pf.copy(); Ps[:, :3] += d
    flags[reached] |= SMOOTHED
    if reached.any():
        status |= RTS_APPLIED
    return dict(xf=xf, g=g, quat=qf, Pf=Pf, Pp=Pp, avail=avail, starts=starts, reached=reached, e=e, d=d, xs=xf + e, Ps=Ps, flags=flags, status=status,
                rates=rates, bad=bad, nis=nis, xr=xr, disp=disp, w=wts, dt=dts)


# ------------------------------------------------------------------------------------------------ the 50-digit yardstick
def yardstick(w, aligned, meas_var, ip, cfg):
    """The recurrences of include/gsf.h in 50 digits on the restatement's decisions (avail, span starts, blend weights), displacements and
    dt, each taken as the exact double it is -> float64 arrays Pf, Ps (n,3); xf, xs (n,3) absolute and xr (n,3) relative to init_pos, e, d
    (n,3); nis (n,) (NaN off the used rows)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    F = mp.mpf
    n = len(w["avail"])
    P0, Q = ([F(float(v)) for v in cfg["ekf"][k][:3]] for k in ("initial_cov_diag", "process_noise_diag"))
    Pf = [[None] * 3 for _ in range(n)]; Pp = [[None] * 3 for _ in range(n)]; x = [[None] * 3 for _ in range(n)]; g = [[F(0)] * 3 for _ in range(n)]
    nis = [None] * n
    for c in range(3):
        Pf[0][c], Pp[0][c], x[0][c] = P0[c], P0[c], F(0)
    for i in range(1, n):
        dt = F(float(w["dt"][i]))
        tot = F(0)
        for c in range(3):
            Pp[i][c] = Pf[i - 1][c] + Q[c] * dt
            xp = x[i - 1][c] + F(float(w["disp"][i, c]))
            Pf[i][c], x[i][c] = Pp[i][c], xp
            if w["avail"][i]:
                r = F(float(meas_var[i][c]))
                k = Pp[i][c] / (Pp[i][c] + r)
                y = (F(float(aligned[i][c])) - F(float(ip[c]))) - xp
                g[i][c] = F(float(w["w"][i])) * k * y
                x[i][c] = xp + g[i][c]
                Pf[i][c] = (1 - k) * Pp[i][c] * (1 - k) + k * r * k
                tot += y * y / (Pp[i][c] + r)
        nis[i] = tot if w["avail"][i] else None
    e = [[F(0)] * 3 for _ in range(n)]; d = [[F(0)] * 3 for _ in range(n)]
    starts = list(w["starts"])
    for s, end in zip(starts, starts[1:] + [n]):
        for k in range(end - 2, s - 1, -1):
            for c in range(3):
                A = Pf[k][c] / Pp[k + 1][c] if Pp[k + 1][c] > 0 else F(0)
                e[k][c] = A * (e[k + 1][c] + g[k + 1][c])
                d[k][c] = A * A * (d[k + 1][c] + (Pf[k + 1][c] - Pp[k + 1][c]))
    fl = lambda rows: np.array([[float(v) for v in row] for row in rows], float).reshape(n, 3)
    ipm = [F(float(v)) for v in ip]
    reached = np.asarray(w["reached"], bool)
    for k in range(n):
        if not reached[k]:
            e[k], d[k] = [F(0)] * 3, [F(0)] * 3
    return dict(Pf=fl(Pf), Ps=fl([[Pf[k][c] + d[k][c] for c in range(3)] for k in range(n)]), xr=fl(x), e=fl(e), d=fl(d),
                xf=fl([[ipm[c] + x[k][c] for c in range(3)] for k in range(n)]),
                xs=fl([[ipm[c] + x[k][c] + e[k][c] for c in range(3)] for k in range(n)]),
                nis=np.array([np.nan if v is None else float(v) for v in nis], float))


# ------------------------------------------------------------------------------------------------ the bracket rule
def fix_var_at_poses_ref(ts, slam_offsets, gps_t, gps_offsets, fix_var, keep=None, valid=None):
    """pose_var (P,3) of gsf_fix_var_at_poses_dev, by linear search over the kept fixes of each log (ascending stamps)"""
    P = len(ts)
    out = np.full((P, 3), np.inf)
    fix_var = np.asarray(fix_var, float).reshape(-1, 3)
    for b in range(len(slam_offsets) - 1):
        g0, g1 = int(gps_offsets[b]), int(gps_offsets[b + 1])
        kept = [j for j in range(g0, g1) if keep is None or keep[j]]
        for i in range(int(slam_offsets[b]), int(slam_offsets[b + 1])):
            if valid is not None and not valid[i]:
                continue
            lo = [j for j in kept if gps_t[j] <= ts[i]]
            hi = [j for j in kept if gps_t[j] >= ts[i]]
            if not lo or not hi:
                continue
            a, c = fix_var[lo[-1]], fix_var[hi[0]]
            out[i] = np.where(np.isnan(a) | np.isnan(c), np.nan, np.where(a > c, a, c))
    return out


# ------------------------------------------------------------------------------------------------ inputs shared by both tiers
def variances(kind, n, R, rng):
    """per-row variances (n,3) of one kind, all inside the stated range"""
    R = np.asarray(R, float)
    if kind == "constant":
        return np.tile(R, (n, 1))
    if kind == "two-class":                                             # RTK-fixed at 5 cm, single-point at 3 m
        good = rng.random(n) < 0.7
        return np.where(good[:, None], 0.05 ** 2, 3.0 ** 2) * np.ones((n, 3))
    if kind == "log-uniform":
        return 10.0 ** rng.uniform(-8, 8, (n, 3))
    if kind == "xy-equal":
        v = 10.0 ** rng.uniform(-4, 2, (n, 2))
        return np.column_stack((v[:, 0], v[:, 0], v[:, 1]))
    if kind == "all-differ":
        return 10.0 ** rng.uniform(-4, 2, (n, 3))
    if kind == "range-ends":                                            # both ends of the stated range, jumping inside a chunk and across its boundary
        v = np.where(rng.random((n, 3)) < 0.5, VAR_MIN, VAR_MAX)
        for k in (1, 2, 3, 62, 63, 64, 65, 127, 128):
            if k < n:
                v[k] = VAR_MIN if k % 2 else VAR_MAX
        return v
    raise ValueError(kind)


VAR_KINDS = ("constant", "two-class", "log-uniform", "xy-equal", "all-differ")
UTM = np.array([4.5e5, 5.4e6, 110.0])


def yardstick_tracks():
    """[(name, ts, pos, quat, aligned, valid, ip, iq, meas_var)]: 2, 65 and 129 poses with variances at both ends of the stated range
    (test_cov_gpu's planted tracks: no outage, sharp and gentle outages in one chunk, an outage that recovers at lane 0 of a chunk)"""
    from test_cov_gpu import planted_cov_tracks
    out = []
    for n, kind in ((2, 0), (65, 0), (65, 9), (129, 0), (129, 5)):
        ts, quat, aligned, valid, pos = planted_cov_tracks(n, 100 + n, with_pos=True)[kind]
        ip = aligned[0] if not np.isnan(aligned[0]).any() else pos[0] * 1.03 + UTM
        mv = variances("range-ends", n, None, np.random.default_rng(7000 + 10 * n + kind))
        out.append((f"n{n}_kind{kind}", ts, pos, quat, aligned, valid, ip, quat[0] / np.linalg.norm(quat[0]), mv))
    return out


def motivation_track(seed=0, n=271):
    """a planted track of n poses, every fix drawn at sigma = 0.05 m or 3 m with its true variance known ->
    (ts, pos, quat, aligned, valid, ip, iq, meas_var, truth (n,3))"""
    rng = np.random.default_rng(seed)
    dt = np.full(n, 0.1); dt[0] = 0.0
    ts = 500.0 + np.cumsum(dt)
    yaw = np.cumsum(np.deg2rad(2.0) * dt)
    quat = np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    truth = np.cumsum(np.c_[np.cos(yaw), np.sin(yaw), 0.01 + 0 * yaw] * 0.8, axis=0) + UTM
    # SLAM odometry: the true steps with a slow drift, so that the filter needs its fixes
    drift = np.cumsum(rng.normal(0, 0.02, (n, 3)), axis=0)
    pos = (truth - UTM) + drift
    sigma = np.where(rng.random(n) < 0.7, 0.05, 3.0)
    aligned = truth + rng.normal(0, 1, (n, 3)) * sigma[:, None]
    mv = np.repeat((sigma ** 2)[:, None], 3, axis=1)
    return ts, pos, quat, aligned, np.ones(n, bool), truth[0].copy(), quat[0].copy(), mv, truth


def bracket_case():
    """Logs for the bracket rule, one batch: 0, 1, 2 and 7 fixes; removed fixes inside and at the ends of a bracket; repeated stamps; poses
    before the first and after the last kept fix, exactly on a stamp, on a removed fix's stamp; an empty log; an empty SLAM track;
    valid = 0; a NaN variance and a NaN stamp of a pose -> dict(ts, slam_offsets, gps_t, gps_offsets, keep, fix_var, valid)"""
    rng = np.random.default_rng(11)
    grid = np.arange(-1.0, 8.01, 0.25)
    logs = [(np.empty(0), np.empty(0, np.uint8), np.array([9.0, 10.0, 11.0])),                               # an empty log
            (np.array([10.0]), np.array([1], np.uint8), np.array([9.0, 10.0, 11.0])),                        # one fix
            (np.array([10.0, 11.0]), np.array([1, 1], np.uint8), np.array([9.5, 10.0, 10.5, 11.0, 11.5])),   # two
            (np.arange(7.0), np.array([1, 0, 1, 0, 0, 1, 1], np.uint8), grid),                               # seven, removed inside
            (np.arange(7.0), np.array([0, 1, 1, 0, 1, 0, 0], np.uint8), grid),                               # removed at the ends
            (np.arange(7.0), np.zeros(7, np.uint8), grid[::4]),                                              # every fix removed
            (np.array([0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0]), np.ones(7, np.uint8), np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, np.nan])),   # repeated stamps
            (np.array([0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0]), np.array([1, 1, 0, 1, 0, 1, 1], np.uint8), np.array([1.0, 2.0, 1.5])),
            (np.array([5.0, 6.0]), np.array([1, 1], np.uint8), np.empty(0))]                                 # a log without poses
    ts = np.concatenate([l[2] for l in logs])
    so = np.zeros(len(logs) + 1, np.int64); so[1:] = np.cumsum([len(l[2]) for l in logs])
    gt = np.concatenate([l[0] for l in logs])
    go = np.zeros(len(logs) + 1, np.int64); go[1:] = np.cumsum([len(l[0]) for l in logs])
    keep = np.concatenate([l[1] for l in logs]).astype(np.uint8)
    fv = 10.0 ** rng.uniform(-6, 2, (len(gt), 3))
    fv[go[3] + 2, 1] = np.nan                                           # a NaN variance on a kept fix
    fv[go[6] + 3] = [np.inf, 1e-9, -1.0]                                # whatever a fix holds is carried, not judged, here
    valid = (rng.random(len(ts)) < 0.8).astype(np.uint8)
    return dict(ts=ts, slam_offsets=so, gps_t=gt, gps_offsets=go, keep=keep, fix_var=np.ascontiguousarray(fv), valid=valid)


# ------------------------------------------------------------------------------------------------ a track that needs the rescaled scan
def long_short_track(n=129, seed=5):
    """(name, ts, pos, quat, aligned, valid, ip, iq, meas_var): every odd row lies 1e14 s behind the row before it and carries r = 1e8, every
    even row repeats the stamp (dt = the floor 1e-6) and carries r = 1e-8.  P climbs to about 1e8 on the odd rows (Q dt <= 7e13, inside
    the stated Q dt <= 1e14) and a fix of 1e-8 follows over a step of Q 1e-6: the innovation variance S is 1e15 times the step's own D,
    thirty-two times per chunk.  The product of the scaled steps of a chunk is then 1e480: no double."""
    rng = np.random.default_rng(seed)
    dt = np.where(np.arange(n) % 2 == 1, 1e14, 0.0); dt[0] = 0.0
    ts = 500.0 + np.cumsum(dt)
    assert (np.diff(ts)[0::2] == 1e14).all() and (np.diff(ts)[1::2] == 0.0).all()      # the stamps are exact doubles
    yaw = np.deg2rad(0.5) * np.arange(n)
    quat = np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    pos = np.cumsum(np.c_[np.cos(yaw), np.sin(yaw), 0.01 + 0 * yaw] * 0.8, axis=0)
    aligned = pos * 1.03 + UTM + rng.normal(0, 0.3, (n, 3))
    mv = np.where((np.arange(n) % 2 == 1)[:, None], VAR_MAX, VAR_MIN) * np.ones((n, 3))
    return "long_short_steps", ts, pos, quat, aligned, np.ones(n, bool), aligned[0].copy(), quat[0].copy(), mv


# The smoothed variance is formed as Ps = Pf + d.  On long_short_track the row before a good fix has Pf = 1e8 and Ps = 1.1e-7: d cancels Pf
# to 1e-15 of it, and a rounding of d -- u Pf, u = 2^-53 -- is 0.1 of Ps.  No arithmetic in doubles that forms Ps this way (the reference's
# does: :786-801) can do better, so for that track |Ps - yardstick| is bounded by VAR_TOL Ps + 8 C u Pf per row: the project's relative gate
# where the ratio Pf / Ps is benign, and C u Pf where it is not.  C = the restatement's worst |Ps - yardstick| / (u Pf) over the track under
# both configs, measured 0.51 and written 0.55; 8 = the project's factor (another summation order moves a result by a few roundings).
U = 2.0 ** -53
PS_C = 0.55


def ps_within_bound(Ps, y, var_tol):
    """-> (ok, worst |dPs| / (u Pf), largest Pf / Ps of the track) for Ps (n,3) against the yardstick dict y"""
    err = np.abs(Ps - y["Ps"])
    ok = bool((err <= var_tol * y["Ps"] + 8 * PS_C * U * y["Pf"]).all())
    return ok, float((err / (U * y["Pf"])).max()), float((y["Pf"] / y["Ps"]).max())


def _pow2_rcp_below(d):
    """2^-e for d = m 2^e, 1 <= m < 2 (pow2_rcp_below of gsf_wave_common.hpp)"""
    return np.ldexp(1.0, 1 - np.frexp(d)[1])


def scan_variances(dt, avail, r, q, P0, rescale):
    """Pf (n,) of ONE axis as the wave kernels form it: chunks of 64 poses, every used fix's Moebius step scaled by a power of two, the six
    scan stages of GSF_SCAN_STAGES (row_shr 1, 2, 4, 8, row_bcast 15 and 31) composed lane by lane, the carry applied at the end.
    rescale: variance_scan<6, true>'s rescale of every lane's composed map after the third and the fifth stage (False: variance_scan as it stands)."""
    n = len(dt)
    Pf = np.empty(n)
    Pf[0] = P0
    carry = P0
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, n, 64):
            A, B, C, D = np.ones(64), np.zeros(64), np.zeros(64), np.ones(64)
            for l in range(64):
                i = c0 + l
                if i == 0 or i >= n:
                    continue
                b0 = q * dt[i]
                B[l] = b0
                if avail[i]:
                    d = b0 + r[i]; sc = _pow2_rcp_below(d)
                    A[l], B[l], C[l], D[l] = r[i] * sc, (r[i] * b0) * sc, sc, d * sc
            lane = np.arange(64)
            sources = [np.where(lane % 16 >= s, lane - s, -1) for s in (1, 2, 4, 8)]
            sources.append(np.where((lane // 16) % 2 == 1, (lane // 16) * 16 - 1, -1))      # row_bcast:15, rows 1 and 3
            sources.append(np.where(lane >= 32, 31, -1))                                     # row_bcast:31, rows 2 and 3
            for stage, src in enumerate(sources):
                has = src >= 0
                oA, oB, oC, oD = (np.where(has, v[np.maximum(src, 0)], ident) for v, ident in ((A, 1.0), (B, 0.0), (C, 0.0), (D, 1.0)))
                A, B, C, D = A * oA + B * oC, A * oB + B * oD, C * oA + D * oC, C * oB + D * oD
                if rescale and stage in (2, 4):
                    sc = _pow2_rcp_below(D)
                    A, B, C, D = A * sc, B * sc, C * sc, D * sc
            out = (A * carry + B) / (C * carry + D)
            m = min(64, n - c0)
            Pf[c0:c0 + m] = out[:m]
            if c0 == 0:
                Pf[0] = P0
            carry = Pf[c0 + m - 1]
    return Pf
