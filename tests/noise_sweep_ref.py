"""Per-pose NumPy restatement of the EKF noise sweep (include/gsf.h, gsf_ekf_noise_sweep_dev): the specification the kernel is tested against.

Everything is a plain loop over the poses of one track, vectorised over the K candidates only.  tests/test_noise_sweep_host.py pins y and S
of this file to what the reference's own process_step gave (tests/golden/noise_sweep_tracks.npz); tests/test_noise_sweep.py compares the
kernel with it.  Also here: the tolerances of the twelve sums, propagated to first order from the project's per-pose gates, the picks,
and the planted-noise batch both tiers use."""
import numpy as np

EPS_Y, EPS_S = 1e-6, 1e-10             # the project's gates: positions in metres, variances relative
LN_2PI = 1.8378770664093453
NS_NONE, NS_TIE = 1, 2


# ------------------------------------------------------------------------------------------------ quaternions (scalar last)
def _unit(q):
    n = np.sqrt(np.dot(q, q))
    if not (np.isfinite(n) and n > 0.0):
        return None                                                     # Rotation.from_quat raises ValueError
    return q / n


def _mul(p, q):
    return np.array([p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1],
                     p[3] * q[1] - p[0] * q[2] + p[1] * q[3] + p[2] * q[0],
                     p[3] * q[2] + p[0] * q[1] - p[1] * q[0] + p[2] * q[3],
                     p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]])


def _conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def _rot(q, v):
    u = q[:3]
    t = 2.0 * np.cross(u, v)
    return v + q[3] * t + np.cross(u, t)


def _ekf_normalize(q):                                                  # ref :697-700
    n = np.sqrt(np.dot(q, q))
    return q / n if n > 1e-9 else np.array([0.0, 0.0, 0.0, 1.0])


def _yaw(q):                                                            # as_euler('zyx')[0] = atan2(-m01, m00), scale-free
    x, y, z, w = q
    return np.arctan2(2.0 * (z * w - x * y), w * w + x * x - y * y - z * z)


def _max_yaw_rate(ts, quat, a, b):                                      # is_sharp_turn_in_segment over the poses a..b-1 (ref :808-826)
    rate = 0.0
    for k in range(a + 1, b):
        if ts[k] > ts[k - 1]:
            if _unit(quat[k - 1]) is None or _unit(quat[k]) is None:
                return np.inf                                           # :821 returns True whatever the threshold
            d = _yaw(quat[k]) - _yaw(quat[k - 1])
            rate = max(rate, abs(np.arctan2(np.sin(d), np.cos(d)) / (ts[k] - ts[k - 1])))
    return rate


# ------------------------------------------------------------------------------------------------ the restatement
def restate(ts, pos, quat, aligned, valid, init_pos, init_quat, cand, cfg, skip_seconds=0.0):
    """One track, K candidates.  -> dict: y (K,n,3), S (K,n,3) (NaN where no update), upd (n,) bool, counted (n,) bool, w (n,), stats (K,12),
    p (K,n,3) the filter's positions, Pf (K,n,3)."""
    ts, pos, quat, aligned = (np.asarray(a, float) for a in (ts, pos, quat, aligned))
    cand = np.asarray(cand, float).reshape(-1, 9)
    K, n = cand.shape[0], len(ts)
    P0, Q, R = cand[:, 0:3], cand[:, 3:6], cand[:, 6:9]
    thr = np.deg2rad(cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"])
    steps = int(cfg["rts_decision"]["default_ekf_transition_steps_on_sharp_turn"])
    y, S = np.full((K, n, 3), np.nan), np.full((K, n, 3), np.nan)
    p, Pf = np.empty((K, n, 3)), np.empty((K, n, 3))
    upd, counted, w = np.zeros(n, bool), np.zeros(n, bool), np.ones(n)
    stats = np.zeros((K, 12))
    if n == 0:
        return dict(y=y, S=S, upd=upd, counted=counted, w=w, stats=stats, p=p, Pf=Pf)
    p[:, 0], Pf[:, 0] = np.asarray(init_pos, float), P0
    q_state = _ekf_normalize(np.asarray(init_quat, float))              # ref :842, :683
    in_outage, start = (not bool(valid[0])), 0                          # :848, :861 -- the raw mask
    nu_prev, counted_prev = np.zeros((K, 3)), False
    for i in range(1, n):
        dt = max(1e-6, ts[i] - ts[i - 1])                               # :865
        r1, r2 = _unit(quat[i - 1]), _unit(quat[i])
        if r1 is None or r2 is None:                                    # calculate_relative_pose's except branch (:84-86)
            dpl, dq = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
        else:
            dpl, dq = _rot(_conj(r1), pos[i] - pos[i - 1]), _mul(_conj(r1), r2)
        d = _rot(q_state, dpl)                                          # :707
        q_state = _ekf_normalize(_mul(q_state, dq))                     # :708-709
        av = bool(valid[i]) and not np.isnan(aligned[i]).any()          # :867-869
        wi = 1.0
        if not av and not in_outage:                                    # :875-877
            in_outage, start = True, i
        elif av and in_outage:                                          # :879-894
            if i - start >= 2 and _max_yaw_rate(ts, quat, start, i) > thr and steps > 1:
                wi = 1.0 / steps                                        # :889, :742, :755
            in_outage = False
        pm = p[:, i - 1] + d                                            # :707
        Pp = Pf[:, i - 1] + Q * dt                                      # :712-714
        if av:
            yi, Si = aligned[i] - pm, Pp + R                            # :722-723
            g = Pp / Si
            Pf[:, i] = (1 - g) ** 2 * Pp + g ** 2 * R                   # :731
            p[:, i] = pm + wi * g * yi                                  # :727, :764
            y[:, i], S[:, i], upd[i], w[i] = yi, Si, True, wi
            cnt = (skip_seconds <= 0.0) or (ts[i] > ts[0] + skip_seconds)
            nu = yi / np.sqrt(Si) if cnt else np.zeros((K, 3))
            if cnt:
                counted[i] = True
                stats[:, 0] += 1.0
                stats[:, 1:4] += yi * yi / Si
                stats[:, 4:7] += np.log(Si)
                stats[:, 7:10] += yi * yi
                if counted_prev:
                    stats[:, 10] += (nu * nu_prev).sum(axis=1)
                    stats[:, 11] += 1.0
            nu_prev, counted_prev = nu, cnt
        else:
            Pf[:, i], p[:, i] = Pp, pm
            nu_prev, counted_prev = np.zeros((K, 3)), False
    return dict(y=y, S=S, upd=upd, counted=counted, w=w, stats=stats, p=p, Pf=Pf)


def stat_bounds(r):
    """First-order bounds of the twelve sums of restate()'s result r for a kernel whose y is within EPS_Y and whose S is within EPS_S
    relative of r's: NIS sum (2|y| ey + y^2 eS) / S; log S: n eS; y^2: sum 2 |y| ey; lag term: sum (|nu_i| + |nu_{i-1}|) ey / sqrt(S) --
    each with 1e-12 sum |term| on top for the order of summation.  Counts are exact.  -> (K,12)"""
    y, S, c = r["y"], r["S"], r["counted"]
    K = y.shape[0]
    b = np.zeros((K, 12))
    if not c.any():
        return b
    yc, Sc = np.abs(y[:, c]), S[:, c]                                   # (K, m, 3)
    b[:, 1:4] = ((2 * yc * EPS_Y + yc ** 2 * EPS_S) / Sc).sum(axis=1) + 1e-12 * (yc ** 2 / Sc).sum(axis=1)
    b[:, 4:7] = c.sum() * EPS_S + 1e-12 * np.abs(np.log(Sc)).sum(axis=1)
    b[:, 7:10] = (2 * yc * EPS_Y).sum(axis=1) + 1e-12 * (yc ** 2).sum(axis=1)
    idx = np.flatnonzero(c)
    pairs = idx[1:][np.diff(idx) == 1]                                  # i with i and i-1 both counted
    if len(pairs):
        nu = np.abs(y / np.sqrt(S))
        a, bb = nu[:, pairs], nu[:, pairs - 1]
        b[:, 10] = ((a + bb) * EPS_Y / np.sqrt(S[:, pairs])).sum(axis=(1, 2)) + 1e-12 * (a * bb).sum(axis=(1, 2))
    return b


def derived(rows):
    """nll, mean_nis, rho1 of rows (..., 12), in the library's association"""
    rows = np.asarray(rows, float)
    n = rows[..., 0]
    nis = (rows[..., 1] + rows[..., 2]) + rows[..., 3]
    ls = (rows[..., 4] + rows[..., 5]) + rows[..., 6]
    with np.errstate(invalid="ignore", divide="ignore"):
        return 0.5 * (((3.0 * n) * LN_2PI + ls) + nis), nis / n, rows[..., 10] / (3.0 * rows[..., 11])


def picks(rows, min_updates=1):
    """(first k with the smallest nll, first k with the smallest |mean_nis - 3|) over rows (K,12); -1 without enough updates or a finite row"""
    rows = np.asarray(rows, float)
    if not rows[0, 0] >= min_updates:
        return -1, -1
    nll, nis, _ = derived(rows)
    fin = np.isfinite(rows).all(axis=1)
    out = []
    for s in (nll, np.abs(nis - 3.0)):
        s = np.where(fin & np.isfinite(s), s, np.inf)
        out.append(int(np.argmin(s)) if np.isfinite(s).any() else -1)
    return tuple(out)


def status_of(b0, b1):
    return NS_NONE if (b0 < 0 or b1 < 0) else (NS_TIE if b0 != b1 else 0)


# ------------------------------------------------------------------------------------------------ planted noise
def default_candidate(cfg):
    e = cfg["ekf"]
    return np.array([float(x) for x in e["initial_cov_diag"][:3]] + [float(x) for x in e["process_noise_diag"][:3]]
                    + [float(x) for x in e["meas_noise_diag"][:3]])


def planted_batch(cfg, seed, B=16, N=65):
    """B tracks of N poses drawn from the filter's OWN model under cfg's noise: the true position starts at init_pos + N(0, P0), moves by
    the odometry increment plus N(0, Q dt) per step, and every fix is the truth plus N(0, R).  The SLAM orientation stays the identity,
    so the world-frame increment is the SLAM position difference.  One outage of 3..8 poses per track.
    -> list of (ts, pos, quat, aligned, valid, init_pos, init_quat)"""
    rng = np.random.default_rng(seed)
    c = default_candidate(cfg)
    P0, Q, R = c[0:3], c[3:6], c[6:9]
    out = []
    for _ in range(B):
        dt = rng.uniform(0.08, 0.12, N); dt[0] = 0.0
        ts = 100.0 + np.cumsum(dt)
        step = np.c_[0.8 + 0.1 * rng.normal(size=N), 0.2 * rng.normal(size=N), 0.02 * rng.normal(size=N)] * (dt[:, None] / 0.1)
        pos = np.cumsum(step, axis=0)
        quat = np.tile([0.0, 0.0, 0.0, 1.0], (N, 1))
        init_pos = np.array([4.5e5, 5.4e6, 110.0]) + rng.normal(0, 5.0, 3)
        truth = np.empty((N, 3))
        truth[0] = init_pos + rng.normal(0, 1, 3) * np.sqrt(P0)
        for i in range(1, N):
            truth[i] = truth[i - 1] + (pos[i] - pos[i - 1]) + rng.normal(0, 1, 3) * np.sqrt(Q * dt[i])
        aligned = truth + rng.normal(0, 1, (N, 3)) * np.sqrt(R)
        valid = np.ones(N, bool)
        a = int(rng.integers(5, N - 12)); L = int(rng.integers(3, 9))
        valid[a:a + L] = False
        aligned[~valid] = np.nan
        out.append((ts, pos, quat, aligned, valid, init_pos, np.array([0.0, 0.0, 0.0, 1.0])))
    return out


def scale_grid(cfg, q_scales=(0.25, 1.0, 4.0), r_scales=(0.25, 1.0, 4.0)):
    """(K,9) candidates: cfg's position noise with Q and R scaled, C order over (q, r); and the index of the (1, 1) point"""
    c = default_candidate(cfg)
    rows = []
    for qs in q_scales:
        for rs in r_scales:
            k = c.copy(); k[3:6] *= qs; k[6:9] *= rs
            rows.append(k)
    return np.array(rows), list(q_scales).index(1.0) * len(r_scales) + list(r_scales).index(1.0)


def pooled_rows(track_stats, min_updates=1):
    """sum of the per-track rows (list of (K,12)) with enough updates, in ascending order"""
    tot = np.zeros_like(track_stats[0])
    for s in track_stats:
        if s[0, 0] >= min_updates:
            tot = tot + s
    return tot


# ------------------------------------------------------------------------------------------------ the fixture
def fixture_cases(golden):
    """the cases of tests/golden/noise_sweep_tracks.npz in file order:
    [dict(name, ts, pos, quat, aligned, valid, init_pos, init_quat, cfg, rows = slice into the flat per-pose arrays)], the candidates, the file"""
    import json
    g, kat = golden("noise_sweep_tracks.npz"), golden("kat_bundled.npz")
    cfgs = [json.loads(str(s)) for s in g["cfgs"]]
    off, ho = g["offsets"], g["hand_offsets"]
    tags = [str(t) for t in g["bundled_tags"]]
    cases = []
    for t, name in enumerate(g["names"]):
        if t < len(tags):
            c1 = golden(f"c1_{tags[t]}.npz")
            tr = dict(ts=kat["ts"], pos=kat["pos"], quat=kat["quat"], aligned=c1["ekf_aligned"], valid=c1["ekf_valid"],
                      init_pos=c1["sim3_pos"][0], init_quat=c1["sim3_quat"][0])
        else:
            sl = slice(ho[t - len(tags)], ho[t - len(tags) + 1])
            tr = dict(ts=g["hand_ts"][sl], pos=g["hand_pos"][sl], quat=g["hand_quat"][sl], aligned=g["hand_aligned"][sl], valid=g["hand_valid"][sl])
            tr.update(init_pos=tr["pos"][0], init_quat=tr["quat"][0])
        tr.update(name=str(name), cfg=cfgs[int(g["cfg_index"][t])], rows=slice(off[t], off[t + 1]))
        assert len(tr["ts"]) == off[t + 1] - off[t], name
        cases.append(tr)
    return cases, g["cand"], g
