"""Robust smoothing (gsf_ekf_smooth_reweighted_dev): the rule of include/gsf.h restated per pose on top of weighted_ref.weighted_restate.

reweight_restate() is the loop the kernel runs: solve 0 on the given variances, then up to `rounds` solves on min(v / w, 1e8), the
weights formed from every used fix's residual against the smoothed track relative to init_pos.  Every solve IS weighted_restate on the
effective variances, so law B holds here by construction and law A is one comparison (tests/test_reweight_host.py).  yardstick() runs the
same recurrences AND the weight rule in 50 digits (mpmath) across all solves and rounds once at the end; the decisions (availability,
spans, blend weights, the Huber branch, the cap at 1e8, the number of solves) and the displacements are the restatement's, as
weighted_ref.yardstick takes them.  objective() is the M-estimator's cost on a one-span track."""
import numpy as np

import weighted_ref as W
from weighted_ref import GNSS_USED

HUBER, CAUCHY = 0, 1                                                    # GSF_REWEIGHT_*
LOSSES = {"huber": HUBER, "cauchy": CAUCHY}
MAX_ROUNDS = 32
CAP = W.VAR_MAX


def weight_of(loss, u2, c2):
    """w (n,) of u2 (n,): the statements of gsf_reweight_core.hpp in their order"""
    u2 = np.asarray(u2, float)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if loss == CAUCHY:
            t = u2 / c2
            d = 1.0 + t
            return 1.0 / d
        t = c2 / u2
        w = np.sqrt(t)
        return np.where(u2 <= c2, 1.0, w)


def u2_of(res, var):
    """sum_c res_c^2 / v_c, three quotients summed left to right"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = res * res
        q = s / var
        return (q[:, 0] + q[:, 1]) + q[:, 2]


def effective_var(given, w):
    """min(v / w, 1e8) on the rows where w is a number, the given variance elsewhere"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = given / w[:, None]
        capped = np.where(q < CAP, q, CAP)
    return np.where(np.isnan(w)[:, None], given, capped)


def relative_correction(sol, aligned, ip, r_eff):
    """e (n,3) of a solve with the applied correction g formed relative to init_pos, as the kernel forms it: g = w k ((z - init_pos) - xp_rel).
    weighted_restate forms g from UTM positions (1e-9 m of rounding, which a weight of a good fix would inherit); its decisions, gains
    and variances are used as they are."""
    n = len(sol["avail"])
    Pf, Pp, xr = sol["Pf"][:, :3], sol["Pp"][:, :3], sol["xr"]
    g = np.zeros((n, 3))
    for i in range(1, n):
        if sol["avail"][i]:
            k = Pp[i] / (Pp[i] + r_eff[i])
            y = (np.asarray(aligned[i], float) - np.asarray(ip, float)) - (xr[i - 1] + sol["disp"][i])
            g[i] = sol["w"][i] * k * y
    e = np.zeros((n, 3))
    starts = list(sol["starts"])
    for a, end in zip(starts, starts[1:] + [n]):
        for k in range(end - 2, a - 1, -1):
            Ppn = Pp[k + 1]
            A = np.where(Ppn > 0, Pf[k] / np.where(Ppn > 0, Ppn, 1.0), 0.0)
            e[k] = A * (e[k + 1] + g[k + 1])
    e[~np.asarray(sol["reached"], bool)] = 0.0
    return e


def same_bits(a, b):
    return np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)


def reweight_restate(ts, pos, quat, aligned, valid, meas_var, ip, iq, cfg, loss, c2, rounds):
    """-> weighted_restate's dict of the LAST solve plus weight (n,) (NaN off the used rows), rounds_used, w_change, given (n,3), and
    history = [dict(sol, u2, w, w_used, r_eff)] per solve"""
    assert loss in (HUBER, CAUCHY) and 0 <= rounds <= MAX_ROUNDS and 0.0 < c2 < np.inf
    n = len(ts)
    given = np.tile(np.array(cfg["ekf"]["meas_noise_diag"], float), (n, 1)) if meas_var is None else np.asarray(meas_var, float)
    w_used = np.full(n, np.nan)                                         # solve 0: no weight yet, the given variances as they are
    history = []
    s = 0
    while True:
        r_eff = effective_var(given, w_used)
        sol = W.weighted_restate(ts, pos, quat, aligned, valid, r_eff, ip, iq, cfg)
        used = (sol["flags"] & GNSS_USED) != 0
        sol["e_rel"] = relative_correction(sol, aligned, ip, r_eff)
        res = (np.asarray(aligned, float) - np.asarray(ip, float)) - (sol["xr"] + sol["e_rel"])
        u2 = np.where(used, u2_of(np.where(used[:, None], res, 0.0), np.where(used[:, None], given, 1.0)), np.nan)
        w_new = np.where(used, weight_of(loss, np.where(used, u2, 0.0), c2), np.nan)
        before = np.where(used, 1.0 if s == 0 else w_used, np.nan)
        changed = bool((~same_bits(w_new, before) & used).any())
        w_change = float(np.max(np.abs(w_new[used] - before[used]), initial=0.0))
        history.append(dict(sol=sol, u2=u2, w=w_new, w_used=before, r_eff=r_eff))
        w_used = w_new
        if s >= rounds or not changed:
            break
        s += 1
    out = dict(sol)
    out.update(weight=w_new, rounds_used=s, w_change=w_change, given=given, history=history)
    return out


# ------------------------------------------------------------------------------------------------ the 50-digit yardstick
def yardstick(r, aligned, ip, cfg, loss, c2):
    """The solves of reweight_restate's result r in 50 digits: the filter and smoother recurrences of weighted_ref.yardstick with the
    effective variances carried in 50 digits from solve to solve, the residual, u2 and the weight in 50 digits; the restatement's
    decisions.  Rounded once, after the last solve -> float64 arrays Pf, Ps, xf, xs (n,3), nis (n,), weight (n,) (NaN off the used rows)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    F = mp.mpf
    hist = r["history"]
    w0 = hist[0]["sol"]
    n = len(w0["avail"])
    avail, starts, reached = w0["avail"], list(w0["starts"]), np.asarray(w0["reached"], bool)
    P0, Q = ([F(float(v)) for v in cfg["ekf"][k][:3]] for k in ("initial_cov_diag", "process_noise_diag"))
    given = [[F(float(v)) for v in row] for row in r["given"]]
    z = [[F(float(aligned[i][c])) - F(float(ip[c])) if avail[i] else None for c in range(3)] for i in range(n)]
    cap, c2m = F(CAP), F(float(c2))
    wts = [None] * n                                                    # the weights in 50 digits (None: solve 0 / not used)
    for s, h in enumerate(hist):
        assert (h["sol"]["avail"] == avail).all() and list(h["sol"]["starts"]) == starts      # the same decisions in every solve
        rr = [[None] * 3 for _ in range(n)]
        for i in range(n):
            if avail[i]:
                for c in range(3):
                    if wts[i] is None:
                        rr[i][c] = given[i][c]
                    else:                                               # the cap as the restatement decided it
                        rr[i][c] = cap if h["r_eff"][i][c] == CAP else given[i][c] / wts[i]
        Pf = [[None] * 3 for _ in range(n)]; Pp = [[None] * 3 for _ in range(n)]; x = [[None] * 3 for _ in range(n)]; g = [[F(0)] * 3 for _ in range(n)]
        nis = [None] * n
        for c in range(3):
            Pf[0][c], Pp[0][c], x[0][c] = P0[c], P0[c], F(0)
        for i in range(1, n):
            dt = F(float(w0["dt"][i]))
            tot = F(0)
            for c in range(3):
                Pp[i][c] = Pf[i - 1][c] + Q[c] * dt
                xp = x[i - 1][c] + F(float(w0["disp"][i, c]))
                Pf[i][c], x[i][c] = Pp[i][c], xp
                if avail[i]:
                    k = Pp[i][c] / (Pp[i][c] + rr[i][c])
                    y = z[i][c] - xp
                    g[i][c] = F(float(w0["w"][i])) * k * y
                    x[i][c] = xp + g[i][c]
                    Pf[i][c] = (1 - k) * Pp[i][c] * (1 - k) + k * rr[i][c] * k
                    tot += y * y / (Pp[i][c] + rr[i][c])
            nis[i] = tot if avail[i] else None
        e = [[F(0)] * 3 for _ in range(n)]; d = [[F(0)] * 3 for _ in range(n)]
        for a, end in zip(starts, starts[1:] + [n]):
            for k in range(end - 2, a - 1, -1):
                for c in range(3):
                    A = Pf[k][c] / Pp[k + 1][c] if Pp[k + 1][c] > 0 else F(0)
                    e[k][c] = A * (e[k + 1][c] + g[k + 1][c])
                    d[k][c] = A * A * (d[k + 1][c] + (Pf[k + 1][c] - Pp[k + 1][c]))
        for k in range(n):
            if not reached[k]:
                e[k], d[k] = [F(0)] * 3, [F(0)] * 3
        new = [None] * n
        for i in range(n):
            if avail[i]:
                u2 = sum(((z[i][c] - (x[i][c] + e[i][c])) ** 2) / given[i][c] for c in range(3))
                if loss == CAUCHY:
                    new[i] = 1 / (1 + u2 / c2m)
                else:                                                   # the branch as the restatement took it
                    new[i] = F(1) if h["u2"][i] <= c2 else mp.sqrt(c2m / u2)
        wts = new
    fl = lambda rows: np.array([[float(v) for v in row] for row in rows], float).reshape(n, 3)
    ipm = [F(float(v)) for v in ip]
    return dict(Pf=fl(Pf), Ps=fl([[Pf[k][c] + d[k][c] for c in range(3)] for k in range(n)]), xr=fl(x), e=fl(e),
                xf=fl([[ipm[c] + x[k][c] for c in range(3)] for k in range(n)]),
                xs=fl([[ipm[c] + x[k][c] + e[k][c] for c in range(3)] for k in range(n)]),
                nis=np.array([np.nan if v is None else float(v) for v in nis], float),
                weight=np.array([np.nan if v is None else float(v) for v in wts], float))


def yard_errors(got, y):
    """largest deviation of a result (keys xf, xs, Pf, Ps, nis, weight) from the yardstick: positions (m); variances, nis, weights (relative)"""
    from test_smooth_host import var_err
    ep = max(np.abs(got["xf"] - y["xf"]).max(), np.abs(got["xs"] - y["xs"]).max())
    ev = max(var_err(got["Pf"][:, :3], y["Pf"]), var_err(got["Ps"][:, :3], y["Ps"]))
    out = [ep, ev]
    for key in ("nis", "weight"):
        used = ~np.isnan(y[key])
        assert (np.isnan(got[key]) == ~used).all(), key
        out.append(float(np.max(np.abs(got[key][used] - y[key][used]) / y[key][used], initial=0.0)))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the objective
def objective(sol, aligned, ip, given, cfg, c2):
    """The Huber M-estimator's cost of a solve's smoothed track on a ONE-SPAN track without a blended update:
    J = sum_used rho(u_i) + 1/2 sum (dxs - disp)^2 / (Q dt) + 1/2 xs_rel[0]^2 / P0, rho(u) = u^2 / 2 for u^2 <= c2, else c |u| - c2 / 2"""
    assert list(sol["starts"]) == [0] and (sol["w"] == 1.0).all()
    P0, Q = (np.array(cfg["ekf"][k], float)[:3] for k in ("initial_cov_diag", "process_noise_diag"))
    used = (sol["flags"] & GNSS_USED) != 0
    xs = sol["xr"] + sol["e_rel"]
    res = (np.asarray(aligned, float) - np.asarray(ip, float)) - xs
    u2 = u2_of(res[used], given[used])
    rho = np.where(u2 <= c2, 0.5 * u2, np.sqrt(c2 * u2) - 0.5 * c2)
    step = xs[1:] - xs[:-1] - sol["disp"][1:]
    proc = 0.5 * np.sum(step * step / (Q[None, :] * sol["dt"][1:, None]))
    prior = 0.5 * np.sum(xs[0] * xs[0] / P0)
    return float(rho.sum() + proc + prior)


# ------------------------------------------------------------------------------------------------ inputs shared by both tiers
def plant_outliers(aligned, seed, fraction=0.1, sigma=(25.0, 25.0, 10.0)):
    """a copy of aligned with a fraction of the fixes (never row 0) displaced by N(0, sigma) m -> (aligned, rows)"""
    rng = np.random.default_rng(1000 + seed)
    rows = rng.random(len(aligned)) < fraction
    rows[0] = False
    out = np.array(aligned, float)
    out[rows] += rng.normal(0.0, 1.0, (int(rows.sum()), 3)) * np.asarray(sigma)
    return out, rows


def motivation(seed, n):
    """weighted_ref.motivation_track(seed, n) with planted outliers -> (ts, pos, quat, aligned, valid, ip, iq, meas_var, truth, rows)"""
    ts, pos, quat, aligned, valid, ip, iq, mv, truth = W.motivation_track(seed, n)
    bad, rows = plant_outliers(aligned, seed)
    return ts, pos, quat, bad, valid, ip, iq, mv, truth, rows


def one_span(cfg):
    """a copy of cfg whose sharp-turn threshold no pair exceeds: one smoothing span, no blended update"""
    import copy
    c = copy.deepcopy(cfg)
    c["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"] = 1e12
    return c
