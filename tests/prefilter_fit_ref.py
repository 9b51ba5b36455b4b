"""The yardstick of the GPS pre-filter's least-squares polynomial fit (one RANSAC trial of filter_gps_outliers_ransac, EKFGPSSLAM.py:136-247:
LinearRegression on PolynomialFeatures(d)(t) of min_samples rows) and the problems both tiers run.  Never imports the product and holds no
test functions.

Models.  exact_fit(): in 50 digits (mpmath), from the stored float64 rows, the least-squares polynomial of a sample in WINDOW-LOCAL time
tau = t - t0 (t0: the problem's first stamp; the subtraction is exact for every problem of cases(), which cases() asserts, so this is the
least-squares polynomial of the stored rows whatever the clock's zero) -- by the normal equations, or by Householder QR (route="qr": the
second route the CPU tier checks the first against); its prediction at any stamp; the weights w_i(t) of that prediction on the sample's
targets, Lambda(t) = sum |w_i(t)|; and kappa, the 2-norm condition of the sample's centred power columns in local time, each scaled to
unit norm.

Bound.  Every prediction has its own:  b(t) = u kappa Lambda(t) max|y_i - ybar| + 4 u max|y|,  u = 2^-53.  A gate is C_GATE x b(t), with
C_GATE = 8 x the worst ratio to b(t) of a float64 reference -- numpy.linalg.lstsq on the centred window-local columns with the rcond the
oracle's restatement uses -- over all probe rows of cases() (the Sim3 recipe; measured by tests/test_prefilter_fit_host.py, which also
asserts that the constant recorded below still is that).

Classes.  A sample is determined when its distinct stamps number at least degree + 1, otherwise rank-open; the rank rule of the product
(gsf_poly_core.hpp) gives a rank-open sample with m distinct stamps the least-squares polynomial of degree m - 1 (coefficient 0 for the
dependent columns), which is what exact_fit() returns for it.  Only the cases named in OPEN_CASES are open, and no determined case of the
fast kernels has C_GATE b(t) above 1e-6 of its threshold: cases() asserts both.

RANSAC replay.  replay_fed() walks RANSACRegressor.fit's loop over fed sample sets on exact models; replay_log() does the whole filter of a
log -- the reference's window walk, per window and axis the draws by scikit-learn's own sampler on NumPy's legacy global generator, as the
oracle draws them.  Residuals are the exact model's (50-digit coefficients, evaluated in 64-bit-mantissa long double in local time: 1e-12 m)
and are reported for every row under every drawn trial; usable_seed() is False when a row lies within 1e-6 thr of the threshold under
any drawn trial or two trials of a walk tie in count with scores closer than 1e-9 -- the tiers take the first seeds that are usable and
assert that at most one in ten was thrown away."""
import functools

import numpy as np

DPS = 50
U = 2.0 ** -53
SEED = 20261020
OPEN_CASES = ("open-2of6", "open-3of6", "open-1of6")     # two / three distinct stamps among six rows; all six rows on one stamp
FIRST_STAMPS = (0.0, 130.0, 1e4, 1e6, 1.3e9, 1.7e9)
UNITS = (1.0, 1e3, 1e6)                                  # stamps in seconds, milliseconds, microseconds
WINDOWS = ((1.5, 50.0), (15.0, 10.0), (60.0, 5.0), (15.0, 1.0), (60.0, 1.0), (15.0, 20.0))   # (seconds, Hz): at most 300 rows
THR_NORTHING, THR_ALTITUDE = 10.0, 5.0

# ---- the gate: measured by tests/test_prefilter_fit_host.py::test_float64_reference_against_the_yardstick (the worst ratio of
# numpy.linalg.lstsq in local time to b(t) over the probe rows of cases(); the per-route figures are in DESIGN.md)
LSTSQ_WORST = 0.68                                       # measured 0.676 (fast-d1-s9-t0-u1000-w15x1); wide route 0.651
C_GATE = 8 * LSTSQ_WORST


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ------------------------------------------------------------------------------------------------ the exact fit
class Fit:
    """least-squares polynomial of one sample: coef[k] multiplies tau^k, k = 0 .. deg_eff (mp numbers), in tau = t - t0"""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def predict(self, t):
        mp = _mp()
        tau = mp.mpf(float(t)) - self.t0
        return mp.fsum(c * tau ** k for k, c in enumerate(self.coef))

    def weights(self, t):
        """w_i(t): prediction(t) = sum_i w_i(t) y_i over the sample's rows"""
        mp = _mp()
        tau = mp.mpf(float(t)) - self.t0
        phi = mp.matrix([tau ** k for k in range(self.deg_eff + 1)])
        return [mp.fsum(self.pinv[k, i] * phi[k] for k in range(self.deg_eff + 1)) for i in range(self.pinv.cols)]

    def lam(self, t):
        mp = _mp()
        return mp.fsum(abs(w) for w in self.weights(t))

    def bound(self, t):
        return float(U * self.kappa * self.lam(t) * self.yspread + 4 * U * self.ymax)

    def coef64(self):
        """float64 [intercept, c1 .. c_degree] (zeros for the dependent columns)"""
        out = np.zeros(self.degree + 1)
        out[:self.deg_eff + 1] = [float(c) for c in self.coef]
        return out


def _solve_normal(mp, A):
    """pinv(A) = (A^T A)^-1 A^T by the normal equations"""
    return mp.inverse(A.T * A) * A.T


def _solve_qr(mp, A):
    """pinv(A) = R^-1 Q^T by Householder QR"""
    Q, R = mp.qr(A)
    n = A.cols
    return mp.inverse(R[:n, :n]) * Q[:, :n].T


def exact_fit(t, y, idx, degree, t0, route="normal"):
    mp = _mp()
    ts = [mp.mpf(float(t[i])) - mp.mpf(float(t0)) for i in idx]
    ys = [mp.mpf(float(y[i])) for i in idx]
    distinct = len(set(float(t[i]) for i in idx))
    deg_eff = min(int(degree), distinct - 1)
    # (the columns are formed in sigma = tau / max|tau| -- an exact change of variable that keeps the Gram matrix of a degree-8 sample in
    # microsecond stamps inside 50 digits -- and the rows of the pseudo-inverse are scaled back to the powers of tau)
    scale = max([abs(tau) for tau in ts] + [mp.mpf(0)])
    scale = scale if scale > 0 else mp.mpf(1)
    A = mp.matrix(len(ts), deg_eff + 1)
    for i, tau in enumerate(ts):
        for k in range(deg_eff + 1):
            A[i, k] = (tau / scale) ** k
    pinv = (_solve_qr if route == "qr" else _solve_normal)(mp, A)
    for k in range(deg_eff + 1):
        for i in range(len(ts)):
            pinv[k, i] = pinv[k, i] / scale ** k
    coef = pinv * mp.matrix(ys)
    ybar = mp.fsum(ys) / len(ys)
    # kappa: centred power columns tau^1 .. tau^deg_eff, unit norm, 2-norm condition from the Gram matrix's eigenvalues
    kappa = mp.mpf(1)
    if deg_eff >= 1:
        cols = []
        for k in range(1, deg_eff + 1):
            col = [tau ** k for tau in ts]
            m = mp.fsum(col) / len(col)
            col = [c - m for c in col]
            nrm = mp.sqrt(mp.fsum(c * c for c in col))
            cols.append([c / nrm for c in col])
        G = mp.matrix(deg_eff, deg_eff)
        for a in range(deg_eff):
            for b in range(deg_eff):
                G[a, b] = mp.fsum(p * q for p, q in zip(cols[a], cols[b]))
        ev = mp.eigsy(G, eigvals_only=True)
        ev = [ev[i] for i in range(deg_eff)]
        kappa = mp.sqrt(max(ev) / min(ev))
    return Fit(coef=[coef[k] for k in range(deg_eff + 1)], pinv=pinv, t0=mp.mpf(float(t0)), degree=int(degree), deg_eff=deg_eff, distinct=distinct,
               determined=distinct >= degree + 1, kappa=kappa, yspread=max(abs(v - ybar) for v in ys), ymax=max(abs(v) for v in ys))


def lstsq_fit64(t, y, idx, degree, t0):
    """the float64 reference C_GATE is measured on: LinearRegression as the oracle restates it, on window-local columns.  Returns a
    function tq -> predictions."""
    tau = np.asarray(t, dtype=np.float64) - float(t0)
    X = np.vander(tau[idx], degree + 1, increasing=True)
    ys = np.asarray(y, dtype=np.float64)[idx]
    xo, yo = X.mean(axis=0), ys.mean()
    Xc = X - xo
    # columns scaled to unit norm, as kappa is defined: with stamps in milliseconds or microseconds the raw columns tau, tau^2, tau^3 differ
    # by 1e7 and more per degree, and lstsq's rcond would then cut real singular values off -- a truncation, not the rounding C is about
    nrm = np.sqrt((Xc * Xc).sum(axis=0))
    nrm[nrm == 0.0] = 1.0
    coef = np.linalg.lstsq(Xc / nrm, ys - yo, rcond=max(X.shape) * np.finfo(float).eps)[0] / nrm
    return lambda tq: np.vander(np.asarray(tq, dtype=np.float64) - float(t0), degree + 1, increasing=True) @ coef + (yo - xo @ coef)


# ------------------------------------------------------------------------------------------------ the problems
def _log(rng, first, unit, width, hz, base, n_cap=300):
    """one window of a GNSS log: stamps (first + k / hz + jitter) x unit, stored in float64; a 5.4e6 m / 110 m target with 3 m/s, 0.2 m/s^2
    of curvature and 0.4 m of noise"""
    n = int(min(n_cap, round(width * hz)))
    sec = np.arange(n) / hz + np.concatenate(([0.0], rng.uniform(0.0, 0.3 / hz, n - 1)))
    sec *= width / max(sec[-1] + 1.0 / hz, width)                                 # inside [0, width)
    t = (first + sec) * unit                                                       # the stored stamps
    tau = (t - t[0]) / unit
    y = base + 3.0 * tau + 0.1 * tau * tau + rng.normal(0.0, 0.4, n)
    return t, y


@functools.lru_cache(maxsize=None)
def cases():
    """[dict(name, route 'fast' | 'wide', klass 'determined' | name of OPEN_CASES, t, y, idx, degree, ms, thr, probes (row numbers), fit (Fit))]"""
    rng = np.random.default_rng(SEED)
    out = []

    def add(name, route, t, y, idx, degree, thr, klass="determined"):
        n = len(t)
        probes = sorted(set(np.linspace(0, n - 1, min(n, 7)).round().astype(int).tolist()) | set(int(i) for i in idx[:3]))
        out.append(dict(name=name, route=route, klass=klass, t=t, y=y, idx=np.asarray(idx, dtype=np.int32), degree=int(degree), ms=len(idx),
                        thr=float(thr), probes=probes))

    k = 0
    for route, degrees, sizes in (("fast", (1, 2, 3), (4, 6, 8, 9, 12, 16)), ("wide", (4, 5, 8), (10, 17, 24, 40, 64))):
        for degree in degrees:
            for ms in sizes:
                if ms < degree + 2:
                    continue
                for fi, first in enumerate(FIRST_STAMPS):
                    k += 1
                    unit = UNITS[(k + fi) % 3]
                    width, hz = WINDOWS[(k // 2 + fi) % len(WINDOWS)]
                    while width * hz < ms + 4:                                     # a window that holds the sample
                        width, hz = WINDOWS[(WINDOWS.index((width, hz)) + 1) % len(WINDOWS)]
                    alt = (k // 3) % 2 == 1
                    bunched = k % 4 == 0
                    t, y = _log(rng, first, unit, width, hz, 110.0 if alt else 5.4e6)
                    n = len(t)
                    if bunched:                                                    # the sample from one end of the window: Lambda grows
                        span = max(ms + 2, n // 3)
                        pool = np.arange(n - span, n) if k % 8 == 0 else np.arange(span)
                    else:
                        pool = np.arange(n)
                    idx = rng.choice(pool, ms, replace=False)
                    add(f"{route}-d{degree}-s{ms}-t{first:g}-u{unit:g}-w{width:g}x{hz:g}{'-alt' if alt else ''}{'-bunched' if bunched else ''}",
                        route, t, y, idx, degree, THR_ALTITUDE if alt else THR_NORTHING)
    # every unit at every first stamp, at the CONFIG's degree 2 / 6 samples / 15 s
    for first in FIRST_STAMPS:
        for unit in UNITS:
            t, y = _log(rng, first, unit, 15.0, 10.0, 5.4e6)
            add(f"fast-d2-s6-t{first:g}-u{unit:g}-w15x10-grid", "fast", t, y, rng.choice(len(t), 6, replace=False), 2, THR_NORTHING)
    # rank-open samples: a receiver that repeats stamps.  Six rows on two / three / one distinct stamps; two stamps 1e-3 of the window
    # apart are NOT open.
    for first in (0.0, 130.0, 1.3e9):
        for degree in (2, 3):
            t, y = _log(rng, first, 1.0, 15.0, 10.0, 5.4e6)
            t2 = t.copy(); t2[40:43] = t2[40]; t2[90:93] = t2[90]
            add(f"open-2of6-d{degree}-t{first:g}", "fast", t2, y, [40, 41, 42, 90, 91, 92], degree, THR_NORTHING, "open-2of6")
            t1 = t.copy(); t1[60:66] = t1[60]
            add(f"open-1of6-d{degree}-t{first:g}", "fast", t1, y, [60, 61, 62, 63, 64, 65], degree, THR_NORTHING, "open-1of6")
        t, y = _log(rng, first, 1.0, 15.0, 10.0, 5.4e6)
        t3 = t.copy(); t3[20:22] = t3[20]; t3[70:72] = t3[70]; t3[120:122] = t3[120]
        add(f"open-3of6-d3-t{first:g}", "fast", t3, y, [20, 21, 70, 71, 120, 121], 3, THR_NORTHING, "open-3of6")
        tn = t.copy(); tn[80:83] = tn[80]; tn[83:86] = tn[80] + 15.0e-3            # two stamps 1e-3 of the window apart: determined at degree 1
        add(f"near-2of6-d1-t{first:g}", "fast", tn, y, [80, 81, 82, 83, 84, 85], 1, THR_NORTHING)
    # the CPU-side conditions
    mp = _mp()
    for c in out:
        t0 = c["t"][0]
        for ti in c["t"]:
            assert mp.mpf(float(ti - t0)) == mp.mpf(float(ti)) - mp.mpf(float(t0)), (c["name"], "window-local time is not exact")
        c["fit"] = f = exact_fit(c["t"], c["y"], c["idx"], c["degree"], t0)
        assert f.determined == (c["klass"] == "determined"), (c["name"], f.distinct, "only the named cases are open")
        assert c["klass"] == "determined" or c["klass"] in OPEN_CASES
        c["exact"] = {i: f.predict(c["t"][i]) for i in c["probes"]}
        c["bound"] = {i: f.bound(c["t"][i]) for i in c["probes"]}
        if c["route"] == "fast" and f.determined:
            worst = max(c["bound"].values())
            assert C_GATE * worst <= 1e-6 * c["thr"], (c["name"], C_GATE * worst, "the gate is not far inside the threshold")
    assert len(out) <= 400 and max(len(c["t"]) for c in out) <= 300
    return out


# ------------------------------------------------------------------------------------------------ RANSAC on exact models
def _dynamic_max_trials(n_inliers, n, ms, p):
    eps = np.spacing(1)
    ratio = n_inliers / float(n)
    nom, denom = max(eps, 1 - p), max(eps, 1 - ratio ** ms)
    return 0 if nom == 1 else (np.inf if denom == 1 else abs(float(np.ceil(np.log(nom) / np.log(denom)))))


def exact_residuals(t, y, idx, degree, t0):
    """|y - exact prediction| at every row, long double (the 50-digit coefficients rounded to 64 bits of mantissa, Horner in local time)"""
    f = exact_fit(t, y, idx, degree, t0)
    mp = _mp()
    coef = [np.longdouble(mp.nstr(c, 30)) for c in f.coef]
    tau = np.asarray(t, dtype=np.longdouble) - np.longdouble(float(t0))
    acc = np.zeros(len(tau), dtype=np.longdouble)
    for c in reversed(coef):
        acc = acc * tau + c
    return np.abs(np.asarray(y, dtype=np.longdouble) - acc), acc


def replay_fed(t, y, samples, degree, thr, stop_probability=0.99, draw=None):
    """RANSACRegressor.fit's loop on exact models.  samples[max_trials][ms] are fed; with draw (a callable returning the next sample set)
    they are drawn as the loop goes, max_trials = samples.  Returns dict(mask, n_trials, n_inliers, status, residuals [per drawn trial],
    margin (the smallest |residual - thr| / thr seen), tie (the smallest score gap between two trials of equal count that were compared),
    n_open (drawn samples with fewer distinct stamps than degree + 1), best_idx (the accepted sample set, None without one))."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(t)
    max_trials = samples if draw is not None else len(samples)
    best_mask, best_n, best_score, trials, max_tr = None, 1, -np.inf, 0, max_trials
    res_all, margin, tie, n_open, best_idx = [], np.inf, np.inf, 0, None
    while trials < max_tr:
        idx = draw() if draw is not None else samples[trials]
        trials += 1
        n_open += int(len(set(t[np.asarray(idx)].tolist())) < degree + 1)       # a rank-open sample: the rank rule decides its model
        res, pred = exact_residuals(t, y, idx, degree, t[0])
        res_all.append(res)
        margin = min(margin, float(np.abs(res - thr).min() / thr))
        mask = res <= thr
        cnt = int(mask.sum())
        if cnt < best_n:
            continue
        if cnt < 2:
            score = np.nan
        else:
            yi, pi = y[mask].astype(np.longdouble), pred[mask]
            num, den = ((yi - pi) ** 2).sum(), ((yi - yi.mean()) ** 2).sum()
            score = float(1.0 - num / den) if den != 0.0 else (1.0 if num == 0.0 else 0.0)
        if cnt == best_n and np.isfinite(best_score) and np.isfinite(score):
            tie = min(tie, abs(score - best_score))
        if cnt == best_n and score < best_score:
            continue
        best_mask, best_n, best_score, best_idx = mask, cnt, score, np.asarray(idx).copy()
        max_tr = min(max_tr, _dynamic_max_trials(best_n, n, len(idx), stop_probability))
    ok = best_mask is not None
    return dict(mask=(best_mask if ok else np.zeros(n, dtype=bool)), n_trials=trials, n_inliers=best_n if ok else 0, status=0 if ok else 1,
                residuals=res_all, margin=margin, tie=tie, n_open=n_open, best_idx=best_idx)


def windows(times, width, step_factor, need):
    """row ranges [r0, r1) of the windows the reference visits, in its order (ref :199-234), for sorted stamps; windows with fewer than
    `need` rows are left out, as the reference skips them"""
    times = np.asarray(times, dtype=np.float64)
    stride = width * step_factor
    out = []
    t_first, t_last = times[0], times[-1]
    w0 = t_first
    while w0 < t_last:
        w1 = w0 + width
        rows = np.where((times >= w0) & (times < w1))[0]
        if len(rows) >= need:
            out.append((int(rows[0]), int(rows[-1]) + 1))
        if stride <= 1e-6:
            later = np.where(times > w0)[0]
            if len(later) == 0:
                break
            w0 = times[later[0]]
        else:
            w0 += stride
        if w0 >= t_last and times[-1] >= w1:
            w0 = max(t_first, times[-1] - width + 1e-6)
    return out


def replay_log(times, pos, seed, degree, ms, thr, max_trials, width=None, step_factor=0.5, stop_probability=0.99):
    """the whole filter of one log on exact models: the reference's windows (width None: one global window), per window the axes in order,
    a failing axis drops its window and draws nothing further for it; draws by scikit-learn's sampler on NumPy's legacy global generator
    seeded with `seed`.  Returns dict(keep uint8[n], windows [(r0, r1)], win_status, state uint32[625] (the generator afterwards),
    n_trials [per window-axis problem run], margin, tie, n_open, fits [per problem run: window, axis, best_idx, mask, n_trials])."""
    from sklearn.utils.random import sample_without_replacement
    times, pos = np.asarray(times, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(times)
    wins = [(0, n)] if width is None else windows(times, width, step_factor, ms)
    np.random.seed(seed)
    rs = np.random.mtrand._rand
    keep = np.zeros(n, dtype=bool)
    status, ntr, margin, tie, n_open, fits = [], [], np.inf, np.inf, 0, []
    for r0, r1 in wins:
        wmask, st = np.ones(r1 - r0, dtype=bool), 0
        for ax in range(3):
            r = replay_fed(times[r0:r1], pos[r0:r1, ax], max_trials, degree, thr, stop_probability,
                           draw=lambda: sample_without_replacement(r1 - r0, ms, random_state=rs))
            ntr.append(r["n_trials"]); margin = min(margin, r["margin"]); tie = min(tie, r["tie"]); n_open += r["n_open"]
            fits.append(dict(window=(r0, r1), axis=ax, best_idx=r["best_idx"], mask=r["mask"], n_trials=r["n_trials"]))
            if r["status"]:
                st = 1
                break
            wmask &= r["mask"]
        status.append(st)
        if st == 0:
            keep[r0:r1] |= wmask
    _, key, p, _, _ = np.random.get_state()
    state = np.concatenate([key.astype(np.uint32), np.array([p], dtype=np.uint32)])
    return dict(keep=keep.astype(np.uint8), windows=wins, win_status=np.array(status, dtype=np.int32), state=state, n_trials=ntr, margin=margin, tie=tie, n_open=n_open, fits=fits)


def seed_state(seed):
    """uint32[625]: NumPy's legacy generator after seed(seed), the layout the device chain takes"""
    rs = np.random.RandomState(seed)
    _, key, p, _, _ = rs.get_state()
    return np.concatenate([key.astype(np.uint32), np.array([p], dtype=np.uint32)])


def usable(replay):
    return replay["margin"] > 1e-6 and replay["tie"] >= 1e-9


def usable_seeds(make_log, run, count, first_seed=0):
    """the first `count` seeds whose replay keeps clear of every decision (usable()); asserts that at most one seed in ten was thrown away.
    make_log(seed) -> log, run(log, seed) -> replay.  Returns [(seed, log, replay)]."""
    out, tried = [], 0
    seed = first_seed
    while len(out) < count:
        log = make_log(seed)
        r = run(log, seed)
        tried += 1
        if usable(r):
            out.append((seed, log, r))
        seed += 1
        assert tried - len(out) <= max(1, (tried + 9) // 10), ("more than one seed in ten thrown away", tried, len(out))
    return out


def dyadic_log(seed, n=150, width=15.0, spikes=0.08, repeat=0, thrice=False):
    """a log whose stamps lie on a 2^-20 s grid inside [0, width), so that adding 130, 2^20 or 1.3e9 s changes no window-local number
    (1.3e9 + width < 2^31: the grid is kept to 2^-21 s).  pos[n][3] at UTM magnitude with `spikes` outliers.  repeat: that many places where
    the receiver repeats a stamp three times running; thrice: it does so at every stamp."""
    rng = np.random.default_rng(1000 + seed)
    grid = 2.0 ** -20
    sec = np.sort(rng.choice(int(width / grid) - 1, n - 1, replace=False) + 1) * grid
    sec = np.concatenate(([0.0], sec))
    for k in range(repeat):
        j = int(rng.integers(2, n - 3))
        sec[j + 1] = sec[j + 2] = sec[j]
    if thrice:                                                                     # EVERY stamp three times running: n / 3 distinct stamps
        sec = np.repeat(sec[::3][:n // 3], 3)
        n = len(sec)
    sec = np.sort(sec)
    pos = np.column_stack((4.5e5 + 9.0 * sec, 5.4e6 - 4.0 * sec + 0.1 * sec * sec, 110.0 + 0.1 * sec)) + rng.normal(0.0, 0.4, (n, 3))
    bad = rng.random(n) < spikes
    pos[bad] += rng.choice([-1.0, 1.0], (int(bad.sum()), 3)) * rng.uniform(30.0, 200.0, (int(bad.sum()), 3))
    return sec, pos


SHIFTS = (0.0, 130.0, 2.0 ** 20, 1.3e9)
