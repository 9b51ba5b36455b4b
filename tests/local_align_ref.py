"""Pose-by-pose, knot-by-knot NumPy restatement of the local Sim3 alignment (include/gsf.h, gsf_sim3_local_fit_dev /
gsf_sim3_local_apply_dev): the specification the kernels and gsf_local_core.hpp are tested against, and the cases both tiers run.  Never
imports the product and holds no test functions.

Rules (the header's [grid] ... [blend] paragraphs):
  grid        t0 = ts[0];  K = floor((ts[-1] - t0) / spacing) + 2;  tau_k = fma(k, spacing, t0)
  status      EMPTY (no pose), UNSORTED (a stamp below its predecessor, or NaN), TOO_MANY (K > Kmax): NaN rows, zero knots
  window      usable rows (valid != 0, finite fix) with -hw <= (ts - tau_k) <= hw -- the difference first, then the comparisons
  fit         mode 0: R_k = the global R, s_k = tr(R H) / sum |a|^2;  mode 1: the closed form of EKFGPSSLAM.py:436-451 (two-pass centring,
              LAPACK SVD, scale = (sigma1 + sigma2 + sigma3) / sum |a|^2), mode 0 where (sigma2 + d sigma3) <= rot_open sigma1
  validity    FEW (n < min_rows), VAR0 (sum |a|^2 / n < 1e-12), SCALE (s_k <= 1e-6 or s_k / s outside [1 / ratio_max, ratio_max])
  neighbours  k = min(floor((ts - t0) / spacing), K - 2); L = nearest valid knot <= k, Rr = nearest valid knot >= k + 1
  blend       pos' = T_L(p) + w (T_Rr(p) - T_L(p));  quat' = nlerp(R_L (x) q, R_Rr (x) q, w), the product itself where both are the same
              numbers;  scale_at = s_L + w (s_Rr - s_L)

blend_track() evaluates the blend in exactly the operations gsf_local_core.hpp spells out when no multiply-add is contracted (explicit
fma() calls are single roundings, everything else rounds operation by operation): tests/test_local_align_host.py compiles that header
with g++ -ffp-contract=off and asks for the same bits.  The device build contracts a * b + c inside an expression, so the GPU tier
compares with tolerances instead.

The mode-0 scale has no bound in tests/sim3_ref.py.  scale_yardstick() evaluates s = tr(R H) / sum |a_i|^2 on the centred rows in 50
digits and the bound  b0 = u sum |a_i| |b_i| / tr(R H) + u  (u = 2^-53; _shift: the rows minus the window's first usable row, which is
what the kernel's raw moments hold).  Measured by tests/test_local_align_host.py::test_restatement_knots_against_the_yardstick on this
restatement over every valid knot of host_cases() (2026-10-20, 74 mode-0 scales: worst ratio 1.95, len130_scale_jump knot 1, median 0.59): C_S0 = 8 x the figure below."""
import functools
import math
from fractions import Fraction

import numpy as np

import sim3_ref as SR

LOC_SCALE, LOC_SIM3, LOC_KMAX = 0, 1, 4096
LOC_EMPTY, LOC_UNSORTED, LOC_TOO_MANY, LOC_SKIPPED = 1, 2, 4, 8
KNOT_FEW, KNOT_VAR0, KNOT_SCALE, KNOT_ROT_FALLBACK = 1, 2, 4, 8
KNOT_INVALID = KNOT_FEW | KNOT_VAR0 | KNOT_SCALE
LP_BRIDGED, LP_HELD, LP_GLOBAL, LP_BAD_QUAT, LP_TRACK = 1, 2, 4, 8, 16

SPACING, HALF_WINDOW, MIN_ROWS, ROT_OPEN, RATIO_MAX = 4.0, 3.2, 8, 1e-3, 2.0      # the grid of both tiers' cases
U = 2.0 ** -53
MEASURED_WORST_S0 = 2.0
C_S0 = 8 * MEASURED_WORST_S0
NAN = float("nan")


# ---------------------------------------------------------------------------- arithmetic
def fma(a, b, c):
    """a * b + c with one rounding (IEEE fusedMultiplyAdd), by exact rational arithmetic"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:                                                        # the sign of an exact zero: the sum of two zeros, or a cancellation (+0)
        p = math.copysign(1.0, a) * math.copysign(1.0, b)
        if (a == 0.0 or b == 0.0) and c == 0.0:
            return -0.0 if (p < 0 and math.copysign(1.0, c) < 0) else 0.0
        return 0.0
    return float(exact)


def tau(t0, spacing, k):
    return fma(float(k), spacing, t0)


def knot_count(ts, spacing):
    q = math.floor((float(ts[-1]) - float(ts[0])) / spacing) if math.isfinite((float(ts[-1]) - float(ts[0])) / spacing) else None
    if q is None or q > LOC_KMAX - 1:
        return LOC_KMAX + 1
    return 2 if q < 0 else int(q) + 2


def track_status(ts, spacing, Kmax):
    ts = np.asarray(ts, np.float64)
    if len(ts) == 0:
        return LOC_EMPTY, 0
    if np.isnan(ts).any() or (np.diff(ts) < 0).any():
        return LOC_UNSORTED, 0
    K = knot_count(ts, spacing)
    return (LOC_TOO_MANY, 0) if K > Kmax else (0, K)


def cell(t, t0, spacing, K):
    q = (float(t) - float(t0)) / spacing
    top = K - 2 if K >= 2 else 0
    if not q >= 0.0:
        return 0
    q = math.floor(q)
    return top if q >= top else int(q)


def usable(gps, valid):
    return (np.asarray(valid) != 0) & np.isfinite(np.asarray(gps, np.float64)).all(axis=1)


def window(ts, t_k, hw):
    d = np.asarray(ts, np.float64) - t_k                                  # the one written order: the difference, then the comparisons
    return (d >= -hw) & (d <= hw)


# ---------------------------------------------------------------------------- one knot
def fit_knot(src, fix, mode, min_rows, rot_open, ratio_max, Rg, sg):
    """the knot of the usable rows src / fix (n,3) -> dict(flags, n, R (3,3), t, s, rms, gap = (sigma2 + d sigma3) / sigma1 or None)"""
    n = len(src)
    out = dict(flags=0, n=n, R=np.full((3, 3), NAN), t=np.full(3, NAN), s=NAN, rms=NAN, gap=None, var=None)
    if n < min_rows:
        out["flags"] = KNOT_FEW
        return out
    ma, mb = src.mean(0), fix.mean(0)
    a, b = src - ma, fix - mb
    ssq = float((a * a).sum())
    out["var"] = ssq / n
    if not ssq / n >= 1e-12:
        out["flags"] = KNOT_VAR0
        return out
    H = a.T @ b
    flags, R, tr = 0, None, None
    if mode == LOC_SIM3 and np.isfinite(H).all():
        Um, S, Vt = np.linalg.svd(H)
        R = Vt.T @ Um.T
        d = 1.0
        if np.linalg.det(R) < 0:
            Vt = Vt.copy(); Vt[2] *= -1.0; d = -1.0
            R = Vt.T @ Um.T
        out["gap"] = float((S[1] + d * S[2]) / S[0]) if S[0] > 0 else 0.0
        if (S[1] + d * S[2]) <= rot_open * S[0]:
            flags, R = KNOT_ROT_FALLBACK, None
        else:
            tr = float(S.sum())                                           # (:444 with det(R) = +1 after the flip)
    if R is None:
        R = np.asarray(Rg, np.float64).reshape(3, 3)
        tr = float(np.trace(R @ H))
    s = tr / ssq
    ratio = s / sg
    if not s > 1e-6 or not ratio >= 1.0 / ratio_max or not ratio <= ratio_max:
        out["flags"] = flags | KNOT_SCALE
        out["s_raw"] = s
        return out
    t = mb - s * (R @ ma)
    e = s * src @ R.T + t - fix
    out.update(flags=flags, R=R, t=t, s=s, rms=float(np.sqrt((e * e).sum() / n)))
    return out


def fit_track(ts, pos, gps, valid, Rg, sg, mode=LOC_SCALE, spacing=SPACING, hw=HALF_WINDOW, min_rows=MIN_ROWS, rot_open=ROT_OPEN,
              ratio_max=RATIO_MAX, Kmax=LOC_KMAX):
    """-> dict(status, K, knots = [fit_knot dict + rows (bool over the track)] of length K)"""
    st, K = track_status(ts, spacing, Kmax)
    knots = []
    if st == 0:
        ok = usable(gps, valid)
        for k in range(K):
            rows = ok & window(ts, tau(float(ts[0]), spacing, k), hw)
            kn = fit_knot(np.asarray(pos, np.float64)[rows], np.asarray(gps, np.float64)[rows], mode, min_rows, rot_open, ratio_max, Rg, sg)
            kn["rows"] = rows
            knots.append(kn)
    return dict(status=st, K=K, knots=knots)


def knot_arrays(fit, Kmax):
    """the Kmax slots of one track as the entry writes them: slots beyond K are NaN-filled with n = 0, flags = 0"""
    R, t, s = np.full((Kmax, 9), NAN), np.full((Kmax, 3), NAN), np.full(Kmax, NAN)
    n, rms, fl = np.zeros(Kmax, np.int32), np.full(Kmax, NAN), np.zeros(Kmax, np.int32)
    for k, kn in enumerate(fit["knots"]):
        R[k], t[k], s[k], n[k], rms[k], fl[k] = np.asarray(kn["R"]).reshape(9), kn["t"], kn["s"], kn["n"], kn["rms"], kn["flags"]
    return R, t, s, n, rms, fl


# ---------------------------------------------------------------------------- neighbours and blend
def index_track(flags, K):
    nl, nr, last = [-1] * K, [-1] * K, -1
    for k in range(K):
        if int(flags[k]) & KNOT_INVALID == 0:
            last = k
        nl[k] = last
    last = -1
    for k in range(K - 1, -1, -1):
        if int(flags[k]) & KNOT_INVALID == 0:
            last = k
        nr[k] = last
    return nl, nr


def _quat_unit(q):
    x, y, z, w = (float(v) for v in q)
    n2 = fma(w, w, fma(z, z, fma(y, y, x * x)))
    ok = (n2 >= 1e-280) and (n2 <= 1e280)
    r = 1.0 / math.sqrt(n2 if ok else 1.0)
    return (x * r, y * r, z * r, w * r), ok


def _quat_mul(p, q):
    px, py, pz, pw = p
    qx, qy, qz, qw = q
    return (fma(pw, qx, fma(qw, px, fma(py, qz, -(pz * qy)))), fma(pw, qy, fma(qw, py, fma(pz, qx, -(px * qz)))),
            fma(pw, qz, fma(qw, pz, fma(px, qy, -(py * qx)))), fma(pw, qw, -fma(pz, qz, fma(py, qy, px * qx))))


def _quat_from_matrix(M):
    M = [float(v) for v in M]
    tr = M[0] + M[4] + M[8]
    c, best = 0, M[0]
    if M[4] > best:
        best, c = M[4], 1
    if M[8] > best:
        best, c = M[8], 2
    if tr > best:
        c = 3
    q = [0.0] * 4
    if c == 0:
        q[0] = 1.0 - tr + 2.0 * M[0]; q[1] = M[3] + M[1]; q[2] = M[6] + M[2]; q[3] = M[7] - M[5]
    elif c == 1:
        q[1] = 1.0 - tr + 2.0 * M[4]; q[2] = M[7] + M[5]; q[0] = M[1] + M[3]; q[3] = M[2] - M[6]
    elif c == 2:
        q[2] = 1.0 - tr + 2.0 * M[8]; q[0] = M[2] + M[6]; q[1] = M[5] + M[7]; q[3] = M[3] - M[1]
    else:
        q[0] = M[7] - M[5]; q[1] = M[2] - M[6]; q[2] = M[3] - M[1]; q[3] = 1.0 + tr
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    r = 1.0 / math.sqrt(n2) if n2 == n2 and n2 > 0 else NAN
    return (q[0] * r, q[1] * r, q[2] * r, q[3] * r)


def _nlerp(q1, q2, weight):
    dot = fma(q1[3], q2[3], fma(q1[2], q2[2], fma(q1[1], q2[1], q1[0] * q2[0])))
    if dot < 0.0:
        q2 = tuple(-v for v in q2)
    w = min(max(weight if weight == weight else 0.0, 0.0), 1.0)            # fmin(fmax(w, 0), 1); fmax(NaN, 0) = 0
    qi = tuple((1.0 - w) * a + w * b for a, b in zip(q1, q2))
    n = math.sqrt(qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3]) if all(v == v for v in qi) else NAN
    if n < 1e-9:
        return q1 if weight < 0.5 else q2
    r = 1.0 / n
    return tuple(v * r for v in qi)


def _map(R, t, s, p):
    x, y, z = p
    return tuple(s * (x * R[3 * r] + y * R[3 * r + 1] + z * R[3 * r + 2]) + t[r] for r in range(3))


def blend_track(ts, pos, quat, Rg, tg, sg, kR, kt, ks, kflags, K, status, spacing=SPACING):
    """the apply entry on one track with the knots kR (.,9), kt (.,3), ks, kflags -> dict(pos, quat, scale, flags, cell, L, Rr, w)"""
    n = len(ts)
    out = dict(pos=np.full((n, 3), NAN), quat=np.full((n, 4), NAN), scale=np.full(n, NAN), flags=np.zeros(n, np.int32),
               cell=np.full(n, -1, np.int32), L=np.full(n, -1, np.int32), Rr=np.full(n, -1, np.int32), w=np.zeros(n))
    if status != 0:
        out["flags"][:] = LP_TRACK
        return out
    K = min(max(int(K), 0), len(ks))
    nl, nr = index_track(kflags, K)
    g = ([float(v) for v in np.asarray(Rg).reshape(9)], [float(v) for v in tg], float(sg))
    knot = lambda k: ([float(v) for v in kR[k]], [float(v) for v in kt[k]], float(ks[k]))
    t0 = float(ts[0])
    for i in range(n):
        t = float(ts[i])
        k = cell(t, t0, spacing, K)
        L = nl[k] if 0 <= k < K else -1
        Rr = nr[k + 1] if 0 <= k + 1 < K else -1
        p = tuple(float(v) for v in pos[i])
        qn, ok = _quat_unit(quat[i])
        w = 0.0
        if L >= 0 and Rr >= 0:
            tl, tr = tau(t0, spacing, L), tau(t0, spacing, Rr)
            w = (t - tl) / (tr - tl)
            A, B = knot(L), knot(Rr)
            a, b = _map(*A, p), _map(*B, p)
            po = tuple(x + w * (y - x) for x, y in zip(a, b))
            qa, qb = _quat_mul(_quat_from_matrix(A[0]), qn), _quat_mul(_quat_from_matrix(B[0]), qn)
            qo = qa if qa == qb else _nlerp(qa, qb, w)
            sc = A[2] + w * (B[2] - A[2])
            fl = LP_BRIDGED if Rr - L > 1 else 0
        else:
            A = knot(L) if L >= 0 else (knot(Rr) if Rr >= 0 else g)
            po, qo, sc = _map(*A, p), _quat_mul(_quat_from_matrix(A[0]), qn), A[2]
            fl = LP_HELD if (L >= 0 or Rr >= 0) else LP_GLOBAL
        if not ok:
            qo, fl = (NAN,) * 4, fl | LP_BAD_QUAT
        out["pos"][i], out["quat"][i], out["scale"][i], out["flags"][i] = po, qo, sc, fl
        out["cell"][i], out["L"][i], out["Rr"][i], out["w"][i] = k, L, Rr, w
    return out


def align_track(tr, mode=LOC_SCALE, Kmax=LOC_KMAX, **kw):
    """fit then apply on one track dict (see make_track) -> (fit, blend)"""
    f = fit_track(tr["ts"], tr["pos"], tr["gps"], tr["valid"], tr["R"], tr["s"], mode=mode, Kmax=Kmax, **kw)
    kmax = max(f["K"], 1)
    R, t, s, _, _, fl = knot_arrays(f, kmax)
    return f, blend_track(tr["ts"], tr["pos"], tr["quat"], tr["R"], tr["t"], tr["s"], R, t, s, fl, f["K"], f["status"], kw.get("spacing", SPACING))


# ---------------------------------------------------------------------------- the mode-0 yardstick
def scale_yardstick(src, fix, Rg):
    """-> SR.Fit with s, t (the mode-0 knot of the rows in 50 digits, rounded once), the relative bounds b0 / b0_shift of the scale (see the
    module text) and bimg / bimg_shift = b0 s max|a_i| + 4 u max|fix_i|, the error of an image s R src_i + t (tests/sim3_ref.py's form
    without the rotation's term: R is given)"""
    import mpmath as mp
    n = len(src)
    with mp.workdps(SR.DPS):
        S = [[mp.mpf(float(v)) for v in r] for r in src]
        D = [[mp.mpf(float(v)) for v in r] for r in fix]
        R = [[mp.mpf(float(v)) for v in r] for r in np.asarray(Rg, np.float64).reshape(3, 3)]
        sc = [mp.fsum(r[k] for r in S) / n for k in range(3)]
        dc = [mp.fsum(r[k] for r in D) / n for k in range(3)]
        A = [[r[k] - sc[k] for k in range(3)] for r in S]
        Bc = [[r[k] - dc[k] for k in range(3)] for r in D]
        trRH = mp.fsum(R[r][c] * mp.fsum(x[c] * y[r] for x, y in zip(A, Bc)) for r in range(3) for c in range(3))
        ssq = mp.fsum(x[0] ** 2 + x[1] ** 2 + x[2] ** 2 for x in A)
        norm = lambda v: mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
        Asum = mp.fsum(norm(x) * norm(y) for x, y in zip(A, Bc))
        shifted = [[x[k] - S[0][k] for k in range(3)] for x in S]
        Ashift = mp.fsum(norm(x) * norm([y[k] - D[0][k] for k in range(3)]) for x, y in zip(shifted, D))
        u = mp.mpf(2) ** -53
        s = trRH / ssq
        t = [dc[r] - s * mp.fsum(R[r][c] * sc[c] for c in range(3)) for r in range(3)]
        b0, b0s = u * Asum / trRH + u, u * Ashift / trRH + u
        dmax = max(max(abs(v) for v in row) for row in D)
        return SR.Fit(s=float(s), t=np.array([float(v) for v in t]), b0=float(b0), b0_shift=float(b0s),
                      bimg=float(b0 * s * max(norm(x) for x in A) + 4 * u * dmax), bimg_shift=float(b0s * s * max(norm(x) for x in shifted) + 4 * u * dmax))


@functools.lru_cache(maxsize=None)
def knot_yardstick(name, mode, k, Kmax=8):
    """the 50-digit yardstick of knot k of the named track under reference(mode, Kmax), computed once: ("sim3", SR.yardstick(...)) for a knot
    with a rotation of its own, ("scale", scale_yardstick(...)) for a mode-0 knot or a rotation-open fall-back"""
    tr = track(name)
    kn = reference(mode, Kmax)[[t["name"] for t in gpu_tracks()].index(name)][0]["knots"][k]
    src, fix = tr["pos"][kn["rows"]], tr["gps"][kn["rows"]]
    if mode == LOC_SIM3 and not kn["flags"] & KNOT_ROT_FALLBACK:
        return "sim3", SR.yardstick(src, fix)
    return "scale", scale_yardstick(src, fix, tr["R"])


# ---------------------------------------------------------------------------- tracks
def _rot(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def global_fit(pos, gps, ok):
    """a plain Umeyama fit on the usable rows (what the chain hands in as the track's global transform); identity-like where there are < 3"""
    if ok.sum() < 3:
        return None
    a, b = pos[ok], gps[ok]
    ma, mb = a.mean(0), b.mean(0)
    H = (a - ma).T @ (b - mb)
    Um, S, Vt = np.linalg.svd(H)
    R = Vt.T @ Um.T
    if np.linalg.det(R) < 0:
        Vt[2] *= -1.0
        R = Vt.T @ Um.T
    s = float(S.sum() / ((a - ma) ** 2).sum())
    return R, mb - s * R @ ma, s


def make_track(name, n, rng, shape="curved", off=SR.OFFSET_N, t_start=0.0, drift=0.0, noise=0.05, s0=1.7):
    """n poses at 10 Hz.  The SLAM track integrates the true steps divided by the local scale s0 (1 - drift i / (n - 1)); the fixes are the
    rotated true path at `off` plus noise.  shape: curved (heading turns at ~0.3 rad/s, a gentle hill) / straight (exactly collinear)."""
    i = np.arange(n, dtype=np.float64)
    ts = t_start + 0.1 * i
    if shape == "straight":
        u = np.array([0.6, 0.8, 0.0])
        true = (1.05 * i)[:, None] * u                                    # ~10.5 m/s along one line
        slam = (1.05 * i / s0)[:, None] * u + np.array([3.0, -2.0, 0.5])
        head = np.full(n, math.atan2(0.8, 0.6))
    else:
        head = 0.3 + 0.03 * i + 0.2 * np.sin(i / 37.0)
        step = np.c_[np.cos(head), np.sin(head), 0.02 * np.cos(i / 50.0)] * 1.0
        local = s0 * (1.0 - drift * i / max(n - 1, 1))
        true = np.cumsum(step, axis=0)
        slam = np.cumsum(step / local[:, None], axis=0)
    Rt = _rot(rng)
    gps = true @ Rt.T + off + rng.normal(size=(n, 3)) * noise
    quat = np.c_[np.zeros(n), np.zeros(n), np.sin(head / 2), np.cos(head / 2)] * 1.25      # (not unit: the entry normalises)
    valid = np.ones(n, np.uint8)
    return dict(name=name, ts=ts, pos=np.ascontiguousarray(slam), quat=quat, gps=gps, valid=valid)


def finish(tr, rng):
    ok = usable(tr["gps"], tr["valid"]) if len(tr["ts"]) else np.zeros(0, bool)
    g = global_fit(tr["pos"], tr["gps"], ok) if len(tr["ts"]) else None
    if g is None:                                                         # nothing to fit: any proper transform
        g = (_rot(rng), np.array([10.0, -20.0, 5.0]), 1.3)
    tr["R"], tr["t"], tr["s"] = np.ascontiguousarray(g[0]), np.ascontiguousarray(g[1]), float(g[2])
    return tr


HW_EXACT = float(HALF_WINDOW)


@functools.lru_cache(maxsize=None)
def gpu_tracks():
    """the ragged batch of the GPU tier (lengths 0, 1, 2, 3, 63, 64, 65, 130, 271 at 10 Hz), in a fixed order"""
    rng = np.random.default_rng(20261020)
    T = []
    add = lambda tr: T.append(finish(tr, rng))
    add(make_track("len0", 0, rng))
    add(make_track("len1", 1, rng))
    add(make_track("len2", 2, rng))
    add(make_track("len3", 3, rng))
    add(make_track("len63", 63, rng))
    # a row exactly on tau_1 - hw and one exactly on tau_1 + hw (t0 = 0, tau_1 = 4): 4 -+ float(3.2) are exact in binary, so are the
    # differences ts - tau_1 = -+ float(3.2), and the inclusive comparison is decidable; the rows next to them lie one ulp of hw outside
    tr = make_track("len130_on_the_bound", 130, rng)
    lo, hi = 4.0 - HW_EXACT, 4.0 + HW_EXACT
    assert Fraction(lo) == Fraction(4) - Fraction(HW_EXACT) and Fraction(hi) == Fraction(4) + Fraction(HW_EXACT)
    below = 4.0 - float(np.nextafter(HW_EXACT, 10.0))                      # (the next stamp below `lo` still rounds onto the bound: one ulp of hw)
    assert Fraction(below) == Fraction(4) - Fraction(float(np.nextafter(HW_EXACT, 10.0)))
    tr["ts"][7], tr["ts"][8], tr["ts"][72], tr["ts"][73] = below, lo, hi, np.nextafter(hi, 10.0)
    assert (np.diff(tr["ts"]) > 0).all()
    add(tr)
    add(make_track("len64", 64, rng))
    tr = make_track("len65_no_usable_row", 65, rng)
    tr["valid"][::2] = 0; tr["gps"][1::2, 1] = np.nan
    add(tr)
    tr = make_track("len271_usable_rows_stop", 271, rng)                  # knots 3, 4, 5 lose their rows: BRIDGED between knots 2 and 6
    tr["valid"][(tr["ts"] > 9.05) & (tr["ts"] < 22.95)] = 0
    add(tr)
    tr = make_track("len271_last_third", 271, rng)                        # usable from 18 s on: HELD on the left of knot 4
    tr["gps"][tr["ts"] < 17.95] = np.nan
    add(tr)
    add(make_track("len271_straight", 271, rng, shape="straight"))
    add(make_track("len271_curved", 271, rng))
    tr = make_track("len130_zero_quat", 130, rng)
    tr["quat"][41] = 0.0
    add(tr)
    tr = make_track("len65_unsorted", 65, rng)
    tr["ts"][30], tr["ts"][31] = tr["ts"][31], tr["ts"][30]
    add(tr)
    add(make_track("len271_unix_south", 271, rng, off=SR.OFFSET_S, t_start=1.3e9))
    add(make_track("len271_drifting", 271, rng, drift=0.10))
    add(make_track("len130", 130, rng, noise=0.3))
    add(make_track("len65", 65, rng))
    tr = make_track("len130_standstill", 130, rng)                        # the SLAM track stands still over knot 2's whole window: VAR0
    rows = (tr["ts"] > 4.75) & (tr["ts"] < 11.25)
    tr["pos"][rows] = tr["pos"][np.flatnonzero(rows)[0]]
    add(tr)
    tr = make_track("len130_scale_jump", 130, rng)                        # ... or runs at a third of its scale there: SCALE (ratio 3 > ratio_max)
    anchor = tr["pos"][np.flatnonzero(rows)[0]].copy()
    tr["pos"][rows] = anchor + (tr["pos"][rows] - anchor) / 3.0
    add(tr)
    for tr in T:
        for k in ("ts", "pos", "quat", "gps", "valid", "R", "t"):
            tr[k].setflags(write=False)
    return tuple(T)


@functools.lru_cache(maxsize=None)
def motivation_track():
    """90 s of the drifting kind (901 poses, the scale falls by 10 % end to end): the outage of the CPU tier's motivation check"""
    rng = np.random.default_rng(20261021)
    return finish(make_track("len901_drifting", 901, rng, drift=0.10), rng)


def track(name):
    return next(t for t in gpu_tracks() if t["name"] == name)


def host_cases():
    """the shared small cases of the CPU tier: every track of the GPU batch, in both modes"""
    return [(tr, mode) for mode in (LOC_SCALE, LOC_SIM3) for tr in gpu_tracks()]


@functools.lru_cache(maxsize=None)
def reference(mode, Kmax):
    """[(fit, blend)] of gpu_tracks() under the cases' grid, computed once"""
    return tuple(align_track(tr, mode=mode, Kmax=Kmax) for tr in gpu_tracks())


def pack(tracks):
    """-> dict of the flat arrays of a ragged batch: ts, pos, quat, gps, valid, offsets, R (B,9), t (B,3), s (B,)"""
    n = [len(t["ts"]) for t in tracks]
    cat = lambda k, w: np.concatenate([np.asarray(t[k]).reshape(-1, w) if w else np.asarray(t[k]).reshape(-1) for t in tracks])
    return dict(ts=cat("ts", 0).astype(np.float64), pos=cat("pos", 3), quat=cat("quat", 4), gps=cat("gps", 3), valid=cat("valid", 0).astype(np.uint8),
                offsets=np.concatenate([[0], np.cumsum(n)]).astype(np.int64), R=np.stack([t["R"].reshape(9) for t in tracks]),
                t=np.stack([t["t"] for t in tracks]), s=np.array([t["s"] for t in tracks]))


def clear_of_switches(fit, mode, min_rows=MIN_ROWS, rot_open=ROT_OPEN, ratio_max=RATIO_MAX, s_global=None):
    """no knot of the fit sits within a factor 2 of a threshold that a rounding difference could flip: the rotation-open test, the
    variance floor, the scale bounds (row counts are integers: exact)"""
    for kn in fit["knots"]:
        if kn["flags"] & KNOT_FEW:
            continue
        if not (kn["var"] > 2e-12 or kn["var"] < 0.5e-12):
            return False
        if mode == LOC_SIM3 and kn["gap"] is not None and 0.5 * rot_open <= kn["gap"] <= 2.0 * rot_open:
            return False
        s = kn["s"] if kn["s"] == kn["s"] else kn.get("s_raw", NAN)
        if s == s and s_global:
            r = s / s_global
            if any(0.98 * b <= r <= 1.02 * b for b in (1.0 / ratio_max, ratio_max)) or 0.5e-6 <= s <= 2e-6:
                return False
    return True
