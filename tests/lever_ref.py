"""Row-by-row NumPy restatement of the antenna lever arm (include/gsf.h, gsf_lever_fit_dev / gsf_lever_apply_dev): the specification the
kernels and gsf_lever_core.hpp are tested against, the 50-digit yardstick of the same iteration, and the cases both tiers run.  Never
imports the product and holds no test functions.

Rules (the header's [rows] ... [flags] paragraphs):
  rows        usable: valid != 0, finite fix, finite position, |q| > 1e-9 (a NaN fails); n_bad_quat: rows whose only defect is the quaternion
  shift       f = the first usable row;  v_i = pos_i - pos_f,  u_i = R^T (gps_i - gps_f),  t = R (c - s pos_f) + gps_f
  iteration   x = (s, c, l, dtheta);  w_i = s v_i + c + M_i l,  r_i = u_i - w_i,  J_i = [ v_i | I | M_i | -[w_i]x ];
              N = sum J^T J + priors, g = sum J^T r + priors;  Cholesky of D N D, D = diag(N)^(-1/2);  R <- R exp([dtheta]x)
  flags       FEW, VAR0, SINGULAR, SCALE, TRACK keep the starting values; WEAK_X/Y/Z, NOT_CONVERGED inform

fit_track() runs the iteration in float64 (sums by NumPy), yardstick() the SAME iteration -- same rows, same rounds -- with every sum, the
solve and the rotation update in 50 digits.  apply_track() evaluates out = gps + sign R (M(q) l) in exactly the operations
gsf_lever_core.hpp spells out when no multiply-add is contracted: tests/test_lever_host.py compiles that header with g++
-ffp-contract=off and asks for the same bits.  The device build contracts a * b + c inside an expression, so the GPU tier compares the
apply with a tolerance and the fit with the bounds below.

Bounds.  Both runs follow the same trajectory of iterates; they differ by the rounding of the sums (u E per row, E = max |u_i| the track's
extent in metres) and of the solve, amplified by kappa = the condition number of the scaled normal matrix D N D of the last round, taken
from the yardstick.  With u = 2^-53:
  l   |l - l_y|_inf <= C u kappa E              R   |R - R_y|_max <= C u kappa
  s   |s - s_y|     <= C u kappa s_y            t   |t - t_y|_inf <= C u kappa (E + s |pos_f|) + 2 u |t_y|_inf
      (t is UTM-sized: 2 u |t| is one unit in its last place, what two correctly rounded values of nearly the same number may differ by)
  l_cov   |l_cov - l_cov_y|_max <= C u kappa |l_cov_y|_max      (a block of the inverse of N: its relative error is kappa x that of N)
MEASURED_WORST = the worst ratio of this restatement to those bounds with C = 1 over YARDSTICK_CASES, measured by
tests/test_lever_host.py::test_restatement_against_the_yardstick and rounded up (2026-10-20: l 0.0045 at len130_bad_quats, s 0.0093 at
len63, R 0.0139 at len271_L3, l_cov 2.01 at len72_bend; the u kappa bounds of l, s and R are pessimistic by two orders of magnitude
because the right-hand side g is small at the last rounds).  t never left the last place of its yardstick on these cases, which gives
no figure; it is made of c and the same solve as l and takes l's.  The gate is C = 8 x that figure, the factor tests/sim3_ref.py and
tests/local_align_ref.py use: the device's sums run in another order (64 partial sums per total, fused multiply-adds) and its Cholesky
divides where NumPy's may not, which moves a result by a few roundings of the same size but not by an order of magnitude."""
import functools
import math

import numpy as np

import local_align_ref as LR
import sim3_ref as SR

FEW, VAR0, SINGULAR, SCALE, WEAK_X, WEAK_Y, WEAK_Z, NOT_CONVERGED, TRACK = 1, 2, 4, 8, 16, 32, 64, 128, 256
KEPT = FEW | VAR0 | SINGULAR | SCALE | TRACK
WEAK = WEAK_X | WEAK_Y | WEAK_Z
LVP_BAD_QUAT = 1
U = 2.0 ** -53
NAN = float("nan")
DPS = 50

DEFAULTS = dict(sigma_fix=0.5, sigma_prior=(1.0, 1.0, 1.0), sigma_rot=0.05, ratio_max=2.0, pivot_min=1e-10, weak_ratio=0.5, conv_tol=1e-6,
                min_rows=8, iters=4, fit_scale=1, fit_rotation=1)

MEASURED_WORST = dict(l=0.005, s=0.01, R=0.015, t=0.005, cov=2.1)         # (see the module text; the test keeps these figures honest)
GATE_FACTOR = 8.0
GATE = {k: GATE_FACTOR * v for k, v in MEASURED_WORST.items()}


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    c["sigma_prior"] = tuple(float(v) for v in c["sigma_prior"])
    return c


# ---------------------------------------------------------------------------- rows
def quat_unit_rows(quat):
    """(qn (n,4), ok (n,)) as lev_quat_unit forms them on the host: n2 by a chain of fma, q * (1 / sqrt(n2))"""
    quat = np.asarray(quat, np.float64).reshape(-1, 4)
    n2 = np.array([LR.fma(q[3], q[3], LR.fma(q[2], q[2], LR.fma(q[1], q[1], q[0] * q[0]))) for q in quat.tolist()], np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (n2 > 1e-18) & (n2 <= 1e280)
    r = 1.0 / np.sqrt(np.where(ok, n2, 1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        return quat * r[:, None], ok


def quat_matrix_rows(qn):
    """quat_matrix of gsf_math.hpp, operation by operation -> (n,3,3)"""
    x, y, z, w = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    xy, xz, yz, xw, yw, zw = x * y, x * z, y * z, x * w, y * w, z * w
    M = np.empty((len(qn), 3, 3), qn.dtype)
    M[:, 0, 0] = xx - yy - zz + ww; M[:, 0, 1] = 2.0 * (xy - zw); M[:, 0, 2] = 2.0 * (xz + yw)
    M[:, 1, 0] = 2.0 * (xy + zw); M[:, 1, 1] = -xx + yy - zz + ww; M[:, 1, 2] = 2.0 * (yz - xw)
    M[:, 2, 0] = 2.0 * (xz - yw); M[:, 2, 1] = 2.0 * (yz + xw); M[:, 2, 2] = -xx - yy + zz + ww
    return M


def row_kinds(pos, quat, gps, valid):
    """0 usable, 1 only the quaternion is bad, 2 not a row of the fit"""
    n = len(np.asarray(valid).reshape(-1))
    if n == 0:
        return np.zeros(0, np.int32)
    _, q_ok = quat_unit_rows(quat)
    rest = (np.asarray(valid).reshape(-1) != 0) & np.isfinite(np.asarray(gps, np.float64).reshape(-1, 3)).all(1) & np.isfinite(np.asarray(pos, np.float64).reshape(-1, 3)).all(1)
    return np.where(rest, np.where(q_ok, 0, 1), 2).astype(np.int32)


# ---------------------------------------------------------------------------- the iteration, in float64 or in 50 digits
class _F64:
    zero, one = 0.0, 1.0
    dtype = np.float64
    conv = staticmethod(lambda a: np.asarray(a, np.float64))
    sqrt = staticmethod(math.sqrt)
    sin = staticmethod(math.sin)
    cos = staticmethod(math.cos)
    sqrt_rows = staticmethod(np.sqrt)
    num = staticmethod(float)


def _mp_backend():
    import mpmath as mp

    class _MP:
        zero, one = mp.mpf(0), mp.mpf(1)
        dtype = object
        conv = staticmethod(lambda a: np.frompyfunc(lambda v: mp.mpf(float(v)), 1, 1)(np.asarray(a, np.float64)).astype(object))
        sqrt, sin, cos = staticmethod(mp.sqrt), staticmethod(mp.sin), staticmethod(mp.cos)
        sqrt_rows = staticmethod(lambda a: np.frompyfunc(mp.sqrt, 1, 1)(a))
        num = staticmethod(lambda v: mp.mpf(v) if not isinstance(v, float) or math.isfinite(v) else (mp.inf if v > 0 else -mp.inf))
    return _MP


def _weight(F, sigma_fix, sigma):
    if math.isinf(sigma):
        return F.zero
    q = F.num(sigma_fix) / F.num(sigma)
    return q * q


def _rotate(F, R, d):
    """R exp([d]x), lev_rotate's formula"""
    d0, d1, d2 = d
    t2 = d0 * d0 + d1 * d1 + d2 * d2
    if t2 < 1e-6:
        ca = 1 - t2 * (F.one / 6 - t2 * (F.one / 120)); cb = F.one / 2 - t2 * (F.one / 24 - t2 * (F.one / 720))
        if F.dtype is object:                                              # (50 digits: the closed forms themselves)
            th = F.sqrt(t2)
            ca, cb = (F.sin(th) / th, (1 - F.cos(th)) / t2) if t2 > 0 else (F.one, F.one / 2)
    else:
        th = F.sqrt(t2)
        ca, cb = F.sin(th) / th, (1 - F.cos(th)) / t2
    E = np.array([[1 - cb * (d1 * d1 + d2 * d2), cb * d0 * d1 - ca * d2, cb * d0 * d2 + ca * d1],
                  [cb * d0 * d1 + ca * d2, 1 - cb * (d0 * d0 + d2 * d2), cb * d1 * d2 - ca * d0],
                  [cb * d0 * d2 - ca * d1, cb * d1 * d2 + ca * d0, 1 - cb * (d0 * d0 + d1 * d1)]], dtype=F.dtype)
    return R.dot(E)


def _cholesky(F, A):
    """lower factor of the 10 x 10 A by rows of pivots -> (L as lists, pivots)"""
    L = [[F.zero] * 10 for _ in range(10)]
    piv = []
    for j in range(10):
        p = A[j][j] - sum((L[j][k] * L[j][k] for k in range(j)), F.zero)
        piv.append(p)
        if not p > 0:                                                      # (a NaN pivot as well)
            return None, piv
        ljj = F.sqrt(p)
        L[j][j] = ljj
        for i in range(j + 1, 10):
            L[i][j] = (A[i][j] - sum((L[i][k] * L[j][k] for k in range(j)), F.zero)) / ljj
    return L, piv


def _chol_solve(F, L, b):
    y = [F.zero] * 10
    for i in range(10):
        y[i] = (b[i] - sum((L[i][k] * y[k] for k in range(i)), F.zero)) / L[i][i]
    x = [F.zero] * 10
    for i in range(9, -1, -1):
        x[i] = (y[i] - sum((L[k][i] * x[k] for k in range(i + 1, 10)), F.zero)) / L[i][i]
    return x


def _cross_cols(F, w):
    """(n,3,3): column k = e_k x w_i  (= -[w_i]x)"""
    n = len(w)
    z = np.full(n, F.zero, dtype=F.dtype)
    C = np.empty((n, 3, 3), dtype=F.dtype)
    C[:, :, 0] = np.stack([z, -w[:, 2], w[:, 1]], 1)
    C[:, :, 1] = np.stack([w[:, 2], z, -w[:, 0]], 1)
    C[:, :, 2] = np.stack([-w[:, 1], w[:, 0], z], 1)
    return C


def _iterate(F, pos, quat, gps, R0, t0, s0, l0, cfg):
    """the iteration on the usable rows pos / quat / gps (float64 arrays) in the arithmetic F -> dict"""
    n = len(pos)
    P, G = F.conv(pos), F.conv(gps)
    if F.dtype is object:
        Q = F.conv(quat)
        Q = Q / F.sqrt_rows((Q * Q).sum(1))[:, None]
    else:
        Q, _ = quat_unit_rows(quat)
    M = quat_matrix_rows(Q)
    pf, gf = P[0], G[0]
    v, dg = P - pf, G - gf
    R, s, l, phi = F.conv(R0).reshape(3, 3), F.num(s0), F.conv(l0), np.full(3, F.zero, dtype=F.dtype)
    l_start = F.conv(l0)
    c = R.T.dot(F.conv(t0) - gf) + s * pf
    wl = [_weight(F, cfg["sigma_fix"], sp) for sp in cfg["sigma_prior"]]
    wr = _weight(F, cfg["sigma_fix"], cfg["sigma_rot"])
    out = dict(flags=0, rms_before=NAN, rms_after=NAN, last_step=NAN, min_pivot=math.inf, var=None, kappa=None, steps=[], E=None, pf=np.asarray(pos[0], np.float64),
               gf=np.asarray(gps[0], np.float64))

    def residual(R, s, c, l):
        u = dg.dot(R)                                                      # rows R^T dg
        w = s * v + c + (M * l[None, None, :]).sum(2)
        return u, w, u - w

    Ninv_ll = None
    for it in range(cfg["iters"]):
        u, w, r = residual(R, s, c, l)
        if it == 0:
            out["rms_before"] = float(F.sqrt((r * r).sum() / n))
            sv = v.sum(0)
            var = ((v * v).sum() - (sv * sv).sum() / n) / n
            var = var if var > 0 else F.zero
            out["var"] = float(var)
            out["E"] = float(max(F.sqrt(x) for x in (u * u).sum(1)))
            if not var >= 1e-12:
                out["flags"] |= VAR0
            if n < cfg["min_rows"]:
                out["flags"] |= FEW
            if out["flags"]:
                break
        J = np.empty((n, 3, 10), dtype=F.dtype)
        J[:, :, 0] = v
        J[:, :, 1:4] = np.eye(3)
        J[:, :, 4:7] = M
        J[:, :, 7:10] = _cross_cols(F, w)
        Jf = J.reshape(n * 3, 10)
        N = Jf.T.dot(Jf)
        g = Jf.T.dot(r.reshape(n * 3))
        for j in range(3):
            N[4 + j, 4 + j] = N[4 + j, 4 + j] + wl[j]; g[4 + j] = g[4 + j] + wl[j] * (l_start[j] - l[j])
            N[7 + j, 7 + j] = N[7 + j, 7 + j] + wr; g[7 + j] = g[7 + j] - wr * phi[j]
        pins = ([0] if not cfg["fit_scale"] else []) + ([7, 8, 9] if not cfg["fit_rotation"] else [])
        for k in pins:
            N[k, :] = F.zero; N[:, k] = F.zero; N[k, k] = F.one; g[k] = F.zero
        diag = [N[j, j] for j in range(10)]
        if not all(dj > 0 for dj in diag):
            out["flags"] |= SINGULAR; out["min_pivot"] = min(out["min_pivot"], 0.0)
            break
        D = [1 / F.sqrt(dj) for dj in diag]
        A = [[N[i, j] * D[i] * D[j] for j in range(10)] for i in range(10)]
        L, piv = _cholesky(F, A)
        out["min_pivot"] = min(out["min_pivot"], float(min(piv)))
        if L is None or not all(p > cfg["pivot_min"] for p in piv):
            out["flags"] |= SINGULAR
            break
        x = _chol_solve(F, L, [g[j] * D[j] for j in range(10)])
        d = [x[j] * D[j] for j in range(10)]
        Ninv_ll = [[_chol_solve(F, L, [D[4 + a] if k == 4 + a else F.zero for k in range(10)])[4 + b] * D[4 + b] for b in range(3)] for a in range(3)]
        if it == cfg["iters"] - 1:
            ev = np.linalg.eigvalsh(np.array([[float(A[i][j]) for j in range(10)] for i in range(10)]))
            out["kappa"] = float(ev[-1] / ev[0])
        s = s + d[0]
        c = c + np.array(d[1:4], dtype=F.dtype); l = l + np.array(d[4:7], dtype=F.dtype); phi = phi + np.array(d[7:10], dtype=F.dtype)
        R = _rotate(F, R, d[7:10])
        out["steps"].append(float(max(abs(dk) for dk in d[4:7])))
        ratio = s / F.num(s0)
        if not s > 1e-6 or not ratio >= 1.0 / cfg["ratio_max"] or not ratio <= cfg["ratio_max"]:
            out["flags"] |= SCALE
            out["s_raw"] = float(s)
            break
    if not out["flags"]:
        _, _, r = residual(R, s, c, l)
        out["rms_after"] = float(F.sqrt((r * r).sum() / n))
        out["last_step"] = out["steps"][-1]
        sf2 = F.num(cfg["sigma_fix"]) ** 2
        t = R.dot(c - s * pf) + gf
        out.update(R=np.array(R, dtype=np.float64), t=np.array(t, dtype=np.float64), s=float(s), l=np.array(l, dtype=np.float64),
                   l_cov=np.array([[float(sf2 * Ninv_ll[a][b]) for b in range(3)] for a in range(3)]))
    return out


def fit_track(tr, cfg=None, backend=None):
    """the fit entry on one track dict (see finish()) -> dict(flags, n_rows, n_bad_quat, first, R (3,3), t, s, l, l_cov (3,3), rms_before,
    rms_after, last_step + the diagnostics min_pivot, var, kappa, steps, E, weak = l_cov[jj] / sigma_prior[j]^2)"""
    cfg = cfg or config()
    F = backend or _F64
    sp2 = np.array(cfg["sigma_prior"]) ** 2
    out = dict(flags=0, n_rows=0, n_bad_quat=0, first=-1, R=np.array(tr["R"], np.float64).reshape(3, 3), t=np.array(tr["t"], np.float64), s=float(tr["s"]),
               l=np.array(tr["l0"], np.float64), l_cov=np.diag(sp2), rms_before=NAN, rms_after=NAN, last_step=NAN, min_pivot=math.inf, var=None,
               kappa=None, steps=[], E=None, s_start=float(tr["s"]))
    if tr.get("run_status", 0) != 0:
        out["flags"] = TRACK
    else:
        kinds = row_kinds(tr["pos"], tr["quat"], tr["gps"], tr["valid"])
        ok = kinds == 0
        out["n_rows"], out["n_bad_quat"] = int(ok.sum()), int((kinds == 1).sum())
        out["first"] = int(np.flatnonzero(ok)[0]) if ok.any() else -1
        if out["n_rows"] < cfg["min_rows"]:
            out["flags"] |= FEW
        if out["n_rows"] >= 1:
            it = _iterate(F, tr["pos"][ok], tr["quat"][ok], tr["gps"][ok], tr["R"], tr["t"], tr["s"], tr["l0"], cfg)
            flags = out["flags"] | it.pop("flags")
            out.update(it)
            out["flags"] = flags
            if flags:
                out["rms_after"], out["last_step"] = out["rms_before"], NAN
    with np.errstate(invalid="ignore"):
        out["weak"] = np.diag(out["l_cov"]) / sp2
        for j in range(3):
            if out["l_cov"][j, j] > cfg["weak_ratio"] * sp2[j]:
                out["flags"] |= WEAK_X << j
    if out["last_step"] > cfg["conv_tol"]:
        out["flags"] |= NOT_CONVERGED
    return out


def yardstick(tr, cfg=None):
    """the same iteration with every sum, the solve and the rotation in 50 digits, rounded once at the end"""
    import mpmath as mp
    with mp.workdps(DPS):
        return fit_track(tr, cfg, backend=_mp_backend())


def bounds(y, tr):
    """the four bounds of the module text with C = 1, from the yardstick's kappa / E / s"""
    k, E, s = y["kappa"], y["E"], abs(y["s"])
    return dict(cov=U * k * float(np.abs(y["l_cov"]).max()), l=U * k * E, s=U * k * s, R=U * k, t=U * k * (E + s * float(np.abs(y["pf"]).max())))


def ratios(y, tr, R, t, s, l, l_cov):
    """|result - yardstick| over the bounds with C = 1"""
    b = bounds(y, tr)
    return dict(cov=float(np.abs(np.asarray(l_cov).reshape(3, 3) - y["l_cov"]).max()) / b["cov"],
                l=float(np.abs(np.asarray(l) - y["l"]).max()) / b["l"], s=abs(float(s) - y["s"]) / b["s"],
                R=float(np.abs(np.asarray(R).reshape(3, 3) - y["R"]).max()) / b["R"], t=max(0.0, float(np.abs(np.asarray(t) - y["t"]).max()) - 2 * U * float(np.abs(y["t"]).max())) / b["t"])


# ---------------------------------------------------------------------------- the apply entry
def apply_track(quat, xyz, R, l, sign):
    """out = xyz + sign R (M(q) l) row by row in lev_apply_row's operations -> (out (n,3), flags (n,) int32)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(xyz)
    out, flags = np.full((n, 3), NAN), np.zeros(n, np.int32)
    if n == 0:
        return out, flags
    qn, ok = quat_unit_rows(quat)
    R = np.asarray(R, np.float64).reshape(9)
    l = np.asarray(l, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        M = quat_matrix_rows(qn)
        a = [M[:, r, 0] * l[0] + M[:, r, 1] * l[1] + M[:, r, 2] * l[2] for r in range(3)]
        for r in range(3):
            d = sign * (R[r * 3] * a[0] + R[r * 3 + 1] * a[1] + R[r * 3 + 2] * a[2])
            out[:, r] = np.where(d == 0.0, xyz[:, r], xyz[:, r] + d)
    out[~ok] = NAN
    flags[~ok] = LVP_BAD_QUAT
    return out, flags


# ---------------------------------------------------------------------------- tracks
def _qmul(p, q):
    px, py, pz, pw = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([pw * qx + qw * px + py * qz - pz * qy, pw * qy + qw * py + pz * qx - px * qz, pw * qz + qw * pz + px * qy - py * qx,
                     pw * qw - px * qx - py * qy - pz * qz], -1)


def _axis_quat(axis, ang):
    q = np.zeros((len(ang), 4))
    q[:, axis] = np.sin(ang / 2); q[:, 3] = np.cos(ang / 2)
    return q


def heading_L(n, turn=math.pi / 2):
    """constant, then a turn by `turn` over the middle fifth, then constant"""
    i = np.arange(n, dtype=np.float64)
    a, b = 0.4 * (n - 1), 0.6 * (n - 1)
    return turn * np.clip((i - a) / max(b - a, 1.0), 0.0, 1.0)


def make_track(name, n, rng, shape="L3", l_true=(-0.3, 0.2, -1.1), s_true=0.97, off=SR.OFFSET_N, noise=0.05, turn=math.pi / 2):
    """n poses, 1 m apart.  World orientation Q_i = yaw(heading) pitch roll; camera at p_i = the integrated heading; antenna at p_i + Q_i l.
    The SLAM track is the camera track in a rotated, shifted frame at scale 1 / s_true:  pos = R_t^T (p - o) / s_true, M(q_slam) = R_t^T Q_i.
    shape: L3 (a turn and a roll / pitch wiggle: all three axes observable), Lyaw (yaw only), straight (constant quaternion), standstill."""
    i = np.arange(n, dtype=np.float64)
    head = np.zeros(n) if shape in ("straight", "standstill") else heading_L(n, turn)
    roll = 0.25 * np.sin(i / 4.0) if shape == "L3" else np.zeros(n)
    pitch = 0.2 * np.cos(i / 6.0) if shape == "L3" else np.zeros(n)
    step = np.c_[np.cos(head), np.sin(head), 0.03 * np.cos(i / 40.0) if shape == "L3" else np.zeros(n)]
    cam = np.cumsum(step, axis=0) if shape != "standstill" else np.zeros((n, 3))
    qw = _qmul(_qmul(_axis_quat(2, head), _axis_quat(1, pitch)), _axis_quat(0, roll))
    qt = rng.normal(size=4); qt /= np.linalg.norm(qt)
    Rt = quat_matrix_rows(qt[None])[0]
    o = np.array([12.0, -7.0, 3.0])
    pos = (cam - o) @ Rt / s_true                                          # rows R_t^T (p - o) / s
    qs = _qmul(np.broadcast_to(qt * [-1, -1, -1, 1], (n, 4)), qw) * 1.25   # (not unit: the entry normalises)
    Qw = quat_matrix_rows(qw)
    l_true = np.asarray(l_true, np.float64)
    gps = cam + Qw @ l_true + off + rng.normal(size=(n, 3)) * noise
    return dict(name=name, pos=np.ascontiguousarray(pos), quat=np.ascontiguousarray(qs), gps=gps, valid=np.ones(n, np.uint8), cam=cam + off,
                l_true=l_true, s_true=s_true, run_status=0, ts=0.1 * i)


def finish(tr, rng, s_factor=1.0):
    """the starting values: the plain Umeyama fit of the usable rows (what the chain hands in), l0 = 0"""
    n = len(tr["valid"])
    ok = row_kinds(tr["pos"], tr["quat"], tr["gps"], tr["valid"]) == 0 if n else np.zeros(0, bool)
    with np.errstate(all="ignore"):
        g = LR.global_fit(tr["pos"], tr["gps"], ok) if n else None
    if g is None or not np.isfinite(g[2]) or not np.isfinite(g[0]).all():
        g = (LR._rot(rng), np.array([10.0, -20.0, 5.0]) + (tr["gps"][ok][0] if ok.any() else 0.0), 1.3)
    tr["R"], tr["t"], tr["s"] = np.ascontiguousarray(g[0]), np.ascontiguousarray(g[1]), float(g[2]) * s_factor
    tr["l0"] = np.zeros(3)
    return tr


@functools.lru_cache(maxsize=None)
def gpu_tracks():
    """the ragged batch of both tiers (lengths 0, 1, 2, 7, 8, 63, 64, 65, 130, 271), in a fixed order"""
    rng = np.random.default_rng(20261020)
    T = []
    add = lambda tr, **kw: T.append(finish(tr, rng, **kw))
    add(make_track("len0", 0, rng))
    add(make_track("len1", 1, rng))
    add(make_track("len2", 2, rng))
    add(make_track("len7_few", 7, rng))
    add(make_track("len8_min_rows", 8, rng, shape="Lyaw", noise=0.01))
    add(make_track("len63", 63, rng))
    add(make_track("len64", 64, rng))
    add(make_track("len65", 65, rng))
    add(make_track("len130_yaw_L", 130, rng, shape="Lyaw"))
    add(make_track("len271_L3", 271, rng))
    add(make_track("len271_L3_noiseless", 271, rng, noise=0.0))
    add(make_track("len271_straight", 271, rng, shape="straight"))
    add(make_track("len72_bend", 72, rng, shape="Lyaw", turn=0.2))        # (72 poses: clear of weak_ratio under every switch, see clear_of_switches)
    add(make_track("len130_standstill", 130, rng, shape="standstill"))
    tr = make_track("len130_bad_quats", 130, rng)
    tr["quat"][41] = 0.0; tr["quat"][77, 2] = np.nan; tr["quat"][5] *= 1e-12
    add(tr)
    tr = make_track("len130_masked", 130, rng)                            # rows masked out (the first ones among them) and NaN fixes
    tr["valid"][:3] = 0; tr["valid"][50:60] = 0; tr["gps"][20:25, 1] = np.nan; tr["gps"][100] = np.nan; tr["pos"][110, 0] = np.inf
    add(tr)
    add(make_track("len271_south", 271, rng, off=SR.OFFSET_S))
    tr = make_track("len65_run_failed", 65, rng)
    tr["run_status"] = 8
    add(tr)
    add(make_track("len130_scale_jump", 130, rng), s_factor=3.0)           # the caller's scale is 3 x the data's: s / s0 -> 1/3 < 1 / ratio_max
    add(make_track("len65_all_masked", 65, rng))
    T[-1]["valid"][:] = 0
    for tr in T:
        for k in ("pos", "quat", "gps", "valid", "R", "t", "l0", "cam", "ts"):
            tr[k].setflags(write=False)
    return tuple(T)


def track(name):
    return next(t for t in gpu_tracks() if t["name"] == name)


FITTED = ("len8_min_rows", "len63", "len64", "len65", "len130_yaw_L", "len271_L3", "len271_L3_noiseless", "len271_straight", "len72_bend",
          "len130_bad_quats", "len130_masked", "len271_south")
SWITCHES = ((1, 1), (1, 0), (0, 1), (0, 0))                                # (fit_scale, fit_rotation)


def configs():
    """name -> config of every call the tiers make on the batch"""
    c = {f"s{a}r{b}": config(fit_scale=a, fit_rotation=b) for a, b in SWITCHES}
    c["rot_free"] = config(sigma_rot=math.inf)
    return c


@functools.lru_cache(maxsize=None)
def reference(cname):
    """[fit_track dict] of gpu_tracks() under configs()[cname], computed once"""
    return tuple(fit_track(tr, configs()[cname]) for tr in gpu_tracks())


@functools.lru_cache(maxsize=None)
def track_yardstick(name, cname="s1r1"):
    return yardstick(track(name), configs()[cname])


YARDSTICK_CASES = tuple((n, "s1r1") for n in FITTED) + tuple(("len65", c) for c in ("s1r0", "s0r1", "s0r0"))


@functools.lru_cache(maxsize=None)
def motivation_track():
    """the planted L with 0.1 m noise: 271 poses, l = (-0.3, 0.2, -1.1)"""
    rng = np.random.default_rng(20261022)
    return finish(make_track("len271_L3_motivation", 271, rng, noise=0.1), rng)


def pack(tracks):
    """-> dict of the flat arrays of a ragged batch: ts, pos, quat, gps, valid, offsets, R (B,9), t (B,3), s (B,), l0 (B,3), run_status (B,)"""
    n = [len(t["valid"]) for t in tracks]
    cat = lambda k, w: np.concatenate([np.asarray(t[k]).reshape(-1, w) if w else np.asarray(t[k]).reshape(-1) for t in tracks])
    return dict(ts=cat("ts", 0).astype(np.float64), pos=cat("pos", 3), quat=cat("quat", 4), gps=cat("gps", 3), valid=cat("valid", 0).astype(np.uint8),
                offsets=np.concatenate([[0], np.cumsum(n)]).astype(np.int64), R=np.stack([t["R"].reshape(9) for t in tracks]),
                t=np.stack([t["t"] for t in tracks]), s=np.array([t["s"] for t in tracks]), l0=np.stack([t["l0"] for t in tracks]),
                run_status=np.array([t["run_status"] for t in tracks], np.int32))


def clear_of_switches(fit, cfg):
    """no decision of the fit sits where a rounding difference could flip it: every pivot a factor 100 clear of pivot_min; the variance and
    last_step a factor 2 clear of their thresholds (row counts are integers: exact); the information the data added to an axis over the
    prior's, (1 - q) / q with q = l_cov[jj] / sigma_prior^2 in [0, 1], a factor 2 clear of its value at q = weak_ratio; the scale ratio 2 % clear of its bounds (with ratio_max = 2 no fitted scale
    can be a factor 2 clear of both), as tests/local_align_ref.py has it"""
    if fit["flags"] & TRACK or fit["n_rows"] == 0:
        return True
    if fit["var"] is not None and not (fit["var"] > 2e-12 or fit["var"] < 0.5e-12):
        return False
    if fit["flags"] & (FEW | VAR0):
        return True
    if not (fit["min_pivot"] > 100 * cfg["pivot_min"] or fit["min_pivot"] < cfg["pivot_min"] / 100):
        return False
    if fit["flags"] & SINGULAR:
        return True
    r = (fit["s_raw"] if fit["flags"] & SCALE else fit["s"]) / fit["s_start"]
    if any(0.98 * b <= r <= 1.02 * b for b in (1.0 / cfg["ratio_max"], cfg["ratio_max"])):
        return False
    if fit["flags"] & SCALE:
        return True
    w = cfg["weak_ratio"]
    for j in range(3):
        q = fit["weak"][j]
        if math.isfinite(cfg["sigma_prior"][j]) and not ((1.0 - q) / q > 2.0 * (1.0 - w) / w or (1.0 - q) / q < 0.5 * (1.0 - w) / w):
            return False
    return fit["last_step"] < cfg["conv_tol"] / 2 or fit["last_step"] > 2 * cfg["conv_tol"]
