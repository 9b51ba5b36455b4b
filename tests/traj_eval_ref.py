"""The yardstick of the trajectory evaluation (gsf_traj_eval_dev) and the batch both tiers run.  Never imports the product and holds no test
functions.

Values.  Everything is restated in 50-digit arithmetic (mpmath, sim3_ref.DPS) on the stored float64 inputs, in plain loops: the association
(nearest stamp by a scan over every truth pose; the interpolation rule of gsf_pose_query_dev), the alignment (sim3_ref.yardstick on the matched
pairs for R, t, s), the aligned pose p' = s R p + t, q' = q_R (x) q (transform_trajectory, EKFGPSSLAM.py:461-468, q_R by Rotation.from_matrix's
branch on the largest diagonal), the absolute errors, and the KITTI devkit's calcSequenceErrors: the truth path length d[m] over matched poses,
lastFrameFromSegmentLength, and the pair error from 3x3 rotation matrices and translations, E = (g_f^-1 g_l)^-1 (e_f^-1 e_l), whose angle is
atan2(|axis part of E.R - E.R^T| / 2, (trace - 1) / 2) -- no quaternion product, unlike the code under test.

A condition on the inputs, asserted here: no comparison that selects an index lies within CLEAR = 1e-9 relative of equality unless it is an
exact tie of the float64 inputs -- a time difference against max_diff, the two candidates of the nearest search against each other, a bracket
against max_diff, d[l] against d[f] + value, ts[l] against ts[f] + value.  Then every index the device returns must be exact.

Bounds.  A value's bound is gamma_k x scale, gamma_k = k u / (1 - k u), u = 2^-53, k = the rounded operations on the value's longest path
through gsf_traj_eval_core.hpp (a function documented to 1 ulp counts 2, the device's atan2 at 2 ulp counts 4), scale = the sum of the
magnitudes entering it.  The counts, path by path:
  unit quaternion (quat_unit): 4 for x^2 + y^2 + z^2 + w^2 as one chain, 2 for 1 / sqrt, 1 for the product                       =  7
  truth quaternion, interpolated: w = (tau - ti) / (tj - ti) 2, 1 - w 1, blend 2, |blend| 4 + sqrt 1, 1 / n 1, product 1, unit 7  = 19
  q_R (quat_from_matrix): trace 2, numerator 2, sum of squares 4, 1 / sqrt 2, product 1                                           = 11
  q' = q_R (x) q (quat_mul: one product and three fma): max(11, 7) + 4                                                            = 15
  K_APE_T: s (R p) + t 3 + 1, p' - g 1, sum of squares 3, sqrt 1                                                                  =  9
  K_APE_R: conj(q_g) (x) q': max(19, 15) + 4 = 23, |v| 3 + 1, atan2 4 (times 2 is exact)                                          = 31
  K_RPE_T: conj(q'_f) rotates p'_l - p'_f (quat_rotate: 5 on the path of q): 15 + 5 = 20, t_B - t_A 1, norm 3 + 1                 = 25
  K_RPE_R: conj(g_f) (x) g_l: 19 + 4 = 23, conj(q_A) (x) q_B: 23 + 4 = 27, |v| 3 + 1, atan2 4                                     = 35
Scales: ape_t: |s| |p|_1 + |t|_1 + |g|_1; rpe_t: the same over the four poses of the pair; the angles: 1 + theta (radians)."""
import functools

import numpy as np

import sim3_ref as S

DPS = S.DPS
U = 2.0 ** -53
CLEAR = 1e-9
K_APE_T, K_APE_R, K_RPE_T, K_RPE_R = 9, 31, 25, 35

NEAREST, INTERP = 0, 1
ALIGN_NONE, ALIGN_SE3, ALIGN_SIM3 = 0, 1, 2
FRAMES, METRES, SECONDS = 0, 1, 2
MATCHED, NO_TRUTH, P_NAN, BAD_QUAT, P_TRACK = 1, 2, 4, 8, 16
T_SKIPPED, T_EMPTY, T_UNSORTED, T_FEW, T_DEGENERATE = 1, 2, 4, 8, 16
ALIGN_OF = {"none": ALIGN_NONE, "se3": ALIGN_SE3, "sim3": ALIGN_SIM3}
ASSOC_OF = {"nearest": NEAREST, "interp": INTERP}

DT = 0.125                              # stamps live on a binary grid: ties can be planted exactly
MAX_DIFF = {NEAREST: 0.0625, INTERP: 0.3}     # NEAREST: half a truth step, so a midway stamp is a tie of the candidates AND of the threshold


def gamma(k):
    return k * U / (1.0 - k * U)


def _mp():
    import mpmath
    return mpmath


def _clear(mp, a, b, what):
    """a and b (mp numbers) are exactly equal, or at least CLEAR apart relative to the larger"""
    if a == b:
        return
    assert abs(a - b) > mp.mpf(CLEAR) * max(abs(a), abs(b)), (what, float(a), float(b))


# ---------------------------------------------------------------------------------------------------------------- quaternions, 50 digits
def _vec(mp, row):
    return [mp.mpf(float(v)) for v in row]


def _unit(mp, q):
    """q / |q| or None (norm 0, NaN or infinite: Rotation.from_quat raises)"""
    if not all(np.isfinite(float(v)) for v in q):
        return None
    n2 = mp.fsum(v * v for v in q)
    if not (mp.mpf("1e-280") <= n2 <= mp.mpf("1e280")):
        return None
    n = mp.sqrt(n2)
    return [v / n for v in q]


def _rot_of(mp, q):
    """as_matrix() of a unit quaternion [x, y, z, w]"""
    x, y, z, w = q
    return [[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]]


def _quat_of(mp, M):
    """Rotation.from_matrix's quaternion of a 3x3 matrix as it stands (branch on the largest of the diagonal and the trace), normalised"""
    tr = M[0][0] + M[1][1] + M[2][2]
    c, best = 0, M[0][0]
    if M[1][1] > best:
        c, best = 1, M[1][1]
    if M[2][2] > best:
        c, best = 2, M[2][2]
    if tr > best:
        c = 3
    if c == 3:
        q = [M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1], 1 + tr]
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q = [None] * 4
        q[i] = 1 - tr + 2 * M[i][i]
        q[j] = M[j][i] + M[i][j]
        q[k] = M[k][i] + M[i][k]
        q[3] = M[k][j] - M[j][k]
    n = mp.sqrt(mp.fsum(v * v for v in q))
    return [v / n for v in q]


def _matmul(A, B):
    return [[sum(A[r][k] * B[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def _tr(A):
    return [[A[c][r] for c in range(3)] for r in range(3)]


def _apply(A, v):
    return [sum(A[r][k] * v[k] for k in range(3)) for r in range(3)]


def _angle(mp, R):
    """the rotation angle of a 3x3 rotation matrix in [0, pi], well conditioned at both ends"""
    ax = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    return mp.atan2(mp.sqrt(mp.fsum(v * v for v in ax)) / 2, (R[0][0] + R[1][1] + R[2][2] - 1) / 2)


def nlerp(mp, q1, q2, w):
    """quaternion_nlerp, EKFGPSSLAM.py:94-105"""
    dot = mp.fsum(a * b for a, b in zip(q1, q2))
    if dot < 0:
        q2 = [-v for v in q2]
    wc = min(max(w, mp.mpf(0)), mp.mpf(1))
    qi = [(1 - wc) * a + wc * b for a, b in zip(q1, q2)]
    n = mp.sqrt(mp.fsum(v * v for v in qi))
    if n < mp.mpf("1e-9"):
        return q1 if w < mp.mpf("0.5") else q2
    return [v / n for v in qi]


# ---------------------------------------------------------------------------------------------------------------- track state, association
def _unsorted(t):
    t = np.asarray(t, np.float64)
    if len(t) == 0:
        return False
    return bool(np.isnan(t[0]) or not np.all(t[1:] >= t[:-1]))


def track_state0(ts, rts, skipped):
    """the bits decided before anything is searched"""
    if skipped:
        return T_SKIPPED
    if len(ts) == 0 or len(rts) == 0:
        return T_EMPTY
    return T_UNSORTED if (_unsorted(ts) or _unsorted(rts)) else 0


def associate(ts, pos, quat, rts, rpos, rquat, assoc, max_diff):
    """one usable track -> flags (n,) uint8, index (n,) int32, pairs: {i: (g [3 mp], qg [4 mp unit], qe [4 mp unit])} of the matched poses"""
    mp = _mp()
    n, G = len(ts), len(rts)
    flags, index, pairs = np.zeros(n, np.uint8), np.full(n, -1, np.int32), {}
    md = mp.mpf(float(max_diff))
    RT = [mp.mpf(float(v)) for v in rts]
    for i in range(n):
        if not np.isfinite(pos[i]).all():
            flags[i] = P_NAN
            continue
        qe = _unit(mp, _vec(mp, quat[i]))
        if qe is None:
            flags[i] = BAD_QUAT
            continue
        tau = mp.mpf(float(ts[i]))
        if assoc == NEAREST:
            best, bj = None, -1
            for j in range(G):                                        # the earlier j on a tie, the first among equal stamps: strict <
                dj = abs(RT[j] - tau)
                if best is None or dj < best:
                    if best is not None:
                        _clear(mp, dj, best, ("nearest candidates", i, j))
                    best, bj = dj, j
                elif dj != best and j == bj + 1:
                    _clear(mp, dj, best, ("nearest candidates", i, j))
            _clear(mp, best, md, ("max_diff", i))
            if not best <= md:
                flags[i] = NO_TRUTH
                continue
            g, qg_raw = _vec(mp, rpos[bj]), _vec(mp, rquat[bj])
            finite_g = bool(np.isfinite(rpos[bj]).all())
        else:
            if tau < RT[0] or tau > RT[-1]:
                flags[i] = NO_TRUTH
                continue
            bj = max(j for j in range(G) if RT[j] <= tau)             # among equal stamps the last, as gsf_pose_query_dev
            if RT[bj] == tau:
                g, qg_raw = _vec(mp, rpos[bj]), _vec(mp, rquat[bj])
                finite_g = bool(np.isfinite(rpos[bj]).all())
            else:
                gap = RT[bj + 1] - RT[bj]
                _clear(mp, gap, md, ("bracket against max_diff", i))
                if md > 0 and gap > md:
                    flags[i] = NO_TRUTH
                    continue
                finite_g = bool(np.isfinite(rpos[bj]).all() and np.isfinite(rpos[bj + 1]).all())
                qa, qb = rquat[bj], rquat[bj + 1]
                if not (np.isfinite(qa).all() and np.isfinite(qb).all()):
                    g, qg_raw = None, [mp.nan] * 4
                else:
                    w = (tau - RT[bj]) / gap
                    if finite_g:
                        g = [a + w * (b - a) for a, b in zip(_vec(mp, rpos[bj]), _vec(mp, rpos[bj + 1]))]
                    qg_raw = nlerp(mp, _vec(mp, qa), _vec(mp, qb), w)
        if not finite_g:
            flags[i] = P_NAN
            continue
        qg = _unit(mp, qg_raw)
        if qg is None:
            flags[i] = BAD_QUAT
            continue
        flags[i], index[i] = MATCHED, bj
        pairs[i] = (g, qg, qe)
    return flags, index, pairs


# ---------------------------------------------------------------------------------------------------------------- one track
class TrackEval:
    """the yardstick's answer for one track (see evaluate_track)"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def pair_frames(mp, kind, value, stride, d, tsm, M):
    """[(f, l)] over matched indices: first frames 0, stride, ...; the last frame by the rule of the kind (KITTI: lastFrameFromSegmentLength)"""
    out = []
    if stride < 1:
        return out
    val = mp.mpf(float(value))
    for f in range(0, M, stride):
        l = -1
        if kind == FRAMES:
            if value >= 1 and f + int(value) < M:
                l = f + int(value)
        elif kind == METRES:
            for i in range(f + 1, M):
                _clear(mp, d[i], d[f] + val, ("d[l] against d[f] + value", f, i))
                if d[i] > d[f] + val:
                    l = i
                    break
        else:
            for i in range(f + 1, M):
                _clear(mp, tsm[i], tsm[f] + val, ("ts[l] against ts[f] + value", f, i))
                if tsm[i] >= tsm[f] + val:
                    l = i
                    break
        if l >= 0:
            out.append((f, l))
    return out


def evaluate_track(ts, pos, quat, rts, rpos, rquat, skipped, assoc, align, max_diff, scenarios=(), errors_for=(), fit=None):
    """-> TrackEval: state, flags, index, M, rows (the estimate rows of the matched poses), y (sim3_ref's Fit of the matched pairs, or None),
    R / t / s (float64; NaN where the state says so; `fit` = (R, t, s) replaces the yardstick's own), ape_t / ape_r (n,) float64 with their
    bounds b_ape_t / b_ape_r, and per scenario k: pairs[k] = [(row of f, row of l)], and for k in errors_for: rpe_t[k] / rpe_r[k] /
    b_rpe_t[k] / b_rpe_r[k] as arrays over the pairs.  src / dst: the matched float64 rows the fit is gated on (NEAREST only)."""
    mp = _mp()
    n = len(ts)
    nan = float("nan")
    out = TrackEval(state=track_state0(ts, rts, skipped), flags=np.full(n, P_TRACK, np.uint8), index=np.full(n, -1, np.int32), M=0, rows=[],
                    y=None, R=np.full((3, 3), nan), t=np.full(3, nan), s=nan, ape_t=np.full(n, nan), ape_r=np.full(n, nan),
                    b_ape_t=np.full(n, nan), b_ape_r=np.full(n, nan), pairs=[[] for _ in scenarios], rpe_t={}, rpe_r={}, b_rpe_t={}, b_rpe_r={},
                    src=None, dst=None)
    if out.state:
        return out
    with mp.workdps(DPS):
        out.flags, out.index, pairs = associate(ts, pos, quat, rts, rpos, rquat, assoc, max_diff)
        rows = sorted(pairs)
        M = len(rows)
        if assoc == NEAREST and M:
            out.src, out.dst = np.ascontiguousarray(pos[rows]), np.ascontiguousarray(rpos[out.index[rows]])
        if align != ALIGN_NONE:
            if M < 3:
                out.state |= T_FEW
                return out
            if fit is None:
                dst = out.dst if assoc == NEAREST else np.array([[float(v) for v in pairs[i][0]] for i in rows])
                y = S.yardstick(np.ascontiguousarray(pos[rows]), dst)
                out.y, out.src, out.dst = y, np.ascontiguousarray(pos[rows]), dst
                if y.status == S.SIM3_NONE:
                    out.state |= T_DEGENERATE
                    return out
                R, s = y.R, (y.s if align == ALIGN_SIM3 else 1.0)
                if align == ALIGN_SIM3:
                    t = y.t
                else:
                    sc = [mp.fsum(mp.mpf(float(pos[i][k])) for i in rows) / M for k in range(3)]
                    dc = [mp.fsum(pairs[i][0][k] for i in rows) / M for k in range(3)]
                    Rm = [[mp.mpf(float(v)) for v in r] for r in R]
                    t = np.array([float(dc[k] - _apply(Rm, sc)[k]) for k in range(3)])
            else:
                R, t, s = (np.asarray(fit[0], np.float64).reshape(3, 3), np.asarray(fit[1], np.float64).reshape(3), float(fit[2]))
                if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)):
                    out.state |= T_DEGENERATE
                    return out
        else:
            R, t, s = np.eye(3), np.zeros(3), 1.0
        out.R, out.t, out.s, out.M, out.rows = np.asarray(R, np.float64), np.asarray(t, np.float64), float(s), M, rows
        Rm = [[mp.mpf(float(v)) for v in r] for r in out.R]
        tm, sm = _vec(mp, out.t), mp.mpf(out.s)
        RqR = _rot_of(mp, _quat_of(mp, Rm)) if align != ALIGN_NONE else [[mp.mpf(int(r == c)) for c in range(3)] for r in range(3)]
        t1 = float(np.abs(out.t).sum())
        # ---- aligned poses and absolute errors
        G_, RG, PE, RE, scale = [], [], [], [], []
        for i in rows:
            g, qg, qe = pairs[i]
            p = _vec(mp, pos[i])
            pa = [sm * v + tk for v, tk in zip(_apply(Rm, p), tm)]
            Rg, Re = _rot_of(mp, qg), _matmul(RqR, _rot_of(mp, qe))
            G_.append(g); RG.append(Rg); PE.append(pa); RE.append(Re)
            sc_i = abs(out.s) * float(np.abs(pos[i]).sum()) + t1 + float(sum(abs(v) for v in g))
            scale.append(sc_i)
            et = mp.sqrt(mp.fsum((a - b) ** 2 for a, b in zip(pa, g)))
            er = _angle(mp, _matmul(_tr(Rg), Re))
            out.ape_t[i], out.ape_r[i] = float(et), float(er)
            out.b_ape_t[i], out.b_ape_r[i] = gamma(K_APE_T) * sc_i, gamma(K_APE_R) * (1.0 + float(er))
        # ---- the pairs of every scenario, the errors of the asked ones
        d = [mp.mpf(0)] * M
        for m in range(1, M):
            d[m] = d[m - 1] + mp.sqrt(mp.fsum((a - b) ** 2 for a, b in zip(G_[m], G_[m - 1])))
        tsm = [mp.mpf(float(ts[i])) for i in rows]
        out.d = np.array([float(v) for v in d])
        for k, (kind, value, stride) in enumerate(scenarios):
            fl = pair_frames(mp, kind, value, int(stride), d, tsm, M)
            out.pairs[k] = [(rows[f], rows[l]) for f, l in fl]
            if k not in errors_for:
                continue
            et_, er_, bt_, br_ = [], [], [], []
            for f, l in fl:
                # relative poses A = g_f^-1 g_l and B = e_f^-1 e_l as (rotation, translation); E = A^-1 B
                RA, tA = _matmul(_tr(RG[f]), RG[l]), _apply(_tr(RG[f]), [a - b for a, b in zip(G_[l], G_[f])])
                RB, tB = _matmul(_tr(RE[f]), RE[l]), _apply(_tr(RE[f]), [a - b for a, b in zip(PE[l], PE[f])])
                tE = _apply(_tr(RA), [a - b for a, b in zip(tB, tA)])
                et, er = mp.sqrt(mp.fsum(v * v for v in tE)), _angle(mp, _matmul(_tr(RA), RB))
                et_.append(float(et)); er_.append(float(er))
                bt_.append(gamma(K_RPE_T) * (scale[f] + scale[l])); br_.append(gamma(K_RPE_R) * (1.0 + float(er)))
            out.rpe_t[k], out.rpe_r[k], out.b_rpe_t[k], out.b_rpe_r[k] = (np.array(v, np.float64) for v in (et_, er_, bt_, br_))
    return out


def evaluate(c, assoc, align, scenarios=(), errors_for=(), fits=None, only=None):
    """the batch of build_cases() (or any dict with its keys) -> [TrackEval]; fits = (R (B,9), t (B,3), s (B,)) of the device; only: a subset
    of track numbers (the others come back as None)"""
    out = []
    for b in range(c["B"]):
        if only is not None and b not in only:
            out.append(None)
            continue
        lo, hi, glo, ghi = c["offsets"][b], c["offsets"][b + 1], c["ref_offsets"][b], c["ref_offsets"][b + 1]
        fit = None if fits is None else (fits[0][b], fits[1][b], fits[2][b])
        out.append(evaluate_track(c["ts"][lo:hi], c["pos"][lo:hi], c["quat"][lo:hi], c["ref_ts"][glo:ghi], c["ref_pos"][glo:ghi],
                                  c["ref_quat"][glo:ghi], bool(c["run_status"][b]), assoc, align, MAX_DIFF[assoc], scenarios, errors_for, fit))
    return out


K_SE3_T = 8     # centroid about the first pair: difference 1, the sum's last addition 1 (the earlier ones act on the track's extent), division 1,
                # the origin added back 1; R sc 3; dc - R sc 1


def se3_ratios(w, R, t):
    """an SE3 result against the yardstick w (a TrackEval with y / src / dst, NEAREST): the rotation's ratios of sim3_ref.ratios (the scale
    and the image belong to the Sim3 fit), and t against dc - R sc formed in 50 digits with the RESULT's R, in units of gamma_8 (|dc|_1 +
    |sc|_1) under the key "t" (gate 1: sim3_ref.gate_of does not know it, so callers assert it themselves)"""
    mp = _mp()
    out = {k: v for k, v in S.ratios(w.y, w.src, w.dst, None, R, w.y.t, w.y.s).items() if k in ("R", "det", "orth")}
    with mp.workdps(DPS):
        M = len(w.src)
        sc = [mp.fsum(mp.mpf(float(v)) for v in w.src[:, k]) / M for k in range(3)]
        dc = [mp.fsum(mp.mpf(float(v)) for v in w.dst[:, k]) / M for k in range(3)]
        Rm = [[mp.mpf(float(v)) for v in r] for r in np.asarray(R, np.float64).reshape(3, 3)]
        want = [dc[k] - _apply(Rm, sc)[k] for k in range(3)]
        bound = gamma(K_SE3_T) * float(sum(abs(v) for v in dc) + sum(abs(v) for v in sc))
        t_ratio = max(abs(float(mp.mpf(float(t[k])) - want[k])) for k in range(3)) / bound
    return out, t_ratio


K_INTERP_POS = 3    # an interpolated truth position: w = (tau - ti) / (tj - ti) 2, one fma


def interp_fit_ratios(w, align, R, t, s, pos_rows):
    """A fit under INTERP against its yardstick w (w.y = sim3_ref's Fit on the estimate rows `pos_rows` and the interpolated truth rounded
    once to float64, w.dst).  The code under test interpolates in float64, so its dst rows differ from those by e_i <= gamma_3 |g_i|_inf +
    u |g_i|_inf per component; first-order perturbation of the closed form adds to sim3_ref's bounds
        R: sum |a_i| e_i sqrt(3) / (sigma2 + d sigma3),   s: sum |a_i| e_i sqrt(3) / (sigma1 + sigma2 + sigma3) (relative),
        image: the two times s max|a_i|, plus max e_i for the centroid of dst
    (a_i = the centred estimate rows).  Ratios are to gate x (sim3_ref's bound) + the addition, so 1 is the gate; determined fits only
    (the others -> {})."""
    y = w.y
    if y.cls != "determined":
        return {}
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    a = pos_rows - pos_rows.mean(0)
    na = np.linalg.norm(a, axis=1)
    e = (gamma(K_INTERP_POS) + U) * np.abs(w.dst).max(axis=1) * np.sqrt(3.0)
    addR = float((na * e).sum() / (y.sigma[1] + y.d * y.sigma[2]))
    adds = float((na * e).sum() / y.sigma.sum())
    out = {"R": float(np.abs(R - y.R).max()) / (S.C_R * y.bR + addR)}
    if align == ALIGN_SIM3:
        out["s"] = abs(float(s) - y.s) / (S.C_S * y.bs * y.s + adds * y.s)
        img, want = float(s) * pos_rows @ R.T + t, y.s * pos_rows @ y.R.T + y.t
        out["img"] = float(np.abs(img - want).max()) / (S.C_IMG * y.bimg + (addR + adds) * y.s * float(na.max()) + float(e.max()))
    return out


def gate_fit(fits, worst, name, w, align, R, t, s):
    """a fitted R, t, s of a NEAREST track against its yardstick w: `fits` is the Worst of tests/test_sim3_yardstick_host.py (the gates of the
    Sim3 yardstick tests for a non-polar route: sim3_ref.gate_of on the two-pass bounds), `worst` collects the SE3 translation's ratio"""
    if align == ALIGN_SIM3:
        fits.add(name, S.ratios(w.y, w.src, w.dst, None, R, t, s))
    else:
        assert s == 1.0, (name, s)
        rot, t_ratio = se3_ratios(w, R, t)
        fits.add(name, rot)
        worst["se3_t"] = max(worst.get("se3_t", 0.0), t_ratio)


def with_fit(c, b, assoc, align, fit, scenarios=None, errors_for=None):
    """the yardstick of track b evaluated with a result's own R, t, s, so that the conditioning of the fit does not enter a second time"""
    lo, hi, glo, ghi = c["offsets"][b], c["offsets"][b + 1], c["ref_offsets"][b], c["ref_offsets"][b + 1]
    return evaluate_track(c["ts"][lo:hi], c["pos"][lo:hi], c["quat"][lo:hi], c["ref_ts"][glo:ghi], c["ref_pos"][glo:ghi], c["ref_quat"][glo:ghi],
                          bool(c["run_status"][b]), assoc, align, MAX_DIFF[assoc], SCENARIOS if scenarios is None else scenarios,
                          TRACED if errors_for is None else errors_for, fit)


def flat(c, evs, name, fill):
    """a per-pose field of [TrackEval] as one array over the P poses"""
    first = next(e for e in evs if e is not None)
    out = np.full(c["P"], fill, dtype=getattr(first, name).dtype)
    for b, e in enumerate(evs):
        if e is not None:
            out[c["offsets"][b]:c["offsets"][b + 1]] = getattr(e, name)
    return out


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the rows where want is a number; NaN patterns must agree -> (ratio, same_nan)"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    same = bool((np.isnan(got) == np.isnan(want)).all())
    ok = ~np.isnan(want) & ~np.isnan(got)
    return (float(np.max(np.abs(got[ok] - want[ok]) / bound[ok])) if ok.any() else 0.0), same


# ---------------------------------------------------------------------------------------------------------------- the batch
SCENARIOS = ((FRAMES, 1.0, 1), (FRAMES, 300.0, 1), (SECONDS, 1.0, 1), (SECONDS, 2.5, 3), (METRES, 20.0, 1), (METRES, 50.0, 10),
             (METRES, 100.0, 10), (METRES, 200.0, 10), (FRAMES, 10.0, 7))
TRACED = (0, 2, 4, 5)                   # the scenarios whose pair errors both tiers compare value by value

MATCHED_COUNTS = (0, 1, 2, 3, 63, 64, 65, 129, 271)


def _quat_mul(p, q):
    px, py, pz, pw = p
    qx, qy, qz, qw = q
    return np.array([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw,
                     pw * qw - px * qx - py * qy - pz * qz])


def _axis_quat(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.r_[axis * np.sin(ang / 2), np.cos(ang / 2)]


def _rot_np(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_truth(G, rng, t0, dt=DT, off=S.OFFSET_N, step=1.4):
    """a gently curving drive: stamps t0 + k dt (exact), positions about `off`, orientations along the heading with small roll and pitch"""
    k = np.arange(G)
    head = 0.6 * np.sin(k * dt * 0.35) + 0.004 * k * dt * 8
    steps = step * (dt / DT) * np.c_[np.cos(head), np.sin(head), 0.05 * np.sin(k * dt * 0.9)]
    pos = np.cumsum(steps, axis=0) + off
    quat = np.array([_quat_mul(_axis_quat([0, 0, 1], h), _axis_quat([1, 0.3, 0], 0.03 * np.sin(0.7 * j * dt))) for j, h in enumerate(head)])
    quat[rng.random(G) < 0.2] *= -1.0                                  # q and -q are the same rotation
    return t0 + k / float(round(1.0 / dt)), pos, quat                 # (k / 80 is exact wherever the quotient is on the grid; k * 0.0125 is not)


def make_estimate(ts, gpos, gquat, rng, scale=1.3, noise=0.05, rot_noise=0.01, off=S.OFFSET_N):
    """the truth poses seen from a SLAM frame: p = R0^T (g - off - t0) / scale + noise, q = conj(q0) (x) q_g (x) q_noise"""
    q0 = _axis_quat(rng.normal(size=3), rng.uniform(0.3, 2.5))
    R0 = _rot_np(q0)
    pos = ((gpos - off - np.array([12.0, -7.0, 1.5])) @ R0) / scale + rng.normal(size=gpos.shape) * noise
    quat = np.array([_quat_mul(_quat_mul(q0 * np.array([-1, -1, -1, 1]), q), _axis_quat(rng.normal(size=3), rot_noise * rng.normal())) for q in gquat])
    return np.asarray(ts, float).copy(), pos, quat


def _build_cases():
    rng = np.random.default_rng(S.SEED + 77)
    tracks, notes = [], {}

    def add(name, est, truth, skipped=False):
        notes[name] = len(tracks)
        tracks.append((name, [np.ascontiguousarray(v, dtype=np.float64) for v in est], [np.ascontiguousarray(v, dtype=np.float64) for v in truth], skipped))

    def holed(M, hole=5):
        """M matched poses and `hole` estimate poses inside a stretch the truth does not cover"""
        G = M + hole
        tt, gp, gq = make_truth(G, rng, 1000.0)
        est = make_estimate(tt, gp, gq, rng)
        at = M // 2 if M >= 2 else M
        keep = np.r_[np.arange(at), np.arange(at + hole, G)]
        return est, (tt[keep], gp[keep], gq[keep])

    for M in MATCHED_COUNTS:
        if M == 0:                                                     # every estimate stamp lies past the truth
            tt, gp, gq = make_truth(6, rng, 1000.0)
            est = make_estimate(tt + 50.0, gp, gq, rng)
            add("m0", est, (tt, gp, gq))
        else:
            add(f"m{M}", *holed(M))
    # truth ten times denser than the estimate, sparser than it, shorter than it at both ends
    tt, gp, gq = make_truth(400, rng, 2000.0, dt=DT / 10)
    add("dense", make_estimate(tt[::10], gp[::10], gq[::10], rng), (tt, gp, gq))
    tt, gp, gq = make_truth(100, rng, 2000.0)
    add("sparse", make_estimate(tt, gp, gq, rng), (tt[::10], gp[::10], gq[::10]))
    tt, gp, gq = make_truth(60, rng, 2000.0)
    add("short", make_estimate(tt, gp, gq, rng), (tt[10:50], gp[10:50], gq[10:50]))
    # estimate stamps exactly midway between two truth stamps (a tie of the two candidates and of the threshold), and a quarter step off
    tt, gp, gq = make_truth(31, rng, 3000.0)
    et, ep, eq = make_estimate(tt[:30], gp[:30], gq[:30], rng)
    et[3::4] += DT / 2
    et[1::4] += DT / 4
    add("midway", (et, ep, eq), (tt, gp, gq))
    # repeated truth stamps: rows 7, 8 and 20, 21, 22 share a stamp and hold different poses
    tt, gp, gq = make_truth(40, rng, 3000.0)
    est = make_estimate(tt, gp, gq, rng)
    tt = tt.copy(); tt[8] = tt[7]; tt[21] = tt[20]; tt[22] = tt[20]
    add("repeated", est, (tt, gp, gq))
    tt, gp, gq = make_truth(20, rng, 3000.0)
    add("skipped", make_estimate(tt, gp, gq, rng), (tt, gp, gq), skipped=True)
    add("empty", (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 4))), (tt, gp, gq))
    add("no_truth", make_estimate(tt, gp, gq, rng), (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 4))))
    et, ep, eq = make_estimate(tt, gp, gq, rng)
    et[5], et[6] = et[6], et[5]
    add("unsorted", (et, ep, eq), (tt, gp, gq))
    t2 = tt.copy(); t2[9] = np.nan
    add("nan_truth_stamp", make_estimate(tt, gp, gq, rng), (t2, gp, gq))
    # collinear: exactly representable rows on a line, the truth on another line
    k = np.round(rng.uniform(-500, 500, size=33) * 16) / 16
    k.sort()
    tt = 4000.0 + DT * np.arange(33)
    ident = np.tile([0.0, 0.0, 0.0, 1.0], (33, 1))
    add("collinear", (tt, np.c_[k, np.zeros(33), np.zeros(33)] + np.array([3.0, 4.0, 5.0]), ident),
        (tt, np.c_[np.zeros(33), 2.0 * k, np.zeros(33)] + S.OFFSET_N, ident))
    # quaternions: every one scaled (non-unit), a zero and a NaN one on either side, a NaN position on either side
    tt, gp, gq = make_truth(24, rng, 5000.0)
    et, ep, eq = make_estimate(tt, gp, gq, rng)
    eq = eq * 3.7; gq = gq * 0.01
    eq[4] = 0.0; gq[9] = 0.0; eq[12, 2] = np.nan; gq[15, 0] = np.nan; ep[18, 1] = np.nan; gp[20, 2] = np.nan; eq[22] = np.inf
    add("quats", (et, ep, eq), (tt, gp, gq))
    # the estimate is the truth rotated by 1e-12 rad and shifted by 1e-9 m: local coordinates, where 1e-9 m is far above the spacing
    tt, gp, gq = make_truth(20, rng, 6000.0, off=np.zeros(3))
    tiny = _axis_quat([0.3, -0.5, 0.8], 1e-12)
    add("tiny", (tt, gp + np.array([1e-9, 0.0, 0.0]), np.array([_quat_mul(q, tiny) for q in gq])), (tt, gp, gq))
    return tracks, notes


@functools.lru_cache(maxsize=None)
def build_cases():
    """one ragged batch -> dict: ts / pos / quat / offsets, ref_ts / ref_pos / ref_quat / ref_offsets, run_status, B, P, names, notes (name ->
    track number); arrays are read-only"""
    tracks, notes = _build_cases()
    cat = lambda k, j, cols: np.concatenate([t[k][j].reshape((-1,) + cols) for t in tracks])
    c = dict(ts=cat(1, 0, ()), pos=cat(1, 1, (3,)), quat=cat(1, 2, (4,)), ref_ts=cat(2, 0, ()), ref_pos=cat(2, 1, (3,)), ref_quat=cat(2, 2, (4,)),
             offsets=np.concatenate([[0], np.cumsum([len(t[1][0]) for t in tracks])]).astype(np.int64),
             ref_offsets=np.concatenate([[0], np.cumsum([len(t[2][0]) for t in tracks])]).astype(np.int64),
             run_status=np.array([1 if t[3] else 0 for t in tracks], np.int32))
    for v in c.values():
        v.setflags(write=False)
    c.update(B=len(tracks), P=int(c["offsets"][-1]), names=[t[0] for t in tracks], notes=notes)
    return c


def single(c, b):
    """track b of a batch as a batch of its own"""
    lo, hi, glo, ghi = c["offsets"][b], c["offsets"][b + 1], c["ref_offsets"][b], c["ref_offsets"][b + 1]
    return dict(ts=c["ts"][lo:hi], pos=c["pos"][lo:hi], quat=c["quat"][lo:hi], ref_ts=c["ref_ts"][glo:ghi], ref_pos=c["ref_pos"][glo:ghi],
                ref_quat=c["ref_quat"][glo:ghi], offsets=np.array([0, hi - lo], np.int64), ref_offsets=np.array([0, ghi - glo], np.int64),
                run_status=c["run_status"][b:b + 1], B=1, P=int(hi - lo), names=[c["names"][b]], notes={c["names"][b]: 0})


@functools.lru_cache(maxsize=None)
def reference(assoc, align):
    """the yardstick of build_cases() under its own fit, with the pairs of SCENARIOS and the pair errors of TRACED: computed once per
    process and shared; treat it as read-only"""
    return tuple(evaluate(build_cases(), assoc, align, SCENARIOS, TRACED))
