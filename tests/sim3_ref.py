"""The yardstick of the Umeyama / Sim3 fits (compute_sim3_transform, EKFGPSSLAM.py:428-459) and the point sets both tiers run.  Never
imports the product and holds no test functions.

Values.  yardstick(): lines :436-451 restated in 50-digit arithmetic (mpmath) on the stored float64 inputs and rounded once to float64:
centroids, centred rows, H = sum a_i b_i^T, mp.svd_r(H), R = Vt^T U^T, the last row of Vt negated if det(R) < 0 (d = -1), scale =
(sigma1 + sigma2 + sigma3) / sum |a_i|^2 -- as :444 is written: after the flip det(R) = +1, so the sum carries +sigma3, NOT the textbook
sigma1 + sigma2 - sigma3 -- with var_src < 1e-12 -> scale 1 (VAR0), scale <= 1e-6 -> scale 1 (SMALL_SCALE), fewer than 3 usable rows or an
unmasked non-finite row -> NONE.

Bounds (all from the inputs, in 50 digits; u = 2^-53, a_i / b_i the centred rows, A = sum |a_i| |b_i|):
    bR   = u A / (sigma2 + d sigma3)                      first-order error of R for inputs rounded to float64 products
    bs   = u A / (sigma1 + sigma2 + sigma3) + u           relative error of the scale
    bimg = (bR + bs) s max|a_i| + 4 u max|dst_i|          error of the image s R src_i + t of a row (how t is checked)
    bR_shift = u sum |src_i - src_0| |dst_i - dst_0| / (sigma2 + d sigma3), src_0 / dst_0 the FIRST USABLE ROW: what a reduction can hold
               that accumulates raw moments of the rows shifted by that row (H = Sab - n ma mb^T) -- the short-set path of
               umeyama_batch_kernel and the equal-size-window kernels.  bs_shift / bimg_shift likewise.
A gate is C x bound; the C constants are measured on the oracle (float64 restatement, LAPACK-class SVD, two-pass centring) over cases()
by tests/test_sim3_yardstick_host.py: 8 x the worst ratio seen.  A device reduction adds in another order with other contractions, which
moves the rounding error by a small factor; a cancellation defect moves it by 20 x and more.

Classes.  determined: R, s and the image are gated.  reflection-open (sigma3 <= 1e-13 sigma1: exactly planar clouds, three rows): the
sign the reference's SVD picks is arbitrary -- R against the nearer of the d = +1 / d = -1 candidates, s, |det R - 1|.  rotation-open
(sigma2 + d sigma3 <= 1e-9 sigma1: collinear rows): s, R^T R = I, det R = +1 and the image along the first singular direction.  Only the
cases named in OPEN_CASES may be open; cases() asserts that, and that no case sits within 10 % of a switch it is not built to probe."""
import functools

import numpy as np

DPS = 50
U = 2.0 ** -53
SEED = 20250702

SIM3_OK, SIM3_NONE, SIM3_FLAG_VAR0, SIM3_FLAG_SMALL_SCALE, SIM3_FLAG_SVD_FALLBACK = 0, 1, 2, 4, 16

OFFSET_N = np.array([4.5e5, 5.4e6, 100.0])          # a UTM-sized offset, northern hemisphere
OFFSET_S = np.array([4.5e5, 9.4e6, 100.0])          # southern hemisphere (false northing 1e7)

REFL_OPEN = 1e-13                                   # sigma3 / sigma1
ROT_OPEN = 1e-9                                     # (sigma2 + d sigma3) / sigma1
POLAR_SWITCHES = (3e-3, 0.3, 0.47)                  # umeyama_rotation_polar: e0 / nc20 against these (det H < 0 only)
POLAR_SINGULAR = 1e-28                              # det^2 > 1e-28 nc2, else the SVD
LENGTHS = (3, 4, 15, 16, 17, 31, 32, 33, 50, 63, 64, 65, 255, 256, 257, 271, 700)
LADDER = (1e-4, 2e-3, 4e-3, 0.1, 0.25, 0.35, 0.5, 0.8)   # sigma3 / sigma2 of the mirrored clouds; the polar route hands over past 0.70

# ---- gates: measured by tests/test_sim3_yardstick_host.py::test_oracle_against_the_yardstick (2026-10-19, 138 cases, 19 001 rows): the
# worst ratio of the oracle's error to the bound was 3.01 for R (tiny-271), 7.50 for the scale (curve-256), 3.50 for the image (walk-700)
ORACLE_WORST_R, ORACLE_WORST_S, ORACLE_WORST_IMG = 3.1, 7.6, 3.6
C_R, C_S, C_IMG = 8 * ORACLE_WORST_R, 8 * ORACLE_WORST_S, 8 * ORACLE_WORST_IMG


def _mp():
    import mpmath
    return mpmath


class Fit:
    """the yardstick's answer for one point set (see yardstick())"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def usable_rows(src, dst, mask):
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    keep = np.ones(len(src), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    return src[keep], dst[keep]


def _rot(mp, U_, Vt, flip):
    V = Vt.T.copy()
    if flip:
        for r in range(3):
            V[r, 2] = -V[r, 2]
    return V * U_.T


def yardstick(src, dst, mask=None):
    """-> Fit: status (SIM3_NONE, or the flag bits), R (3,3), t (3,), s float64 (None where NONE), sigma (3,), d (+1 / -1), cls,
    R_alt (the other reflection candidate), u1 / v1 (first singular direction in the source / destination space), bR, bs, bimg, bimg1 (the
    image along v1: bR replaced by u A / sigma1), bR_shift, bs_shift, bimg_shift, q = e0 / nc20 of umeyama_rotation_polar, polar (whether
    that routine accepts H, decided in 50 digits), n"""
    mp = _mp()
    a_, b_ = usable_rows(src, dst, mask)
    n = len(a_)
    if n < 3 or not (np.isfinite(a_).all() and np.isfinite(b_).all()):
        return Fit(status=SIM3_NONE, R=None, t=None, s=None, n=n, cls="none", polar=False)
    with mp.workdps(DPS):
        S = [[mp.mpf(float(v)) for v in row] for row in a_]
        D = [[mp.mpf(float(v)) for v in row] for row in b_]
        sc = [mp.fsum(r[k] for r in S) / n for k in range(3)]
        dc = [mp.fsum(r[k] for r in D) / n for k in range(3)]
        A = [[r[k] - sc[k] for k in range(3)] for r in S]
        Bc = [[r[k] - dc[k] for k in range(3)] for r in D]
        H = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                H[r, c] = mp.fsum(x[r] * y[c] for x, y in zip(A, Bc))
        na = [mp.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2) for x in A]
        nb = [mp.sqrt(y[0] ** 2 + y[1] ** 2 + y[2] ** 2) for y in Bc]
        ssq = mp.fsum(v * v for v in na)
        Asum = mp.fsum(x * y for x, y in zip(na, nb))
        # the same sum with the first usable row as the origin (the shifted raw-moment reductions)
        As = mp.fsum(mp.sqrt(sum((x[k] - S[0][k]) ** 2 for k in range(3))) * mp.sqrt(sum((y[k] - D[0][k]) ** 2 for k in range(3))) for x, y in zip(S, D))
        amax_s = max(mp.sqrt(sum((x[k] - S[0][k]) ** 2 for k in range(3))) for x in S)
        U_, Sv, Vt = mp.svd_r(H)
        sig = [Sv[i] for i in range(3)]
        R0 = _rot(mp, U_, Vt, False)
        flip = mp.det(R0) < 0
        d = -1 if flip else 1
        R, R_alt = _rot(mp, U_, Vt, flip), _rot(mp, U_, Vt, not flip)
        tr = sig[0] + sig[1] + sig[2]                                   # :444 with det(R) = +1 after the flip
        var = ssq / n
        flags = SIM3_OK
        if var < mp.mpf("1e-12"):
            s, flags = mp.mpf(1), flags | SIM3_FLAG_VAR0
        else:
            s = tr / (n * var)
            if s <= mp.mpf("1e-6"):
                s, flags = mp.mpf(1), flags | SIM3_FLAG_SMALL_SCALE
        t = [dc[r] - s * sum(R[r, c] * sc[c] for c in range(3)) for r in range(3)]
        u = mp.mpf(2) ** -53
        gap = sig[1] + d * sig[2]
        inf = mp.mpf("1e300")
        amax = max(na)
        dmax = max(max(abs(v) for v in row) for row in D)
        bR = u * Asum / gap if gap > 0 else inf
        bR1 = u * Asum / sig[0] if sig[0] > 0 else inf
        bs = (u * Asum / tr if tr > 0 else inf) + u
        bRs = u * As / gap if gap > 0 else inf
        bss = (u * As / tr if tr > 0 else inf) + u
        if flags:                                                         # the scale is the constant 1: nothing to lose
            bs = bss = u
        if sig[0] == 0:
            cls = "rotation-open"
        elif gap <= mp.mpf(ROT_OPEN) * sig[0]:
            cls = "rotation-open"
        elif sig[2] <= mp.mpf(REFL_OPEN) * sig[0]:
            cls = "reflection-open"
        else:
            cls = "determined"
        # the quantities umeyama_rotation_polar switches on: X0 = H / |H|_F, e0 = |det X0|, nc20 = |cof X0|_F^2
        nh = mp.sqrt(mp.fsum(H[r, c] ** 2 for r in range(3) for c in range(3)))
        q = det2 = None
        polar = False
        if nh > 0:
            s1, s2, s3 = (v / nh for v in sig)
            nc2 = (s1 * s2) ** 2 + (s1 * s3) ** 2 + (s2 * s3) ** 2
            e0 = s1 * s2 * s3
            q = float(e0 / nc2) if nc2 > 0 else float("inf")
            det2 = float(e0 * e0 / nc2) if nc2 > 0 else 0.0
            polar = bool(det2 > POLAR_SINGULAR and (not flip or q < POLAR_SWITCHES[2]))
        f = lambda M: np.array([[float(M[r, c]) for c in range(3)] for r in range(3)])
        return Fit(status=flags, R=f(R), R_alt=f(R_alt), t=np.array([float(v) for v in t]), s=float(s), sigma=np.array([float(v) for v in sig]),
                   d=d, cls=cls, n=n, u1=np.array([float(U_[r, 0]) for r in range(3)]), v1=np.array([float(Vt[0, c]) for c in range(3)]),
                   bR=float(bR), bs=float(bs), bimg=float((bR + bs) * s * amax + 4 * u * dmax), bimg1=float((bR1 + bs) * s * amax + 4 * u * dmax),
                   bR_shift=float(bRs), bs_shift=float(bss), bimg_shift=float((bRs + bss) * s * amax_s + 4 * u * dmax), q=q, det2=det2, polar=polar)


def polar_factor(H):
    """R = Vt^T U^T of a 3x3 H (its reflection fix included) in 50 digits -> (R float64, sigma, d): the check of umeyama_rotation_polar"""
    mp = _mp()
    with mp.workdps(DPS):
        Hm = mp.matrix([[mp.mpf(float(H[r][c])) for c in range(3)] for r in range(3)])
        U_, Sv, Vt = mp.svd_r(Hm)
        flip = mp.det(_rot(mp, U_, Vt, False)) < 0
        R = _rot(mp, U_, Vt, flip)
        return (np.array([[float(R[r, c]) for c in range(3)] for r in range(3)]), np.array([float(Sv[i]) for i in range(3)]), -1 if flip else 1)


# ---------------------------------------------------------------------------- errors of a result against the yardstick
def ratios(y, src, dst, mask, R, t, s, shifted=False):
    """ratio to its bound of every gated quantity of a result (R (3,3) or (9,), t, s) for a set whose yardstick is y -> dict; the keys
    follow y.cls (see the module text).  shifted: the bounds of the shifted raw-moment reductions."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    a, b = usable_rows(src, dst, mask)
    bR, bs, bimg = (y.bR_shift, y.bs_shift, y.bimg_shift) if shifted else (y.bR, y.bs, y.bimg)
    out = {"s": abs(float(s) - y.s) / (bs * y.s)}
    img = float(s) * a @ R.T + t
    want = y.s * a @ y.R.T + y.t
    if y.cls == "determined":
        out["R"] = float(np.abs(R - y.R).max()) / bR
        out["img"] = float(np.abs(img - want).max()) / bimg
    elif y.cls == "reflection-open":
        out["R"] = min(float(np.abs(R - y.R).max()), float(np.abs(R - y.R_alt).max())) / bR
        out["det"] = abs(float(np.linalg.det(R)) - 1.0) / (16 * U)
    else:
        out["orth"] = float(np.abs(R.T @ R - np.eye(3)).max()) / (16 * U)
        out["det"] = abs(float(np.linalg.det(R)) - 1.0) / (16 * U)
        out["img"] = float(np.abs((img - want) @ y.v1).max()) / y.bimg1
    return out


def gate_of(key):
    """the factor on the bound: C_R / C_S / C_IMG; orthogonality and determinant are held to 16 u themselves (factor 1)"""
    return {"R": C_R, "s": C_S, "img": C_IMG, "det": 1.0, "orth": 1.0}[key]


# ---------------------------------------------------------------------------- point sets
def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def _place(src, R, s, off, noise, rng):
    return s * src @ R.T + off + rng.normal(size=src.shape) * noise


def make_set(kind, n, rng, off=OFFSET_N, **kw):
    """one point set of n rows -> (src, dst).  kinds: walk, curve (vert, refl), road (lat), long, tiny, ladder (e), planar, collinear,
    zerovar, scale (s)"""
    tt = np.linspace(0.0, 1.0, n)
    if kind == "walk":
        src = np.cumsum(rng.normal(size=(n, 3)) * np.array([1.0, 1.0, 0.3]), axis=0)
        return src, _place(src, _rotation(rng), kw.get("s", 1.0), off, 0.05, rng)
    if kind == "curve":                     # a gently curving track whose vertical direction is noise (the fixes carry 0.45 m of it): the sign
        curv, vert = kw.get("curv", 1.5), kw["vert"]                      # of det H is the sign of a noise sum, `mirror` makes it negative by build
        src = np.c_[np.cumsum(np.sin(curv * tt) * 1.4), vert * rng.normal(size=n), np.cumsum(np.cos(curv * tt) * 1.4)]
        th = rng.uniform(0, 2 * np.pi)
        Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) @ np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
        mirror = np.array([1.0, -1.0, 1.0]) if kw.get("mirror") else np.ones(3)
        return src, kw.get("s", 1.0) * (src * mirror) @ Rz.T + off + rng.normal(size=src.shape) * 0.45
    if kind == "road":                      # a straight road: sigma2 / sigma1 ~ (lat / length)^2
        src = np.c_[np.linspace(0, 1000.0, n), kw["lat"] * rng.normal(size=n), kw["lat"] * 0.5 * rng.normal(size=n)]
        return src, _place(src, _rotation(rng), 1.0, off, 0.0, rng)
    if kind == "long":                      # a 100 km track
        src = np.c_[np.cumsum(rng.uniform(0.5, 1.5, n)) * (1e5 / n), np.cumsum(rng.normal(size=n)) * (3e3 / np.sqrt(n)), rng.normal(size=n) * 30.0]
        return src, _place(src, _rotation(rng), 1.0, off, 0.5, rng)
    if kind == "tiny":                      # a 1 mm cloud
        src = rng.normal(size=(n, 3)) * 1e-3 + np.array([12.0, -7.0, 1.5])
        return src, _place(src, _rotation(rng), 1.0, off, 0.0, rng)
    if kind == "ladder":                    # a mirrored cloud with sigma3 / sigma2 = e
        e = kw["e"]
        src = rng.normal(size=(n, 3))
        src -= src.mean(0)
        Qs, _ = np.linalg.qr(src)           # orthonormal columns: the singular values of H are set exactly below
        src = Qs * np.array([30.0, 3.0, 3.0]) * np.sqrt(n)
        dst = 1.3 * (Qs * np.array([30.0, 3.0, -3.0 * e]) * np.sqrt(n)) @ _rotation(rng).T + off
        return src, dst
    if kind == "planar":                    # exactly planar: every z is 0 / a constant, values on a binary grid
        xy = np.round(rng.uniform(-200, 200, size=(n, 2)) * 64) / 64
        src = np.c_[xy, np.zeros(n)]
        dst = np.c_[-xy[:, 1], xy[:, 0], np.zeros(n)] * 2.0 + off
        return src, dst
    if kind == "collinear":                 # exactly collinear, exactly representable
        k = np.round(rng.uniform(-500, 500, size=n) * 16) / 16
        src = np.c_[k, np.zeros(n), np.zeros(n)] + np.array([3.0, 4.0, 5.0])
        dst = np.c_[np.zeros(n), 2.0 * k, np.zeros(n)] + off
        return src, dst
    if kind == "zerovar":                   # every source row the same point
        src = np.tile(np.array([12.5, -3.25, 1.0]), (n, 1))
        return src, off + rng.normal(size=(n, 3))
    if kind == "scale":
        src = rng.normal(size=(n, 3)) * np.array([4e3, 3e3, 1e3])
        return src, _place(src, _rotation(rng), kw["s"], off, 0.0, rng)
    raise ValueError(kind)


def with_outlier(src, dst, which, row):
    """a copy with an outlying row: 'fix' = the GNSS fix 1.5 km off, 'pose4' / 'pose5' = the source pose 1e4 / 1e5 m from the rest, 'both'"""
    src, dst = src.copy(), dst.copy()
    if which in ("fix", "both"):
        dst[row] += np.array([900.0, -1200.0, 0.0])
    if which in ("pose4", "both"):
        src[row] += np.array([6e3, 8e3, 0.0])
    if which == "pose5":
        src[row] += np.array([6e4, 8e4, 0.0])
    return src, dst


MASKS = ("first5", "first17", "second", "nanrow", "few", "nan-unmasked")
MASK_CYCLE = ("first5", "first17", "second", "nanrow", "first17", "first5", "second", "few", "nan-unmasked")     # the k-th set of a batch


def make_mask(src, dst, how):
    """-> (src, dst, mask): first5 / first17 = the first rows masked out (the search for the shift goes past one 16-row trip), second =
    every second row, nanrow = a masked-out row holds NaN, few = fewer than 3 rows left, nan-unmasked = a NaN in a row that counts"""
    n = len(src)
    src, dst, m = src.copy(), dst.copy(), np.ones(n, np.uint8)
    if how == "first5":
        m[:5] = 0
    elif how == "first17":
        m[:17] = 0
    elif how == "second":
        m[1::2] = 0
    elif how == "nanrow":
        m[0] = 0; src[0, 1] = np.nan
        if n > 6:
            m[n // 2] = 0; dst[n // 2] = np.nan
    elif how == "few":
        m[:] = 0; m[[0, n - 1]] = 1
    elif how == "nan-unmasked":
        m[1] = 0; dst[n - 2, 2] = np.nan
    else:
        raise ValueError(how)
    return src, dst, m


# the cases allowed to be open (everything else must come out `determined`), and the cases that probe a switch of the polar route
OPEN_CASES = ("planar-50", "planar-271", "planar-mask", "collinear-64", "collinear-257", "walk-3", "curve-3", "three-left", "zerovar-3", "zerovar-40")


def clear_of_switches(y, ladder=False):
    """is the set at least 10 % away from every switch it is not built to probe?  (the 1e-12 / 1e-6 tests of :445 / :450, the two open
    classes, the singular test and -- for sets with det H < 0 -- the three quotients of umeyama_rotation_polar)"""
    if y.status == SIM3_NONE:
        return True
    far = lambda v, sw: not (0.9 * sw <= v <= 1.1 * sw)
    ok = True
    if y.sigma[0] > 0:
        ok = ok and far(y.sigma[2] / y.sigma[0], REFL_OPEN) and far((y.sigma[1] + y.d * y.sigma[2]) / y.sigma[0], ROT_OPEN)
        if y.cls == "determined":
            ok = ok and far(y.det2, POLAR_SINGULAR)
            if y.d < 0 and not ladder:
                ok = ok and all(far(y.q, sw) for sw in POLAR_SWITCHES)
    return ok


def _build_cases():
    rng = np.random.default_rng(SEED)
    out = []

    def add(name, src, dst, mask=None, y=None, **tags):
        y = y if y is not None else yardstick(src, dst, mask)
        out.append(dict(name=name, src=np.ascontiguousarray(src), dst=np.ascontiguousarray(dst), mask=mask, y=y, **tags))

    def drawn(kind, n, ladder=False, want_d=None, tries=200, **kw):
        """a set of the kind that is clear of the switches (and has the wanted sign of det H): drawn again from the same stream until it is,
        so the list is a function of SEED"""
        for _ in range(tries):
            src, dst = make_set(kind, n, rng, **kw)
            y = yardstick(src, dst)
            if clear_of_switches(y, ladder) and (want_d is None or y.cls != "determined" or y.d == want_d):
                return src, dst, y
        raise AssertionError(f"{kind}-{n}: no draw clear of the switches")

    def put(name, drawn_, **tags):
        add(name, drawn_[0], drawn_[1], y=drawn_[2], **tags)

    for n in LENGTHS:                                                     # random walks, every length, scales 0.2 ... 5
        put(f"walk-{n}", drawn("walk", n, s=[0.2, 0.5, 1.0, 2.0, 5.0][n % 5]), kind="walk")
    verts = [1e-7, 1e-5, 1e-3, 1e-2, 0.1, 0.5, 1.0, 3.0]
    for i, n in enumerate(LENGTHS):                                       # curving tracks, every length, both signs of det H
        for refl in (False, True):
            if n == 3 and refl:
                continue
            v = max(verts[(i + refl) % len(verts)], 3e-11 * n * n)           # (a longer track needs more of it to stay clear of sigma3 = 1e-13 sigma1)
            put(f"curve{'-refl' if refl else ''}-{n}", drawn("curve", n, want_d=-1 if refl else 1, vert=v, mirror=refl and v >= 0.1, curv=[0.3, 1.5, 2.8][i % 3],
                                                             off=OFFSET_S if i % 4 == 3 else OFFSET_N), kind="curve", refl=refl, vert=v)
    for lat, n in ((30.0, 50), (1.0, 64), (0.1, 33), (0.03, 255), (0.014, 271), (0.02, 700)):    # straight roads: sigma2 / sigma1 from 1e-2 down to 2e-9
        put(f"road-{lat:g}-{n}", drawn("road", n, lat=lat), kind="road")
    for n in (50, 257, 700):
        put(f"long-{n}", drawn("long", n, off=OFFSET_S if n == 257 else OFFSET_N), kind="long")
    for n in (16, 65, 271):
        put(f"tiny-{n}", drawn("tiny", n), kind="tiny")
    for e in LADDER:                                                      # mirrored clouds at 60 rows, and at the two lengths the pipeline tests fit
        for n in (60, 65, 271):
            put(f"ladder-{e:g}-{n}", drawn("ladder", n, ladder=True, e=e), kind="ladder", e=e)
    for n in (50, 271):
        add(f"planar-{n}", *make_set("planar", n, rng), kind="planar")
    for n in (64, 257):
        add(f"collinear-{n}", *make_set("collinear", n, rng), kind="collinear")
    for n in (3, 40):
        add(f"zerovar-{n}", *make_set("zerovar", n, rng), kind="zerovar")
    for s in (1e-7, 2e-6):                                                # both sides of :450
        for n in (32, 256):
            put(f"scale-{s:g}-{n}", drawn("scale", n, s=s), kind="scale")
    for s, n in ((0.2, 17), (0.7, 63), (3.0, 255), (5.0, 31)):
        put(f"scale-{s:g}-{n}", drawn("scale", n, s=s, off=OFFSET_S if n == 63 else OFFSET_N), kind="scale")
    # an outlying first usable row, and the twin with the same outlier in the last row
    for which in ("fix", "pose4", "pose5", "both"):
        for n in (50, 200, 257):
            for _ in range(50):                                           # both twins clear of the switches
                base = drawn("curve", n, want_d=1, vert=0.5, curv=1.5)[:2]
                twins = [(where, with_outlier(*base, which, row)) for where, row in (("first", 0), ("last", n - 1))]
                ys = [yardstick(*sd) for _, sd in twins]
                if all(clear_of_switches(y, False) and y.cls == "determined" for y in ys):
                    break
            for (where, (src, dst)), y in zip(twins, ys):
                add(f"outlier-{which}-{where}-{n}", src, dst, y=y, kind="outlier", where=where, twin=f"outlier-{which}-{'last' if where == 'first' else 'first'}-{n}")
    # masks
    for how, n in (("first5", 50), ("first17", 64), ("first17", 257), ("second", 65), ("second", 16), ("nanrow", 33), ("nanrow", 271)):
        src, dst, m = make_mask(*drawn("walk", n)[:2], how)
        add(f"mask-{how}-{n}", src, dst, m, kind="mask")
    src, dst, m = make_mask(*with_outlier(*drawn("curve", 100, want_d=1, vert=0.5)[:2], "pose4", 17), "first17")
    add("mask-first17-outlier-100", src, dst, m, kind="outlier", where="first")           # the first USABLE row is the outlier
    src, dst, m = make_mask(*make_set("planar", 40, rng), "second")
    add("planar-mask", src, dst, m, kind="planar")
    src, dst, m = make_mask(*make_set("walk", 40, rng), "few")
    add("few-left", src, dst, m, kind="none")
    src, dst = make_set("walk", 20, rng)
    m = np.zeros(20, np.uint8); m[[2, 9, 19]] = 1
    add("three-left", src, dst, m, kind="mask")
    src, dst, m = make_mask(*make_set("walk", 50, rng), "nan-unmasked")
    add("nan-unmasked", src, dst, m, kind="none")
    src, dst = make_set("walk", 17, rng); src[4, 0] = np.inf
    add("inf-nomask", src, dst, None, kind="none")
    add("two-rows", *make_set("walk", 2, rng), kind="none")
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """the case list with its yardstick (case["y"]), built and checked once per process; arrays are read-only"""
    cs = _build_cases()
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    for c in cs:
        c["ladder"] = c["kind"] == "ladder"
        for k in ("src", "dst", "mask"):
            if c[k] is not None:
                c[k].setflags(write=False)
    # ---- the generator's self-checks
    opened = [c["name"] for c in cs if c["y"].cls in ("reflection-open", "rotation-open")]
    assert set(opened) <= set(OPEN_CASES), sorted(set(opened) - set(OPEN_CASES))         # only the named cases are open ...
    assert set(OPEN_CASES) <= set(names) and all(n in opened for n in OPEN_CASES), sorted(set(OPEN_CASES) - set(opened))   # ... and they are
    assert 10 * len(opened) <= len(cs), (len(opened), len(cs))
    for c in cs:
        assert (c["kind"] == "none") == (c["y"].status == SIM3_NONE), c["name"]
        assert clear_of_switches(c["y"], c["ladder"]), c["name"]
        if c["ladder"]:                                                   # the rungs are where they were put, and the hand-over is where the header says
            e = c["y"].sigma[2] / c["y"].sigma[1]
            assert abs(e / c["e"] - 1) < 1e-3 and c["y"].d == -1 and c["y"].polar == (c["e"] < 0.70), (c["name"], e, c["y"].q)
        if c["kind"] == "curve" and c["y"].cls == "determined":
            assert (c["y"].d < 0) == c["refl"], c["name"]
        if c["kind"] == "scale":
            assert bool(c["y"].status & SIM3_FLAG_SMALL_SCALE) == (c["name"].startswith("scale-1e-07")), c["name"]
        if c["kind"] == "zerovar":
            assert c["y"].status & SIM3_FLAG_VAR0, c["name"]
    return tuple(cs)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def totals():
    return len(cases()), int(sum(len(c["src"]) for c in cases()))


# ---------------------------------------------------------------------------- the shapes the device entries take
N_SETS = 70                             # 64 sets in block 0 and 6 in block 1 of umeyama_batch_kernel; 17.5 row groups of four windows


@functools.lru_cache(maxsize=None)
def short_batch(masked):
    """70 sets of at most 256 rows from cases() -- every outlier twin, NONE case, open case, scale and ladder rung of that size, and an even
    pick of the rest -- as (names, src, dst, mask or None, offsets, [yardstick]).  masked: the k-th set under make_mask(MASK_CYCLE[k % 9])
    (first5 where it is too short for first17), with its own yardstick."""
    pool = [c for c in cases() if c["mask"] is None and len(c["src"]) <= 256]
    must = [c for c in pool if c["kind"] in ("outlier", "none", "planar", "collinear", "zerovar", "scale") or (c["ladder"] and len(c["src"]) == 60)]
    rest = [c for c in pool if not any(c is m for m in must)]
    rest = [rest[i] for i in np.unique(np.linspace(0, len(rest) - 1, N_SETS - len(must)).round().astype(int))]
    chosen = rest[:3] + must + rest[3:]
    assert len(chosen) == N_SETS, (len(must), len(rest))
    return _pack(chosen, masked)


@functools.lru_cache(maxsize=None)
def long_batch(masked):
    """the same 70 sets with a 257-row set placed in each block of 64 (72 sets: every set then goes the two-pass way)"""
    names = list(short_batch(False)[0])
    chosen = [case(n) for n in names]
    chosen.insert(5, case("walk-257"))
    chosen.insert(66, case("outlier-pose5-first-257"))
    assert len(chosen[:64]) == 64 and max(len(c["src"]) for c in chosen[:64]) == 257 and max(len(c["src"]) for c in chosen[64:]) == 257
    return _pack(chosen, masked)


def _pack(chosen, masked):
    srcs, dsts, masks, ys = [], [], [], []
    for k, c in enumerate(chosen):
        src, dst, m, y = c["src"], c["dst"], np.ones(len(c["src"]), np.uint8), c["y"]
        if masked and len(src) <= 256:
            how = MASK_CYCLE[k % len(MASK_CYCLE)]
            if how == "first17" and len(src) < 24:
                how = "first5"
            if how == "first5" and len(src) < 9:
                how = "second"
            src, dst, m = make_mask(src, dst, how)
            y = yardstick(src, dst, m)
        srcs.append(src); dsts.append(dst); masks.append(m); ys.append(y)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in srcs])]).astype(np.int64)
    return (tuple(c["name"] for c in chosen), np.concatenate(srcs), np.concatenate(dsts), np.concatenate(masks) if masked else None, offs, ys)


@functools.lru_cache(maxsize=None)
def windows(W):
    """70 windows of W rows each: walks, curving tracks of both signs, roads, a 100 km track, 1 mm clouds, the mirrored ladder, planar /
    collinear / zero-variance sets, scales on both sides of :450, the four outliers as first and as last row; windows 56 ... 69 carry a
    mask pattern (the others all ones) -> (src (70,W,3), dst, mask (70,W), [yardstick], [kind])"""
    rng = np.random.default_rng(SEED + W)
    plan = ([("walk", {})] * 6 + [("curve", dict(vert=v, mirror=mr)) for v in (1e-3, 0.1, 1.0) for mr in (False, True)] +
            [("road", dict(lat=l)) for l in (30.0, 1.0, 0.1)] + [("long", {})] * 2 + [("tiny", {})] * 2 + [("ladder", dict(e=e)) for e in LADDER] +
            [("planar", {}), ("collinear", {}), ("zerovar", {})] + [("scale", dict(s=s_)) for s_ in (1e-7, 2e-6, 0.2, 5.0)] +
            [("outlier", dict(which=w_, where=wh)) for w_ in ("fix", "pose4", "pose5", "both") for wh in ("first", "last")])
    plan = plan + [("walk", {})] * (56 - len(plan)) + [("walk", {}), ("curve", dict(vert=0.5, mirror=False))] * 7
    assert len(plan) == N_SETS
    src, dst, mask, ys, kinds = np.empty((N_SETS, W, 3)), np.empty((N_SETS, W, 3)), np.ones((N_SETS, W), np.uint8), [], []
    for k, (kind, kw) in enumerate(plan):
        for _ in range(200):
            if kind == "outlier":
                a, b = with_outlier(*make_set("curve", W, rng, vert=0.5), kw["which"], 0 if kw["where"] == "first" else W - 1)
            else:
                a, b = make_set(kind, W, rng, **kw)
            m = None
            if k >= 56:
                how = MASK_CYCLE[k % len(MASK_CYCLE)]
                if how == "first17" and W < 24:
                    how = "first5"
                if how == "first5" and W < 9:
                    how = "second"
                a, b, m = make_mask(a, b, how)
            y = yardstick(a, b, m)
            if clear_of_switches(y, kind == "ladder"):
                break
        else:
            raise AssertionError((W, k, kind))
        src[k], dst[k] = a, b
        if m is not None:
            mask[k] = m
        ys.append(y); kinds.append(kind + ("-" + kw["where"] if kind == "outlier" else ""))
    for x in (src, dst, mask):
        x.setflags(write=False)
    return src, dst, mask, ys, kinds
