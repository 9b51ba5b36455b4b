"""CPU tier of the Sim3 yardstick tests (tests/sim3_ref.py): the oracle and the host builds of the product's fit arithmetic against the
50-digit restatement of compute_sim3_transform, under gates that follow from each set's own conditioning instead of a flat tolerance.

    test_oracle_against_the_yardstick   measures the oracle on every case and pins the C constants of sim3_ref (8 x the worst ratio)
    test_host_routes_hold_the_gates     umeyama_finalize (Jacobi SVD) and umeyama_finalize<true> (polar iteration) of gsf_math.hpp on two-pass
                                        centred moments, and on the one-pass moments shifted by the first usable row (the arithmetic of the
                                        short-set, window and pipeline reductions; their bound is the yardstick's *_shift one)
    test_fallback_bit_*                 SIM3_FLAG_SVD_FALLBACK == the polar route declined, and on the mirrored ladder exactly past 0.70
    test_shift_by_the_last_row_*        the gates have teeth: the same arithmetic shifted by the LAST row misses them on the outlier-last twins
    test_header_claims_of_gsf_math      the figures quoted in the header comments of umeyama_rotation_polar, re-measured in 50 digits

Every test prints, per route, the worst ratio to each bound before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_ref as S
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
FALLBACK = S.SIM3_FLAG_SVD_FALLBACK
ORTH_GATE = 2.0                         # R^T R - I and det R - 1 in units of 16 u: V U^T of two matrices orthonormal to a few u each (<= 32 u)


@pytest.fixture(scope="module")
def hh():
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libhost_harness_sim3.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_harness.cpp")])
    L = C.CDLL(so)
    for fn in (L.hh_umeyama, L.hh_umeyama_polar):
        fn.restype = C.c_int
        fn.argtypes = [f64p, f64p, C.c_int64, f64p, f64p, C.POINTER(C.c_double)]
    L.hh_umeyama_shifted.restype = C.c_int
    L.hh_umeyama_shifted.argtypes = [f64p, f64p, C.c_void_p, C.c_int64, C.c_int, C.c_int, f64p, f64p, C.POINTER(C.c_double)]
    L.hh_polar_applies.restype = C.c_int
    L.hh_polar_applies.argtypes = [f64p]
    L.hh_polar_rotation.restype = C.c_int
    L.hh_polar_rotation.argtypes = [f64p, f64p, C.POINTER(C.c_double)]
    L.hh_svd_rotation.restype = None
    L.hh_svd_rotation.argtypes = [f64p, f64p, C.POINTER(C.c_double)]
    return L


@pytest.fixture(scope="module")
def cases():
    return S.cases()


class Worst:
    """the worst ratio per gated quantity of one route, and the misses"""
    def __init__(self, route):
        self.route, self.worst, self.misses = route, {}, []

    def add(self, name, r, gates=S.gate_of):
        for k, v in r.items():
            if not v <= self.worst.get(k, (0.0, ""))[0]:
                self.worst[k] = (v, name)
            g = ORTH_GATE if k in ("det", "orth") else gates(k)
            if not v <= g:
                self.misses.append((name, k, f"{v:.3g} x bound, gate {g:.3g}"))

    def report(self):
        print(f"{self.route}: " + ", ".join(f"{k} {v:.3g} x bound ({n})" for k, (v, n) in sorted(self.worst.items())))


def _two_pass(fn, c):
    a, b = S.usable_rows(c["src"], c["dst"], c["mask"])
    R, t, s = np.full((3, 3), np.nan), np.full(3, np.nan), C.c_double(np.nan)
    with np.errstate(invalid="ignore"):
        rc = fn(np.ascontiguousarray(a), np.ascontiguousarray(b), len(a), R, t, C.byref(s))
    return rc, R, t, s.value


def _shifted(hh, c, polar, last=False):
    R, t, s = np.full((3, 3), np.nan), np.full(3, np.nan), C.c_double(np.nan)
    m = None if c["mask"] is None else np.ascontiguousarray(c["mask"]).ctypes.data
    rc = hh.hh_umeyama_shifted(np.ascontiguousarray(c["src"]), np.ascontiguousarray(c["dst"]), m, len(c["src"]), int(polar), int(last), R, t, C.byref(s))
    return rc, R, t, s.value


def test_case_list(cases):
    n, rows = S.totals()
    opened = [c["name"] for c in cases if c["y"].cls.endswith("open")]
    print(f"{n} cases, {rows} rows; open: {opened}; NONE: {[c['name'] for c in cases if c['y'].status == S.SIM3_NONE]}")
    assert sorted(opened) == sorted(S.OPEN_CASES) and n >= 130 and rows <= 30000
    assert {len(c["src"]) for c in cases} >= set(S.LENGTHS)
    for c in cases:                                                       # every outlier-first case has its twin
        if c.get("twin"):
            assert S.case(c["twin"])["twin"] == c["name"]


def test_oracle_against_the_yardstick(cases):
    """The oracle (float64, two-pass centring, LAPACK-class SVD) on every case: status words equal to the yardstick's, worst ratio to each
    bound.  The written constants of sim3_ref must cover what is measured here, and the gates must be 8 x them."""
    w = Worst("oracle")
    for c in cases:
        y = c["y"]
        a, b = S.usable_rows(c["src"], c["dst"], c["mask"])
        with np.errstate(invalid="ignore"):
            R, t, s, fl = orc.compute_sim3_transform(a, b, return_flags=True)
        assert fl == y.status, (c["name"], fl, y.status)
        if fl != S.SIM3_NONE:
            w.add(c["name"], S.ratios(y, c["src"], c["dst"], c["mask"], R, t, s))
    w.report()
    assert w.worst["R"][0] <= S.ORACLE_WORST_R and w.worst["s"][0] <= S.ORACLE_WORST_S and w.worst["img"][0] <= S.ORACLE_WORST_IMG, w.worst
    # ... and not far below it either: the written figures are measurements, not allowances
    assert w.worst["R"][0] > 0.8 * S.ORACLE_WORST_R and w.worst["s"][0] > 0.8 * S.ORACLE_WORST_S and w.worst["img"][0] > 0.8 * S.ORACLE_WORST_IMG, w.worst
    assert (S.C_R, S.C_S, S.C_IMG) == (8 * S.ORACLE_WORST_R, 8 * S.ORACLE_WORST_S, 8 * S.ORACLE_WORST_IMG)
    assert not w.misses, w.misses


ROUTES = {
    "two-pass + Jacobi SVD (hh_umeyama)": (lambda hh, c: _two_pass(hh.hh_umeyama, c), False, False),
    "two-pass + polar (hh_umeyama_polar)": (lambda hh, c: _two_pass(hh.hh_umeyama_polar, c), False, True),
    "shifted one-pass + Jacobi SVD": (lambda hh, c: _shifted(hh, c, False), True, False),
    "shifted one-pass + polar": (lambda hh, c: _shifted(hh, c, True), True, True),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_host_routes_hold_the_gates(hh, cases, route):
    fn, shifted, polar = ROUTES[route]
    w = Worst(route)
    for c in cases:
        y = c["y"]
        rc, R, t, s = fn(hh, c)
        assert (rc & ~FALLBACK) == y.status and (polar or not rc & FALLBACK), (c["name"], rc, y.status)
        if y.status == S.SIM3_NONE:
            continue
        w.add(c["name"], S.ratios(y, c["src"], c["dst"], c["mask"], R, t, s, shifted=shifted))
    w.report()
    assert not w.misses, w.misses


def test_fallback_bit_is_the_polar_predicate(hh, cases):
    """FALLBACK == not hh_polar_applies(H) on every case; where the yardstick decides the predicate in 50 digits clear of its switches,
    both equal that; on the mirrored ladder the SVD takes over exactly past sigma3 / sigma2 = 0.70"""
    took = 0
    for c in cases:
        y = c["y"]
        if y.status == S.SIM3_NONE:
            continue
        a, b = S.usable_rows(c["src"], c["dst"], c["mask"])
        H = np.ascontiguousarray((a - a.mean(0)).T @ (b - b.mean(0)))
        rc = _two_pass(hh.hh_umeyama_polar, c)[0]
        applies = bool(hh.hh_polar_applies(H))
        assert bool(rc & FALLBACK) == (not applies), c["name"]
        if y.cls == "determined":                                         # (an open case sits AT the singular test by construction)
            assert applies == y.polar, (c["name"], y.q, y.det2)
        if c["ladder"]:
            assert applies == (c["e"] < 0.70), c["name"]
        took += applies
    assert took > 100


def test_shift_by_the_last_row_misses_the_gates(hh, cases):
    """What the twins are for: the one-pass arithmetic shifted by the set's LAST row misses the gates on the outlier-last twins, whose bound
    -- written with the first row as the shift -- is that of a harmless set.  Asserted where the outlier is a source pose 1e4 / 1e5 m off in
    a set of 200 rows or more (measured: R 6 ... 65 x, scale 92 ... 382 x the bound; gates 24.8 / 60.8).  A fix 1.5 km off moves the error
    by 7 x at the most and the 50-row sets by 3 ... 60 x: inside the factor of 8 that the gates leave, so those twins are printed only."""
    caught = []
    for c in cases:
        if not c.get("twin"):
            continue
        rc, R, t, s = _shifted(hh, c, False, last=True)
        r = S.ratios(c["y"], c["src"], c["dst"], c["mask"], R, t, s, shifted=True)
        missed = any(v > S.gate_of(k) for k, v in r.items())
        print(f"{c['name']}: shifted by the last row: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()) + ("  <-- misses" if missed else ""))
        if c["where"] == "last" and "-fix-" not in c["name"] and len(c["src"]) >= 200:
            assert missed, (c["name"], r)
            caught.append(c["name"])
        if c["where"] == "first":                                         # ... and there the last row is a harmless shift
            assert not missed, (c["name"], r)
    assert len(caught) == 6, caught


def _track_shaped(rng):
    n = int(rng.integers(8, 400)); tt = np.linspace(0, 1, n); curv = rng.uniform(0.02, 3.0)
    vert = 10.0 ** rng.uniform(-7, 0.5)
    src = np.c_[np.cumsum(np.sin(curv * tt) * 1.4), vert * rng.normal(size=n), np.cumsum(np.cos(curv * tt) * 1.4)]
    th = rng.uniform(0, 2 * np.pi)
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) @ np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    dst = rng.uniform(0.5, 2.0) * src @ Rz.T + np.array([4.5e5, 5.4e6, 100.0]) + rng.normal(size=src.shape) * 0.45
    return np.ascontiguousarray((src - src.mean(0)).T @ (dst - dst.mean(0)))


# the figures the header of umeyama_rotation_polar (gsf_math.hpp) quotes; measured here, 400 + 400 + 240 matrices
POLAR_CLAIM = 7.1                       # |Q - Q_true| <= 7.1e-15 without a reflection (measured 7.05e-15; the Jacobi SVD route 8.4e-15, NumPy's SVD 6.9e-13)
REFLECT_CLAIM = 3.3                     # |R - R_true| (1 - sigma3 / sigma2) <= 3.3e-15 with one, sigma3 / sigma2 up to 0.70 (measured 3.25e-15)


def test_header_claims_of_gsf_math(hh):
    """umeyama_rotation_polar against the 50-digit polar factor (reflection fix included) of the same float64 H: 400 track-shaped H (the
    vertical direction is noise; about half have det H < 0) and 240 mirrored clouds with sigma3 / sigma2 from 1e-4 to 0.70; the Jacobi
    SVD route on the same matrices for comparison.  The reflected direction is conditioned like 1 / (sigma2 - sigma3) relative to sigma2,
    so its figure is quoted times (1 - sigma3 / sigma2)."""
    rng = np.random.default_rng(3)
    Hs = [_track_shaped(rng) for _ in range(400)]
    for e in np.r_[10.0 ** rng.uniform(-4, -0.5, 120), rng.uniform(0.3, 0.70, 120)]:
        n = 60
        src = rng.normal(size=(n, 3)); src -= src.mean(0)
        Qs, _ = np.linalg.qr(src)
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Hs.append(np.ascontiguousarray((Qs * [30.0, 3.0, 3.0]).T @ ((Qs * [30.0, 3.0, -3.0 * e]) @ Q.T) * n))
    worst = {"plain": 0.0, "reflected": 0.0, "svd plain": 0.0, "svd reflected": 0.0, "numpy": 0.0}
    n_plain = n_refl = declined = 0
    cond = [np.inf, 0.0]
    for H in Hs:
        Rt, sig, d = S.polar_factor(H)
        R, tr = np.full((3, 3), np.nan), C.c_double()
        ok = hh.hh_polar_rotation(H, R, C.byref(tr))
        R2, tr2 = np.empty((3, 3)), C.c_double()
        hh.hh_svd_rotation(H, R2, C.byref(tr2))
        e = sig[2] / sig[1]
        f = (1.0 - e) if d < 0 else 1.0
        key = "reflected" if d < 0 else "plain"
        worst["svd " + key] = max(worst["svd " + key], float(np.abs(R2 - Rt).max()) * f)
        if d < 0 and e > 0.69:
            continue
        if not ok:                                                        # only what the routine says it declines: sigma3 < 1e-14 sigma1
            assert sig[2] < 1.1e-14 * sig[0], sig
            declined += 1
            continue
        Un, _, Vn = np.linalg.svd(H)
        if np.linalg.det(Vn.T @ Un.T) < 0:
            Vn[-1] *= -1
        worst["numpy"] = max(worst["numpy"], float(np.abs(Vn.T @ Un.T - Rt).max()) * f)
        assert abs(tr.value - sig.sum()) <= 8 * S.U * sig.sum()
        worst[key] = max(worst[key], float(np.abs(R - Rt).max()) * f)
        n_plain += d > 0; n_refl += d < 0
        cond = [min(cond[0], sig[0] / sig[2]), max(cond[1], sig[0] / sig[2])]
    print(f"umeyama_rotation_polar against the 50-digit factor: {n_plain} plain |R - R_true| <= {worst['plain']:.3g}, {n_refl} reflected "
          f"|R - R_true| (1 - e) <= {worst['reflected']:.3g}; sigma1 / sigma3 from {cond[0]:.3g} to {cond[1]:.3g}; {declined} declined; "
          f"Jacobi SVD route: {worst['svd plain']:.3g} / {worst['svd reflected']:.3g}; NumPy's SVD: {worst['numpy']:.3g}")
    assert n_plain > 150 and n_refl > 300 and declined <= 2
    assert worst["plain"] <= POLAR_CLAIM * 1e-15 and worst["reflected"] <= REFLECT_CLAIM * 1e-15, worst
