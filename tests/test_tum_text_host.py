"""CPU tier of step 7's text (gps_optimize_slam_amd/csrc/gsf_text.hpp): the routine gsf_tum_text_dev runs on the device, compiled with g++
into a test-only harness (tests/host_text_harness.cpp), against Python's '%.{p}f' -- what np.savetxt writes (EKFGPSSLAM.py:1091-1092,
:1098-1101) -- byte for byte, for p = 3, 6, 8 over more than 10^6 values each: random bit patterns of every exponent below 2^63, exact ties
k / 2^j, values a few ulp around decimal midpoints, signed zeros, negatives that round to zero, subnormals, NaN payloads of both signs,
infinities, values about 2^63 and the flag above it.  Whole rows: the length routine == len(fmt % row), and the text == np.savetxt."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
STRIDE = 32
UTM_FMT = ["%.6f"] + ["%.6f"] * 3 + ["%.8f"] * 4
WGS_FMT = ["%.6f"] + ["%.8f", "%.8f", "%.3f"] + ["%.8f"] * 4
HEADERS = ("timestamp x y z qx qy qz qw (UTM)", "timestamp lon lat alt qx qy qz qw (WGS84)")


@pytest.fixture(scope="module")
def ht():
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libhost_text_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, os.path.join(HERE, "host_text_harness.cpp")])
    L = C.CDLL(so)
    L.ht_fixed.restype = None
    L.ht_fixed.argtypes = [f64p, C.c_int64, C.c_int, u8p, C.c_int64, i64p]
    L.ht_row_lens.restype = None
    L.ht_row_lens.argtypes = [C.c_int, f64p, C.c_int64, i64p]
    L.ht_rows_text.restype = C.c_int64
    L.ht_rows_text.argtypes = [C.c_int, f64p, C.c_int64, u8p]
    return L


def fixed(ht, x, p):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros((x.size, STRIDE), np.uint8)
    lens = np.empty(x.size, np.int64)
    ht.ht_fixed(x, x.size, p, out.reshape(-1), STRIDE, lens)
    return out, lens


def check_fixed(ht, x, p):
    """every value with |x| < 2^63 (or not finite) printed as Python prints it; the others flagged"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out, lens = fixed(ht, x, p)
    big = np.isfinite(x) & (np.abs(x) >= 2.0 ** 63)
    np.testing.assert_array_equal(lens == -1, big)
    ok = ~big
    fmt = f"%.{p}f"
    want = "\n".join(fmt % v for v in x[ok].tolist()).encode()
    got = b"\n".join(bytes(r[:n]) for r, n in zip(out[ok], lens[ok]))
    if got != want:
        w, g = want.split(b"\n"), got.split(b"\n")
        bad = [i for i in range(len(w)) if w[i] != g[i]]
        xs = x[ok]
        raise AssertionError(f"p={p}: {len(bad)} fields differ, e.g. {xs[bad[0]]!r}: got {g[bad[0]]!r}, want {w[bad[0]]!r}")
    return int(ok.sum())


def random_bits(rng, n):
    """random bit patterns of every exponent whose value is below 2^63 (biased exponent < 1086), both signs"""
    mant = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    exp = rng.integers(0, 1086, n, dtype=np.uint64)
    sign = rng.integers(0, 2, n, dtype=np.uint64)
    return ((sign << np.uint64(63)) | (exp << np.uint64(52)) | mant).view(np.float64)


def ties(rng, n):
    """exact ties and their neighbours: k / 2^j with j up to 40, i.e. values whose binary fraction ends exactly at or near a half"""
    j = rng.integers(1, 41, n)
    k = rng.integers(0, 1 << 40, n).astype(np.float64)
    x = np.ldexp(k, -j)
    return np.concatenate([x, -x])


def midpoints(rng, p, n):
    """±1-3 ulp about decimal midpoints d + 0.5 * 10^-p (9.9999995, 0.0078125-like values and large magnitudes)"""
    scale = 10 ** p
    mag = rng.integers(0, 8, n)
    d = rng.integers(0, 10 ** 6, n).astype(np.float64) * (10.0 ** mag) + rng.integers(0, scale, n) / scale
    mid = d + 0.5 / scale
    out = [mid]
    for u in (1, 2, 3):
        up, dn = mid.copy(), mid.copy()
        for _ in range(u):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        out += [up, dn]
    x = np.concatenate(out)
    return np.concatenate([x, -x])


def specials(rng):
    nan_payloads = rng.integers(1, 1 << 52, 2000, dtype=np.uint64) | np.uint64(0x7FF0000000000000)
    nans = np.concatenate([nan_payloads, nan_payloads | np.uint64(1 << 63)]).view(np.float64)
    sub = rng.integers(1, 1 << 52, 2000, dtype=np.uint64).view(np.float64)
    tiny = rng.random(2000) * 10.0 ** -rng.integers(4, 300, 2000)
    near63 = np.ldexp(1.0, 63) * (1 - rng.random(2000) * 1e-6)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 9.9999995, 0.0078125, 0.5e-6, 0.5e-8, 0.5e-3, 2.0 ** 63, -(2.0 ** 63),
                     np.nextafter(2.0 ** 63, 0), -np.nextafter(2.0 ** 63, 0), 1e300, -1e300, np.finfo(np.float64).max, 5e-324, -5e-324,
                     2.0 ** 53, 2.0 ** 53 + 2, 0.9999999999, 99.9995, 0.0005, 0.0015, 0.0025, 1.0005])
    big = np.ldexp(1.0 + rng.random(2000), rng.integers(63, 1024, 2000))
    return np.concatenate([nans, sub, -sub, tiny, -tiny, near63, -near63, edge, big, -big])


@pytest.mark.parametrize("p", [3, 6, 8])
def test_fields_match_python_percent_format(ht, p):
    rng = np.random.default_rng(1000 + p)
    n = 0
    n += check_fixed(ht, random_bits(rng, 600_000), p)
    n += check_fixed(ht, ties(rng, 150_000), p)
    n += check_fixed(ht, midpoints(rng, p, 30_000), p)
    n += check_fixed(ht, specials(rng), p)
    # the magnitudes a run produces: stamps, UTM metres, degrees, unit quaternions
    vals = np.concatenate([rng.uniform(1.2e9, 1.8e9, 50_000), rng.uniform(-1e7, 1e7, 50_000), rng.uniform(-180, 180, 50_000),
                           rng.uniform(-1, 1, 50_000)])
    n += check_fixed(ht, vals, p)
    assert n >= 1_000_000


def test_documented_cases(ht):
    cases = {(9.9999995, 6): b"9.999999", (0.0078125, 6): b"0.007812", (-0.0, 6): b"-0.000000", (-1e-9, 6): b"-0.000000",
             (float("nan"), 8): b"nan", (-float("nan"), 3): b"nan", (float("inf"), 6): b"inf", (-float("inf"), 6): b"-inf",
             (5e-324, 8): b"0.00000000", (0.0005, 3): b"0.001", (0.0015, 3): b"0.002", (2.0 ** 62, 3): b"4611686018427387904.000"}
    for (x, p), want in cases.items():
        out, lens = fixed(ht, [x], p)
        assert bytes(out[0, :lens[0]]) == want, (x, p)
    assert fixed(ht, [2.0 ** 63], 6)[1][0] == -1 and fixed(ht, [-1e300], 8)[1][0] == -1


@pytest.mark.parametrize("form", [0, 1])
def test_rows_match_savetxt(ht, form):
    rng = np.random.default_rng(7 + form)
    n = 20_000
    rows = np.column_stack([rng.uniform(1.2e9, 1.8e9, n), rng.uniform(-5e5, 5e6, n), rng.uniform(-1e7, 1e7, n), rng.uniform(-500, 9000, n),
                            rng.normal(size=(n, 4))])
    pick = rng.random(rows.shape) < 0.02
    rows[pick] = random_bits(rng, int(pick.sum()))
    rows[rng.random(rows.shape) < 0.002] = -0.0
    rows[5, 2], rows[6, 7], rows[7, 0] = np.nan, -np.inf, 1e-300
    fmt = UTM_FMT if form == 0 else WGS_FMT
    lens = np.empty(n, np.int64)
    ht.ht_row_lens(form, rows, n, lens)
    line = " ".join(fmt) + "\n"
    np.testing.assert_array_equal(lens, [len(line % tuple(r)) for r in rows.tolist()])
    buf = np.zeros(int(lens.sum()) + 64, np.uint8)
    m = ht.ht_rows_text(form, rows, n, buf)
    f = io.BytesIO()
    np.savetxt(f, rows, fmt=fmt, header=HEADERS[form], comments="")
    assert bytes(buf[:m]) == f.getvalue()
    # a row with a finite |x| >= 2^63 is flagged, not printed
    rows[3, 4] = 2.0 ** 64
    ht.ht_row_lens(form, rows, n, lens)
    assert lens[3] == -1 and (np.delete(lens, 3) > 0).all()
    # 0 rows: the header alone, as np.savetxt writes it for a (0, 8) array
    f = io.BytesIO()
    np.savetxt(f, np.zeros((0, 8)), fmt=fmt, header=HEADERS[form], comments="")
    assert ht.ht_rows_text(form, rows[:0], 0, buf) == len(f.getvalue()) and bytes(buf[:len(f.getvalue())]) == f.getvalue()
