"""CPU tier of the wave kernels' routing table (gps_optimize_slam_amd/csrc/gsf_wave_route.hpp): which of the five kernel families runs for
a call, with which scan sizing, chunk count and LDS table.  The header is compiled with g++ into a test-only harness
(tests/host_route_harness.cpp) and compared, over the full product of options, flags, batch sizes and track lengths below, with a
restatement of the launcher as it was before the table existed (nested conditions in launch_ekf_wave, re-derivations in
launch_ekf_wave_early and launch_ekf_block).  The properties the launchers rely on are asserted on their own as well."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_route_harness.cpp")
OPTS = (-1, 0, 1)
BS = (1, 255, 256, 257, 999, 1000, 1024, 1025, 1536, 2048, 2049, 100000)
NS = (0, 1, 16, 17, 32, 33, 63, 64, 65, 80, 96, 97, 128, 255, 256, 271, 320, 384, 385, 640, 641, 1024, 1025, 4000)
DEFAULTS = dict(block_kernel=-1, duo_kernel=-1, early_variances=-1, tail_scan_stages=1)        # gsf_ctx's initial options
FIELDS = ("block_kernel", "duo_kernel", "early_variances", "tail_scan_stages", "pipeline", "xy", "ragged", "B", "N")


@pytest.fixture(scope="module")
def hr():
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libhost_route_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
    L = C.CDLL(so)
    L.hr_route.restype = None
    L.hr_route.argtypes = [np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), C.c_int64,
                           np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    L.hr_families.argtypes = [np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    d3 = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.hr_xy.argtypes = [d3, d3, d3]
    codes = np.zeros(5, np.int32)
    L.hr_families(codes)
    assert len(set(codes.tolist())) == 5
    L.names = dict(zip(codes.tolist(), ("ONE", "DUO", "EARLY", "BIG", "BLOCK")))
    L.FULL, L.EARLY_CHUNKS = L.hr_tail_full(), L.hr_early_chunks()
    assert L.FULL not in (4, 5, 6) and L.EARLY_CHUNKS >= 1
    return L


def route(hr, calls):
    """wave_route on a list of dicts -> [(family name, tail, nch, pv_stride)]"""
    a = np.array([[int(c[f]) for f in FIELDS] for c in calls], np.int64).reshape(len(calls), 9)
    out = np.full((len(calls), 4), -99, np.int32)
    hr.hr_route(a, len(calls), out)
    return [(hr.names[int(f)], int(t), int(c), int(s)) for f, t, c, s in out]


def tail_stages(N, FULL):
    if N <= 0:
        return 6
    last = (N - 1) & 63
    return FULL if last == 63 else (4 if last < 16 else (5 if last < 32 else 6))


def launched_before(c, FULL, EARLY_CHUNKS):
    """The launcher's nested conditions, restated: (family, tail, nch, pv_stride) of the launch, None where that launch took no such value."""
    B, N, offsets, pipeline, xy = c["B"], c["N"], c["ragged"], c["pipeline"], c["xy"]
    if c["block_kernel"] == 1 and (not offsets and N > 64 and N <= 1024):            # launch_ekf_block: W waves, one per chunk
        return ("BLOCK", None, (N + 63) // 64, None)
    tail = tail_stages(N, FULL) if (c["tail_scan_stages"] != 0 and not offsets) else 6
    duo_k, ev = c["duo_kernel"], c["early_variances"]
    ev_applies = pipeline and xy and not offsets and N > 64 and N <= 384 and B <= 2048
    ev_forced = ev_applies and ev == 1 and duo_k != 1
    ev_auto = (ev_applies and ev == -1 and duo_k != 1 and not (duo_k == -1 and B <= 256) and
               (B >= 1000 and B <= 1024 and N >= 256 and N <= 384))
    if not ev_forced and pipeline and not offsets and duo_k != 0 and N > 64 and N <= 640 and (duo_k == 1 or (duo_k == -1 and B <= 256)):
        return ("DUO", tail, None, (N + 1) & ~1)
    if ev_forced or ev_auto:                                                         # launch_ekf_wave_early: switch (nch), default: 6
        nch = (N + 63) // 64
        return ("EARLY", tail, nch if nch in (2, 3, 4, 5) else 6, 64 * min(EARLY_CHUNKS, nch - 1))
    if not B <= 2048:
        return ("BIG", None, None, None)
    return ("ONE", tail, None, None)


@pytest.fixture(scope="module")
def product(hr):
    calls = []
    for bk, dk, ev, ts, p, x, rg in itertools.product(OPTS, OPTS, OPTS, (0, 1), (0, 1), (0, 1), (0, 1)):
        for B, N in itertools.product(BS, NS):
            calls.append(dict(block_kernel=bk, duo_kernel=dk, early_variances=ev, tail_scan_stages=ts, pipeline=p, xy=x, ragged=rg, B=B,
                              N=0 if rg else N))                                     # the ragged entries pass N = 0
    return calls, route(hr, calls)


def test_table_launches_what_the_nested_conditions_launched(hr, product):
    calls, got = product
    assert len(calls) == 3 ** 3 * 2 ** 4 * len(BS) * len(NS)
    seen = set()
    for c, g in zip(calls, got):
        want = launched_before(c, hr.FULL, hr.EARLY_CHUNKS)
        assert all(w is None or w == v for w, v in zip(want, g)), (c, g, want)
        seen.add(g[0])
    assert seen == {"ONE", "DUO", "EARLY", "BIG", "BLOCK"}


def test_stated_invariants(hr, product):
    for c, (fam, tail, nch, stride) in zip(*product):
        B, N, rg = c["B"], c["N"], c["ragged"]
        if fam == "EARLY":
            assert c["pipeline"] and c["xy"] and not rg and 65 <= N <= 384 and B <= 2048, c
            assert nch == -(-N // 64) and 2 <= nch <= 6 and stride == 64 * min(hr.EARLY_CHUNKS, nch - 1), (c, nch, stride)
        if fam == "DUO":
            assert c["pipeline"] and not rg and 65 <= N <= 640 and stride == N + (N & 1), (c, stride)
        assert (fam == "BLOCK") == (c["block_kernel"] == 1 and not rg and 65 <= N <= 1024), (c, fam)
        if fam == "BLOCK":
            assert nch == -(-N // 64) and 2 <= nch <= 16, (c, nch)               # one wave per chunk, 1024 threads at most
        if rg:
            assert fam in ("ONE", "BIG") and tail == 6, (c, fam, tail)
        if c["tail_scan_stages"] == 0:
            assert tail == 6, (c, tail)
        elif not rg:
            # (no pose, no last chunk: six stages, as wave_tail_stages has always answered; the entries return before they get here)
            last = (N - 1) & 63
            want = 6 if N <= 0 else (hr.FULL if last == 63 else (4 if last < 16 else (5 if last < 32 else 6)))
            assert tail == want, (c, tail)
        assert tail in (4, 5, 6, hr.FULL)


def test_headline_shapes_and_corners(hr):
    def one(**kw):
        return route(hr, [{**DEFAULTS, "pipeline": 1, "xy": 1, "ragged": 0, **kw}])[0]
    assert one(B=1000, N=271)[:3] == ("EARLY", 4, 5)                                 # the C2 headline shape
    assert one(B=256, N=271)[0] == "DUO" and one(B=4096, N=271)[0] == "BIG"
    assert one(B=100000, N=271, duo_kernel=1)[0] == "DUO"                            # a forced two-wave build wins at any batch size
    assert one(B=1000, N=271, duo_kernel=1, early_variances=1)[0] == "DUO"           # ... and goes before a forced early build
    assert one(B=256, N=271, early_variances=1)[0] == "EARLY"                        # a forced early build before the automatic two-wave range
    assert one(B=1000, N=271, block_kernel=-1)[0] != "BLOCK" and one(B=1000, N=271, block_kernel=1)[0] == "BLOCK"
    assert one(B=1000, N=0, ragged=1, block_kernel=1, duo_kernel=1, early_variances=1)[:2] == ("ONE", 6)


def test_ragged_calls_change_build_between_2048_and_2049_tracks(hr):
    """a ragged call takes the one-wave build up to 2 048 tracks and the big-batch build from 2 049 on (the batches of
    tests/test_ragged_routes.py stand on either side), K4 and pipeline alike, always the six-stage instance, whatever the options say"""
    for bk, dk, ev, ts, p, x in itertools.product(OPTS, OPTS, OPTS, (0, 1), (0, 1), (0, 1)):
        c = dict(block_kernel=bk, duo_kernel=dk, early_variances=ev, tail_scan_stages=ts, pipeline=p, xy=x, ragged=1, N=0)
        got = route(hr, [{**c, "B": 2048}, {**c, "B": 2049}, {**c, "B": 253}])
        assert [g[:2] for g in got] == [("ONE", 6), ("BIG", 6), ("ONE", 6)], (c, got)
    # block_kernel = 1 takes a dense call of the same shape, never a ragged one
    dense = dict(DEFAULTS, block_kernel=1, pipeline=1, xy=1, ragged=0, B=2049, N=271)
    assert route(hr, [dense])[0][0] == "BLOCK" and route(hr, [dict(dense, ragged=1, N=0)])[0][0] == "BIG"
    assert route(hr, [dict(dense, B=2048)])[0][0] == "BLOCK" and route(hr, [dict(dense, B=2048, ragged=1, N=0)])[0][0] == "ONE"


def test_noise_layout_predicate(hr):
    d = lambda *v: np.array(v, np.float64)
    assert hr.hr_xy(d(1, 1, 2), d(3, 3, 3), d(4, 4, 4)) == 1                         # x and y alike, z differs in one of the three
    assert hr.hr_xy(d(1, 1, 1), d(3, 3, 3), d(4, 4, 4)) == 0                         # all three alike: the generic build shares one scan
    assert hr.hr_xy(d(1, 2, 3), d(3, 3, 3), d(4, 4, 4)) == 0
    assert hr.hr_xy(d(1, 1, 2), d(3, 5, 3), d(4, 4, 4)) == 0 and hr.hr_xy(d(1, 1, 2), d(3, 3, 3), d(4, 5, 4)) == 0
