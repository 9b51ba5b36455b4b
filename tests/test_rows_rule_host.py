"""CPU tier of the row rule as decisions on lane masks (gps_optimize_slam_amd/csrc/gsf_rows_rule.hpp), the wave-uniform part of the
early-variance build's row choice.  The header is compiled with g++ into a test-only harness (tests/host_rows_rule_harness.cpp) that
forms the lane masks as the kernel's lanes do; the chosen rows, the branch and the count are compared with
oracle.pick_sim3_rows(..., return_branch=True) on random tracks of 65..384 rows with holes and gaps and on planted edge cases.  The
harness is also built as a stand-alone program with -fsanitize=address,undefined and run once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_rows_rule_harness.cpp")
MS, GAP, DUR = 4, 5.0, 180.0
NRANDOM = 20000


@pytest.fixture(scope="module")
def rr():
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libhost_rows_rule_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
    L = C.CDLL(so)
    L.rr_choose.restype = None
    L.rr_choose.argtypes = [np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS"),
                            np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), C.c_int64, C.c_int, C.c_double, C.c_double,
                            np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    L.rr_flags.argtypes = [np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    f = np.zeros(3, np.int32)
    L.rr_flags(f)
    L.FEW, L.ALL, L.SEGMENT = (int(x) for x in f)
    assert L.rr_chunks() == 6
    return L


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def choose(rr, tracks, ms=MS, gap=GAP, dur=DUR):
    """[(ts, valid)] -> [(rows mask, info)]"""
    off = np.zeros(len(tracks) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t, _ in tracks])
    ts = np.ascontiguousarray(np.concatenate([t for t, _ in tracks]), dtype=np.float64)
    va = np.ascontiguousarray(np.concatenate([v for _, v in tracks]), dtype=np.uint8)
    rows, info = np.zeros(int(off[-1]), np.uint8), np.zeros((len(tracks), 8), np.int32)
    rr.rr_choose(ts, va, off, len(tracks), ms, gap, dur, rows, info)
    return [(rows[off[c]:off[c + 1]], info[c]) for c in range(len(tracks))]


def check(rr, orc, tracks, ms=MS, gap=GAP, dur=DUR):
    """every track against the oracle: rows, branch, count; returns how often each outcome was seen"""
    seen = {"raise": 0, 0: 0, 1: 0, 2: 0}
    for c, ((ts, va), (rows, info)) in enumerate(zip(tracks, choose(rr, tracks, ms, gap, dur))):
        idx, br = orc.pick_sim3_rows(ts, va, ms, gap, dur, return_branch=True)
        flag, nT = int(info[0]), int(info[1])
        if idx is None:
            assert flag == rr.FEW, (c, flag)
            seen["raise"] += 1
            continue
        assert flag == {0: 0, 1: rr.SEGMENT, 2: rr.ALL}[br], (c, flag, br)
        assert np.array_equal(np.nonzero(rows)[0], idx), (c, br)
        assert nT == len(idx), (c, nT, len(idx))
        v = np.nonzero(va)[0]
        assert int(info[5]) == (int(v[0]) if len(v) else -1), (c, info[5])
        assert 0 <= int(info[4]) <= len(ts)
        seen[br] += 1
    return seen


def base_track(N, step=0.1, t0=1000.0):
    return t0 + step * np.arange(N), np.ones(N, np.uint8)


def with_gap(ts, at, by=GAP + 1.0):
    ts = ts.copy()
    ts[at:] += by
    return ts


def test_random_tracks(rr, orc):
    """at least 20 000 tracks of 65..384 rows with random holes, gaps, repeated stamps, duration limits and min_samples"""
    rng = np.random.default_rng(20260119)
    total = {"raise": 0, 0: 0, 1: 0, 2: 0}
    for ms, dur, n in ((4, 180.0, 8000), (4, 12.0, 4000), (7, 9.0, 4000), (1, 180.0, 2000), (30, 6.5, 2000)):
        tracks = []
        for _ in range(n):
            N = int(rng.integers(65, 385))
            dt = np.where(rng.random(N) < 0.05, 0.0, 0.1)
            ts = 1000.0 + np.cumsum(dt)
            for _ in range(int(rng.integers(0, 3))):
                ts = with_gap(ts, int(rng.integers(1, N)), GAP + float(rng.choice([-0.5, 0.0, 1e-9, 0.5, 3.0])))
            va = np.ones(N, np.uint8)
            for _ in range(int(rng.integers(0, 4))):
                s, L = int(rng.integers(0, N)), int(rng.choice([1, 2, 7, 40, 64, 65, 130]))
                va[s:s + L] = 0
            if rng.random() < 0.1:
                va[rng.random(N) < 0.7] = 0
            if rng.random() < 0.03:
                va[:] = 0
                va[rng.choice(N, size=int(rng.integers(0, ms + 2)), replace=False)] = 1
            tracks.append((ts, va))
        for k, v in check(rr, orc, tracks, ms=ms, dur=dur).items():
            total[k] += v
    print(total)
    assert sum(total.values()) >= NRANDOM and all(v > 100 for v in total.values()), total


@pytest.mark.parametrize("N", [129, 271, 384])
def test_gap_next_to_every_chunk_boundary(rr, orc, N):
    """a gap at every lane next to each chunk boundary, with and without a hole in front of it: the row in front of the gap (left out,
    V[:k]) sits in the previous chunk when the gap's row is lane 0 or when the hole reaches back across the boundary"""
    tracks = []
    for edge in range(64, N, 64):
        for at in range(edge - 3, min(N, edge + 4)):
            ts, va = base_track(N)
            tracks.append((with_gap(ts, at), va))
            for hole in (1, 2, 5, 66):
                v = va.copy()
                v[max(1, at - hole):at] = 0
                tracks.append((with_gap(ts, at), v))
    seen = check(rr, orc, tracks)
    assert seen[0] > 0 and seen["raise"] == 0


def test_gap_across_a_hole(rr, orc):
    """no adjacent pair of rows is max_gap apart; the valid rows either side of the hole are (the stamps are fetched one by one), or
    are exactly max_gap apart (no gap)"""
    tracks, N = [], 271
    for s, L in ((40, 60), (60, 10), (63, 2), (64, 51), (100, 120), (5, 200)):
        for step in (GAP / (L + 1), GAP / (L + 1) * 1.01, 0.2):
            ts, va = base_track(N, step=step)
            va[s:s + L] = 0
            tracks.append((ts, va))
    res = choose(rr, tracks)
    assert any(int(info[6]) > 0 for _, info in res)
    seen = check(rr, orc, tracks)
    assert seen[0] + seen[1] + seen[2] == len(tracks)


def test_first_valid_row_elsewhere(rr, orc):
    """the first valid row is not row 0, and not in chunk 0: the duration limit counts from ITS stamp"""
    tracks = []
    for first in (1, 63, 64, 65, 130, 200):
        for dur in (180.0, 5.0):
            ts, va = base_track(271)
            va[:first] = 0
            tracks.append((ts, va))
            check(rr, orc, [(ts, va)], dur=dur)
            check(rr, orc, [(with_gap(ts, first + 30), va)], dur=dur)
    check(rr, orc, tracks)


def test_exact_thresholds(rr, orc):
    """t - t_prev == max_gap is no gap; t == tlim is inside the limit (binary-exact stamps)"""
    N = 200
    ts = 1024.0 + 0.125 * np.arange(N)
    va = np.ones(N, np.uint8)
    for at in (5, 63, 64, 65, 128):
        exact = ts.copy(); exact[at:] += GAP - 0.125                     # the step is max_gap exactly
        above = ts.copy(); above[at:] += GAP
        r = choose(rr, [(exact, va), (above, va)])
        assert int(r[0][1][2]) == N and int(r[1][1][2]) == at - 1
        check(rr, orc, [(exact, va), (above, va)])
    for k in (10, 63, 64, 150):
        dur = 0.125 * k                                                  # row k sits at tlim exactly
        (rows, info), = choose(rr, [(ts, va)], dur=dur)
        assert int(info[1]) == k + 1 and rows[k] == 1 and rows[k + 1] == 0
        check(rr, orc, [(ts, va)], dur=dur)


def test_first_segment_around_min_samples(rr, orc):
    """a first segment of min_samples - 1, min_samples and min_samples + 1 rows (V[:k] leaves out the row in front of the gap): the first
    falls back to all valid rows"""
    for ms in (4, 64, 65):
        got = []
        for seg in (ms - 1, ms, ms + 1):
            ts, va = base_track(271)
            tracks = [(with_gap(ts, seg + 1), va)]                       # rows 0..seg in front of the gap, the last one left out
            (_, info), = choose(rr, tracks, ms=ms)
            got.append(int(info[0]))
            check(rr, orc, tracks, ms=ms)
        assert got == [rr.ALL, 0, 0], got


def test_duration_limit_leaves_too_few(rr, orc):
    """the limit leaves min_samples - 1 rows of a long enough segment: the whole segment; min_samples rows: the timed subset"""
    ts = 1024.0 + 0.125 * np.arange(271)
    va = np.ones(271, np.uint8)
    for ms in (4, 70):
        a, b = choose(rr, [(ts, va)], ms=ms, dur=0.125 * (ms - 2)), choose(rr, [(ts, va)], ms=ms, dur=0.125 * (ms - 1))
        assert int(a[0][1][0]) == rr.SEGMENT and int(a[0][1][1]) == 271 and int(b[0][1][0]) == 0 and int(b[0][1][1]) == ms
        check(rr, orc, [(ts, va)], ms=ms, dur=0.125 * (ms - 2))
        check(rr, orc, [(ts, va)], ms=ms, dur=0.125 * (ms - 1))
        gapped = with_gap(ts, 200)
        check(rr, orc, [(gapped, va)], ms=ms, dur=0.125 * (ms - 2))


def test_too_few_valid_rows(rr, orc):
    """fewer than min_samples valid rows in all, with and without a gap among them: the reference raises"""
    tracks = []
    for keep in ((), (0,), (270,), (3, 100, 269), (63, 64, 65)):
        ts, va = base_track(271)
        va[:] = 0
        va[list(keep)] = 1
        tracks.append((ts, va))
        tracks.append((with_gap(ts, 64), va))
    seen = check(rr, orc, tracks)
    assert seen["raise"] == len(tracks)


def test_repeated_stamps(rr, orc):
    """repeated and backward-stepping stamps, in and around holes"""
    rng = np.random.default_rng(77)
    tracks = []
    for _ in range(200):
        N = int(rng.integers(65, 385))
        dt = rng.choice([0.0, 0.0, 0.1, -0.05, 6.0], size=N, p=[0.3, 0.2, 0.4, 0.09, 0.01])
        ts = 1000.0 + np.cumsum(dt)
        va = (rng.random(N) < 0.8).astype(np.uint8)
        tracks.append((ts, va))
    check(rr, orc, tracks)
    check(rr, orc, tracks, dur=3.0)


def test_stand_alone_under_sanitizers():
    """the harness as a program of its own with -fsanitize=address,undefined, run once"""
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, "host_rows_rule_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DROWS_RULE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, (out.stdout, out.stderr)
