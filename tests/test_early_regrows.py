"""The early-variance build's chunk sequence from registers (csrc/gsf_ekf_wave_early.hip, step 5; REGCHUNKS of wave_serial_chunks): the chunks of a track
run as straight-line instances of the one chunk body, and chunk k + 1 takes its stamp, mask byte, SLAM position and fix from the registers
the input burst filled -- only its quaternion is requested again.  What can go wrong is a row in those registers that is not the row memory
holds (the fall-back fit after a NaN under a set mask byte, the idle lanes of a short last chunk), a carry that a constant c0 or L folded
the wrong way (outages across chunk boundaries, the carried-outage patch, the generic orientation path), or a stale register after an
early exit (a fit that returns None).

The claim is BITS: option "early_variances" 1 against 0 (the two-wave build off on both sides) gives zero differing bytes in pos / quat /
status / R / t / s under both row rules.  Option 1 also stays inside the tolerances tests/test_gpu_parity.py holds the wave kernels to
against the CPU oracle.  Batches of NB = 32 tracks; every planted kind as ONE track among clean ones, and all kinds in one batch.

| N   | what it exercises                                         |
| 65  | two chunks, last chunk one pose, tail scans of 4 stages   |
| 128 | two full chunks                                           |
| 129 | three chunks, last chunk one pose                         |
| 150 | last chunk ends in lane 21, 5 stages                      |
| 271 | five chunks, last chunk ends in lane 14, 4 stages         |
| 300 | five chunks, last chunk ends in lane 43, 6 stages         |
| 384 | six full chunks                                           |"""
import numpy as np
import pytest

import hygiene
from test_early_rows import POS_TOL, Q_TOL, S_TOL, as_bytes, assert_same_bytes, on_and_off, planted_batch, run_pipeline, with_options

pytestmark = pytest.mark.gpu

LENGTHS = [65, 128, 129, 150, 271, 300, 384]
NB = 32
KINDS = ["nan_set_chunk0", "nan_set_middle", "nan_set_last", "nan_clear_later", "first_valid_chunk1", "outage_to_lane0_next",
         "outage_to_lane0_second", "outage_over_128", "ends_in_outage", "zero_quat_chunk2", "nonunit_quat_chunk2", "repeated_stamps_boundary",
         "fit_none"]
NAN_WORD = int(np.array([np.nan]).view(np.int64)[0])


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


_clean = {}


def clean_tracks(N):
    """NB clean tracks of one length, made once and shared (never changed: the tests plant into copies)"""
    if N not in _clean:
        _clean[N] = planted_batch(NB, N, 7700 + N, clean=True)
    return _clean[N]


def outage(arrs, b, lo, hi):
    """rows lo .. hi - 1 of track b without a fix (mask byte clear, the fix NaN, as the loaders leave such rows)"""
    ts, pos, quat, gps, valid = arrs[:5]
    valid[b, lo:hi] = 0; gps[b, lo:hi] = np.nan


def plant(arrs, b, kind, N):
    """one planted kind into track b of the (copied) arrays"""
    ts, pos, quat, gps, valid = arrs[:5]
    nch = (N + 63) // 64
    mid = min(max(1, nch // 2), nch - 1)
    if kind == "nan_set_chunk0":                                           # the fall-back fit runs; the loop must still see memory's rows
        gps[b, 21, 1] = np.nan
    elif kind == "nan_set_middle":
        gps[b, min(N - 1, 64 * mid + 3), 0] = np.nan
    elif kind == "nan_set_last":
        gps[b, N - 1, 2] = np.nan
    elif kind == "nan_clear_later":                                        # a NaN under a CLEAR mask byte, one component only
        r = min(N - 1, 64 + 5); valid[b, r] = 0; gps[b, r, 1] = np.nan
    elif kind == "first_valid_chunk1":
        outage(arrs, b, 0, min(N - 1, 70))
    elif kind == "outage_to_lane0_next":                                   # starts in lane 63 of chunk 0, recovers in lane 0 of chunk 1
        outage(arrs, b, 63, 64)
    elif kind == "outage_to_lane0_second":                                 # ... in lane 0 of chunk 2 (tracks of two chunks: as far as they reach)
        outage(arrs, b, 63, 128 if N > 128 else N - 1)
    elif kind == "outage_over_128":                                        # recovered three chunks on: the memory patch path behind the ring
        outage(arrs, b, 10, 200 if N > 210 else N - 3)
    elif kind == "ends_in_outage":
        outage(arrs, b, N - min(20, N // 4), N)
    elif kind == "zero_quat_chunk2":                                       # the generic orientation path, with the carried c_r
        quat[b, min(N - 1, 130)] = 0.0
    elif kind == "nonunit_quat_chunk2":
        quat[b, min(N - 1, 131)] *= 1.0e3                                 # (far from unit length, still a rotation: the fast path scales it)
    elif kind == "repeated_stamps_boundary":
        ts[b, 63:min(N, 66)] = ts[b, 63]
    elif kind == "fit_none":                                               # too few rows: the rows in registers are never used
        outage(arrs, b, 0, N); valid[b, 3] = 1; gps[b, 3] = pos[b, 3]
    else:
        raise AssertionError(kind)


def planted(N, kinds, at=17):
    arrs = tuple(a.copy() for a in clean_tracks(N))
    for j, kind in enumerate(kinds):
        plant(arrs, at if len(kinds) == 1 else 1 + 2 * j, kind, N)
    return arrs


@pytest.mark.parametrize("N", LENGTHS)
def test_one_planted_track_among_clean_ones(B, N):
    """every kind, as the only planted track of its batch: option 1 against option 0, raw bytes, both row rules"""
    for kind in KINDS:
        batch = B.TrajectoryBatch.from_host(*planted(N, [kind]), layout=0)
        assert_same_bytes(on_and_off(B, batch), f"N={N} {kind}")


@pytest.mark.parametrize("N", LENGTHS)
def test_all_kinds_in_one_batch(B, orc, N):
    """all kinds in one batch: the same bytes as the one-wave kernel, and option 1 inside the oracle's tolerances"""
    ts, pos, quat, gps, valid, ip, iq = planted(N, KINDS)
    batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
    got = on_and_off(B, batch)
    assert_same_bytes(got, f"N={N} all kinds")
    for rows in ("reference", "all"):
        pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, fit_rows=rows)
        p, q, st, s = (got[1][f"{rows}.{n}"] for n in ("pos", "quat", "status", "s"))
        ok = np.isfinite(pr).all(axis=(1, 2))
        ep, eq = np.abs(p[ok] - pr[ok]).max(initial=0.0), np.abs(q[ok] - qr[ok]).max(initial=0.0)
        es = np.abs(s[ok] - sr[ok]).max(initial=0.0)
        print(f"N={N} pipeline/{rows}: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, max |ds| {es:.2e}, {int((~ok).sum())} non-finite tracks")
        assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, rows)
        assert ok[0] and not ok[1 + 2 * KINDS.index("fit_none")], (N, rows)
        bad = np.nonzero(((st & ~(16 << 8)) != str_) & ok)[0]
        assert len(bad) == 0, (N, rows, bad[:8].tolist(), st[bad[:8]].tolist(), str_[bad[:8]].tolist())
        assert ep < POS_TOL and eq < Q_TOL and es < S_TOL, (N, rows, ep, eq, es)


def test_same_batch_twice_on_a_dirtied_context(B, monkeypatch):
    """one context, the same batch twice: in between a larger foreign call, every workspace overwritten and every output handed out
    pre-filled with NaN words between guard bytes (tests/hygiene.py) -- the second run's bytes are the first's"""
    N = 271
    ctx = B.context()
    batch = B.TrajectoryBatch.from_host(*planted(N, KINDS), layout=0)
    other = B.TrajectoryBatch.synthetic(96, 400, layout=0, seed=11)

    def run():
        alloc = hygiene.GuardedAllocator(NAN_WORD)
        with alloc.installed(monkeypatch):
            res = with_options(B, {"early_variances": 1, "duo_kernel": 0}, lambda: run_pipeline(B, batch))
        alloc.assert_guards_intact()
        return res
    try:
        first = run()
        B.fuse_pipeline_batch(other)
        ctx.set_option("poison_workspaces", 255)
        second = run()
    finally:
        ctx.set_option("poison_workspaces", -1)
    assert_same_bytes({1: second, 0: first}, "second run against the first")
    off = with_options(B, {"early_variances": 0, "duo_kernel": 0}, lambda: run_pipeline(B, batch))
    assert_same_bytes({1: second, 0: off}, "second run against the one-wave kernel")
    assert as_bytes(second["reference.pos"]).size == NB * N * 24
