"""The early-variance build's fit (csrc/gsf_ekf_wave_early.hip, steps 2b and 4): the rows of the fit are chosen from stamps and mask bytes
while the track's rows are in flight (csrc/gsf_rows_rule.hpp; a set mask byte is taken to mean a usable fix), and every chunk is summed
when it arrives.  A NaN fix under a set mask byte in a chunk the choice looks at sends the wave to the one-wave kernel's pass.  A NaN
BEHIND the row at which the first gap was found, when the fit takes the first segment, provably does not matter (the rule never looks
behind that row) and is not waited for: tracks of kind 15 plant exactly that, and their bytes must be the one-wave kernel's all the same.

The claim is BITS: option "early_variances" 1 against 0 (two-wave build off on both sides) gives zero differing bytes in pos / quat /
status / R / t / s under both row rules, for NB = 60 tracks of every length below and four settings of the rule.  Option 1 also stays
inside the tolerances tests/test_gpu_parity.py holds the wave kernels to against the CPU oracle, and the row flags of its status words
are the branch of oracle.pick_sim3_rows."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POS_TOL = 1e-7       # tests/test_gpu_parity.py: positions (the stated gate is 1e-6 m)
Q_TOL = 1e-9         # quaternion components
S_TOL = 1e-10        # scale of the pipeline's fit

LENGTHS = [65, 129, 193, 271, 320, 384]
NB, KINDS = 60, 20
MS, GAP = 4, 5.0
STEP = 0.125                                                             # binary-exact stamps: thresholds can be hit exactly
# max_initial_duration: the default; row 100 of a track sits AT the limit; the limit leaves min_samples - 1 rows; exactly min_samples rows
DURS = [180.0, 100 * STEP, (MS - 2) * STEP, (MS - 1) * STEP]
DEFAULTS = {"early_variances": -1, "duo_kernel": -1}
OFFSET = np.array([4.5e5, 5.4e6, 110.0])
FEW, ROWS_ALL, ROWS_SEG = 32, 64, 128


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def config(B, dur):
    cfg = copy.deepcopy(B.CONFIG)
    cfg["sim3_ransac"]["min_samples"] = MS; cfg["time_alignment"]["max_gps_gap_threshold"] = GAP; cfg["sim3_ransac"]["max_initial_duration"] = dur
    return cfg


def planted_batch(nb, N, seed, clean=False):
    """Host-made tracks, twenty kinds in turn (track b is of kind b % 20, its variant v = b // 20; edge = a chunk boundary of the track):
    0 clean; 1-3 a gap at row edge - 1 / edge / edge + 1; 4 a gap at lane 0 behind a hole, so that the row in front of the gap (left out,
    V[:k]) sits in the chunk before; 5 a gap ACROSS a hole (no adjacent rows max_gap apart): 50 rows, 39 rows (the stamps either side are
    max_gap apart EXACTLY: no gap), 40 rows; 6 the first valid row is row 1 / 37 / 63; 7 it sits in chunk 1 or 2; 8 adjacent rows exactly
    max_gap apart (no gap); 9 a first segment of min_samples - 1 / min_samples / min_samples + 1 rows; 10 one or two valid rows in all;
    11 repeated and backward-stepping stamps; 12 a NaN fix under a set mask byte in chunk 0 only; 13 in a later chunk only; 14 in the last
    chunk only; 15 behind row_end only, the fit taking the first segment: behind the gap's row (cannot matter) / ON the gap's row (the
    rule looked there); 16 behind row_end with a first segment too short, so that every valid row is fitted (matters); 17 a hole across
    the boundary with the gap behind it; 18 a NaN fix under the set mask byte of row 0; 19 random holes and gaps."""
    rng = np.random.default_rng(seed)
    dt = np.full((nb, N), STEP); dt[:, 0] = 0.0
    valid = np.ones((nb, N), dtype=np.uint8)
    nch = (N + 63) // 64
    nan_rows = {}
    for b in range(nb):
        kind, v = (0, 0) if clean else (b % KINDS, b // KINDS)
        edge = 64 * (1 + v % (nch - 1))
        if kind in (1, 2, 3):
            dt[b, min(N - 1, edge + kind - 2)] += GAP + 1.0
        elif kind == 4:
            valid[b, edge - 3:edge] = 0; dt[b, edge] += GAP
        elif kind == 5:
            L = [50, 39, 40][v % 3]
            s = max(2, min(edge - 20, N - L - 2)); valid[b, s:s + L] = 0
        elif kind == 6:
            valid[b, :[1, 37, 63][v % 3]] = 0
        elif kind == 7:
            valid[b, :min(N - 8, [64, 65, 130][v % 3])] = 0
        elif kind == 8:
            dt[b, [edge, min(N - 1, edge + 1), 5][v % 3]] = GAP
        elif kind == 9:
            dt[b, MS + v % 3] += GAP
        elif kind == 10:
            valid[b, :] = 0; valid[b, rng.choice(N, size=1 + v % 2, replace=False)] = 1
        elif kind == 11:
            for _ in range(8):
                dt[b, int(rng.integers(2, N))] = [0.0, -0.0625, 0.0, -0.015625][int(rng.integers(0, 4))]
            if v % 2 == 1:
                s = int(rng.integers(4, N - 12)); valid[b, s:s + 9] = 0
        elif kind == 12:
            nan_rows[b] = [[1, 37, 63][v % 3]]
        elif kind == 13:
            nan_rows[b] = [64 + min(N - 65, 17 * v)] if nch == 2 else [int(rng.integers(64, 64 * (nch - 1)))]
        elif kind == 14:
            nan_rows[b] = [int(rng.integers(64 * (nch - 1), N))]
        elif kind == 15:
            g = 40 + v
            dt[b, g] += GAP + 0.5
            nan_rows[b] = [[g + 10, N - 1, g][v % 3]]
        elif kind == 16:
            dt[b, 3] += GAP + 0.5
            nan_rows[b] = [[N - 1, 64, 10][v % 3]]
        elif kind == 17:
            valid[b, edge - 5:edge + 2] = 0; dt[b, min(N - 1, edge + 2)] += GAP
        elif kind == 18:
            nan_rows[b] = [0]
        elif kind == 19:
            for _ in range(int(rng.integers(1, 4))):
                L = int(rng.choice([1, 2, 3, 7, 20, 64, 65])); s = int(rng.integers(0, max(1, N - L)))
                valid[b, s:s + L] = 0
            if v:
                dt[b, int(rng.integers(1, N))] += GAP + float(rng.choice([0.0, 0.125, 3.0]))
    ts = 1024.0 + np.cumsum(dt, axis=1)
    head = np.cumsum(rng.normal(0, 0.01, size=(nb, N)), axis=1)
    step = 1.4 * np.stack([np.cos(head), np.sin(head), 0.01 * np.ones_like(head)], -1)
    pos = np.cumsum(step, axis=1) + rng.normal(0, 0.01, size=(nb, N, 3))
    quat = np.stack([np.zeros_like(head), np.zeros_like(head), np.sin(head / 2), np.cos(head / 2)], -1) * rng.uniform(0.5, 2.0, size=(nb, N, 1))
    gps = pos * 1.03 + OFFSET + rng.normal(0, 0.4, size=(nb, N, 3))
    gps[valid == 0] = np.nan
    for b, rows in nan_rows.items():
        for i in rows:
            gps[b, i, int(rng.integers(0, 3))] = np.nan
    init_pos = pos[:, 0] * 1.03 + OFFSET
    init_quat = quat[:, 0] / np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    return ts, pos, quat, gps, valid, init_pos, init_quat


def as_bytes(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def run_pipeline(B, batch, config=None, rules=("reference", "all")):
    res = {}
    for rows in rules:
        out, R, t, s = B.fuse_pipeline_batch(batch, config=config, fit_rows=rows)
        p, q, st = out.host_traj_major()
        res[f"{rows}.pos"], res[f"{rows}.quat"], res[f"{rows}.status"] = p, q, st
        res[f"{rows}.R"], res[f"{rows}.t"], res[f"{rows}.s"] = R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy()
    return res


def with_options(B, opts, fn):
    ctx = B.context()
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


def on_and_off(B, batch, config=None):
    """option 1 and option 0 (the one-wave kernel on both sides: no two-wave build)"""
    return {v: with_options(B, {"early_variances": v, "duo_kernel": 0}, lambda: run_pipeline(B, batch, config)) for v in (1, 0)}


def assert_same_bytes(got, what):
    for key in got[0]:
        a, b = as_bytes(got[1][key]), as_bytes(got[0][key])
        assert a.shape == b.shape
        differing = int((a != b).sum())
        print(f"{what} {key}: {differing} differing bytes of {a.size}")
        assert differing == 0, (what, key, differing)


_host = {}


def host_tracks(N):
    """the planted tracks of one length, made once and shared by the tests (never changed)"""
    if N not in _host:
        _host[N] = planted_batch(NB, N, 9900 + N)
    return _host[N]


@pytest.mark.parametrize("N", LENGTHS)
def test_same_bytes_as_the_one_wave_kernel(B, N):
    """option 1 against option 0, raw bytes of every output, both row rules, every kind of track, four duration limits"""
    batch = B.TrajectoryBatch.from_host(*host_tracks(N), layout=0)
    for dur in DURS:
        assert_same_bytes(on_and_off(B, batch, config(B, dur)), f"N={N} max_dur={dur}")


@pytest.mark.parametrize("N", LENGTHS)
def test_against_the_oracle_and_its_branch(B, orc, N):
    """option 1 against oracle.fuse_pipeline_batch inside the tolerances of tests/test_gpu_parity.py; the row flags of the status word
    against the branch of oracle.pick_sim3_rows on the usable rows"""
    ts, pos, quat, gps, valid, ip, iq = host_tracks(N)
    usable = (valid != 0) & np.isfinite(gps).all(axis=2)
    batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
    for dur in DURS[:3]:
        cfg = config(B, dur)
        got = with_options(B, {"early_variances": 1, "duo_kernel": 0}, lambda: run_pipeline(B, batch, cfg))
        seen = set()
        for b in range(NB):
            idx, br = orc.pick_sim3_rows(ts[b], usable[b], MS, GAP, dur, return_branch=True)
            flags = (int(got["reference.status"][b]) >> 8) & (FEW | ROWS_ALL | ROWS_SEG)
            want = FEW if idx is None else {0: 0, 1: ROWS_SEG, 2: ROWS_ALL}[br]
            assert flags == want, (N, dur, b, b % KINDS, flags, want)
            seen.add(want)
        assert FEW in seen and ROWS_ALL in seen and (0 in seen or ROWS_SEG in seen), (N, dur, seen)
        for rows in ("reference", "all"):
            pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, cfg=cfg, fit_rows=rows)
            p, q, st, s = (got[f"{rows}.{n}"] for n in ("pos", "quat", "status", "s"))
            ok = np.isfinite(pr).all(axis=(1, 2))
            ep, eq = np.abs(p[ok] - pr[ok]).max(initial=0.0), np.abs(q[ok] - qr[ok]).max(initial=0.0)
            es = np.abs(s[ok] - sr[ok]).max(initial=0.0)
            print(f"N={N} max_dur={dur} pipeline/{rows}: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, max |ds| {es:.2e}, {int((~ok).sum())} non-finite tracks")
            assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, dur, rows)
            assert ok[0::KINDS].all() and not ok[10::KINDS].any(), (N, dur, rows)
            bad = np.nonzero(((st & ~(16 << 8)) != str_) & ok)[0]
            assert len(bad) == 0, (N, dur, rows, bad[:8].tolist(), st[bad[:8]].tolist(), str_[bad[:8]].tolist())
            assert ep < POS_TOL and eq < Q_TOL and es < S_TOL, (N, dur, rows, ep, eq, es)


@pytest.mark.parametrize("N", [129, 271])
@pytest.mark.parametrize("where", ["chunk0", "later", "last", "behind_row_end"])
def test_one_track_of_a_clean_batch_misses(B, N, where):
    """a clean batch in which ONE track carries a NaN fix under a set mask byte: that wave alone leaves the chunk-wise sums"""
    ts, pos, quat, gps, valid, ip, iq = (a.copy() for a in planted_batch(NB, N, 9950 + N, clean=True))
    nch = (N + 63) // 64
    row = {"chunk0": 21, "later": 64 * (nch // 2) + 3, "last": N - 2, "behind_row_end": 90}[where]
    if where == "behind_row_end":
        ts[17, 70:] += GAP + 1.0                                         # the gap's row is 70: row 90 is never looked at
    gps[17, row, 1] = np.nan
    batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
    assert_same_bytes(on_and_off(B, batch), f"N={N} one miss, {where}")


def test_a_clean_batch_after_a_batch_with_misses(B):
    """one context: the batch with misses, then a clean one -- the clean batch's bytes are the option-off bytes"""
    N = 271
    misses = B.TrajectoryBatch.from_host(*host_tracks(N), layout=0)
    clean = B.TrajectoryBatch.from_host(*planted_batch(NB, N, 9990, clean=True), layout=0)

    def both():
        run_pipeline(B, misses)
        return run_pipeline(B, clean)
    on = with_options(B, {"early_variances": 1, "duo_kernel": 0}, both)
    off = with_options(B, {"early_variances": 0, "duo_kernel": 0}, lambda: run_pipeline(B, clean))
    assert_same_bytes({1: on, 0: off}, "clean after misses")
