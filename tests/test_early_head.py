"""Chunk 0 of the early-variance build (csrc/gsf_ekf_wave_early.hip; the rows part of the head in chunk_body() of csrc/gsf_wave_common.hpp).

Chunk 0 is the chunk the early-variance build treats differently from the one-wave kernel: its variances come from the table formed in
the shadow of the input burst (without y rows where y repeats x), and the fit-independent rows part of its head -- unit quaternions,
previous-lane moves, dt, the GNSS gate and the outage masks -- reads the registers that burst filled.  The one-wave kernel (option 0)
scans the variances inside its chunk loop and loads the chunk's rows itself.  The claim is BITS: with
"early_variances" at 1 and at 0 every byte of pos / quat / status / R / t / s is the same under both row rules, and option 1 agrees with
the CPU oracle inside the tolerances tests/test_gpu_parity.py uses for the same outputs.

Every planted kind aims at the statements of the head and at what reads the table, and sits inside chunk 0 (rows 0..63); see planted_batch()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py: what the wave kernels are held to against the oracle
POS_TOL = 1e-7       # positions (the stated gate is 1e-6 m)
Q_TOL = 1e-9         # quaternion components
S_TOL = 1e-10        # scale of the pipeline's fit

LENGTHS = [128, 271, 384]                                                # two, five and six chunks
NB = 48
KINDS = 14
EMPTY_KINDS = (11, 12)                                                   # bad pose-0 quaternion, fit None: the kernel leaves before the chunk loop
DEFAULTS = {"early_variances": -1, "duo_kernel": -1}
OFFSET = np.array([4.5e5, 5.4e6, 110.0])
THR = np.deg2rad(45.0)                                                   # CONFIG: sharp_turn_yaw_rate_threshold_deg_per_sec
NEAR = 1e-3                                                              # a planted pair turns at THR (1 +- NEAR): six orders above the gate's rounding (HISTORY.md, "Sharp-turn gate")


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def planted_batch(nb, N, seed, kind_of):
    """Host-made tracks; kind_of(b) -> (kind, variant).  Kinds, all inside chunk 0:
    0 clean; 1 an outage with pairs and its recovery in rows 1..63; 2 a recovery at row 63; 3 a recovery at row 1 (pose 0 alone is out);
    4 an outage that starts at pose 0; 5 an outage that starts in chunk 0 and recovers in chunk 1 (odd variants: with a sharp pair in front
    of the boundary, so c_seg_sharp crosses it as well as c_ostart); 6 a pair over the yaw-rate threshold inside an outage; 7 a pair just
    under it; 8 a zero-norm quaternion (the generic orientation path overwrites the telescoped values; odd variants: inside an outage, a pair
    with a bad quaternion); 9 a repeated stamp inside an outage (the pair is not evaluated: t > t_pr fails; dt clamps); 10 a NaN fix under
    a set mask byte (the table is rebuilt; odd variants: next to an outage); 11 a bad pose-0 quaternion; 12 fewer than three valid rows
    (fit None); 13 two outages with two recoveries in the chunk, one of them behind a sharp pair."""
    rng = np.random.default_rng(seed)
    dt = 0.1 + rng.uniform(-0.004, 0.004, size=(nb, N)); dt[:, 0] = 0.0
    head = np.cumsum(rng.normal(0, 0.01, size=(nb, N)), axis=1)
    valid = np.ones((nb, N), dtype=np.uint8)
    exact = {}                                                           # track -> [(row, factor)]: yaw step of row = factor * THR * dt
    zero_q, nan_rows = {}, {}
    for b in range(nb):
        kind, v = kind_of(b)
        if kind == 1:
            lo = int(rng.integers(1, 50)); hi = int(rng.integers(lo + 2, 63))
            valid[b, lo:hi] = 0
        elif kind == 2:
            valid[b, int(rng.integers(2, 61)):63] = 0
        elif kind == 3:
            valid[b, 0] = 0
        elif kind == 4:
            valid[b, :int(rng.integers(2, 41))] = 0
        elif kind == 5:
            lo, hi = int(rng.integers(30, 60)), int(rng.integers(65, 100))
            valid[b, lo:hi] = 0
            if v % 2 == 1:
                exact[b] = [(int(rng.integers(lo + 1, 64)), 1.0 + NEAR)]
        elif kind in (6, 7):
            lo = int(rng.integers(2, 20)); hi = int(rng.integers(lo + 6, 62))
            valid[b, lo:hi] = 0
            exact[b] = [(int(rng.integers(lo + 1, hi)), 1.0 + NEAR if kind == 6 else 1.0 - NEAR)]
        elif kind == 8:
            k = int(rng.integers(1, 64)); zero_q[b] = k
            if v % 2 == 1:
                valid[b, max(1, k - 3):min(63, k + 4)] = 0
        elif kind == 9:
            lo = int(rng.integers(2, 40)); valid[b, lo:lo + 12] = 0
            dt[b, lo + 4] = 0.0
        elif kind == 10:
            k = int(rng.integers(1, 64)); nan_rows[b] = k
            if v % 2 == 1:
                lo = (k + 8) % 50 + 1; valid[b, lo:lo + 6] = 0
                if valid[b, k] == 0:
                    nan_rows[b] = lo + 7
        elif kind == 11:
            zero_q[b] = 0
            valid[b, 5:30] = 0
        elif kind == 12:
            keep = rng.choice(N, size=2, replace=False)
            valid[b, :] = 0; valid[b, keep] = 1
        elif kind == 13:
            valid[b, 4:15] = 0; valid[b, 30:52] = 0
            exact[b] = [(int(rng.integers(32, 52)), 1.0 + NEAR)] if v % 2 == 0 else [(int(rng.integers(6, 15)), 1.0 + NEAR)]
    ts = 1000.0 + np.cumsum(dt, axis=1)
    step = 1.4 * np.stack([np.cos(head), np.sin(head), 0.01 * np.ones_like(head)], -1) * (np.abs(dt[..., None]) / 0.1)
    pos = np.cumsum(step, axis=1) + rng.normal(0, 0.01, size=(nb, N, 3))
    yaw = head.copy()
    for b, rows in exact.items():
        for k, f in rows:
            yaw[b, k:] += f * THR * (ts[b, k] - ts[b, k - 1]) - (yaw[b, k] - yaw[b, k - 1])
    quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], -1) * rng.uniform(0.5, 2.0, size=(nb, N, 1))
    for b, k in zero_q.items():
        quat[b, k] = 0.0
    gps = pos * 1.03 + OFFSET + rng.normal(0, 0.4, size=(nb, N, 3))
    gps[valid == 0] = np.nan
    for b, k in nan_rows.items():
        assert valid[b, k] == 1
        gps[b, k, int(rng.integers(0, 3))] = np.nan
    init_pos = gps[:, 0].copy(); bad0 = np.isnan(init_pos).any(axis=1)
    init_pos[bad0] = pos[bad0, 0] * 1.03 + OFFSET
    n0 = np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    init_quat = np.where(n0 > 0, quat[:, 0] / np.where(n0 > 0, n0, 1.0), np.array([0.0, 0.0, 0.0, 1.0]))
    return ts, pos, quat, gps, valid, init_pos, init_quat


def every_kind(b):
    return b % KINDS, b // KINDS


LONE = {3 * k: k for k in range(1, KINDS)}                               # tracks 3, 6, .., 39: one track of each kind among clean ones


def one_of_each(b):
    return LONE.get(b, 0), b % 2


def as_bytes(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def run_pipeline(B, batch, rules=("reference", "all")):
    """the fused pipeline under both row rules: name -> array, as the caller gets them"""
    res = {}
    for rows in rules:
        out, R, t, s = B.fuse_pipeline_batch(batch, fit_rows=rows)
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


_host, _runs = {}, {}


def host_tracks(N):
    """the planted tracks of one length, made once and shared by the tests (never changed)"""
    if N not in _host:
        _host[N] = planted_batch(NB, N, 9900 + N, every_kind)
    return _host[N]


def option_runs(B, key, tracks):
    """option 1 and option 0 on ONE context (the one-wave kernel on the other side: no two-wave build), run once per batch and shared"""
    if key not in _runs:
        batch = B.TrajectoryBatch.from_host(*tracks, layout=0)
        _runs[key] = {v: with_options(B, {"early_variances": v, "duo_kernel": 0}, lambda: run_pipeline(B, batch)) for v in (1, 0)}
    return _runs[key]


def assert_same_bytes(got, what):
    total = 0
    for key in got[0]:
        a, b = as_bytes(got[1][key]), as_bytes(got[0][key])
        assert a.shape == b.shape
        differing = int((a != b).sum())
        total += differing
        print(f"{what} {key}: {differing} differing bytes of {a.size}")
        assert differing == 0, (what, key, differing)
    assert total == 0


@pytest.mark.parametrize("N", LENGTHS)
def test_chunk_0_gives_the_same_bytes(B, N):
    """option 1 against option 0, raw bytes of pos / quat / status / R / t / s, both row rules, every planted kind"""
    assert_same_bytes(option_runs(B, N, host_tracks(N)), f"N={N} planted")


@pytest.mark.parametrize("N", LENGTHS)
def test_chunk_0_against_the_oracle(B, orc, N):
    """option 1 against oracle.fuse_pipeline_batch: status words equal, positions, quaternions and scale inside the tolerances of
    tests/test_gpu_parity.py; the planted kinds did what they were planted for (the flags of the status words)"""
    ts, pos, quat, gps, valid, ip, iq = host_tracks(N)
    got = option_runs(B, N, host_tracks(N))[1]
    kinds = np.arange(NB) % KINDS
    for rows in ("reference", "all"):
        pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, fit_rows=rows)
        p, q, st, s = (got[f"{rows}.{n}"] for n in ("pos", "quat", "status", "s"))
        ok = np.isfinite(pr).all(axis=(1, 2))
        ep, eq = np.abs(p[ok] - pr[ok]).max(initial=0.0), np.abs(q[ok] - qr[ok]).max(initial=0.0)
        es = np.abs(s[ok] - sr[ok]).max(initial=0.0)
        print(f"N={N} pipeline/{rows}: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, max |ds| {es:.2e}, {int((~ok).sum())} non-finite tracks")
        assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, rows)
        assert (ok == ~np.isin(kinds, EMPTY_KINDS)).all(), (N, rows, np.nonzero(ok == np.isin(kinds, EMPTY_KINDS))[0].tolist())
        bad = np.nonzero(((st & ~(16 << 8)) != str_) & ok)[0]
        assert len(bad) == 0, (N, rows, bad[:8].tolist(), st[bad[:8]].tolist(), str_[bad[:8]].tolist())
        # (the oracle's own status words say what each kind exercised: compared above, so the device agrees)
        flags = str_ & 0xff
        sharp, rts = (flags & 4) != 0, (flags & 2) != 0                  # ST_SHARP_TURN, ST_RTS_APPLIED
        assert sharp[kinds == 6].all() and not sharp[kinds == 7].any(), (N, rows, "the planted pairs sit on their sides of the threshold")
        assert rts[kinds == 7].all() and rts[kinds == 1].all() and rts[kinds == 2].all(), (N, rows)
        assert ep < POS_TOL and eq < Q_TOL and es < S_TOL, (N, rows, ep, eq, es)


def test_one_track_of_each_kind_among_clean_ones(B):
    """a clean batch of 48 in which ONE track of each kind sits: a rare path taken by one wave does not disturb another"""
    N = 271
    assert_same_bytes(option_runs(B, "lone", planted_batch(NB, N, 9950, one_of_each)), f"N={N} one of each kind")
