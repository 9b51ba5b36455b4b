"""The early-variance build of the fused pipeline's one-wave kernel (gsf_set_option "early_variances", csrc/gsf_ekf_wave_early.hip).

For equal-length tracks of 65..384 poses under the default noise layout the build computes the variances of the track's first chunk from
stamps and mask bytes alone -- a set mask byte is taken to mean a usable fix -- while the rest of the track's rows are still in flight,
parks them in LDS and runs that chunk without its Moebius scans; a NaN fix under a set mask byte there (the assumption missed) rebuilds
the table.  The
claim is BITS, not a tolerance: with the option at 1 and at 0 every byte of pos / quat / status / R / t / s of the fused pipeline is
the same under both row rules, and the path with the option on agrees with the CPU oracle inside the tolerances
tests/test_gpu_parity.py uses for the same outputs.  (The two-wave build is switched off on both sides: what is compared is the
early-variance build against the one-wave kernel it stands in for.)"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py: what the wave kernels are held to against the oracle
POS_TOL = 1e-7       # positions (the stated gate is 1e-6 m)
Q_TOL = 1e-9         # quaternion components
S_TOL = 1e-10        # scale of the pipeline's fit

LENGTHS_ON = [65, 66, 80, 81, 128, 129, 192, 193, 271, 320, 383, 384]    # every chunk count 2..6 and every sizing of the last chunk's scans
LENGTHS_OFF = [64, 385, 1000]                                            # the build does not apply: the option must change nothing
NB = 48
KINDS = 10
DEFAULTS = {"early_variances": -1, "duo_kernel": -1, "tail_scan_stages": 1}
OFFSET = np.array([4.5e5, 5.4e6, 110.0])


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def planted_batch(nb, N, seed, clean=False):
    """Host-made tracks, ten kinds in turn (track b is of kind b % 10, its variant v = b // 10):
    0 clean; 1 outage at the start; 2 outage at the end; 3 outage across chunk boundary 1 + v (each boundary of the track in turn);
    4 an outage longer than 128 poses (the RTS patch's memory path; as long as the track allows when it is shorter); 5 NaN fixes with the
    mask byte still set in the first chunk / the first and a middle chunk / the last chunk only / all three (v % 4).  Only the first chunk's
    variances are formed under the assumption, so the variants with a row in 1..63 miss and rebuild the table, and the last-chunk-only
    variant must NOT (its bytes are the one-wave kernel's either way); 6 an invalid
    quaternion (generic orientation path); 7 repeated and backward-stepping stamps, in and out of an outage (the dt clamp); 8 fewer than
    min_samples valid rows (the fit is None, the kernel returns early); 9 several random outages with a yaw burst (sharp-turn recoveries)."""
    rng = np.random.default_rng(seed)
    dt = 0.1 + rng.uniform(-0.004, 0.004, size=(nb, N)); dt[:, 0] = 0.0
    head = np.cumsum(rng.normal(0, 0.01, size=(nb, N)), axis=1)
    valid = np.ones((nb, N), dtype=np.uint8)
    yaw_extra = np.zeros((nb, N))
    nch = (N + 63) // 64
    nan_rows = {}
    for b in range(nb):
        kind, v = (0, 0) if clean else (b % KINDS, b // KINDS)
        if kind == 1:
            valid[b, :int(rng.integers(1, min(N - 8, 70)))] = 0
        elif kind == 2:
            valid[b, N - int(rng.integers(1, min(N - 8, 70))):] = 0
        elif kind == 3:
            edge = 64 * (1 + v % max(1, nch - 1))
            lo = max(1, edge - int(rng.integers(1, 40))); hi = min(N - 1, edge + int(rng.integers(1, 12)))
            valid[b, lo:max(hi, lo + 1)] = 0
        elif kind == 4:
            L = min(N - 12, 130 + int(rng.integers(0, 40)))
            s = int(rng.integers(6, N - L - 4)) if N - L - 4 > 6 else 6
            valid[b, s:s + L] = 0
        elif kind == 5:
            first, mid, last = int(rng.integers(1, 64)), int(rng.integers(64 * (nch // 2), min(N, 64 * (nch // 2) + 64))), int(rng.integers(64 * (nch - 1), N))
            nan_rows[b] = [[first], [first, mid], [last], [first, mid, last, N - 1]][v % 4]
        elif kind == 7:
            for _ in range(6):
                k = int(rng.integers(2, N))
                dt[b, k] = [0.0, -0.05, 0.0, -0.01][int(rng.integers(0, 4))]
            if v % 2 == 1:
                s = int(rng.integers(4, N - 12)); valid[b, s:s + 9] = 0; dt[b, s + 3] = 0.0; dt[b, s + 5] = -0.02
        elif kind == 8:
            keep = rng.choice(N, size=2, replace=False)
            valid[b, :] = 0; valid[b, keep] = 1
        elif kind == 9:
            for _ in range(int(rng.integers(1, 4))):
                L = int(rng.choice([1, 2, 3, 7, 20, 64, 65]))
                s = int(rng.integers(0, max(1, N - L)))
                valid[b, s:s + L] = 0
                if L >= 3 and s + L < N:
                    k = s + 1 + int(rng.integers(0, L - 2))
                    yaw_extra[b, k:] += rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.2)
    ts = 1000.0 + np.cumsum(dt, axis=1)
    step = 1.4 * np.stack([np.cos(head), np.sin(head), 0.01 * np.ones_like(head)], -1) * (np.abs(dt[..., None]) / 0.1)
    pos = np.cumsum(step, axis=1) + rng.normal(0, 0.01, size=(nb, N, 3))
    yaw = head + yaw_extra
    quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], -1) * rng.uniform(0.5, 2.0, size=(nb, N, 1))
    if not clean:
        for b in range(6, nb, KINDS):
            quat[b, int(rng.integers(1, N))] = 0.0
    gps = pos * 1.03 + OFFSET + rng.normal(0, 0.4, size=(nb, N, 3))
    gps[valid == 0] = np.nan
    for b, rows in nan_rows.items():
        for i in rows:
            gps[b, i, int(rng.integers(0, 3))] = np.nan
    init_pos = gps[:, 0].copy(); bad0 = np.isnan(init_pos).any(axis=1)
    init_pos[bad0] = pos[bad0, 0] * 1.03 + OFFSET
    init_quat = quat[:, 0] / np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    return ts, pos, quat, gps, valid, init_pos, init_quat


def as_bytes(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def run_pipeline(B, batch, config=None, rules=("reference", "all")):
    """the fused pipeline under both row rules: name -> array, as the caller gets them"""
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


def on_and_off(B, batch, config=None, extra=None):
    """option 1 and option 0 (the one-wave kernel on both sides: no two-wave build)"""
    extra = extra or {}
    return {v: with_options(B, dict({"early_variances": v, "duo_kernel": 0}, **extra), lambda: run_pipeline(B, batch, config)) for v in (1, 0)}


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


_host = {}


def host_tracks(N):
    """the planted tracks of one length, made once and shared by the tests (never changed)"""
    if N not in _host:
        _host[N] = planted_batch(NB, N, 9100 + N)
    return _host[N]


@pytest.mark.parametrize("N", LENGTHS_ON + LENGTHS_OFF)
def test_early_variances_give_the_same_bytes(B, N):
    """option 1 against option 0, raw bytes of pos / quat / status / R / t / s, both row rules, every kind of track; with sized and with
    six-stage scans of the last chunk (the build is keyed by both)"""
    batch = B.TrajectoryBatch.from_host(*host_tracks(N), layout=0)
    assert_same_bytes(on_and_off(B, batch), f"N={N} planted")
    assert_same_bytes(on_and_off(B, batch, extra={"tail_scan_stages": 0}), f"N={N} planted, six-stage tail")


@pytest.mark.parametrize("N", LENGTHS_ON)
def test_early_variances_against_the_oracle(B, orc, N):
    """the path with the option on against oracle.fuse_pipeline_batch: status words equal, positions, quaternions and scale inside the
    tolerances of tests/test_gpu_parity.py"""
    ts, pos, quat, gps, valid, ip, iq = host_tracks(N)
    batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
    got = with_options(B, {"early_variances": 1, "duo_kernel": 0}, lambda: run_pipeline(B, batch))
    for rows in ("reference", "all"):
        pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, fit_rows=rows)
        p, q, st, s = (got[f"{rows}.{n}"] for n in ("pos", "quat", "status", "s"))
        ok = np.isfinite(pr).all(axis=(1, 2))
        ep, eq = np.abs(p[ok] - pr[ok]).max(initial=0.0), np.abs(q[ok] - qr[ok]).max(initial=0.0)
        es = np.abs(s[ok] - sr[ok]).max(initial=0.0)
        print(f"N={N} pipeline/{rows}: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, max |ds| {es:.2e}, {int((~ok).sum())} non-finite tracks")
        assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, rows)
        assert not ok[8::KINDS].any() and ok[0::KINDS].all(), (N, rows)      # the fit is None where it was planted to be, and only a fit None or a bad pose 0 empties a track
        bad = np.nonzero(((st & ~(16 << 8)) != str_) & ok)[0]
        assert len(bad) == 0, (N, rows, bad[:8].tolist(), st[bad[:8]].tolist(), str_[bad[:8]].tolist())
        assert ep < POS_TOL and eq < Q_TOL and es < S_TOL, (N, rows, ep, eq, es)


@pytest.mark.parametrize("N", [129, 271])
@pytest.mark.parametrize("row", [1, 37, 63])
def test_one_track_of_a_batch_misses(B, N, row):
    """a clean batch in which ONE track carries a NaN fix under a set mask byte in its first chunk -- the chunk whose variances are formed
    under the assumption: that wave alone takes the wave-uniform rebuild, the 47 others do not.  A second track carries such a fix in a
    LATER chunk only, whose variances the chunk loop scans itself: no rebuild there, and no byte changes."""
    ts, pos, quat, gps, valid, ip, iq = (a.copy() for a in planted_batch(NB, N, 9500 + N, clean=True))
    gps[17, row, 1] = np.nan
    gps[30, N // 2, 2] = np.nan                                          # row 64 (chunk 1) / row 135 (chunk 2)
    batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
    assert_same_bytes(on_and_off(B, batch), f"N={N} one miss at row {row}")


def test_another_noise_layout_keeps_the_other_builds(B):
    """x and y with different noise: the build does not apply, the option changes nothing"""
    cfg = copy.deepcopy(B.CONFIG)
    cfg["ekf"]["initial_cov_diag"][:3], cfg["ekf"]["process_noise_diag"][:3], cfg["ekf"]["meas_noise_diag"] = [0.1, 0.2, 0.3], [0.1, 0.3, 0.7], [0.2, 0.25, 0.4]
    batch = B.TrajectoryBatch.from_host(*host_tracks(271), layout=0)
    assert_same_bytes(on_and_off(B, batch, config=cfg), "N=271 x != y")


def test_the_benchmarked_shape(B):
    """1 000 x 271 from the synthetic generator, on against off"""
    batch = B.TrajectoryBatch.synthetic(1000, 271, layout=0, seed=20250523)
    assert_same_bytes(on_and_off(B, batch), "1000 x 271 synthetic")


def test_the_table_of_one_launch_does_not_reach_the_next(B):
    """the table lives in uninitialised LDS: a clean batch, then a batch of misses with other stamps on the same context -- the second
    batch's bytes are the option-off bytes"""
    N = 271
    clean = B.TrajectoryBatch.from_host(*planted_batch(NB, N, 9700, clean=True), layout=0)
    ts, pos, quat, gps, valid, ip, iq = (a.copy() for a in planted_batch(NB, N, 9701, clean=True))
    ts = 5000.0 + (ts - ts[:, :1]) * 1.7
    rng = np.random.default_rng(9702)
    for b in range(NB):
        for i in rng.choice(np.arange(1, N), size=3, replace=False):
            gps[b, i, int(rng.integers(0, 3))] = np.nan
    misses = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)

    def both():
        run_pipeline(B, clean)
        return run_pipeline(B, misses)
    on = with_options(B, {"early_variances": 1, "duo_kernel": 0}, both)
    off = with_options(B, {"early_variances": 0, "duo_kernel": 0}, lambda: run_pipeline(B, misses))
    assert_same_bytes({1: on, 0: off}, "misses after a clean batch")
