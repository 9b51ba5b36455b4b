"""CPU tier of the noise-domain tests: the REFERENCES alone, on the grid the GPU tier (tests/test_ekf_noise_domain.py) runs the kernels on.

The scan-based EKF routes form the variances of a 64-pose chunk as a prefix product of 2x2 Moebius step matrices (variance_scan() in
gsf_wave_common.hpp).  Left unscaled, that product has entries of order lambda^64 (lambda: the larger eigenvalue of the step matrix of a
used fix, lambda + r^2/lambda = 2r + q dt) and leaves the range of a double for noise values and time units a user can put into
CONFIG['ekf'].  The grid below spans the stated contract (include/gsf.h):

    0 <= P0 <= 1e8,   1e-8 <= R <= 1e8,   0 <= Q dt <= 1e14,   finite inputs.

This file holds the grid, the host-made tracks, and `restate_ld`: a plain sequential np.longdouble restatement of the filtered and the
smoothed variances (Joseph update, dt = max(1e-6, delta t), RTS per outage: EKFGPSSLAM.py:712-731, :777-803), and checks on every case
that the references the GPU tier leans on -- restate() of tests/test_cov_host.py in float64, the oracle's dense 7x7 code -- agree with it,
that the oracle returns finite poses there, and that its status words are the restatement's.

Tolerances.  Filtered variances: 1e-10 relative (the suite's TOL): the float64 Joseph recursion was measured against longdouble over
q in {0, 1e-8 .. 1e4} x r in {1e-8 .. 1e8} x dt in {1e-6 .. 1e8}, 200 steps, worst deviation 1.03e-14.  Smoothed variances:
P_f[k] + g^2 (P_f[b] - P_p[b]) cancels, so the float64 form is only as good as the case allows.  Measured here, restate() against
restate_ld over the whole grid (test_references_agree_on_the_grid prints the figure of every case): worst 1.11e-9 relative (case
p1e6: the outage from pose 0 is smoothed from variances 5e6 times the result), 2.5e-10 on r1e-8-q1e-6, 8.9e-12 on q1e-4-r1e-6-100hz,
1.8e-12 on axes-apart, 2.6e-13 on q1e-4-r1e-4 and at most 6e-15 on the thirteen other cases.  The tolerance of a case, for the references here and for the kernels
in the GPU tier, is max(1e-10, 100 x that case's figure): computed from the two references, never from a kernel's output."""
import copy

import numpy as np
import pytest

from test_cov_host import restate

TOL = 1e-10
LENGTHS = [64, 65, 129, 200]            # one exact chunk, a one-pose tail, two chunk carries, a ragged tail
KINDS = ["all-used", "outage-in-chunk-0", "outage-to-lane-0", "sharp-outage", "outage-from-0", "outage-to-end", "repeated-stamps"]
VARIANTS = 9                            # per kind; plus one more all-used track: B = 64 per (case, length)
NB = len(KINDS) * VARIANTS + 1
GPS_OFFSET = np.array([150.0, -200.0, 30.0])
TICK = 1.0 / 8192.0                     # every stamp is a multiple of it: exact in a double under every scale and offset of the grid


def _case(name, P0=0.1, Q=0.1, R=0.2, tscale=1.0, offset=0.0, dn=0.1, beyond=False):
    """P0 / Q / R: a number (all three position axes alike) or three.  tscale: stamps are multiplied by it; offset: added to them;
    dn: nominal sampling step in seconds before the scaling; beyond: the unscaled float64 product of the step matrices over the longest
    run of used fixes of a chunk leaves the normal range (what the GPU tier logs and checks on its inputs)"""
    three = lambda v: [float(v)] * 3 if np.isscalar(v) else [float(x) for x in v]
    return dict(name=name, P0=three(P0), Q=three(Q), R=three(R), tscale=float(tscale), offset=float(offset), dn=float(dn), beyond=beyond)


DEFAULT_Q = [0.1, 0.1, 0.7]
GRID = [
    _case("default", Q=DEFAULT_Q),                                                      # 1: the control, the compiled-in noise layout
    _case("r1e2", R=1e2),                                                               # 2
    _case("r1e4", R=1e4),                                                               # 3
    _case("r1e6", R=1e6, beyond=True),                                                  # 4
    _case("r1e8-q1", R=1e8, Q=1.0, beyond=True),                                        # 5
    _case("q1e-4-r1e-4", Q=1e-4, R=1e-4),                                               # 6
    _case("q1e-4-r1e-6-100hz", Q=1e-4, R=1e-6, dn=0.01, beyond=True),                   # 7
    _case("r1e-8-q1e-6", Q=1e-6, R=1e-8, beyond=True),                                  # 8
    _case("q1e4", Q=[1e4, 1e4, 7e4]),                                                   # 9: x == y, z apart -- the default LAYOUT, so the early-variance build takes it
    _case("q1e6", Q=[1e6, 1e6, 7e6], beyond=True),                                      # 9, second
    _case("q0-p1", Q=0.0, P0=1.0),                                                      # 10
    _case("p1e6", P0=1e6, Q=DEFAULT_Q),                                                 # 11: the huge initial variance meets the carry-in
    _case("axes-apart", Q=[0.1, 1e-4, 0.7], R=[1e6, 1e-6, 0.2], beyond=True),           # 12: the generic build, one axis at each end
    _case("stamps-x1e3", Q=DEFAULT_Q, tscale=1e3),                                      # 13: time units, default noise
    _case("stamps-x1e6", Q=DEFAULT_Q, tscale=1e6, beyond=True),
    _case("stamps-x1e9", Q=DEFAULT_Q, tscale=1e9, beyond=True),
    _case("epoch-offset", Q=DEFAULT_Q, offset=1.7e9),
    _case("0.1hz", Q=DEFAULT_Q, dn=10.0),
]
CASES = {c["name"]: c for c in GRID}
DEFAULT_LAYOUT = [c["name"] for c in GRID if c["P0"][0] == c["P0"][1] and c["Q"][0] == c["Q"][1] and c["R"][0] == c["R"][1]
                  and not (c["P0"][2] == c["P0"][0] and c["Q"][2] == c["Q"][0] and c["R"][2] == c["R"][0])]


def case_config(base, case):
    """`base` (a CONFIG dict) with the case's noise on the position axes; the quaternion axes keep their defaults.  The yaw-rate gate is
    the default 45 deg/s expressed in the case's time unit (4.5 deg per nominal step), so that every case takes the same decisions."""
    cfg = copy.deepcopy(base)
    cfg["ekf"]["initial_cov_diag"] = case["P0"] + list(base["ekf"]["initial_cov_diag"][3:])
    cfg["ekf"]["process_noise_diag"] = case["Q"] + list(base["ekf"]["process_noise_diag"][3:])
    cfg["ekf"]["meas_noise_diag"] = list(case["R"])
    cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"] = 4.5 / (case["dn"] * case["tscale"])
    return cfg


# ------------------------------------------------------------------------------------------------ the tracks
def outages_of(kind, N):
    """[(a, b, sharp)] of a kind at length N (what does not fit a short track shrinks to what does), and the repeated stamps"""
    if kind == "outage-in-chunk-0":
        return [(20, 40, False)], []
    if kind == "outage-to-lane-0":                                       # recovery at lane 0 of the next chunk (N = 64: at the last pose)
        r = 128 if N > 128 else (64 if N > 64 else N - 1)
        return [(r - 14, r, False)], []
    if kind == "sharp-outage":
        return [(10, 20, True)], []
    if kind == "outage-from-0":
        return [(0, 5, False)], []
    if kind == "outage-to-end":
        return [(N - 9, N, False)], []
    if kind == "repeated-stamps":
        return [], [k for k in (1, 10, 24, 25, 50, N - 1) if 0 < k < N]
    return [], []


_tracks = {}


def make_batch(case, N):
    """The NB host-made tracks of a (case, length), trajectory-major, made once and never changed: dict of ts (B,N), pos, quat, gps, valid,
    init_pos, init_quat, kind (B,).  Positions within +-2 km of the origin, 2 m per pose; GNSS = 1.03 pos + offset + noise of sigma =
    min(sqrt(R), 300 m) per axis, NaN where the mask is clear.  Yaw: 0.2 deg per nominal step, 14 deg on the pairs of a sharp outage --
    far from the gate of 4.5 on either side."""
    key = (case["name"], N)
    if key in _tracks:
        return _tracks[key]
    names = [c["name"] for c in GRID]
    rng = np.random.default_rng(7000 + 100 * (names.index(case["name"]) if case["name"] in names else case["seed"]) + N)   # (campaign cases carry a seed)
    kinds = [k for k in KINDS for _ in range(VARIANTS)] + ["all-used"]
    B = len(kinds)
    dn_ticks = case["dn"] / TICK
    ticks = rng.integers(int(round(0.8 * dn_ticks)), int(round(1.2 * dn_ticks)) + 1, size=(B, N)); ticks[:, 0] = 0
    valid = np.ones((B, N), np.uint8)
    deg = np.full((B, N), 0.2) * rng.choice([-1.0, 1.0], size=(B, 1))
    for b, kind in enumerate(kinds):
        outs, rep = outages_of(kind, N)
        for a, e, sharp in outs:
            valid[b, a:e] = 0
            if sharp:
                deg[b, a + 1:min(e, a + 4)] = 14.0
        ticks[b, rep] = 0
    rel = ticks / dn_ticks                                               # the step as a share of the nominal one
    ts = (4096000 + np.cumsum(ticks, axis=1)) * TICK * case["tscale"] + case["offset"]     # 500 s + ...: exact
    yaw = rng.uniform(-np.pi, np.pi, size=(B, 1)) + np.cumsum(np.deg2rad(deg) * rel, axis=1)
    quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    quat = quat * rng.uniform(0.5, 2.0, size=(B, N, 1)) * rng.choice([-1.0, 1.0], size=(B, N, 1))
    step = 2.0 * np.stack([np.cos(yaw), np.sin(yaw), 0.01 * np.ones_like(yaw)], -1) * rel[..., None]
    pos = rng.uniform(-200.0, 200.0, size=(B, 1, 3)) + np.cumsum(step, axis=1)
    sigma = np.minimum(np.sqrt(np.array(case["R"])), 300.0)
    gps = 1.03 * pos + GPS_OFFSET + rng.normal(0.0, 1.0, size=(B, N, 3)) * sigma
    assert np.abs(pos).max() < 2000.0
    gps[valid == 0] = np.nan
    init_pos = np.where(np.isnan(gps[:, 0]), 1.03 * pos[:, 0] + GPS_OFFSET, gps[:, 0])
    init_quat = quat[:, 0] / np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    dts = np.diff(ts, axis=1)
    assert (dts[ticks[:, 1:] > 0] == (ticks[:, 1:] * (TICK * case["tscale"]))[ticks[:, 1:] > 0]).all()   # the steps are exact multiples
    out = dict(ts=ts, pos=pos, quat=quat, gps=gps, valid=valid, init_pos=init_pos, init_quat=init_quat, kind=np.array(kinds))
    for v in out.values():
        v.setflags(write=False)
    _tracks[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the longdouble restatement
def restate_ld(ts, gps, valid, segments, cfg):
    """Filtered, predicted and smoothed variances of a batch of tracks in np.longdouble, per axis, pose after pose.
    ts (B,N), gps (B,N,3), valid (B,N); segments: per track the [(a, b)] ranges handed to the smoother (the DECISIONS are restate()'s, the
    numbers are not).  -> filt, pred, cov, each (B,N,7) longdouble."""
    L = np.longdouble
    B, N = ts.shape
    P0, Q = (np.array(cfg["ekf"][k], dtype=L) for k in ("initial_cov_diag", "process_noise_diag"))
    R = np.array(cfg["ekf"]["meas_noise_diag"], dtype=L)
    filt, pred = np.empty((B, N, 7), L), np.empty((B, N, 7), L)
    filt[:, 0] = pred[:, 0] = P0
    av = (np.asarray(valid) != 0) & ~np.isnan(gps).any(axis=2)
    t = ts.astype(L)
    one = L(1)
    for i in range(1, N):
        dt = np.maximum(L(1e-6), t[:, i] - t[:, i - 1])                  # :865 (the clamp is the double 1e-6, as in the reference)
        Pp = filt[:, i - 1] + Q * dt[:, None]                            # :712-714
        Pf = Pp.copy()
        k = Pp[:, :3] / (Pp[:, :3] + R)                                  # :723-727
        upd = (one - k) * Pp[:, :3] * (one - k) + k * R * k              # :731
        Pf[:, :3] = np.where(av[:, i, None], upd, Pp[:, :3])
        pred[:, i], filt[:, i] = Pp, Pf
    cov = filt.copy()
    for b in range(B):
        for a, e in segments[b]:                                         # :785-801, backwards, as written (no closed form here)
            Ps = filt[b, e].copy()
            for j in range(e - 1, a - 1, -1):
                A = filt[b, j] / pred[b, j + 1]
                Ps = filt[b, j] + A * (Ps - pred[b, j + 1]) * A
                cov[b, j] = Ps
    return filt, pred, cov


def rel_dev(got, want):
    """largest relative deviation of a float64 array from the longdouble reference"""
    want = np.asarray(want, np.longdouble)
    return float(np.max(np.abs(np.asarray(got, np.longdouble) - want) / np.abs(want), initial=0.0))


_refs = {}


def references(case, N):
    """restate() of every track, the longdouble restatement, and the smoothed-variance tolerance of the (case, length), made once"""
    key = (case["name"], N)
    if key not in _refs:
        from oracle import oracle
        cfg = case_config(oracle.DEFAULT_CONFIG, case)
        t = make_batch(case, N)
        rs = [restate(t["ts"][b], t["quat"][b], t["gps"][b], t["valid"][b], cfg) for b in range(NB)]
        for r in rs:
            for rate, thr in r["rates"]:
                assert not (0.5 * thr <= rate <= 2.0 * thr), (key, rate, thr)       # no decision hangs on an ulp
        filt, pred, cov = restate_ld(t["ts"], t["gps"], t["valid"], [r["segments"] for r in rs], cfg)
        dev_f = max(rel_dev(r["filt"], filt[b]) for b, r in enumerate(rs))
        dev_s = max(rel_dev(r["cov"], cov[b]) for b, r in enumerate(rs))
        _refs[key] = dict(cfg=cfg, restate=rs, filt=filt, pred=pred, cov=cov, dev_filtered=dev_f, dev_smoothed=dev_s,
                          tol_smoothed=max(TOL, 100.0 * dev_s))
    return _refs[key]


def scan_product_range(case, N):
    """What the UNSCALED scan would hold: the float64 product of the step matrices [[r, r q dt], [1, q dt + r]] over the longest run of
    used fixes inside one 64-pose chunk of the all-used track, per axis.  -> (largest entry, smallest entry, steps) over the three axes
    (inf / 0 / denormal: the product has left the range)."""
    t = make_batch(case, N)
    dt = np.maximum(1e-6, np.diff(t["ts"][0]))                           # track 0: every fix used; the step into pose i is dt[i - 1]
    lo_, hi_ = (1, min(N, 64)) if N <= 64 or N - 64 < 63 else (64, min(N, 128))
    big, small = 0.0, np.inf
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for q, r in zip(case["Q"], case["R"]):
            M = np.eye(2)
            for i in range(lo_, hi_):
                b = q * dt[i - 1]
                M = np.array([[r, r * b], [1.0, b + r]]) @ M
            ent = M[M == M] if q > 0.0 else np.array([M[0, 0], M[1, 0], M[1, 1]])      # (q = 0: the entry r q dt IS zero)
            big, small = max(big, float(np.max(M))), min(small, float(np.min(ent)) if ent.size else 0.0)
            if not np.isfinite(M).all():
                big = np.inf
    return big, small, hi_ - lo_


def leaves_the_range(big, small):
    return not np.isfinite(big) or big > 1e300 or small < 1e-300


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("name", [c["name"] for c in GRID])
def test_references_agree_on_the_grid(orc, name):
    """restate() (float64) against restate_ld: filtered variances inside 1e-10, smoothed ones inside the case's tolerance (whose source,
    the measured deviation, is printed); flags and decisions consistent with the planted outages"""
    case = CASES[name]
    worst_f = worst_s = 0.0
    for N in LENGTHS:
        ref = references(case, N)
        t = make_batch(case, N)
        worst_f, worst_s = max(worst_f, ref["dev_filtered"]), max(worst_s, ref["dev_smoothed"])
        assert ref["dev_filtered"] < TOL, (name, N, ref["dev_filtered"])
        assert ref["dev_smoothed"] < ref["tol_smoothed"] and ref["tol_smoothed"] < 1e-6, (name, N, ref["dev_smoothed"])
        assert np.isfinite(ref["filt"].astype(float)).all() and (ref["cov"] > 0).all(), (name, N)
        for b, r in enumerate(ref["restate"]):
            outs, _ = outages_of(str(t["kind"][b]), N)
            want_sharp = [(a, e) for a, e, s in outs if s]
            want_seg = [(a, e) for a, e, s in outs if not s and e < N]
            assert r["sharp"] == want_sharp and r["segments"] == want_seg, (name, N, b)
    print(f"{name}: restate() vs longdouble: filtered {worst_f:.2e}, smoothed {worst_s:.2e} (relative)")


@pytest.mark.parametrize("name", [c["name"] for c in GRID])
def test_oracle_handles_the_grid(orc, name):
    """orc.fuse_batch / fuse_pipeline_batch return finite poses on every track of the grid and the status words of restate(); the oracle's
    own dense 7x7 variances (ekf_process_step, rts_smoother_segment) agree with the longdouble restatement on one track of every kind"""
    case = CASES[name]
    for N in LENGTHS:
        ref = references(case, N)
        cfg, t = ref["cfg"], make_batch(case, N)
        p, q, st = orc.fuse_batch(t["ts"], t["pos"], t["quat"], t["gps"], t["valid"], t["init_pos"], t["init_quat"], cfg)
        assert np.isfinite(p).all() and np.isfinite(q).all(), (name, N)
        np.testing.assert_array_equal(st, [r["status"] for r in ref["restate"]], err_msg=f"{name} N={N}")
        pp, qp, stp, Rr, tr, sr = orc.fuse_pipeline_batch(t["ts"], t["pos"], t["quat"], t["gps"], t["valid"], cfg, fit_rows="all")
        assert np.isfinite(pp).all() and np.isfinite(qp).all() and np.isfinite(sr).all(), (name, N)
        np.testing.assert_array_equal(stp & 15, st, err_msg=f"{name} N={N} pipeline")
    # the oracle's variances, N = 129: the first track of every kind
    N = 129
    ref, t = references(case, N), make_batch(case, N)
    cfg = ref["cfg"]
    worst_f = worst_s = 0.0
    for b in range(0, len(KINDS) * VARIANTS, VARIANTS):
        av = (t["valid"][b] != 0) & ~np.isnan(t["gps"][b]).any(axis=1)
        state, cov = np.array([0.0, 0, 0, 0, 0, 0, 1]), np.diag(np.array(cfg["ekf"]["initial_cov_diag"], float))
        Pf, Pp = np.empty((N, 7, 7)), np.empty((N, 7, 7))
        Pf[0] = Pp[0] = cov
        gp, w = bool(t["valid"][b, 0]), 0.0
        for i in range(1, N):
            dt = max(1e-6, t["ts"][b, i] - t["ts"][b, i - 1])
            z = t["gps"][b, i] if av[i] else None
            state, cov, ps, pc, gp, w = orc.ekf_process_step(cfg, state, cov, gp, w, 0, (np.zeros(3), np.array([0.0, 0, 0, 1])), z, bool(av[i]), dt)
            state[:3] = 0.0                                              # (the variances do not depend on the state)
            Pf[i], Pp[i] = cov, pc
        diag = lambda M: np.diagonal(M, axis1=-2, axis2=-1)
        assert (np.abs(Pf - diag(Pf)[..., None] * np.eye(7)) == 0).all(), (name, b)     # the covariance stays diagonal
        worst_f = max(worst_f, rel_dev(diag(Pf), ref["filt"][b]))
        for a, e in ref["restate"][b]["segments"]:
            xs = np.tile(np.array([0.0, 0, 0, 0, 0, 0, 1]), (e - a + 1, 1))
            _, Ps = orc.rts_smoother_segment(xs, Pf[a:e + 1], xs, Pp[a:e + 1])
            worst_s = max(worst_s, rel_dev(diag(Ps)[:-1], ref["cov"][b, a:e]))
    print(f"{name}: oracle vs longdouble: filtered {worst_f:.2e}, smoothed {worst_s:.2e} (relative), tolerance of the smoothed ones {ref['tol_smoothed']:.2e}")
    assert worst_f < TOL and worst_s < ref["tol_smoothed"], (name, worst_f, worst_s)


def test_the_grid_spans_the_contract_and_stresses_the_scan():
    """the unscaled float64 product of the step matrices over a chunk's longest run of used fixes: inside the range of a double for the
    cases the suite covered before, outside it for the ones marked `beyond` -- the inputs are the ones the issue is about"""
    for case in GRID:
        assert all(0.0 <= p <= 1e8 for p in case["P0"]) and all(1e-8 <= r <= 1e8 for r in case["R"])
        assert all(0.0 <= q * 1.2 * case["dn"] * case["tscale"] <= 1e14 for q in case["Q"])
        for N in LENGTHS:
            big, small, steps = scan_product_range(case, N)
            print(f"{case['name']} N={N}: unscaled product over {steps} used fixes: largest entry {big:.3g}, smallest {small:.3g}")
            assert steps >= 63
            assert leaves_the_range(big, small) == case["beyond"], (case["name"], N, big, small)
    assert sorted(DEFAULT_LAYOUT) == sorted(["default", "q1e4", "q1e6", "p1e6", "stamps-x1e3", "stamps-x1e6", "stamps-x1e9", "epoch-offset", "0.1hz"])
