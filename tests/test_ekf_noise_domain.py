"""GPU tier of the noise-domain tests: every scan-based EKF route on the grid of tests/test_ekf_noise_domain_host.py, i.e. over the whole
stated contract  0 <= P0 <= 1e8,  1e-8 <= R <= 1e8,  0 <= Q dt <= 1e14  (include/gsf.h).

The routes form the variances of a chunk as a prefix product of 2x2 Moebius step matrices (variance_scan(), gsf_wave_common.hpp).  Without
a rescale that product is of order lambda^64 and leaves the range of a double on the cases the grid marks `beyond` (GNSS noise of 1e6 and
more or of 1e-6 and less, process noise of 1e6, stamps in microseconds or nanoseconds): the quotient is then inf/inf or 0/0 and the route
returns NaN poses, while the sequential lane kernel and the oracle return the right ones.  test_inputs_stress_the_scan logs the size of
that product for every case.

Gates.  Poses against oracle.fuse_batch / fuse_pipeline_batch under the same config: POS_TOL = 1e-7 m, Q_TOL = 1e-9, status words exact
(tests/test_gpu_parity.py).  Variances against the np.longdouble restatement: filtered 1e-10 relative, smoothed max(1e-10, 100 x what
float64 restate() deviates from longdouble on that case) -- taken from the two references in the host file, never from a kernel.  Flags
exact against restate().  No output word NaN or inf where the oracle's is finite."""
import contextlib

import numpy as np
import pytest

from test_ekf_noise_domain_host import (CASES, DEFAULT_LAYOUT, GRID, LENGTHS, NB, TOL, case_config, leaves_the_range, make_batch, references,
                                        rel_dev, scan_product_range)

pytestmark = pytest.mark.gpu

POS_TOL = 1e-7
Q_TOL = 1e-9
NAMES = [c["name"] for c in GRID]
BIG_B = 2049                            # the smallest batch the big-batch build takes (B > 2 048)
EARLY_B, EARLY_N = 1000, 256            # the smallest shape the early-variance build is chosen for by itself
# the early-variance build exists for the default noise LAYOUT only: the time-unit cases, and case 9
EARLY_CASES = ["stamps-x1e3", "stamps-x1e6", "stamps-x1e9", "epoch-offset", "0.1hz", "q1e4", "q1e6"]
FIT_BIT = 16 << 8                       # (set by the wave kernels' fit, not by the oracle's: masked as in tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@contextlib.contextmanager
def options(B, **opts):
    """context options for the duration of a block, restored to their defaults afterwards"""
    defaults = {"lane_min_traj": 32768, "block_kernel": -1, "duo_kernel": -1, "early_variances": -1}
    ctx = B.context()
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield ctx
    finally:
        for k in opts:
            ctx.set_option(k, defaults[k])


_oracle = {}


def oracle_poses(orc, B, case, N):
    """oracle.fuse_batch and oracle.fuse_pipeline_batch (every valid row) of the 64 tracks of a (case, length): once, shared by the routes"""
    key = (case["name"], N)
    if key not in _oracle:
        from gps_optimize_slam_amd import ekfgpsslam as E
        cfg, t = case_config(E.CONFIG, case), make_batch(case, N)
        k4 = orc.fuse_batch(t["ts"], t["pos"], t["quat"], t["gps"], t["valid"], t["init_pos"], t["init_quat"], cfg)
        pipe = orc.fuse_pipeline_batch(t["ts"], t["pos"], t["quat"], t["gps"], t["valid"], cfg, fit_rows="all")[:3]
        assert all(np.isfinite(x).all() for x in k4[:2] + pipe[:2]), key    # (the CPU tier shows the same: inputs the reference handles)
        for x in k4 + pipe:
            x.setflags(write=False)
        _oracle[key] = dict(cfg=cfg, k4=k4, pipe=pipe)
    return _oracle[key]


def tiled(t, nb):
    """the 64 tracks repeated up to nb tracks"""
    reps = -(-nb // NB)
    return [np.concatenate([t[k]] * reps)[:nb] for k in ("ts", "pos", "quat", "gps", "valid", "init_pos", "init_quat")]


def check_poses(what, got, want, rows, pipeline, problems):
    """got = (pos, quat, status) of the route for the batch rows `rows`; want = the oracle's for the 64 tracks (row b of the batch is track
    b % 64).  Prints the figures, then appends what misses the gates to `problems`."""
    p, q, st = (x[rows] for x in got)
    po, qo, sto = (x[rows % NB] for x in want)
    finite = bool(np.isfinite(p).all() and np.isfinite(q).all())
    with np.errstate(invalid="ignore"):
        ep, eq = float(np.nanmax(np.abs(p - po), initial=0.0)), float(np.nanmax(np.abs(q - qo), initial=0.0))
    bad_st = int(((st & ~FIT_BIT) != sto).sum()) if pipeline else int((st != sto).sum())
    n_bad = int((~(np.isfinite(p).all(axis=(1, 2)) & np.isfinite(q).all(axis=(1, 2)))).sum())
    print(f"{what}: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, {n_bad} of {len(rows)} tracks with NaN/inf, {bad_st} status words differ")
    if not finite:
        problems.append((what, f"{n_bad} tracks hold NaN or inf where the oracle is finite"))
    if bad_st:
        problems.append((what, f"{bad_st} status words differ"))
    if not (ep < POS_TOL and eq < Q_TOL):
        problems.append((what, f"max |dp| {ep:.3e}, max |dq| {eq:.3e}"))


# Every (case, length) through every pose route.  name -> (layout, options, batch size, pipeline, lengths).  The block kernel takes tracks
# of 65 .. 1 024 poses, so N = 64 is left out of ITS list (a forced block_kernel = 1 would run the wave kernel there).
ROUTES = {
    "wave-small": (0, {}, NB, False, LENGTHS),                            # ekf_wave_kernel, the build for B <= 2 048
    "wave-big": (0, {}, BIG_B, False, LENGTHS),                           # ekf_wave_big_kernel: the same tracks tiled to 2 049
    "time-major": (1, {}, NB, False, LENGTHS),                            # through the transposes to the wave kernel (B < lane_min_traj)
    "lane": (1, {"lane_min_traj": 0}, NB, False, LENGTHS),                # the sequential lane-per-trajectory kernel: the control
    "block": (0, {"block_kernel": 1}, NB, False, [N for N in LENGTHS if N > 64]),
    "pipeline-two-wave": (0, {}, NB, True, LENGTHS),                      # fuse_pipeline_batch, B <= 256: ekf_wave_duo_kernel for N > 64
}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_pose_routes_on_the_grid(B, orc, route, name):
    case = CASES[name]
    layout, opts, nb, pipeline, lengths = ROUTES[route]
    problems = []
    for N in lengths:
        want = oracle_poses(orc, B, case, N)
        with options(B, **opts) as ctx:
            # which kernel the launcher picks follows from these (launch_ekf_wave, gsf_ekf_fuse_batch_dev): checked, not assumed
            assert ctx.options.get("lane_min_traj", 32768) == (0 if route == "lane" else 32768)
            assert ctx.options.get("block_kernel", -1) == (1 if route == "block" else -1) and ctx.options.get("duo_kernel", -1) == -1
            assert (nb > 2048) == (route == "wave-big") and (route != "block" or 64 < N <= 1024)
            batch = B.TrajectoryBatch.from_host(*tiled(make_batch(case, N), nb), layout=layout)
            assert batch.layout == layout and batch.B == nb and batch.N == N
            if pipeline:
                got = B.fuse_pipeline_batch(batch, config=want["cfg"], fit_rows="all")[0].host_traj_major()
            else:
                got = B.ekf_fuse_batch(batch, config=want["cfg"]).host_traj_major()
        # the big batch: first and last tile and every 32nd track between (the tiles are copies of the 64 tracks)
        rows = np.arange(nb) if nb == NB else np.unique(np.r_[0:NB, nb - NB:nb, 0:nb:32])
        check_poses(f"{name} N={N} {route}", got, want["pipe" if pipeline else "k4"], rows, pipeline, problems)
    assert not problems, problems


@pytest.mark.parametrize("name", EARLY_CASES)
def test_early_variance_build_on_the_grid(B, orc, name):
    """1 000 equal-length tracks of 256 poses, the build forced as tests/test_early_variances.py forces it (it is the automatic choice at
    this shape as well); the cases that keep the default noise layout"""
    case = CASES[name]
    assert name in DEFAULT_LAYOUT and 64 < EARLY_N <= 384 and EARLY_B <= 2048            # where the build applies (launch_ekf_wave)
    want = oracle_poses(orc, B, case, EARLY_N)
    with options(B, early_variances=1, duo_kernel=0) as ctx:
        assert ctx.options["early_variances"] == 1 and ctx.options["duo_kernel"] == 0
        batch = B.TrajectoryBatch.from_host(*tiled(make_batch(case, EARLY_N), EARLY_B), layout=0)
        got = B.fuse_pipeline_batch(batch, config=want["cfg"], fit_rows="all")[0].host_traj_major()
    problems = []
    rows = np.unique(np.r_[0:NB, EARLY_B - NB:EARLY_B, 0:EARLY_B:32])
    check_poses(f"{name} N={EARLY_N} early-variance build", got, want["pipe"], rows, True, problems)
    assert not problems, problems


@pytest.mark.parametrize("name", NAMES)
def test_covariance_kernel_on_the_grid(B, name):
    """ekf_covariance_ragged on the tracks of all four lengths as ONE ragged batch"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    case = CASES[name]
    cfg = case_config(E.CONFIG, case)
    ts_ = [make_batch(case, N) for N in LENGTHS]
    lens = np.concatenate([[N] * NB for N in LENGTHS])
    offs = np.zeros(len(lens) + 1, np.int64); offs[1:] = np.cumsum(lens)
    dev = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    cat = lambda k, shape: np.concatenate([t[k].reshape(shape) for t in ts_])
    r = B.ekf_covariance_ragged(dev(cat("ts", (-1,))), dev(cat("quat", (-1, 4))), dev(cat("gps", (-1, 3))), dev(cat("valid", (-1,))), dev(offs), config=cfg)
    torch.cuda.synchronize()
    filt, cov, flags, status = (x.cpu().numpy() for x in (r.filtered, r.cov, r.flags, r.status))
    problems = []
    for j, N in enumerate(LENGTHS):
        ref = references(case, N)
        sl = slice(offs[j * NB], offs[(j + 1) * NB])
        f, c = filt[sl].reshape(NB, N, 7), cov[sl].reshape(NB, N, 7)
        finite = bool(np.isfinite(f).all() and np.isfinite(c).all())
        with np.errstate(invalid="ignore"):
            ef, es = rel_dev(np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0), ref["filt"]), rel_dev(np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0), ref["cov"])
        print(f"{name} N={N} covariance kernel: filtered {ef:.2e} (gate {TOL:.0e}), smoothed {es:.2e} (gate {ref['tol_smoothed']:.2e}; float64 restate() "
              f"deviates {ref['dev_smoothed']:.2e}), finite: {finite}")
        if not finite:
            problems.append((N, "NaN or inf variances"))
        if not (ef < TOL and es < ref["tol_smoothed"]):
            problems.append((N, f"filtered {ef:.3e}, smoothed {es:.3e}"))
        want_flags = np.stack([w["flags"] for w in ref["restate"]])
        if not np.array_equal(flags[sl].reshape(NB, N), want_flags):
            problems.append((N, "flags differ"))
        if not np.array_equal(status[j * NB:(j + 1) * NB], [w["status"] for w in ref["restate"]]):
            problems.append((N, "status words differ"))
    assert not problems, (name, problems)


def test_inputs_stress_the_scan():
    """the record of which cases lie beyond the range of the UNSCALED product (float64, host side, the longest run of used fixes of a
    chunk): the cases marked `beyond` are the ones a scan without a rescale cannot pass"""
    for case in GRID:
        for N in LENGTHS:
            big, small, steps = scan_product_range(case, N)
            print(f"{case['name']} N={N}: unscaled product of {steps} step matrices: largest entry {big:.3g}, smallest {small:.3g}"
                  f"{'  <-- outside the range of a double' if leaves_the_range(big, small) else ''}")
            assert steps >= 63 and leaves_the_range(big, small) == case["beyond"], (case["name"], N, big, small)
    assert sum(c["beyond"] for c in GRID) == 8
