"""GPU tier (-m gpu): the HIP path, called through the C ABI, against (i) the reference-generated goldens,
(ii) the CPU oracle on the same seeded inputs, (iii) size-independent properties at larger sizes.

Gates (BASELINE.json north_star): timestamps / masks / indices / status bits exact; fused positions within
1e-6 m of the CPU reference (we assert 1e-7 against goldens and the oracle -- the observed gap is ~1e-9);
quaternion components within 1e-9."""
import copy
import json

import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

POS_GATE = 1e-6      # the stated gate
POS_TOL = 1e-7       # what we actually assert
Q_TOL = 1e-9


@pytest.fixture(scope="module")
def E():
    from gps_optimize_slam_amd import ekfgpsslam
    from gps_optimize_slam_amd import _lib
    assert _lib.load().gsf_device_count() > 0, "GPU tests need a device"
    return ekfgpsslam


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def merged_cfg(E, over):
    c = copy.deepcopy(E.CONFIG)
    for sec, kv in over.items():
        c[sec].update(kv)
    return c


# ------------------------------------------------------------------ goldens through the drop-in surface
def test_kat1_kat2(E, golden):
    g = golden("kat_bundled.npz")
    R, t, s = E.compute_sim3_transform(g["pos"], g["gt"])
    assert abs(s - 0.9983676300208674) < 1e-12
    np.testing.assert_allclose(R, g["kat1_R"], atol=5e-12, rtol=0)
    np.testing.assert_allclose(s * g["pos"] @ R.T + t, g["kat2_pos"], atol=1e-9, rtol=0)
    p, q = E.transform_trajectory(g["pos"], g["quat"], g["kat1_R"], g["kat1_t"], float(g["kat1_s"]))
    np.testing.assert_allclose(p, g["kat2_pos"], atol=1e-10, rtol=0)
    np.testing.assert_allclose(q, g["kat2_quat"], atol=1e-12, rtol=0)


@pytest.mark.parametrize("kat", ["kat3", "kat4"])
def test_kat34_apply_ekf_correction(E, golden, kat):
    g = golden("kat_bundled.npz")
    slam = {"timestamps": g["ts"], "positions": g["pos"], "quaternions": g["quat"]}
    gps = {"timestamps": g["ts"], "positions": g["gt"]} if kat == "kat3" else {"timestamps": g["kat4_gps_t"], "positions": g["kat4_gps_p"]}
    p, q = E.apply_ekf_correction(slam, gps, g["kat2_pos"], g["kat2_quat"], E.CONFIG)
    np.testing.assert_allclose(p, g[f"{kat}_pos"], atol=1e-8, rtol=0)
    np.testing.assert_allclose(q, g[f"{kat}_quat"], atol=1e-12, rtol=0)
    with pytest.raises(ValueError):
        E.apply_ekf_correction(slam, gps, g["kat2_pos"][:-1], g["kat2_quat"][:-1], E.CONFIG)
    pe, qe = E.apply_ekf_correction({"timestamps": np.empty(0), "positions": np.empty((0, 3)), "quaternions": np.empty((0, 4))}, gps,
                                    np.empty((0, 3)), np.empty((0, 4)), E.CONFIG)
    assert pe.shape == (0, 3) and qe.shape == (0, 4)


@pytest.mark.parametrize("tag", ["kitti04gps", "combined"])
def test_c1_pipeline_stages(E, golden, tag):
    """Config C1: bundled KITTI-04 files, every device stage vs the reference's own outputs."""
    g, k = golden(f"c1_{tag}.npz"), golden("kat_bundled.npz")
    proj = E.UtmProjector(int(g["zone"]), bool(g["south"]))
    e, n = proj(g["lon"], g["lat"])
    np.testing.assert_allclose(np.column_stack((e, n)), g["utm"][:, :2], atol=5e-9, rtol=0)      # vs oracle series (unpinned vs pyproj)
    lon2, lat2 = proj(e, n, inverse=True)
    np.testing.assert_allclose(lon2, g["lon"], atol=1e-12); np.testing.assert_allclose(lat2, g["lat"], atol=1e-12)
    idx = g["sim3_idx"]
    R, t, s, mask, nin = E.sim3_ransac_with_indices(k["pos"][idx], g["aligned"][idx], g["sample_idx"], 4.0, 4)
    assert nin == int(g["n_inliers"]) == int(mask.sum())
    np.testing.assert_allclose(R, g["R"], atol=5e-12, rtol=0)
    assert abs(s - float(g["s"])) < 1e-12
    np.testing.assert_allclose(s * k["pos"] @ R.T + t, g["sim3_pos"], atol=POS_TOL, rtol=0)
    sp, sq = E.transform_trajectory(k["pos"], k["quat"], g["R"], g["t"], float(g["s"]))
    np.testing.assert_allclose(sp, g["sim3_pos"], atol=1e-8, rtol=0)
    np.testing.assert_allclose(sq, g["sim3_quat"], atol=1e-12, rtol=0)
    slam = {"timestamps": k["ts"], "positions": k["pos"], "quaternions": k["quat"]}
    p, q = E.apply_ekf_correction(slam, {"timestamps": g["gps_t"], "positions": g["gps_p"]}, g["sim3_pos"], g["sim3_quat"], E.CONFIG)
    np.testing.assert_allclose(p, g["ekf_pos"], atol=POS_TOL, rtol=0)
    np.testing.assert_allclose(q, g["ekf_quat"], atol=Q_TOL, rtol=0)
    ate = np.sqrt(np.mean(np.sum((p - g["ekf_pos"]) ** 2, axis=1)))
    assert ate < POS_GATE


def test_c1_seeded_end_to_end(E, golden, tmp_path):
    """np.random.seed(0) + the same RNG call order as the reference => same RANSAC draws => same result."""
    g, k = golden("c1_combined.npz"), golden("kat_bundled.npz")
    slam = {"timestamps": k["ts"], "positions": k["pos"], "quaternions": k["quat"]}
    gps = {"timestamps": g["gps_t"], "positions": g["gps_p"]}
    aligned, valid = E.dynamic_time_alignment(slam, gps, E.CONFIG["time_alignment"])
    idx = E.pick_sim3_indices(slam, valid)
    np.random.seed(0)
    _ = E.filter_gps_outliers_ransac(g["gps_t_raw"], g["utm"], E.CONFIG["gps_filtering_ransac"])   # consumes the same draws as the golden run
    np.random.seed(0)
    sc = E.CONFIG["sim3_ransac"]
    R, t, s = E.compute_sim3_transform_robust(k["pos"][idx], aligned[idx], sc["min_samples"], sc["residual_threshold"], sc["max_trials"], sc["min_inliers_needed"])
    assert abs(s - float(g["s"])) < 1e-12
    sp, sq = E.transform_trajectory(k["pos"], k["quat"], R, t, s)
    p, q = E.apply_ekf_correction(slam, gps, sp, sq, E.CONFIG)
    np.testing.assert_allclose(p, g["ekf_pos"], atol=POS_TOL, rtol=0)
    out = tmp_path / "yolotum04_corrected_utm.txt"
    E.save_tum_utm(str(out), k["ts"], p, q)
    txt = np.loadtxt(str(out), skiprows=1)
    np.testing.assert_array_equal(txt[:, 0], np.round(k["ts"], 6))          # %.6f of the untouched input column


def test_sim3_cases(E, golden):
    g = golden("sim3_cases.npz")
    for name in g["names"]:
        src, dst = g[f"{name}_src"], g[f"{name}_dst"]
        R, t, s = E.compute_sim3_transform(src, dst)
        if bool(g[f"{name}_none"]):
            assert R is None, name
            continue
        assert R is not None, name
        if name in ("planar", "zerovar"):
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
            assert abs(s - float(g[f"{name}_s"])) < 1e-12
            continue
        np.testing.assert_allclose(R, g[f"{name}_R"], atol=1e-11, rtol=0, err_msg=str(name))
        np.testing.assert_allclose(s * src @ R.T + t, float(g[f"{name}_s"]) * src @ g[f"{name}_R"].T + g[f"{name}_t"], atol=POS_TOL, rtol=0)
        assert abs(s - float(g[f"{name}_s"])) < 1e-11 * max(1.0, s), name
    for k in g["tt_names"]:
        p, q = E.transform_trajectory(g["tt_in_pos"], g["tt_in_quat"], g[f"tt_{k}_R"], g[f"tt_{k}_t"], float(g[f"tt_{k}_s"]))
        np.testing.assert_allclose(p, g[f"tt_{k}_pos"], atol=1e-10, rtol=0)
        np.testing.assert_allclose(q, g[f"tt_{k}_quat"], atol=1e-12, rtol=0)
    qz = g["tt_in_quat"].copy(); qz[3] = 0.0
    with pytest.raises(ValueError):
        E.transform_trajectory(g["tt_in_pos"], qz, np.eye(3), np.zeros(3), 1.0)


def test_ransac_cases(E, golden):
    g = golden("sim3_cases.npz")
    for name in g["rs_names"]:
        ms, thr, trials, need = g[f"rs_{name}_par"]
        src, dst, idx = g[f"rs_{name}_src"], g[f"rs_{name}_dst"], g[f"rs_{name}_idx"]
        if idx.size == 0:
            assert E.compute_sim3_transform_robust(src, dst, int(ms), thr, int(trials), int(need))[0] is None
            continue
        R, t, s, mask, nin = E.sim3_ransac_with_indices(src, dst, idx, thr, int(need))
        if bool(g[f"rs_{name}_none"]):
            assert R is None, name
            continue
        np.testing.assert_array_equal(mask, g[f"rs_{name}_mask"], err_msg=str(name))
        assert nin == int(mask.sum())
        np.testing.assert_allclose(R, g[f"rs_{name}_R"], atol=1e-11, rtol=0)
        np.testing.assert_allclose(s * src @ R.T + t, float(g[f"rs_{name}_s"]) * src @ g[f"rs_{name}_R"].T + g[f"rs_{name}_t"], atol=POS_TOL, rtol=0)


def test_ekf_cases(E, orc, golden):
    g = golden("ekf_cases.npz")
    worst = 0.0
    for name in g["names"]:
        cfg = merged_cfg(E, json.loads(str(g[f"{name}_cfg"])))
        args = (g[f"{name}_ts"], g[f"{name}_pos"], g[f"{name}_quat"], g[f"{name}_aligned"], g[f"{name}_valid"], g[f"{name}_sp0"], g[f"{name}_sq0"])
        p, q, st = E.ekf_fuse_aligned(*args, cfg)
        np.testing.assert_allclose(p, g[f"{name}_out_pos"], atol=POS_TOL, rtol=0, err_msg=str(name))
        np.testing.assert_allclose(q, g[f"{name}_out_quat"], atol=Q_TOL, rtol=0, err_msg=str(name))
        _, _, st_o = orc.apply_ekf_correction_aligned(*args, cfg, return_status=True)
        assert st == st_o, (name, st, st_o)
        worst = max(worst, np.abs(p - g[f"{name}_out_pos"]).max())
    assert worst < POS_GATE


def test_utm_all_zones_vs_mpmath_definition(E, B, golden):
    """K1 on the device, both directions, on the 240 points of all 60 zones (gen_utm_mpmath.py --zones: both hemispheres, zone edges, half
    a degree outside them): forward within 5e-9 m of the 50-digit definition-level values, the inverse (direct Gaussian-latitude series,
    round 5) within 1e-13 degree of the pre-image, round trip within 1e-9 m (easting) / 3e-9 m (northing) -- one batched call per direction, each point in its own zone."""
    import torch
    g = golden("utm_zones_mpmath.npz")
    n = len(g["lat"])
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    offs = torch.arange(0, n + 1, dtype=torch.int64, device="cuda")
    zone, south = dev(g["zone"], torch.int32), dev(g["south"], torch.int32)
    e, nn, _, _ = B.utm_forward_batch(dev(g["lat"]), dev(g["lon"]), offs, zone, south)
    assert (e.cpu().numpy() - g["E"]).__abs__().max() < 5e-9 and (nn.cpu().numpy() - g["N"]).__abs__().max() < 5e-9
    la, lo = B.utm_inverse_batch(dev(g["E"]), dev(g["N"]), offs, zone, south)
    dla, dlo = np.abs(la.cpu().numpy() - g["lat"]).max(), np.abs(lo.cpu().numpy() - g["lon"]).max()
    assert dla < 1e-13 and dlo < 1e-13, (dla, dlo)
    e2, n2, _, _ = B.utm_forward_batch(la, lo, offs, zone, south)
    # (a latitude beyond 64 degrees is spaced 1.6e-9 m, a northing beyond 4.2e6 m up to 1.9e-9 m: eastings hold 1e-9 m, northings 3e-9 m)
    assert np.abs(e2.cpu().numpy() - g["E"]).max() <= 1e-9 and np.abs(n2.cpu().numpy() - g["N"]).max() <= 3e-9


def test_utm_vs_mpmath_definition(E, golden):
    g = golden("utm_mpmath.npz")
    for la, lo, z, s, Ee, Nn in zip(g["lat"], g["lon"], g["zone"], g["south"], g["E"], g["N"]):
        proj = E.UtmProjector(int(z), bool(s))
        e, n = proj(np.array([lo]), np.array([la]))
        if la == 0.0 or lo == 0.0:            # rows the reference's validity mask drops (ref :259) come back NaN
            assert np.isnan(e[0]) and np.isnan(n[0])
            continue
        assert abs(e[0] - Ee) < 5e-9 and abs(n[0] - Nn) < 5e-9, (la, lo, e[0] - Ee, n[0] - Nn)
        lo2, la2 = proj(e, n, inverse=True)
        assert abs(la2[0] - la) < 1e-12 and abs(lo2[0] - lo) < 1e-12
    proj = E.UtmProjector(32, False)
    e, n = proj(np.array([8.4, 0.0, 200.0, 8.4]), np.array([49.0, 49.0, 49.0, 95.0]))     # ref :259 invalid rows -> NaN
    assert np.isfinite(e[0]) and np.isnan(e[1:]).all() and np.isnan(n[1:]).all()


# ------------------------------------------------------------------ batches vs the oracle on the same seeded inputs
@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


import contextlib


@contextlib.contextmanager
def route(B, layout):
    """layout "lane": a time-major batch on the lane-per-trajectory kernel even when it is small (by default time-major batches
    below 32 768 trajectories are transposed and run by the wave-per-trajectory kernel -- layout 1 then exercises that route)."""
    if layout == "lane":
        B.context().set_option("lane_min_traj", 0)
    try:
        yield 1 if layout == "lane" else layout
    finally:
        if layout == "lane":
            B.context().set_option("lane_min_traj", 32768)


LAYOUTS = [0, 1, "lane"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", [271, 64, 65, 1000, 3])
def test_synth_batch_vs_oracle(B, orc, layout, N):
    """Config C2-shaped batch (KITTI-04 length) -- every trajectory against the dense-7x7 CPU oracle."""
    nb = 700 if N < 1000 else 300
    with route(B, layout) as lay:
        batch = B.TrajectoryBatch.synthetic(nb, N, layout=lay, seed=7)
        out = B.ekf_fuse_batch(batch)
    h = batch.host_traj_major()
    p, q, st = out.host_traj_major()
    po, qo, sto = orc.fuse_batch(h["ts"], h["pos"], h["quat"], h["gps"], h["valid"], h["init_pos"], h["init_quat"])
    np.testing.assert_array_equal(st, sto)
    assert np.abs(p - po).max() < POS_TOL
    assert np.abs(q - qo).max() < Q_TOL
    ate = np.sqrt(np.mean(np.sum((p - po) ** 2, axis=2)))
    assert ate < POS_GATE
    # the generator really exercises the outage / RTS / sharp-turn machinery
    if N == 271:
        assert (st & 2).sum() > 20 and (st & 8).sum() > 3 and (st & 4).sum() >= 1


def test_layouts_agree_and_shard_invariant(B):
    """time-major on the lane kernel = lane-per-trajectory recursion, trajectory-major = wave-per-trajectory scans: two different
    evaluation orders of the same filter must agree far inside the gate; the status bits exactly.  A SMALL time-major batch takes
    the transpose -> wave kernel -> transpose route by default and must then equal the trajectory-major result bit for bit."""
    nb, N = 3000, 200
    tm = B.TrajectoryBatch.synthetic(nb, N, layout=1, seed=11)
    pj = tm.to_layout(0)
    with route(B, "lane"):
        p1, q1, s1 = B.ekf_fuse_batch(tm).host_traj_major()
    p0, q0, s0 = B.ekf_fuse_batch(pj).host_traj_major()
    assert np.abs(p1 - p0).max() < POS_TOL and np.abs(q1 - q0).max() < Q_TOL
    np.testing.assert_array_equal(s1, s0)
    pw, qw, sw = B.ekf_fuse_batch(tm).host_traj_major()                 # default route of a small time-major batch
    np.testing.assert_array_equal(pw, p0); np.testing.assert_array_equal(qw, q0); np.testing.assert_array_equal(sw, s0)
    ow, Rw, tw, sw_ = B.fuse_pipeline_batch(tm)
    oj, Rj, tj, sj = B.fuse_pipeline_batch(pj)
    for x, y in zip(ow.host_traj_major(), oj.host_traj_major()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(Rw.cpu().numpy(), Rj.cpu().numpy())
    # shards generated independently (traj0 offset) == slices of the full batch, bit for bit
    parts0 = [B.ekf_fuse_batch(B.TrajectoryBatch.synthetic(1000, N, layout=0, seed=11, traj0=k * 1000)).host_traj_major() for k in range(3)]
    np.testing.assert_array_equal(np.concatenate([x[0] for x in parts0]), p0)
    np.testing.assert_array_equal(np.concatenate([x[1] for x in parts0]), q0)
    np.testing.assert_array_equal(np.concatenate([x[2] for x in parts0]), s0)
    with route(B, "lane"):
        parts = [B.ekf_fuse_batch(B.TrajectoryBatch.synthetic(1000, N, layout=1, seed=11, traj0=k * 1000)).host_traj_major() for k in range(3)]
    np.testing.assert_array_equal(np.concatenate([x[0] for x in parts]), p1)
    np.testing.assert_array_equal(np.concatenate([x[2] for x in parts]), s1)


@pytest.mark.parametrize("fit_rows", ["reference", "all"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pipeline_batch_vs_oracle(B, orc, layout, fit_rows):
    nb, N = 400, 271
    with route(B, layout) as lay:
        batch = B.TrajectoryBatch.synthetic(nb, N, layout=lay, seed=3)
        out, R, t, s = B.fuse_pipeline_batch(batch, fit_rows=fit_rows)
    h = batch.host_traj_major()
    p, q, st = out.host_traj_major()
    R, t, s = R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy()
    for b in range(0, nb, 7):
        m = h["valid"][b].astype(bool) & ~np.isnan(h["gps"][b]).any(axis=1)
        if fit_rows == "reference":                                         # the rows main_process_gui hands to its fit (ref :973-998)
            m = orc.pick_sim3_rows(h["ts"][b], m)
        Ro, to, so = orc.compute_sim3_transform(h["pos"][b][m], h["gps"][b][m])
        np.testing.assert_allclose(R[b].reshape(3, 3), Ro, atol=2e-9, rtol=0)     # straight tracks: R conditioned ~1e3-1e4
        assert abs(s[b] - so) < 1e-11
        sp, sq = orc.transform_trajectory(h["pos"][b][:1], h["quat"][b][:1], R[b].reshape(3, 3), t[b], s[b])
        po, qo, sto = orc.apply_ekf_correction_aligned(h["ts"][b], h["pos"][b], h["quat"][b], h["gps"][b], h["valid"][b], sp[0], sq[0], return_status=True)
        assert np.abs(p[b] - po).max() < POS_TOL and np.abs(q[b] - qo).max() < Q_TOL
        assert (st[b] & 0xff) == sto


@pytest.mark.parametrize("N", [271, 1000, 64, 130, 321])
def test_trajectory_major_kernels_vs_oracle(B, orc, N):
    """The wave-per-trajectory K4 and fused pipeline against the oracle, incl. the generic bad-quaternion path.  (The measured-and-
    rejected builds of round 1 -- several poses per lane, block kernel, single-shot kernel -- live under tools/experiments/.)"""
    import torch
    nb = 300
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=21)
    batch.quat[5, N // 2] = 0.0                      # one invalid quaternion -> generic (non-telescoped) path for track 5
    batch.quat[9, 0] = 0.0
    out = B.ekf_fuse_batch(batch)
    outp, R, t, s = B.fuse_pipeline_batch(batch)
    torch.cuda.synchronize()
    h = batch.host_traj_major()
    p, q, st = out.host_traj_major()
    po, qo, sto = orc.fuse_batch(h["ts"], h["pos"], h["quat"], h["gps"], h["valid"], h["init_pos"], h["init_quat"])
    np.testing.assert_array_equal(st, sto)
    assert np.abs(p - po).max() < POS_TOL and np.abs(q - qo).max() < Q_TOL
    pp, qp, stp = outp.host_traj_major()
    pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(h["ts"], h["pos"], h["quat"], h["gps"], h["valid"])
    ok = np.isfinite(pr).all(axis=(1, 2))
    assert (~ok).sum() == 1 and not ok[9]            # track 9: pose-0 quaternion invalid -> NaN outputs (SciPy would raise)
    assert np.isnan(pp[9]).all()
    # the fitted R is conditioned ~1e3-1e4 on short straight tracks, so the orientation agrees to ~1e-9 only
    assert np.abs(pp[ok] - pr[ok]).max() < 1e-6 and np.abs(qp[ok] - qr[ok]).max() < 1e-8
    np.testing.assert_array_equal(stp[ok] & 0xff, str_[ok] & 0xff)


def test_umeyama_windows_vs_oracle(B, orc):
    """Config C4-shaped: disjoint 50-pair windows, batched Umeyama."""
    import torch
    nb, W = 5000, 50
    rng = np.random.default_rng(5)
    src = np.cumsum(rng.normal(size=(nb, W, 3)) * [0.05, 0.03, 1.4], axis=1)
    ang = rng.uniform(-1, 1, size=nb)
    Rz = np.stack([np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]) for a in ang])
    dst = 1.05 * np.einsum("bij,bwj->bwi", Rz, src) + np.array([4.5e5, 5.4e6, 100.0]) + rng.normal(size=(nb, W, 3)) * 0.45
    R, t, s, st = B.sim3_umeyama_batch(torch.as_tensor(src).cuda(), torch.as_tensor(dst).cuda())
    R, t, s, st = R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all()
    for b in range(0, nb, 97):
        Ro, to, so = orc.compute_sim3_transform(src[b], dst[b])
        np.testing.assert_allclose(R[b].reshape(3, 3), Ro, atol=1e-10, rtol=0)
        assert abs(s[b] - so) < 1e-11
        np.testing.assert_allclose(s[b] * src[b] @ R[b].reshape(3, 3).T + t[b], so * src[b] @ Ro.T + to, atol=POS_TOL, rtol=0)
    # the equal-size-window entry (two launches) against the ragged kernel on the same windows, incl. masked rows, a window whose
    # first rows are masked out / NaN (shift search), windows with fewer than 3 usable rows, and a window count that is not a multiple of 4
    nbw = 1003
    sw, dw = torch.as_tensor(src[:nbw].copy()).cuda(), torch.as_tensor(dst[:nbw].copy()).cuda()
    mk = torch.ones((nbw, W), dtype=torch.uint8).cuda()
    mk[3, :5] = 0; mk[4, :] = 0; mk[5, 2:] = 0; mk[7, ::2] = 0
    sw[8, 0, 1] = float("nan"); mk[8, 0] = 1
    Rw, tw, s_w, stw = B.sim3_umeyama_batch(sw, dw, mask=mk)
    offw = torch.arange(0, (nbw + 1) * W, W, dtype=torch.int64).cuda()
    Rr, tr, sr, str_ = B.sim3_umeyama_batch(sw.reshape(-1, 3), dw.reshape(-1, 3), offw, mk.reshape(-1))
    np.testing.assert_array_equal(stw.cpu().numpy(), str_.cpu().numpy())
    assert stw[4].item() == 1 and stw[5].item() == 1 and stw[3].item() == 0
    okw = (stw == 0).cpu().numpy() & np.isfinite(Rr.cpu().numpy()).all(axis=1)
    np.testing.assert_allclose(Rw.cpu().numpy()[okw], Rr.cpu().numpy()[okw], atol=1e-11, rtol=0)
    np.testing.assert_allclose(s_w.cpu().numpy()[okw], sr.cpu().numpy()[okw], atol=1e-12, rtol=0)
    np.testing.assert_allclose(tw.cpu().numpy()[okw], tr.cpu().numpy()[okw], atol=1e-6, rtol=0)
    # ragged + masked + too-short sets
    offs = torch.tensor([0, 2, 2, 60, 200], dtype=torch.int64).cuda()
    flat_s, flat_d = torch.as_tensor(src.reshape(-1, 3)[:200].copy()).cuda(), torch.as_tensor(dst.reshape(-1, 3)[:200].copy()).cuda()
    mask = torch.ones(200, dtype=torch.uint8).cuda(); mask[100:150] = 0
    R2, t2, s2, st2 = B.sim3_umeyama_batch(flat_s, flat_d, offs, mask)
    st2 = st2.cpu().numpy()
    assert st2[0] == 1 and st2[1] == 1 and st2[2] == 0 and st2[3] == 0
    keep = np.r_[60:100, 150:200]
    Ro, to, so = orc.compute_sim3_transform(src.reshape(-1, 3)[keep], dst.reshape(-1, 3)[keep])
    np.testing.assert_allclose(R2[3].cpu().numpy().reshape(3, 3), Ro, atol=1e-10, rtol=0)


def test_utm_batch_zone_pick(B, orc):
    import torch
    rng = np.random.default_rng(9)
    centers = [(49.03, 8.39), (8.39, 49.03), (-33.9, 18.4), (35.0, -117.0)]
    lat = np.concatenate([c[0] + rng.uniform(-0.02, 0.02, 300) for c in centers])
    lon = np.concatenate([c[1] + rng.uniform(-0.02, 0.02, 300) for c in centers])
    offs = torch.arange(0, 1201, 300, dtype=torch.int64).cuda()
    e, n, zone, south = B.utm_forward_batch(torch.as_tensor(lat).cuda(), torch.as_tensor(lon).cuda(), offs)
    zone, south = zone.cpu().numpy(), south.cpu().numpy()
    assert list(zone) == [32, 39, 34, 11] and list(south) == [0, 0, 1, 0]
    for k in range(4):
        eo, no = orc.utm_forward(lat[k * 300:(k + 1) * 300], lon[k * 300:(k + 1) * 300], zone[k], south[k])
        np.testing.assert_allclose(e.cpu().numpy()[k * 300:(k + 1) * 300], eo, atol=5e-9, rtol=0)
        np.testing.assert_allclose(n.cpu().numpy()[k * 300:(k + 1) * 300], no, atol=5e-9, rtol=0)
    la2, lo2 = B.utm_inverse_batch(e, n, offs, torch.as_tensor(zone).cuda(), torch.as_tensor(south).cuda())
    np.testing.assert_allclose(la2.cpu().numpy(), lat, atol=1e-12); np.testing.assert_allclose(lo2.cpu().numpy(), lon, atol=1e-12)


def test_full_size_properties(B):
    """BASELINE config C3 shape at reduced B (HBM-regime sizes are bench territory): size-independent properties --
    all-invalid GNSS == pure dead reckoning of the same batch; re-running is idempotent; row 0 == init pose."""
    import torch
    nb, N = 20000, 1000
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=1, seed=5)
    out = B.ekf_fuse_batch(batch)
    p_first = out.pos[0].clone()            # (3, B)
    torch.cuda.synchronize()
    q0 = batch.init_quat / batch.init_quat.norm(dim=1, keepdim=True)
    keep = batch.valid[0] != 0              # a track that STARTS in an outage has row 0 rewritten by the RTS pass (Q11)
    assert torch.equal(p_first.T.contiguous()[keep], batch.init_pos[keep])
    assert (out.quat[0].T - q0)[keep].abs().max().item() < 1e-15
    assert 0.005 < (~keep).float().mean().item() < 0.05
    out2 = B.ekf_fuse_batch(batch)
    torch.cuda.synchronize()
    assert torch.equal(out.pos, out2.pos) and torch.equal(out.quat, out2.quat)
    st = out.status.cpu().numpy()
    frac_rts = ((st & 2) > 0).mean()
    assert 0.05 < frac_rts < 0.2
    # trajectories without any outage: status 0 and finite everywhere
    assert torch.isfinite(out.pos).all() and torch.isfinite(out.quat).all()
    unit = out.quat.pow(2).sum(dim=1)
    assert (unit - 1).abs().max().item() < 1e-12


# ------------------------------------------------------------------ helper functions of the EKF surface (a5, a9-a12)
def test_relative_pose_and_nlerp(E, golden):
    g = golden("helper_cases.npz")
    for i in range(len(g["rp_p1"])):
        dp, dq = E.calculate_relative_pose(g["rp_p1"][i], g["rp_q1"][i], g["rp_p2"][i], g["rp_q2"][i])
        np.testing.assert_allclose(dp, g["rp_dp"][i], atol=1e-13, rtol=0)
        np.testing.assert_allclose(dq, g["rp_dq"][i], atol=1e-15, rtol=0)
    for a, b, w, o in zip(g["nl_a"], g["nl_b"], g["nl_w"], g["nl_out"]):
        np.testing.assert_allclose(E.quaternion_nlerp(a, b, w), o, atol=1e-15, rtol=0)


def test_sharp_turn_function(E, golden):
    g = golden("helper_cases.npz")
    for name in g["sh_names"]:
        r = E.is_sharp_turn_in_segment(list(g[f"sh_{name}_q"]), list(g[f"sh_{name}_t"]), float(g[f"sh_{name}_thr"]))
        assert r == bool(g[f"sh_{name}_r"]), name


@pytest.mark.parametrize("tag", ["diag", "dense"])
def test_rts_smoother_segment_function(E, golden, tag):
    g = golden("helper_cases.npz")
    xs, Ps = E.rts_smoother_segment(list(g[f"rts_{tag}_xf"]), list(g[f"rts_{tag}_Pf"]), list(g[f"rts_{tag}_xp"]), list(g[f"rts_{tag}_Pp"]))
    tol = 1e-12 if tag == "diag" else 1e-9
    np.testing.assert_allclose(np.array(xs), g[f"rts_{tag}_xs"], atol=tol, rtol=tol)
    np.testing.assert_allclose(np.array(Ps), g[f"rts_{tag}_Ps"], atol=tol * 10, rtol=tol * 10)
    assert E.rts_smoother_segment([], [], [], []) == ([], [])


@pytest.mark.parametrize("tag", ["hard", "blend4", "override3"])
def test_extended_kalman_filter_class(E, golden, tag):
    g = golden("helper_cases.npz")
    steps, ovr = (int(v) for v in g[f"ps_{tag}_par"])
    f = E.ExtendedKalmanFilter(np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.2, 0.3, 0.9]) * 2, E.CONFIG["ekf"])
    f.current_transition_steps = steps
    f.gnss_available_prev = False
    for i in range(len(g[f"ps_{tag}_dt"])):
        av = bool(g[f"ps_{tag}_avail"][i])
        st, cv, ps, pc = f.process_step((g[f"ps_{tag}_dp"][i], g[f"ps_{tag}_dq"][i]), g[f"ps_{tag}_z"][i] if av else None, av,
                                        float(g[f"ps_{tag}_dt"][i]), override_transition_steps=None if ovr < 0 else ovr)
        np.testing.assert_allclose(st, g[f"ps_{tag}_state"][i], atol=1e-12, rtol=0)
        np.testing.assert_allclose(cv, g[f"ps_{tag}_cov"][i], atol=1e-14, rtol=0)
        np.testing.assert_allclose(ps, g[f"ps_{tag}_ps"][i], atol=1e-12, rtol=0)
        np.testing.assert_allclose(pc, g[f"ps_{tag}_pc"][i], atol=1e-14, rtol=0)
        assert abs(f.gnss_update_weight - float(g[f"ps_{tag}_w"][i])) < 1e-15
    with pytest.raises(ValueError):
        E.ExtendedKalmanFilter(np.zeros(2), np.zeros(4), E.CONFIG["ekf"])


def test_rccl_own_communicator_single_rank(B):
    """gsf_comm_unique_id / gsf_comm_init_rank / gsf_allgather_poses / gsf_comm_destroy on a 1-rank communicator (the box has one
    GPU): both exchange modes must reproduce the send buffer.  (World >= 2 over RCCL needs >= 2 GPUs: the driver's 8-GPU run.)"""
    import ctypes as C
    import torch
    from gps_optimize_slam_amd import _lib
    L = _lib.load()
    ctx = B.context()
    ident = (C.c_uint8 * 128)()
    _lib.check(L.gsf_comm_unique_id(ident))
    comm = C.c_void_p()
    _lib.check(L.gsf_comm_init_rank(ctx.handle, ident, 1, 0, C.byref(comm)))
    try:
        send = torch.randn(100_003, dtype=torch.float64, device="cuda")
        for mode, chunk in ((0, 0), (1, 0), (1, 4096)):
            recv = torch.zeros_like(send)
            _lib.check(L.gsf_allgather_poses(ctx.handle, comm, C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), send.numel(), mode, chunk))
            torch.cuda.synchronize()
            assert torch.equal(send, recv), (mode, chunk)
        assert L.gsf_comm_init_rank(ctx.handle, ident, 1, 3, C.byref(C.c_void_p())) != 0      # rank out of range: refused before RCCL is called
        v = C.c_int32(0)
        _lib.check(L.gsf_comm_rccl_version(C.byref(v)))
        assert 20000 <= v.value < 30000, v.value                           # the resolved librccl.so speaks the NCCL 2.x API the wrapper assumes
    finally:
        _lib.check(L.gsf_comm_destroy(comm))


def _run_ranks(script_args, world, timeout=600):
    """start `world` ranks of a helper script (children of this process; they share the box's one GPU -> gloo rehearsal)"""
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable] + script_args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=timeout)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    return outs


def test_two_rank_real_kernels_gathered_equals_unsharded(tmp_path):
    """SURVEY 8e on hardware as far as a one-GPU box allows: two ranks fuse their shards with the REAL kernels, the collect goes
    through the product's all-gather helpers (both layouts, whole + chunked with a checksum sink + the bench's one-call form), and
    the gathered result equals the unsharded run bit for bit."""
    out = tmp_path / "res.json"
    _run_ranks([os.path.join(ROOT, "tests", "two_rank_worker.py"), str(out), "300", "271"], world=2)
    res = json.load(open(out))
    assert res["world"] == 2 and res["backend"] == "gloo"
    for layout in (0, 1):
        for key in ("pos_equal", "quat_equal", "chunked_checksum_equal", "flat_blocks_equal", "finite"):
            assert res[f"layout{layout}_{key}"] is True, (layout, key, res)


def test_bench_plain_run_dumps_identical_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps, prints the headline line without the --full parts, and with
    --dump-outputs writes the last step's outputs (float64, trajectory-major, under 64 MB); two runs with the same arguments write the same bits."""
    import subprocess
    import sys
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(d)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        res = json.loads(lines[0])
        assert res["steps"] == 7 and res["warmup"] == 2 and res["n_gpus"] == 1
        assert res["metric"].startswith("fused poses/sec") and res["unit"] == "fused poses/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
        poses = res["config"]["trajectories_per_gpu"] * res["config"]["poses_per_trajectory"]
        assert abs(res["value"] - poses / (res["ms_per_step"] * 1e-3)) / res["value"] < 1e-9
        for k in ("extra", "cpu_baseline", "gated", "fit_rows"):
            assert k not in res, k
        names = sorted(f.name for f in d.iterdir())
        assert names == ["R.npy", "pos.npy", "quat.npy", "s.npy", "status.npy", "t.npy"] and res["dump_outputs"]["arrays"] == [n[:-4] for n in names]
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 * 2 ** 20
        a = {n[:-4]: np.load(d / n) for n in names}
        B_, N_ = res["config"]["trajectories_per_gpu"], res["config"]["poses_per_trajectory"]
        assert a["pos"].shape == (B_, N_, 3) and a["quat"].shape == (B_, N_, 4) and a["R"].shape == (B_, 9) and a["status"].shape == (B_,)
        assert all(v.dtype == np.float64 for v in a.values()) and np.isfinite(a["pos"]).mean() > 0.9
        dumps.append(a)
    for k in dumps[0]:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k], err_msg=k)


def test_bench_two_ranks_self_spawned():
    """`python bench.py --gpus 2` with no launcher starts its own ranks (gloo rehearsal on the one GPU), exits 0 and prints ONE JSON
    line with the collect block (gathered blocks == every rank's own checksum) and the C5-shaped leg."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["scaling"] == "weak"
    assert d["collect"]["gathered_blocks_equal_rank_checksums"] is True and d["collect"]["backend"] == "gloo"
    assert d["max_abs_pos_err_m"] < 1e-6 and d["status_bits_equal"] is True
    c5 = d["c5"]
    assert "error" not in c5, c5
    assert c5["chunks"] >= 2 and c5["collect"]["torch_all_gather"]["gathered_checksum_equals_sum_of_rank_checksums"] is True
    assert abs(d["value"] - 2 * d["config"]["trajectories_per_gpu"] * d["config"]["poses_per_trajectory"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9


def test_bench_under_the_drivers_launcher_two_ranks():
    """The driver's own N > 1 command: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P
    bench.py --gpus 2 --steps 20 --warmup 5` -- bench.py is then one of the ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment),
    rank 0 prints ONE JSON line, every rank exits 0 (gloo rehearsal on the one-GPU box; RCCL when each rank has its own GPU)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    port = 29600 + (os.getpid() % 300)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 20 and d["warmup"] == 5 and d["scaling"] == "weak" and d["metric"].startswith("fused poses/sec")
    assert d["collect"]["gathered_blocks_equal_rank_checksums"] is True
    assert d["max_abs_pos_err_m"] < 1e-6 and d["status_bits_equal"] is True
    assert abs(d["value"] - 2 * d["config"]["trajectories_per_gpu"] * d["config"]["poses_per_trajectory"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9


def test_bench_five_ranks_rehearsal_chunked_c5_leg():
    """More ranks than two on the one-GPU box (five: with the test process itself that is the six processes the box admits on the card):
    `bench.py --gpus 5` starts its ranks, every rank fuses its own id block with the real kernels, the collect and the chunked C5-shaped
    leg (4 chunks per pass, double-buffered receive, checksum sink, watchdog bookkeeping) run over gloo with CPU staging; one JSON line,
    gathered blocks equal every rank's checksum, the gate holds.  (The RCCL legs -- ncclAllGather and the rotated direct exchange of
    gsf_comm.hip -- need one GPU per rank and stay unmeasured until an 8-GPU node runs the same command.)"""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "5", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--traj-per-gpu", "512", "--chunk-traj", "128"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 5 and d["config"]["trajectories_per_gpu"] == 512 and d["backend"] == "gloo"
    assert d["collect"]["gathered_blocks_equal_rank_checksums"] is True
    assert d["max_abs_pos_err_m"] < 1e-6 and d["status_bits_equal"] is True
    c5 = d["c5"]
    assert "error" not in c5 and "stalled_leg" not in c5, c5
    assert c5["chunks"] >= 2 and c5["trajectories_per_gpu"] == 512 and c5["chunk_trajectories"] == 128
    assert c5["collect"]["torch_all_gather"]["gathered_checksum_equals_sum_of_rank_checksums"] is True
    assert abs(d["value"] - 5 * 512 * d["config"]["poses_per_trajectory"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9


def test_bench_two_ranks_stalled_collect_leg_exits_nonzero():
    """A collect leg that hangs (injected: every leg sleeps 6 s under a 1.5 s watchdog) ends the run with a NON-ZERO exit code, and
    rank 0 still prints one JSON line that names the stalled leg."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--inject-stall", "6", "--stall-seconds", "1.5", "--traj-per-gpu", "2048"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode != 0, "a stalled leg must not look like success"
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d["c5"]["stalled_leg"] == "torch_all_gather" and "watchdog" in d["c5"]["collect_error"]
    assert d["backend"] == "gloo" and d["value"] > 0            # the C2 part of the line was measured before the stall


# ------------------------------------------------------------------ next-1: time alignment on the device
def test_time_alignment_kernel_vs_goldens_and_oracle(E, orc, golden):
    g = golden("align_cases.npz")
    for name in g["names"]:
        slam = {"timestamps": g[f"{name}_st"]}
        gps = {"timestamps": g[f"{name}_gt"], "positions": g[f"{name}_gp"]}
        al, va = E.dynamic_time_alignment(slam, gps, {"max_samples_for_corr": 500, "max_gps_gap_threshold": float(g[f"{name}_gap"])})
        np.testing.assert_array_equal(va, g[f"{name}_va"], err_msg=str(name))
        np.testing.assert_array_equal(np.isnan(al), np.isnan(g[f"{name}_al"]), err_msg=str(name))
        # vs the reference (scipy's B-spline loses ~1e-7 m on irregular knots, see tests/test_oracle_golden.py) ...
        tol = 5e-7 if str(name) in ("random_knots", "two_gaps", "unsorted_dups", "exact_knots", "small_gap_thr") else 1e-8
        np.testing.assert_allclose(al[va], g[f"{name}_al"][va], atol=tol, rtol=0, err_msg=str(name))
        # ... and vs the oracle's exact-to-2-ulp spline
        alo, vao = orc.dynamic_time_alignment(g[f"{name}_st"], g[f"{name}_gt"], g[f"{name}_gp"], 500, float(g[f"{name}_gap"]))
        np.testing.assert_array_equal(va, vao)
        np.testing.assert_allclose(al[va], alo[va], atol=2e-8, rtol=0, err_msg=str(name))


def test_time_alignment_kat4_and_c1(E, golden):
    k = golden("kat_bundled.npz")
    al, va = E.dynamic_time_alignment({"timestamps": k["ts"]}, {"timestamps": k["kat4_gps_t"], "positions": k["kat4_gps_p"]}, E.CONFIG["time_alignment"])
    np.testing.assert_array_equal(va, k["kat4_valid"])
    np.testing.assert_allclose(al[va], k["kat4_aligned"][va], atol=1e-9, rtol=0)
    for tag in ("kitti04gps", "combined"):
        g = golden(f"c1_{tag}.npz")
        al, va = E.dynamic_time_alignment({"timestamps": k["ts"]}, {"timestamps": g["gps_t"], "positions": g["gps_p"]}, E.CONFIG["time_alignment"])
        np.testing.assert_array_equal(va, g["valid"])
        np.testing.assert_allclose(al[va], g["aligned"][va], atol=1e-8, rtol=0)


def test_time_alignment_batch_ragged(B, orc):
    """Batched device entry: ragged SLAM / GNSS tracks, unsorted + duplicated stamps, gaps, short segments."""
    import ctypes as C
    import torch
    from gps_optimize_slam_amd import _lib
    rng = np.random.default_rng(17)
    st_l, gt_l, gp_l = [], [], []
    for b in range(40):
        ns, ng = int(rng.integers(1, 400)), int(rng.integers(0, 350))
        st = np.sort(rng.uniform(0, 40, ns))
        gt = np.sort(rng.uniform(0, 40, ng))
        if b % 3 == 0 and ng > 30:
            gt = gt[(gt < 10) | (gt > 17)]                     # a gap > 5 s
        gp = np.c_[np.sin(gt) * 50 + 4.5e5, gt * 13 + 5.4e6, np.cos(gt / 3) + 100]
        if b % 4 == 1 and len(gt) > 10:                        # shuffle + duplicate a few stamps (identical positions)
            perm = rng.permutation(len(gt)); gt, gp = np.r_[gt[perm], gt[:5]], np.r_[gp[perm], gp[:5]]
        st_l.append(st); gt_l.append(gt); gp_l.append(gp.reshape(-1, 3))
    so = np.cumsum([0] + [len(x) for x in st_l]).astype(np.int64); go = np.cumsum([0] + [len(x) for x in gt_l]).astype(np.int64)
    d = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
    dst, dgt, dgp, dso, dgo = d(np.concatenate(st_l)), d(np.concatenate(gt_l)), d(np.concatenate(gp_l)), d(so, torch.int64), d(go, torch.int64)
    al = torch.empty((int(so[-1]), 3), dtype=torch.float64, device="cuda"); va = torch.empty(int(so[-1]), dtype=torch.uint8, device="cuda")
    stt = torch.empty(40, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_time_align_batch_dev(B.context().handle, p(dst), p(dso), p(dgt), p(dgp), p(dgo), 40, 512, 5.0, p(al), p(va), p(stt)))
    torch.cuda.synchronize()
    al, va = al.cpu().numpy(), va.cpu().numpy().astype(bool)
    assert (stt.cpu().numpy() == 0).all()
    for b in range(40):
        alo, vao = orc.dynamic_time_alignment(st_l[b], gt_l[b], gp_l[b], 500, 5.0)
        sl = slice(so[b], so[b + 1])
        np.testing.assert_array_equal(va[sl], vao, err_msg=str(b))
        np.testing.assert_allclose(al[sl][vao], alo[vao], atol=5e-8, rtol=0, err_msg=str(b))
        assert np.isnan(al[sl][~vao]).all()


def test_time_alignment_long_track_global_staging(E, orc):
    """More than 2560 fixes: the kernel stages the track in global scratch instead of LDS."""
    rng = np.random.default_rng(23)
    gt = np.sort(rng.uniform(0, 400, 5000)); gt = gt[np.r_[True, np.diff(gt) > 1e-6]]
    gp = np.c_[np.sin(gt / 7) * 500 + 4.5e5, gt * 13 + 5.4e6, np.cos(gt / 30) * 10 + 100]
    st = np.arange(3800) * 0.104
    al, va = E.dynamic_time_alignment({"timestamps": st}, {"timestamps": gt, "positions": gp}, E.CONFIG["time_alignment"])
    alo, vao = orc.dynamic_time_alignment(st, gt, gp, 500, 5.0)
    np.testing.assert_array_equal(va, vao)
    np.testing.assert_allclose(al[va], alo[va], atol=5e-8, rtol=0)


def test_c3_full_size_properties(B, orc):
    """BASELINE config C3 at FULL size (100 000 x 1 000 poses, 14.5 GB): size-independent properties of the fused batch, and a sample of
    48 trajectories spread over it (first / middle / last slice) against the oracle on the same inputs."""
    import torch
    nb, N = 100_000, 1000
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=20250523)
    out, R, t, s = B.fuse_pipeline_batch(batch)
    torch.cuda.synchronize()
    idx = np.concatenate([np.arange(16), nb // 2 + np.arange(16), nb - 16 + np.arange(16)])
    ix = torch.as_tensor(idx, device="cuda")
    hh = {k: getattr(batch, k).index_select(0, ix).cpu().numpy() for k in ("ts", "pos", "quat", "gps", "valid")}
    po, qo, sto, Ro, _, so = orc.fuse_pipeline_batch(hh["ts"], hh["pos"], hh["quat"], hh["gps"], hh["valid"])
    pg, qg, sg = out.pos.index_select(0, ix).cpu().numpy(), out.quat.index_select(0, ix).cpu().numpy(), out.status.index_select(0, ix).cpu().numpy()
    assert np.abs(pg - po).max() < POS_TOL and np.abs(qg - qo).max() < Q_TOL and ((sg & ~(16 << 8)) == sto).all()
    assert np.abs(R.index_select(0, ix).cpu().numpy() - Ro).max() < 2e-9 and np.abs(s.index_select(0, ix).cpu().numpy() - so).max() < 1e-11
    assert torch.isfinite(out.pos).all() and torch.isfinite(out.quat).all() and torch.isfinite(s).all()
    assert ((out.quat.pow(2).sum(dim=2) - 1).abs().max().item()) < 1e-12                 # unit quaternions
    assert (s - 1.0).abs().max().item() < 0.12                                            # planted scales are U(0.9, 1.1)
    st = out.status.cpu().numpy()
    assert (((st >> 8) & ~16) == 0).all()                                                  # every fit succeeded (bit 16: which route made the rotation)
    assert ((st >> 8) & 16).mean() < 0.04                                                  # the Jacobi fallback stays rare on this distribution (2.8 % under the reference's row choice: outage tracks fit their first segment only; 0.1 % over all valid rows)
    frac_out, frac_rts, frac_end = ((st & 1) > 0).mean(), ((st & 2) > 0).mean(), ((st & 8) > 0).mean()
    assert 0.12 < frac_out < 0.16 and 0.09 < frac_rts < 0.13 and 0.015 < frac_end < 0.025
    # fused track stays within a few GNSS sigmas of the valid fixes (sigma = 0.45 m)
    err = (out.pos - batch.gps).norm(dim=2)
    ok = batch.valid.bool() & torch.isfinite(err)
    assert err[ok].mean().item() < 1.0
    # shard invariance at full size: a checksum of a 1 000-trajectory slice regenerated as its own batch matches bit for bit
    sub = B.TrajectoryBatch.synthetic(1000, N, layout=0, seed=20250523, traj0=54_000)
    outs, _, _, _ = B.fuse_pipeline_batch(sub)
    torch.cuda.synchronize()
    assert torch.equal(outs.pos, out.pos[54_000:55_000]) and torch.equal(outs.quat, out.quat[54_000:55_000])
    # idempotence
    out2, _, _, _ = B.fuse_pipeline_batch(batch)
    torch.cuda.synchronize()
    assert torch.equal(out.pos, out2.pos)


# ------------------------------------------------------------------ next-4: the reference's error metric on the device
@pytest.mark.parametrize("tag", ["kitti04gps", "combined"])
def test_error_metric_kernel_vs_reference(E, golden, tag):
    g, k = golden(f"c1_{tag}.npz"), golden("kat_bundled.npz")
    for traj, ref in ((g["sim3_pos"], g["err_sim3"]), (g["ekf_pos"], g["err_ekf"])):
        r = E.evaluate_trajectory_errors(k["ts"], traj, g["aligned"], g["valid"])
        post = g["valid"] & (k["ts"] > k["ts"][0] + 5.0)
        assert r["count"] == int(post.sum())
        np.testing.assert_allclose([r["mean"], r["median"], r["rmse"]], ref, atol=1e-9, rtol=0)
        assert np.isnan(r["errors"][~post]).all() and np.isfinite(r["errors"][post]).all()


@pytest.mark.parametrize("N", [5, 30, 64, 65, 130, 271, 400, 700, 1000, 1536, 1700])
def test_error_metric_kernel_every_tile_shape(B, N):
    """eval_errors_lds_kernel spreads the M x M pair work (nearest fix, :1030-1031; rank count of the median, :1033) as a register tile of
    1 .. 8 queries per thread over S = 1 .. 64 lanes per query -- one template instance per tile length: track lengths that reach every
    instance (M * S / 256 = 1 .. 8 passes, S from 64 down to 1), N = 1 700 beyond the LDS kernel (one thread per query), tracks with no,
    one and two evaluated poses, duplicated errors (the tie rule of the rank count) -- against NumPy's cdist-min / mean / median / RMSE of
    the same rows.  (The three-tracks-per-launch form runs in tests/test_run_chain.py against the goldens' step-6 rows.)"""
    import torch
    rng = np.random.default_rng(N)
    nb = 12
    ts = np.cumsum(rng.uniform(0.05, 0.15, size=(nb, N)), axis=1)
    p = np.cumsum(rng.normal(size=(nb, N, 3)), axis=1)
    g = p + rng.normal(size=(nb, N, 3)) * 0.5
    valid = (rng.random((nb, N)) < 0.8).astype(np.uint8)
    valid[0] = 0                                                            # nothing to evaluate
    valid[1] = 0; valid[1, N - 1] = 1                                       # one pose
    valid[2] = 0; valid[2, N - 1] = 1; valid[2, N - 2] = 1                  # two poses
    p[3] = 0.0; p[3, :, 0] = 100.0 * np.arange(N); g[3] = p[3] + np.array([3.0, 0.0, 4.0])   # every error exactly 5: ranks decided by the row order alone
    g[4, ::7] = np.nan                                                      # NaN fixes leave the set (:1016)
    skip = 0.5
    T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    stats, err = B.eval_errors_batch(T(ts), T(p), T(g), T(valid, torch.uint8), skip)
    stats, err = stats.cpu().numpy(), err.cpu().numpy()
    for b in range(nb):
        sel = (valid[b] != 0) & (ts[b] > ts[b, 0] + skip) & np.isfinite(g[b]).all(axis=1)
        assert stats[b, 0] == sel.sum() and np.isnan(err[b][~sel]).all()
        if not sel.any():
            assert np.isnan(stats[b, 1:]).all()
            continue
        d = np.sqrt(((p[b][sel][:, None, :] - g[b][sel][None, :, :]) ** 2).sum(axis=2)).min(axis=1)
        np.testing.assert_allclose(err[b][sel], d, atol=1e-9, rtol=0)
        np.testing.assert_allclose(stats[b, 1:], [d.mean(), np.median(d), np.sqrt((d ** 2).mean())], atol=1e-9, rtol=0)
        assert stats[b, 2] == np.median(err[b][sel])                         # the median is an order statistic of the kernel's own errors: exact
    assert (err[3][np.isfinite(err[3])] == 5.0).all()


@pytest.mark.parametrize("shape", ["line", "circle", "shaft", "stacked", "two_clusters", "walk"])
def test_error_metric_pruned_search_is_the_all_pairs_minimum(B, shape):
    """Tracks of more than 400 evaluated poses take the pruned nearest-fix search (fixes sorted along their longest axis, walk outwards from the
    query's place until the axis gap alone exceeds the best distance).  It must return the all-pairs minimum (:1030-1031) on geometries that
    prune well (a line), badly (a circle: no long axis; a vertical shaft: the long axis is z), not at all (every fix at the same place along
    two axes; two far clusters with the queries of one nearest to fixes of the other), and on a 3-D random walk -- against NumPy's cdist-min of
    the same rows; N = 1 000 and 1 536 (the largest track the LDS kernel takes)."""
    import torch
    for N in (1000, 1536):
        rng = np.random.default_rng(N + len(shape))
        nb = 6
        ts = np.tile(np.arange(N) * 0.1, (nb, 1))
        u = np.arange(N)
        if shape == "line": g = np.stack([3.0 * u, 0.5 * u, 0 * u], axis=1)[None].repeat(nb, 0) + rng.normal(size=(nb, N, 3)) * 0.3
        elif shape == "circle": g = np.stack([200 * np.cos(u * 2 * np.pi / N), 200 * np.sin(u * 2 * np.pi / N), 0 * u], axis=1)[None].repeat(nb, 0) + rng.normal(size=(nb, N, 3)) * 0.3
        elif shape == "shaft": g = np.stack([0 * u, 0 * u, 2.0 * u], axis=1)[None].repeat(nb, 0) + rng.normal(size=(nb, N, 3)) * 0.3
        elif shape == "stacked": g = np.stack([np.full(N, 5.0), np.full(N, -7.0), rng.permutation(N) * 0.01], axis=1)[None].repeat(nb, 0).copy()
        elif shape == "two_clusters": g = np.where((u % 2 == 0)[None, :, None], 0.0, 5000.0) + rng.normal(size=(nb, N, 3))
        else: g = np.cumsum(rng.normal(size=(nb, N, 3)), axis=1)
        p = g + rng.normal(size=(nb, N, 3)) * (2.0 if shape != "two_clusters" else 1.0)
        p[nb - 1] += np.array([4.0e5, 5.4e6, 100.0])                       # one track in another frame (step 6's raw SLAM row): the all-pairs fall-back + sorted median
        if shape == "two_clusters": p = np.roll(p, 1, axis=1)               # a pose sits in the OTHER cluster than the fix of its own row
        valid = (rng.random((nb, N)) < 0.9).astype(np.uint8)
        T = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
        stats, err = B.eval_errors_batch(T(ts), T(p), T(g), T(valid, torch.uint8), 1.0)
        stats, err = stats.cpu().numpy(), err.cpu().numpy()
        for b in range(nb):
            sel = (valid[b] != 0) & (ts[b] > ts[b, 0] + 1.0)
            assert sel.sum() > 400 and stats[b, 0] == sel.sum()
            d = np.sqrt(((p[b][sel][:, None, :] - g[b][sel][None, :, :]) ** 2).sum(axis=2)).min(axis=1)
            np.testing.assert_allclose(err[b][sel], d, atol=2e-9, rtol=1e-12)
            np.testing.assert_allclose(stats[b, 1:], [d.mean(), np.median(d), np.sqrt((d ** 2).mean())], atol=2e-9, rtol=1e-12)
            assert stats[b, 2] == np.median(err[b][sel])


def test_run_fusion_headless_driver(E, golden, tmp_path):
    """Steps 1-7 of main_process_gui without the GUI, file in / file out, on a copy of the bundled-shaped data."""
    g, k = golden("c1_combined.npz"), golden("kat_bundled.npz")
    slam_f, gps_f = tmp_path / "traj.txt", tmp_path / "gps.txt"
    np.savetxt(slam_f, np.column_stack((k["ts"], k["pos"], k["quat"])))
    np.savetxt(gps_f, np.column_stack((g["gps_t_raw"], g["lat"], g["lon"], g["alt"], np.full(len(g["lat"]), 4), np.full(len(g["lat"]), 5))), fmt="%.18e")
    np.random.seed(0)
    out = E.run_fusion(str(slam_f), str(gps_f), out_path_utm=str(tmp_path / "traj_corrected_utm.txt"))
    assert out["gps"]["utm_zone"] == "32N"
    np.testing.assert_allclose(out["pos"], g["ekf_pos"], atol=POS_TOL, rtol=0)       # same seed, same RNG order as the reference run
    assert abs(out["err_ekf"]["rmse"] - g["err_ekf"][2]) < 1e-8
    assert (tmp_path / "traj_corrected_utm.txt").exists() and (tmp_path / "traj_corrected_wgs84.txt").exists()
    w = np.loadtxt(tmp_path / "traj_corrected_wgs84.txt", skiprows=1)
    assert abs(w[0, 1] - 8.395) < 1e-2 and abs(w[0, 2] - 49.0336) < 1e-2             # lon, lat of KITTI-04


@pytest.mark.parametrize("dist", ["white_noise", "random_walk_drift_8d", "c1_track_replicated"])
def test_pipeline_on_three_input_distributions_vs_oracle(B, orc, golden, dist):
    """The fused pipeline's fit takes its rotation from a Newton polar iteration with a Jacobi-SVD fallback whose thresholds were chosen
    on the default generator: the same parity gate on SURVEY 8d's random-walk-drift generator and on the real KITTI-04 track replicated
    with per-copy GNSS noise, and the fallback rate of each (status bit 16 << 8) stays small."""
    nb, N = 384, 271
    if dist == "c1_track_replicated":
        k, g = golden("kat_bundled.npz"), golden("c1_combined.npz")
        bt = B.TrajectoryBatch.replicated(k["ts"], k["pos"], k["quat"], g["aligned"], g["valid"], nb, 0.45, seed=2)
    else:
        bt = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=77, variant=1 if dist == "random_walk_drift_8d" else 0)
    h = bt.host_traj_major()
    if dist == "random_walk_drift_8d":
        # the drift really is a random walk: the SLAM track's deviation from its own smooth path grows with the pose index
        d2 = np.diff(h["pos"], n=2, axis=1)                               # second differences: white noise -> sigma*sqrt(6), a walk -> sigma*sqrt(2)
        assert 0.02 * 1.2 < d2[:, :, 1].std() < 0.02 * 1.7                # (the y axis: 0.2 % of the forward step, so the stamp jitter does not show)
    out, R, t, s = B.fuse_pipeline_batch(bt)
    p, q, st = out.host_traj_major()
    po, qo, sto, Ro, to, so = orc.fuse_pipeline_batch(h["ts"], h["pos"], h["quat"], h["gps"], h["valid"])
    ok = np.isfinite(po).all(axis=(1, 2))
    assert ok.all() and np.isfinite(p).all()
    assert np.abs(p - po).max() < POS_TOL and np.abs(q - qo).max() < 1e-8
    np.testing.assert_array_equal(st & 0xff, sto & 0xff)
    np.testing.assert_allclose(R.cpu().numpy(), Ro, atol=1e-10, rtol=0)
    fallbacks = int(((st >> 8) & 16 != 0).sum())
    assert ((st >> 8) & ~16 == 0).all() and fallbacks <= nb // 20, f"{fallbacks} of {nb} tracks fell back to the Jacobi SVD"


def test_c4_full_size_planted_transforms(B, orc):
    """BASELINE config C4 at FULL size (1 000 000 windows x 50 point pairs, 2.5 GB): every planted (R, t, s) is recovered to the noise
    level, every status is 0, and a sample of the windows agrees with the oracle's compute_sim3_transform to rounding."""
    import sys
    import torch
    sys.path.insert(0, ROOT)
    import bench
    nw, W = 1_000_000, 50
    src, dst, Rp, tp, sp = bench.planted_windows(torch, nw, W, 7)
    R, t, s, st = B.sim3_umeyama_batch(src, dst)
    torch.cuda.synchronize()
    assert int((st != 0).sum().item()) == 0
    # 2 cm noise on windows of ~70 m x a few metres: scale to ~1e-4, rotation about the drive axis weakly determined (lateral extent ~ 1 m)
    assert (s - sp).abs().max().item() < 2e-3 and (s - sp).abs().mean().item() < 3e-4
    resid = (s[:, None, None] * torch.einsum("bij,bwj->bwi", R.view(nw, 3, 3), src) + t[:, None, :] - dst).norm(dim=2)
    assert resid.max().item() < 0.2 and resid.mean().item() < 0.05         # the fit explains the points to the noise (sigma 2 cm per axis)
    idx = torch.randint(0, nw, (256,), generator=torch.Generator().manual_seed(0))
    for b in idx.tolist():
        Ro, to, so = orc.compute_sim3_transform(src[b].cpu().numpy(), dst[b].cpu().numpy())
        np.testing.assert_allclose(R[b].cpu().numpy().reshape(3, 3), Ro, atol=1e-9, rtol=0)
        np.testing.assert_allclose(t[b].cpu().numpy(), to, atol=1e-6, rtol=0)
        assert abs(s[b].item() - so) < 1e-10


def test_c5_shard_full_size_checksum_invariance(B):
    """BASELINE config C5's per-GPU shard at FULL size (1 245 184 x 1 000 poses = 181 GB of inputs, sized down symmetrically to what the
    GPU has free): fused chunk by chunk as the 8-GPU run does; the integer checksum of a chunk equals the checksum of the same trajectory
    ids generated and fused on their own (what another rank, or another sharding, would compute), also in sub-batches of other sizes."""
    import ctypes as C
    import torch
    from gps_optimize_slam_amd import _lib
    torch.cuda.empty_cache()
    N, chunk, seed = 1000, 32768, 20250523
    free_b, _ = torch.cuda.mem_get_info()
    T = int(min(1_245_184, (free_b * 0.90) // (N * 145 + 64)))
    T -= T % chunk
    assert T >= 4 * chunk, "not enough free HBM for a meaningful shard"
    L, ctx = _lib.load(), B.context()
    ctx.set_sim3_rows("reference", B.CONFIG)                              # the raw launches below follow the context's row rule (gsf_set_sim3_rows)
    cfg = _lib.EkfConfig.from_config(B.CONFIG)
    bt = B.TrajectoryBatch(0, T, N)
    for lo in range(0, T, 65536):
        n = min(65536, T - lo)
        _lib.check(L.gsf_synth_batch_dev(ctx.handle, 0, C.c_uint64(seed), lo, n, N, B._p(bt.ts[lo:]), B._p(bt.pos[lo:]), B._p(bt.quat[lo:]),
                                         B._p(bt.gps[lo:]), B._p(bt.valid[lo:]), None, None))
    f = dict(dtype=torch.float64, device="cuda")
    out = torch.empty((T * N * 7,), **f)
    R, t, s = torch.empty((T, 9), **f), torch.empty((T, 3), **f), torch.empty((T,), **f)
    status = torch.empty((T,), dtype=torch.int32, device="cuda")
    P = chunk * N
    for k in range(T // chunk):
        lo, o = k * chunk, out[k * P * 7:]
        _lib.check(L.gsf_fuse_pipeline_batch_dev(ctx.handle, 0, B._p(bt.ts[lo:]), B._p(bt.pos[lo:]), B._p(bt.quat[lo:]), B._p(bt.gps[lo:]), B._p(bt.valid[lo:]),
                                                 C.byref(cfg), chunk, N, B._p(R[lo:]), B._p(t[lo:]), B._p(s[lo:]), B._p(o), B._p(o[P * 3:]), B._p(status[lo:])))
    torch.cuda.synchronize()
    assert torch.isfinite(s).all() and (((status >> 8) & ~16) == 0).all()
    sums = out.view(torch.int64).view(T // chunk, -1).sum(dim=1)          # one wrapping int64 checksum per chunk
    nch = T // chunk
    for k in (0, nch // 2, nch - 1):
        part = B.TrajectoryBatch.synthetic(chunk, N, layout=0, seed=seed, traj0=k * chunk)
        o1, _, _, _ = B.fuse_pipeline_batch(part)
        assert int(o1.buf.view(torch.int64).sum().item()) == int(sums[k].item()), f"chunk {k}"
        # ... and in sub-batches of other sizes (1 000 tracks take the small-batch build, 5 000 the streaming one): the same bits
        for lo, n in ((0, 1000), (20000, 5000)):
            sub = B.TrajectoryBatch.synthetic(n, N, layout=0, seed=seed, traj0=k * chunk + lo)
            o2, _, _, _ = B.fuse_pipeline_batch(sub)
            full_pos = out[k * P * 7: k * P * 7 + P * 3].view(chunk, N, 3)[lo:lo + n]
            full_quat = out[k * P * 7 + P * 3: (k + 1) * P * 7].view(chunk, N, 4)[lo:lo + n]
            assert torch.equal(o2.pos, full_pos) and torch.equal(o2.quat, full_quat)
        del part, o1
    del bt, out
    torch.cuda.empty_cache()


def test_verbose_sim3_diagnostics(E, golden, capsys):
    """ekfgpsslam.VERBOSE prints the reference's progress lines of the Sim3 functions (ref :396-425, :446, :450) with the same numbers;
    off (the default) the functions are silent."""
    g = golden("kat_bundled.npz")
    src, dst = g["pos"], g["gt"]
    np.random.seed(1)
    E.compute_sim3_transform_robust(src, dst, 4, 4.0, 50, 4, "pts")
    assert capsys.readouterr().out == ""
    E.VERBOSE = True
    try:
        np.random.seed(1)
        R, t, s = E.compute_sim3_transform_robust(src, dst, 4, 4.0, 50, 4, "pts")
        out = capsys.readouterr().out
        assert f"Sim3 RANSAC on {len(src)} pts (threshold=4.0m, trials=50, min samples=4)" in out
        assert f"best inlier count {len(src)}/{len(src)}" in out and f"scale={s:.4f}" in out
        assert E.compute_sim3_transform_robust(src[:3], dst[:3], 4, 4.0, 50, 4, "pts")[0] is None
        assert "too few input points (3 from pts), at least 4 needed" in capsys.readouterr().out
        E.compute_sim3_transform(np.zeros((5, 3)), dst[:5])
        assert "zero variance" in capsys.readouterr().out
    finally:
        E.VERBOSE = False


def test_run_fusion_with_ground_truth_gnss(E, golden, tmp_path):
    """Step 6 with the optional second GNSS file (ref :949-966, :1013-1075): primary = the 'combined' log, ground truth = the
    kitti04gps log loaded with CONFIG['ground_truth_gps_filtering']; the raw-SLAM / Sim3 / EKF rows against both and the reference's
    choice of plot reference, against the golden computed with the reference's own functions (tests/golden/gen_golden.py)."""
    g, k, s6 = golden("c1_combined.npz"), golden("kat_bundled.npz"), golden("step6_gt.npz")
    slam_f, gps_f, gt_f = tmp_path / "traj.txt", tmp_path / "gps.txt", tmp_path / "gt.txt"
    np.savetxt(slam_f, np.column_stack((k["ts"], k["pos"], k["quat"])), fmt="%.18e")
    fill = lambda n: (np.full(n, 4), np.full(n, 5))
    np.savetxt(gps_f, np.column_stack((g["gps_t_raw"], g["lat"], g["lon"], g["alt"], *fill(len(g["lat"])))), fmt="%.18e")
    np.savetxt(gt_f, np.column_stack((s6["gt_t_raw"], s6["gt_lat"], s6["gt_lon"], s6["gt_alt"], *fill(len(s6["gt_lat"])))), fmt="%.18e")
    np.random.seed(0)
    out = E.run_fusion(str(slam_f), str(gps_f), gt_gps_path=str(gt_f))
    assert out["ground_truth_gps"]["utm_zone"] == f"{int(s6['gt_zone'])}N" and out["plot_error_ref"] == "ground_truth" and str(s6["plot_ref"]) == "gt"
    np.testing.assert_allclose(out["ground_truth_gps"]["positions"], s6["gt_p"], atol=5e-9, rtol=0)      # GT filtering is disabled by default (:42-45)
    for tag, key in (("primary", "primary"), ("ground_truth", "gt")):
        e = out["errors"][tag]
        np.testing.assert_array_equal(e["valid"], s6[f"valid_{key}"])
        for row, label in enumerate(("raw_slam", "sim3", "ekf")):
            want = s6[f"err_{key}"][row]
            got = np.array([e[label]["count"], e[label]["mean"], e[label]["median"], e[label]["rmse"]])
            assert got[0] == want[0] == len(s6[f"post_idx_{key}"])
            np.testing.assert_allclose(got[1:], want[1:], rtol=1e-12, atol=1e-7, err_msg=f"{tag} {label}")
    # no ground truth file, or one that the loader empties: the primary GPS is the plot reference (:1070-1074)
    np.random.seed(0)
    out2 = E.run_fusion(str(slam_f), str(gps_f))
    assert out2["errors"]["ground_truth"] is None and out2["plot_error_ref"] == "primary"
    np.testing.assert_allclose(out2["pos"], out["pos"], atol=0, rtol=0)


def test_ragged_batch_vs_oracle(B, orc):
    """Trajectories of different lengths in one launch (flat arrays + offsets), incl. lengths 0, 1, 2, 63, 64, 65."""
    import torch
    lens = [271, 0, 1, 2, 63, 64, 65, 128, 129, 400, 1000, 33, 700]
    parts = [B.TrajectoryBatch.synthetic(1, max(n, 1), layout=0, seed=31, traj0=k).host_traj_major() for k, n in enumerate(lens)]
    cat = lambda key, n_: np.concatenate([p[key][0][:n] for p, n in zip(parts, lens)]) if n_ else None
    ts, pos, quat, gps, valid = (cat(k, 1) for k in ("ts", "pos", "quat", "gps", "valid"))
    ip = np.stack([p["init_pos"][0] for p in parts]); iq = np.stack([p["init_quat"][0] for p in parts])
    offs = np.cumsum([0] + lens).astype(np.int64)
    d = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
    po, qo, st = B.ekf_fuse_ragged(d(ts), d(pos), d(quat), d(gps), d(valid, torch.uint8), d(offs, torch.int64), d(ip), d(iq))
    pp, qp, stp, R, t, s = B.fuse_pipeline_ragged(d(ts), d(pos), d(quat), d(gps), d(valid, torch.uint8), d(offs, torch.int64))
    torch.cuda.synchronize()
    po, qo, st, pp, stp = po.cpu().numpy(), qo.cpu().numpy(), st.cpu().numpy(), pp.cpu().numpy(), stp.cpu().numpy()
    for k, n in enumerate(lens):
        sl = slice(offs[k], offs[k + 1])
        if n == 0:
            assert st[k] == 0
            continue
        ro, rq, rs = orc.apply_ekf_correction_aligned(ts[sl], pos[sl], quat[sl], gps[sl], valid[sl], ip[k], iq[k], return_status=True)
        assert np.abs(po[sl] - ro).max() < POS_TOL and np.abs(qo[sl] - rq).max() < Q_TOL and st[k] == rs, (k, n)
        rp, rqq, rst, _, _, _ = orc.fuse_pipeline_batch(ts[sl][None], pos[sl][None], quat[sl][None], gps[sl][None], valid[sl][None])
        if np.isfinite(rp).all():
            assert np.abs(pp[sl] - rp[0]).max() < 1e-6 and (stp[k] & 0xff) == (rst[0] & 0xff), (k, n)
        else:
            assert np.isnan(pp[sl]).all() and (stp[k] >> 8) == (rst[0] >> 8) == (1 | 32), (k, n)   # fewer than min_samples valid rows: the reference raises (:975)
    # every valid row instead of the reference's choice: the fit is None below 3 rows (:430)
    pa, _, sta, _, _, _ = B.fuse_pipeline_ragged(d(ts), d(pos), d(quat), d(gps), d(valid, torch.uint8), d(offs, torch.int64), fit_rows="all")
    pa, sta = pa.cpu().numpy(), sta.cpu().numpy()
    for k, n in enumerate(lens):
        if n == 0:
            continue
        sl = slice(offs[k], offs[k + 1])
        rp, _, rst, _, _, _ = orc.fuse_pipeline_batch(ts[sl][None], pos[sl][None], quat[sl][None], gps[sl][None], valid[sl][None], fit_rows="all")
        if np.isfinite(rp).all():
            assert np.abs(pa[sl] - rp[0]).max() < 1e-6 and (sta[k] & 0xff) == (rst[0] & 0xff), (k, n)
        else:
            assert np.isnan(pa[sl]).all() and (sta[k] >> 8) == 1, (k, n)


def test_geodetic_to_enu_kernel(B, orc, golden):
    """The additional ENU projection (north star wording): vs the oracle's long-double ECEF form, and vs UTM locally (a tangent-plane
    frame and a conformal projection agree to ~1e-3 relative over a few hundred metres after removing grid convergence/scale)."""
    import torch
    g = golden("c1_combined.npz")
    lat, lon, alt = g["lat"], g["lon"], g["alt"]
    offs = torch.tensor([0, len(lat)], dtype=torch.int64).cuda()
    ref = torch.tensor([[lat[0], lon[0], alt[0]]], dtype=torch.float64).cuda()
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    e, n, u = B.geodetic_to_enu_batch(d(lat), d(lon), d(alt), offs, ref)
    eo, no, uo = orc.geodetic_to_enu(lat, lon, alt, lat[0], lon[0], alt[0])
    # the double ECEF difference cancels ~6.4e6 m coordinates: one ulp there is 9.3e-10 m and a handful of roundings add up
    np.testing.assert_allclose(e.cpu().numpy(), eo, atol=1e-8, rtol=0)
    np.testing.assert_allclose(n.cpu().numpy(), no, atol=1e-8, rtol=0)
    np.testing.assert_allclose(u.cpu().numpy(), uo, atol=1e-8, rtol=0)
    assert abs(eo[0]) < 1e-9 and abs(no[0]) < 1e-9 and abs(uo[0]) < 1e-9
    # path length agrees with the UTM track to the projection scale (k ~ 0.9996..1.0004) over this ~400 m drive
    d_enu = np.hypot(np.diff(eo), np.diff(no)).sum(); d_utm = np.hypot(np.diff(g["utm"][:, 0]), np.diff(g["utm"][:, 1])).sum()
    assert abs(d_enu / d_utm - 1.0) < 1e-3


def test_capi_error_paths(B):
    """Error behaviour of the boundary: bad arguments return GSF_ERR_INVALID_ARG with a message (no launch, no crash)."""
    import ctypes as C
    import torch
    from gps_optimize_slam_amd import _lib
    L = _lib.load(); h = B.context().handle
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    offs = torch.tensor([0, 8], dtype=torch.int64, device="cuda")
    assert L.gsf_utm_forward_batch_dev(h, x.data_ptr(), x.data_ptr(), None, None, None, 1, x.data_ptr(), x.data_ptr()) == 1
    assert "NULL" in _lib.last_error()
    assert L.gsf_utm_forward_batch_dev(None, x.data_ptr(), x.data_ptr(), offs.data_ptr(), None, None, 1, x.data_ptr(), x.data_ptr()) == 1
    assert L.gsf_geodetic_to_enu_batch_dev(h, x.data_ptr(), x.data_ptr(), x.data_ptr(), offs.data_ptr(), x.data_ptr(), -1, x.data_ptr(), x.data_ptr(), x.data_ptr()) == 1
    assert L.gsf_set_option(h, b"no_such_option", 1) != 0
    with pytest.raises(_lib.GsfError):
        _lib.check(L.gsf_set_option(h, b"no_such_option", 1))
    # B == 0 is a no-op success on every batched entry
    assert L.gsf_utm_forward_batch_dev(h, None, None, offs.data_ptr(), offs.data_ptr(), offs.data_ptr(), 0, None, None) == 0
    # the row rule of the global Sim3 (gsf_set_sim3_rows) and the mask entry (gsf_sim3_fit_rows_batch*)
    assert L.gsf_set_sim3_rows(h, 2, 4, 5.0, 180.0) == 1 and "mode" in _lib.last_error()
    assert L.gsf_set_sim3_rows(h, 1, -1, 5.0, 180.0) == 1
    assert L.gsf_set_sim3_rows(None, 1, 4, 5.0, 180.0) == 1
    m = torch.zeros(64, dtype=torch.uint8, device="cuda"); n = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert L.gsf_sim3_fit_rows_batch_dev(h, None, None, m.data_ptr(), None, 1, 8, 4, 5.0, 180.0, m.data_ptr(), n.data_ptr(), n.data_ptr()) == 1
    assert L.gsf_sim3_fit_rows_batch_dev(h, x.data_ptr(), None, m.data_ptr(), None, -1, 8, 4, 5.0, 180.0, m.data_ptr(), n.data_ptr(), n.data_ptr()) == 1
    assert L.gsf_sim3_fit_rows_batch_dev(h, x.data_ptr(), None, m.data_ptr(), None, 0, 8, 4, 5.0, 180.0, m.data_ptr(), n.data_ptr(), n.data_ptr()) == 0
    assert L.gsf_sim3_fit_rows_batch(h, None, None, None, None, 1, 8, 4, 5.0, 180.0, None, None, None) == 1
    assert L.gsf_trim(None) == 1
    B.context().set_sim3_rows("reference", B.CONFIG)                      # (the failed calls above changed nothing)


def test_trim_releases_the_workspaces_and_the_next_call_regrows_them(B):
    """gsf_trim: the grow-only arenas of a context (staging of the host-pointer entries, K2b rows, draw tape) go back to the driver; the same
    call afterwards allocates again and returns the same bits."""
    import torch
    from gps_optimize_slam_amd import _lib
    ctx = B.context()
    bt = B.TrajectoryBatch.synthetic(64, 271, layout=0, seed=3)
    seeds = torch.arange(64, dtype=torch.int64)
    a = B.fuse_pipeline_robust_batch(bt, B.mt19937_seed(seeds))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ctx.trim()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 >= free0                                                  # nothing is held that was not held before; usually strictly more is free
    b = B.fuse_pipeline_robust_batch(bt, B.mt19937_seed(seeds))
    for u, v in zip(a[:4], b[:4]):
        u = u.pos if hasattr(u, "pos") else u; v = v.pos if hasattr(v, "pos") else v
        assert torch.equal(torch.nan_to_num(u, nan=-1.0), torch.nan_to_num(v, nan=-1.0))
    ctx.trim(); ctx.trim()                                                 # idempotent


def _random_outage_batch(nb, N, seed):
    """Host-made stress batch: several outages per track with lengths from 1 pose to half the track, fixes that are NaN with the
    mask still set (demoted by the gate, Q10), yaw bursts inside outages (sharp-turn recoveries), outages at both ends,
    jittered and occasionally repeated stamps."""
    rng = np.random.default_rng(seed)
    dt = 0.1 + rng.uniform(-0.004, 0.004, size=(nb, N)); dt[:, 0] = 0.0
    dt[rng.random((nb, N)) < 0.01] = 0.0                                  # repeated stamps -> the dt clamp (Q9)
    ts = np.cumsum(dt, axis=1)
    head = np.cumsum(rng.normal(0, 0.01, size=(nb, N)), axis=1)
    valid = np.ones((nb, N), dtype=np.uint8)
    yaw_extra = np.zeros((nb, N))
    for b in range(nb):
        for _ in range(rng.integers(0, 5)):
            L = int(rng.choice([1, 2, 3, 7, 40, 64, 65, 130, N // 2]))
            s = int(rng.integers(0, max(1, N - L)))
            valid[b, s:s + L] = 0
            if L >= 3 and rng.random() < 0.5:                             # a turn faster than the 45 deg/s gate, inside the outage
                k = s + 1 + int(rng.integers(0, L - 2))
                yaw_extra[b, k:] += rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.2)
        if rng.random() < 0.2: valid[b, :int(rng.integers(1, 90))] = 0
        if rng.random() < 0.2: valid[b, N - int(rng.integers(1, 90)):] = 0
    step = 1.4 * np.stack([np.cos(head), np.sin(head), 0.01 * np.ones_like(head)], -1) * (dt[..., None] / 0.1)
    pos = np.cumsum(step, axis=1) + rng.normal(0, 0.01, size=(nb, N, 3))
    yaw = head + yaw_extra                                                # rotation about z: what the reference's yaw gate sees
    quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], -1) * rng.uniform(0.5, 2.0, size=(nb, N, 1))
    gps = pos * 1.03 + np.array([4.5e5, 5.4e6, 110.0]) + rng.normal(0, 0.4, size=(nb, N, 3))
    gps[valid == 0] = np.nan
    nanfix = (rng.random((nb, N)) < 0.01) & (valid == 1)
    gps[nanfix, rng.integers(0, 3)] = np.nan                              # NaN fix, mask still set
    init_pos = gps[:, 0].copy(); init_pos[np.isnan(init_pos)] = 0.0
    init_pos += np.array([4.5e5, 5.4e6, 110.0]) * np.isnan(gps[:, 0]).any(axis=1, keepdims=True)
    init_quat = quat[:, 0] / np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    return ts, pos, quat, gps, valid, init_pos, init_quat


@pytest.mark.parametrize("N", [257, 1000, 1025])
def test_big_batch_build_outage_stress_vs_oracle(B, orc, N):
    """The big-batch build of the wave kernel (ekf_wave_big_kernel, gsf_ekf_wave_big.hip: B > 2 048 -- slab loads / stores through LDS,
    its own translation unit and scheduler; the kernel behind the C3 and C5 figures) DIRECTLY against the oracle, not through its
    bit-equality with the small build: 4 096 outage-stress tracks per length, K4 with the default noise and the fused pipeline under
    both row rules.  Status words exact, positions inside the gate."""
    nb = 4096
    ts, pos, quat, gps, valid, ip, iq = _random_outage_batch(nb, N, 4000 + N)
    batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
    po, qo, sto = orc.fuse_batch(ts, pos, quat, gps, valid, ip, iq)
    p, q, st = B.ekf_fuse_batch(batch).host_traj_major()
    bad = np.nonzero(st != sto)[0]
    assert len(bad) == 0, (N, bad[:8].tolist())
    assert np.abs(p - po).max() < POS_TOL and np.abs(q - qo).max() < Q_TOL, (N, np.abs(p - po).max())
    for rows in ("reference", "all"):
        pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, fit_rows=rows)
        ok = np.isfinite(pr).all(axis=(1, 2))
        out, R, t, s = B.fuse_pipeline_batch(batch, fit_rows=rows)
        p, q, st = out.host_traj_major()
        assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, rows)
        assert ((st & ~(16 << 8)) == str_).all(), (N, rows, np.nonzero((st & ~(16 << 8)) != str_)[0][:8].tolist())
        assert np.abs(p[ok] - pr[ok]).max() < POS_TOL and np.abs(q[ok] - qr[ok]).max() < Q_TOL, (N, rows, np.abs(p[ok] - pr[ok]).max())
        assert np.abs(s.cpu().numpy()[ok] - sr[ok]).max() < 1e-10


@pytest.mark.parametrize("N", [300, 777, 4099])
def test_random_outage_patterns_every_kernel_vs_oracle(B, orc, N):
    """Outage structure stress: every K4 kernel (both layouts, both routes of the time-major one) against the dense oracle on tracks with up to
    four outages of 1..N/2 poses, NaN fixes, sharp-turn recoveries, outages at both ends -- positions inside the gate, status bits
    and therefore every start / recovery / sharp-turn / RTS decision exact."""
    nb = 192 if N < 1000 else 48                      # N = 4099: outages of up to 2 049 poses, i.e. carried over 32 chunks
    ts, pos, quat, gps, valid, ip, iq = _random_outage_batch(nb, N, seed=100 + N)
    po, qo, sto = orc.fuse_batch(ts, pos, quat, gps, valid, ip, iq)
    for bit in (1, 2, 4, 8):                          # outage, RTS, sharp-turn recovery, ended-in-outage all occur in the batch
        assert (sto & bit).any(), bit
    for layout in LAYOUTS:                            # wave kernel, time-major via the wave kernel, time-major lane kernel
        with route(B, layout) as lay:
            batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=lay)
            p, q, st = B.ekf_fuse_batch(batch).host_traj_major()
        np.testing.assert_array_equal(st, sto, err_msg=f"layout {layout}")
        assert np.abs(p - po).max() < POS_TOL and np.abs(q - qo).max() < Q_TOL, (layout, np.abs(p - po).max())


def test_gps_ransac_filter_vs_reference_goldens(E, golden):
    """next-3: filter_gps_outliers_ransac with the RANSAC on the GPU against runs of the reference itself (scikit-learn's
    RANSACRegressor, seeded global RNG): the same rows kept, bit for bit, and the RNG left in the same state (the draw that follows)."""
    g = golden("gpsfilter_cases.npz")
    for name in g["names"]:
        sliding, width, stepf, deg, ms, thr, trials = g[f"{name}_cfg"]
        cfg = {"enabled": name != "disabled", "use_sliding_window": bool(sliding), "window_duration_seconds": float(width),
               "window_step_factor": float(stepf), "polynomial_degree": int(deg), "min_samples": int(ms),
               "residual_threshold_meters": float(thr), "max_trials": int(trials)}
        np.random.seed(int(g[f"{name}_seed"]))
        ft, fp = E.filter_gps_outliers_ransac(g[f"{name}_t"].copy(), g[f"{name}_p"].copy(), cfg)
        after = np.random.random()
        np.testing.assert_array_equal(ft, g[f"{name}_ft"], err_msg=name)
        np.testing.assert_array_equal(fp, g[f"{name}_fp"], err_msg=name)
        assert after == float(g[f"{name}_after"]), (name, "RNG stream position differs from the reference's")


def test_ransac_poly_batch_kernel(B):
    """The batched entry: many problems in one launch agree with the same problems launched one by one; no-consensus status."""
    import torch
    rng = np.random.default_rng(3)
    P, n, trials, ms = 300, 150, 50, 6
    t = np.tile(np.arange(n) * 0.1, P) + rng.uniform(0, 0.01, P * n)
    y = 5.4e6 + 3.0 * t + 0.2 * t * t + rng.normal(0, 0.5, P * n)
    bad = rng.random(P * n) < 0.1
    y[bad] += rng.choice([-1, 1], bad.sum()) * rng.uniform(30, 200, bad.sum())
    offs = np.arange(0, (P + 1) * n, n, dtype=np.int64)
    idx = np.stack([np.stack([rng.choice(n, ms, replace=False) for _ in range(trials)]) for _ in range(P)]).astype(np.int32)
    d = lambda a: torch.as_tensor(a).cuda()
    mask, ntr, nin, st = B.ransac_poly_batch(d(t), d(y), d(offs), d(idx), 2, 10.0)
    mask, ntr, nin, st = mask.cpu().numpy(), ntr.cpu().numpy(), nin.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all() and (ntr >= 1).all() and (ntr <= trials).all()
    assert (mask.reshape(P, n).sum(axis=1) == nin).all()
    assert (mask.astype(bool) & bad).sum() < 0.02 * bad.sum()          # the spikes are rejected
    for p in (0, 17, 299):
        m1, n1, i1, s1 = B.ransac_poly_batch(d(t[p * n:(p + 1) * n].copy()), d(y[p * n:(p + 1) * n].copy()), d(np.array([0, n], dtype=np.int64)), d(idx[p:p + 1].copy()), 2, 10.0)
        np.testing.assert_array_equal(m1.cpu().numpy(), mask[p * n:(p + 1) * n]); assert int(n1.item()) == ntr[p]
    # an impossible threshold: every trial has zero inliers -> status 1, empty mask, all trials consumed
    m0, n0, i0, s0 = B.ransac_poly_batch(d(t[:n].copy()), d(y[:n].copy()), d(np.array([0, n], dtype=np.int64)), d(idx[:1].copy()), 2, -1.0)
    assert int(s0.item()) == 1 and int(n0.item()) == trials and int(m0.sum().item()) == 0


def test_gps_ransac_problems_vs_live_sklearn(E):
    """Randomised next-3 problems against scikit-learn itself (the reference's dependency), run live with the same seed: inlier
    mask, and the RNG position afterwards, for degrees 1-3, 4-10 samples, thresholds from tight to loose, 0-45 % outliers.
    Stamps are track-relative (0..130 s, as in the reference's data), where scikit-learn's float64 solve on raw stamps is itself within
    1e-7 m of the least-squares polynomial.  With epoch-sized stamps it is tens of metres off (the centred t^2 column's part orthogonal
    to t lies below its own rounding), so there the product follows the exact fit in window-local time and is held to the 50-digit
    yardstick of tests/prefilter_fit_ref.py instead ("Domain of the pre-filter's fit"; tests/test_prefilter_fit.py)."""
    from sklearn.linear_model import RANSACRegressor
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import PolynomialFeatures
    rng = np.random.default_rng(77)
    for case in range(60):
        n = int(rng.integers(12, 260)); deg = int(rng.integers(1, 4)); ms = int(rng.integers(max(deg + 1, 4), 11))
        thr = float(rng.choice([0.8, 2.0, 10.0, 50.0])); trials = int(rng.choice([5, 50, 100]))
        t = np.sort(rng.uniform(0, 30, n)) + (0.0 if case % 3 else 100.0)
        y = 5.4e6 + 3.0 * (t - t[0]) + 0.2 * (t - t[0]) ** 2 + rng.normal(0, 0.4, n)
        bad = rng.random(n) < rng.uniform(0, 0.45)
        y[bad] += rng.choice([-1, 1], bad.sum()) * rng.uniform(5, 300, bad.sum())
        np.random.seed(case)
        model = make_pipeline(PolynomialFeatures(degree=deg), RANSACRegressor(min_samples=ms, residual_threshold=thr, max_trials=trials))
        try:
            model.fit(t.reshape(-1, 1), y); ref_mask = model[-1].inlier_mask_
        except ValueError:
            ref_mask = None
        ref_after = np.random.random()
        np.random.seed(case)
        try:
            mask = E._ransac_axes_mask(t, y.reshape(-1, 1), deg, ms, thr, trials)
        except ValueError:
            mask = None
        after = np.random.random()
        assert (mask is None) == (ref_mask is None), case
        if mask is not None:
            np.testing.assert_array_equal(mask, ref_mask, err_msg=f"case {case}: n={n} deg={deg} ms={ms} thr={thr}")
        assert after == ref_after, case


def test_prefilter_windows_of_exactly_min_samples_rows(E, orc):
    """A window that holds exactly min_samples fixes (the tail of a log, a sparse log): scikit-learn's sampler leaves its permutation range
    (min_samples / n = 1) and returns rows 0 .. min_samples-1 by reservoir sampling WITHOUT a draw.  The device chain restates that (round 5;
    before, such a log went to the window-by-window host route): same rows kept and same generator position as the oracle, which calls
    scikit-learn's own sampler -- on sparse logs whose sliding windows shrink to min_samples rows and below."""
    rng = np.random.default_rng(19)
    hit = 0
    for case in range(40):
        n = int(rng.integers(8, 40)); ms = int(rng.choice([4, 6, 8]))
        cfg = {"enabled": True, "use_sliding_window": True, "window_duration_seconds": float(rng.choice([1.5, 3.0, 6.0])), "window_step_factor": float(rng.choice([0.25, 0.5, 1.0])),
               "polynomial_degree": int(rng.choice([1, 2])), "min_samples": ms, "residual_threshold_meters": float(rng.choice([2.0, 10.0])), "max_trials": 30}
        t = np.cumsum(rng.uniform(0.2, 0.6, n))
        p = np.column_stack((4.5e5 + 9.0 * t, 5.4e6 - 4.0 * t + 0.3 * t * t, 110.0 + 0.1 * t)) + rng.normal(0, 0.3, (n, 3))
        p[rng.choice(n, size=2, replace=False)] += rng.normal(0, 40.0, (2, 3))
        ranges, _ = E._prefilter_windows(t, cfg, ms)
        hit += int(any(b - a == ms for a, b in (ranges or [])))
        np.random.seed(case)
        ft_o, fp_o = orc.filter_gps_outliers_ransac(t, p, cfg)
        after_o = np.random.random()
        np.random.seed(case)
        ft, fp = E.filter_gps_outliers_ransac(t, p, cfg)
        after = np.random.random()
        np.testing.assert_array_equal(ft, ft_o, err_msg=f"case {case}: n={n} ms={ms} {cfg}")
        np.testing.assert_array_equal(fp, fp_o)
        assert after == after_o, case
    assert hit >= 15                                                       # the n == min_samples windows really occur


def test_configs_beyond_the_fast_kernels_take_the_wide_routes(E):
    """Any CONFIG the reference accepts runs (no GsfError for being out of a kernel's range): polynomial_degree 4-5, min_samples 10-24
    and max_trials 1 500-3 000 in the GPS pre-filter take the wide fed-sample kernel (host draws by scikit-learn's sampler) and still
    reproduce scikit-learn's inlier mask and RNG position; the full filter with such a CONFIG equals the window-by-window route; a Sim3
    RANSAC with min_samples 10 / 70 draws on the device / on the host like np.random.choice."""
    from sklearn.linear_model import RANSACRegressor
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import PolynomialFeatures
    rng = np.random.default_rng(5)
    agree = 0
    for case in range(12):
        n = int(rng.integers(60, 260)); deg = int(rng.choice([4, 5, 2])); ms = int(rng.choice([10, 17, 24])); trials = int(rng.choice([60, 1500, 3000]))
        thr = float(rng.choice([2.0, 10.0]))
        t = np.sort(rng.uniform(0, 15, n))                                 # one 15 s window, track-relative stamps
        y = 5.4e6 + 3.0 * t + 0.2 * t ** 2 - 0.01 * t ** 3 + rng.normal(0, 0.4, n)
        bad = rng.random(n) < rng.uniform(0, 0.3)
        y[bad] += rng.choice([-1, 1], bad.sum()) * rng.uniform(20, 300, bad.sum())
        np.random.seed(case)
        model = make_pipeline(PolynomialFeatures(degree=deg), RANSACRegressor(min_samples=ms, residual_threshold=thr, max_trials=trials))
        model.fit(t.reshape(-1, 1), y); ref_mask = model[-1].inlier_mask_
        ref_after = np.random.random()
        np.random.seed(case)
        mask = E._ransac_axes_mask(t, y.reshape(-1, 1), deg, ms, thr, trials)
        assert np.random.random() == ref_after, case                        # same number of sample sets consumed
        # degree 4-5 on 15 s of stamps: the power columns are collinear to ~1e-9, LAPACK's SVD solve and a QR differ in the last digits
        # of the fit, which can move a row that sits on the threshold; everything else must agree
        assert (mask != ref_mask).sum() <= 1, (case, deg, ms, trials)
        agree += int(np.array_equal(mask, ref_mask))
    assert agree >= 10
    # the whole pre-filter with an out-of-range CONFIG == the reference's window loop on the same draws
    cfg = copy.deepcopy(E.CONFIG["gps_filtering_ransac"])
    cfg.update(enabled=True, polynomial_degree=4, min_samples=10, max_trials=1500)
    t = np.arange(400) * 0.1
    p = np.column_stack((4.5e5 + 10.0 * t, 5.4e6 + 3.0 * t + 0.1 * t ** 2, 110.0 + 0.01 * t)) + rng.normal(0, 0.3, (400, 3))
    p[::37] += 80.0
    np.random.seed(3)
    ft, fp = E.filter_gps_outliers_ransac(t, p, cfg)
    assert 350 <= len(ft) < 400 and not np.isin(t[::37], ft).any()       # the spikes are gone, the track stays
    # Sim3 RANSAC beyond the former cap of 8 samples: 10 (device draws) and 70 (host draws), same draws as the reference's call
    src = rng.normal(size=(300, 3)).cumsum(axis=0); dst = 1.07 * src + np.array([4.5e5, 5.4e6, 100.0]) + rng.normal(size=(300, 3)) * 0.02
    for ms in (10, 70):
        np.random.seed(11)
        R, tt, sc = E.compute_sim3_transform_robust(src, dst, ms, 1.0, 50, ms)
        after = np.random.random()
        np.random.seed(11)
        for _ in range(50):
            np.random.choice(300, ms, replace=False)
        assert np.random.random() == after and abs(sc - 1.07) < 1e-3


def test_fed_sample_sets_are_validated_and_trials_stride(B):
    """caller-fed row indices outside [0, n) must not be dereferenced (K2b and the polynomial RANSAC skip such a sample
    set and flag it), and max_trials above the block size is strided over the threads (200 trials on 128 threads)."""
    import torch
    rng = np.random.default_rng(0)
    n, trials = 120, 200
    tt = np.arange(n) * 0.1
    y = 3.0 + 0.5 * tt + 0.02 * tt * tt + rng.normal(size=n) * 0.05
    y[::11] += 30.0
    idx = np.stack([rng.permutation(n)[:6] for _ in range(trials)]).astype(np.int32)
    td, yd = torch.as_tensor(tt).cuda(), torch.as_tensor(y).cuda()
    offs = torch.tensor([0, n], dtype=torch.int64).cuda()
    mask, ntr, nin, st = B.ransac_poly_batch(td, yd, offs, torch.as_tensor(idx.reshape(1, trials, 6)).cuda(), 2, 1.0)
    assert int(st.item()) == 0 and int(nin.item()) >= n - 12 and 1 <= int(ntr.item()) <= trials
    bad = idx.copy(); bad[0, 2] = n + 5; bad[3, 0] = -1
    mask2, ntr2, nin2, st2 = B.ransac_poly_batch(td, yd, offs, torch.as_tensor(bad.reshape(1, trials, 6)).cuda(), 2, 1.0)
    assert int(st2.item()) == 2 and int(nin2.item()) >= n - 12                     # flagged, still a consensus set from the valid trials
    # K2b
    src = rng.normal(size=(n, 3)).cumsum(axis=0); dst = 1.1 * src + np.array([10.0, -3.0, 2.0]) + rng.normal(size=(n, 3)) * 0.01
    sidx = np.stack([rng.permutation(n)[:4] for _ in range(64)]).astype(np.int32)
    sidx[5, 1] = n; sidx[6, 3] = -7
    R, t, s, stt, m, ni = B.sim3_ransac_batch(torch.as_tensor(src).cuda(), torch.as_tensor(dst).cuda(), offs, torch.as_tensor(sidx.reshape(1, 64, 4)).cuda(), 1.0, 4)
    assert int(stt.item()) & 8 and not int(stt.item()) & 1 and abs(float(s.item()) - 1.1) < 1e-3


def test_device_chain_from_geodetic_log_vs_oracle(B, orc):
    """K1 (mask, zone pick, UTM forward) -> time alignment -> fit -> EKF+RTS from a ragged geodetic GNSS log without leaving the
    device, against the oracle chained the same way (load_gps_data's geodesy slice :258-271, dynamic_time_alignment :325-387,
    steps 3-5 :1002-1010)."""
    nb, N = 96, 271
    gb = B.GeodeticBatch.synthetic(nb, N, seed=5)
    out, R, t, s, aux = B.fuse_from_geodetic(gb)
    p, q, st = out.host_traj_major()
    offs = gb.gps_offsets.cpu().numpy()
    gt, llh = gb.gps_t.cpu().numpy(), gb.gps_llh.cpu().numpy()
    ts, pos, quat = gb.ts.cpu().numpy(), gb.pos.cpu().numpy(), gb.quat.cpu().numpy()
    utm, aligned, valid = aux["utm_rows"].cpu().numpy(), aux["aligned"].cpu().numpy(), aux["valid"].cpu().numpy()
    zone, south = aux["zone"].cpu().numpy(), aux["south"].cpu().numpy()
    assert (zone == 32).all() and (south == 0).all()                    # 8.395 E, 49.03 N (lon 8.39 -> zone 32)
    n_gap = 0
    for b in range(nb):
        lo, hi = offs[b], offs[b + 1]
        zo, hemi = orc.auto_utm_projection(llh[lo:hi, 1], llh[lo:hi, 0])
        assert zo == zone[b] and ("south" in hemi) == bool(south[b])
        e, n = orc.utm_forward(llh[lo:hi, 0], llh[lo:hi, 1], zo, "south" in hemi)
        rows = np.column_stack((e, n, llh[lo:hi, 2]))
        np.testing.assert_allclose(utm[lo:hi], rows, atol=5e-9, rtol=0)
        al, va = orc.dynamic_time_alignment(ts[b], gt[lo:hi], rows, 500, 5.0)
        np.testing.assert_array_equal(valid[b].astype(bool), va)
        np.testing.assert_allclose(aligned[b][va], al[va], atol=1e-8, rtol=0)
        n_gap += int(not va[1:-1].all())
    assert n_gap >= 5                                                   # outages (missing fixes, gap > 5 s) really occur
    po, qo, sto, Ro, to, so = orc.fuse_pipeline_batch(ts, pos, quat, aligned, valid)
    ok = np.isfinite(po).all(axis=(1, 2))
    assert ok.sum() >= nb - 2
    assert np.abs(p[ok] - po[ok]).max() < POS_TOL and np.abs(q[ok] - qo[ok]).max() < 1e-8
    np.testing.assert_array_equal(st[ok] & 0xff, sto[ok] & 0xff)
    # shards of the generator: ids [k, k+32) generated separately == rows of the full batch
    part = B.GeodeticBatch.synthetic(32, N, seed=5, traj0=32)
    o32 = offs[32]
    np.testing.assert_array_equal(part.ts.cpu().numpy(), ts[32:64])
    np.testing.assert_array_equal(part.gps_llh.cpu().numpy(), llh[o32:offs[64]])


def test_device_chain_drops_the_rows_the_loader_removes(B, orc):
    """A geodetic log with rows load_gps_data throws away before the projection (lat or lon zero / out of range, ref :259-264): the
    device chain must align on the remaining fixes only -- checked against the oracle chained on the filtered log, the way the
    reference's loader hands it to dynamic_time_alignment.  (A NaN row fed to the spline would wipe out the whole cubic segment.)"""
    import torch
    nb, N = 48, 271
    gb = B.GeodeticBatch.synthetic(nb, N, seed=11)
    offs = gb.gps_offsets.cpu().numpy()
    llh = gb.gps_llh.cpu().numpy().copy()
    rng = np.random.default_rng(4)
    bad_rows = []
    for b in range(nb):
        lo, hi = offs[b], offs[b + 1]
        if b % 4 == 3:
            continue                                                       # some logs stay clean
        for k in rng.choice(np.arange(lo + 2, hi - 2), size=3, replace=False):
            kind = rng.integers(0, 4)
            if kind == 0: llh[k, 0] = 0.0                                  # lat == 0
            elif kind == 1: llh[k, 1] = 0.0                                # lon == 0
            elif kind == 2: llh[k, 0] = 97.5                               # |lat| > 90
            else: llh[k, 1] = -200.0                                       # |lon| > 180
            bad_rows.append(k)
    gb.gps_llh = torch.as_tensor(llh).cuda()
    out, R, t, s, aux = B.fuse_from_geodetic(gb)
    p, q, st = out.host_traj_major()
    gt = gb.gps_t.cpu().numpy()
    ts, pos, quat = gb.ts.cpu().numpy(), gb.pos.cpu().numpy(), gb.quat.cpu().numpy()
    utm, aligned, valid = aux["utm_rows"].cpu().numpy(), aux["aligned"].cpu().numpy(), aux["valid"].cpu().numpy()
    assert np.isnan(utm[bad_rows, 0]).all() and np.isnan(utm[bad_rows, 1]).all()          # the geodesy slice marks them
    al_ref = np.full((nb, N, 3), np.nan); va_ref = np.zeros((nb, N), dtype=bool)
    for b in range(nb):
        lo, hi = offs[b], offs[b + 1]
        keep = orc.valid_latlon_mask(llh[lo:hi, 0], llh[lo:hi, 1])
        assert keep.sum() == (hi - lo) - sum(lo <= k < hi for k in bad_rows)
        la, lo_, alt, tt = llh[lo:hi, 0][keep], llh[lo:hi, 1][keep], llh[lo:hi, 2][keep], gt[lo:hi][keep]
        zo, hemi = orc.auto_utm_projection(lo_, la)
        e, n = orc.utm_forward(la, lo_, zo, "south" in hemi)
        al_ref[b], va_ref[b] = orc.dynamic_time_alignment(ts[b], tt, np.column_stack((e, n, alt)), 500, 5.0)
        np.testing.assert_array_equal(valid[b].astype(bool), va_ref[b], err_msg=f"log {b}")
        np.testing.assert_allclose(aligned[b][va_ref[b]], al_ref[b][va_ref[b]], atol=1e-8, rtol=0)
    assert va_ref.mean() > 0.8                                             # the bad rows did not take their segments with them
    po, qo, sto, Ro, to, so = orc.fuse_pipeline_batch(ts, pos, quat, al_ref, va_ref.astype(np.uint8))
    ok = np.isfinite(po).all(axis=(1, 2))
    assert ok.sum() >= nb - 2
    assert np.abs(p[ok] - po[ok]).max() < POS_TOL and np.abs(q[ok] - qo[ok]).max() < 1e-8
    np.testing.assert_array_equal(st[ok] & 0xff, sto[ok] & 0xff)


def test_device_mt19937_choice_matches_numpy(B):
    """np.random.choice(n, k, replace=False) of NumPy's legacy generator reproduced on the device: the same sample sets trial by
    trial AND the same generator state afterwards (the next NumPy draw continues the stream), for seeded streams and for a state
    handed over from the host's global generator; streams with n < k stay untouched."""
    import torch
    cases = [(7, 271, 50, 4), (123456, 1000, 20, 4), (0, 5, 40, 4), (2**32 - 1, 64, 30, 6), (99, 4, 10, 4), (5, 1730, 7, 4), (31, 300, 25, 1),
             (77, 3, 5, 4)]
    seeds = [c[0] for c in cases]
    for trials_mult in (1,):
        st = B.mt19937_seed(seeds)
        # one launch per case (trials / k differ); streams of the other cases are masked out by n < k
        for ci, (seed, n, trials, k) in enumerate(cases):
            npop = [0] * len(cases); npop[ci] = n
            idx = B.mt19937_choice_batch(st, npop, trials, k).cpu().numpy()[ci]
            np.random.seed(seed)
            if n >= k:
                ref = np.stack([np.random.choice(n, k, replace=False) for _ in range(trials)])
                np.testing.assert_array_equal(idx, ref, err_msg=f"case {ci}")
            key, pos = np.random.get_state()[1:3]
            got = st[ci].cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(got[:624], key, err_msg=f"state of case {ci}")
            assert int(got[624]) == int(pos), (ci, got[624], pos)
    # a state taken over from the host's global generator, mid-stream
    np.random.seed(2024); np.random.random(1000)
    st1 = B.mt19937_from_numpy()
    idx = B.mt19937_choice_batch(st1, [271], 300, 4).cpu().numpy()[0]
    ref = np.stack([np.random.choice(271, 4, replace=False) for _ in range(300)])
    np.testing.assert_array_equal(idx, ref)
    after = np.random.random()
    key, pos = st1[0].cpu().numpy().view(np.uint32)[:624], int(st1[0].cpu().numpy().view(np.uint32)[624])
    np.random.set_state(("MT19937", key, pos))
    assert np.random.random() == after


def test_k3_slab_build_equals_the_per_pose_build(B):
    """K3 moves its rows as slabs through LDS (apply_sim3_slab_kernel, the default) -- same arithmetic per pose as the per-pose kernel
    (gsf_set_option "ekf_variant" 11): identical bits on ragged sets with every kind of length (1, odd, 63 / 64 / 65, longer than a
    block's stride), invalid quaternions included."""
    import torch
    rng = np.random.default_rng(4)
    g = torch.Generator(device="cuda"); g.manual_seed(9)
    for trial in range(3):
        lens = np.array([1, 2, 3, 63, 64, 65, 127, 129, 271, 1000, 1025]) if trial == 0 else rng.integers(1, 500, size=int(rng.integers(1, 200)))
        offs = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device="cuda")
        n, nb = int(offs[-1]), len(lens)
        pos = torch.randn(n, 3, dtype=torch.float64, device="cuda", generator=g) * 100
        quat = torch.randn(n, 4, dtype=torch.float64, device="cuda", generator=g)
        quat[rng.integers(0, n, size=max(1, n // 300))] = 0.0
        A = torch.linalg.qr(torch.randn(nb, 3, 3, dtype=torch.float64, device="cuda", generator=g))[0]
        R = (A * torch.sign(torch.linalg.det(A)).reshape(nb, 1, 1)).reshape(nb, 9).contiguous()
        t = torch.randn(nb, 3, dtype=torch.float64, device="cuda", generator=g) * 1e5
        s_ = torch.rand(nb, dtype=torch.float64, device="cuda", generator=g) + 0.5
        out = {}
        try:
            for var in (0, 11):
                B.context().set_option("ekf_variant", var)
                out[var] = [o.cpu().numpy() for o in B.apply_sim3_batch(pos, quat, offs, R, t, s_)]
        finally:
            B.context().set_option("ekf_variant", 0)
        for a, b_ in zip(out[0], out[11]):
            np.testing.assert_array_equal(a, b_)
        assert np.isnan(out[0][1]).any()                                 # the invalid quaternions did come out as NaN rows


def test_k2b_single_precision_screen_keeps_the_double_counts(B):
    """K2b counts the inliers of every hypothesis with a packed single-precision screen and re-checks in double every row inside the
    rounding band (csrc/gsf_sim3.hip): counts, masks, fits and statuses must be those of the all-double count -- also with rows planted
    from nanometres to centimetres off the threshold sphere, a threshold inside the noise, one tiny enough that the band swallows it,
    a NaN row, wild rows 5 000 km away (set apart and screened with a band of their own), a set that starts with wild rows, and for one
    set (hypotheses spread over single-wave blocks) as well as many."""
    import torch
    rng = np.random.default_rng(12)

    def run(nt, npts, trials, thr, band_rows, wild=False):
        bt = B.TrajectoryBatch.synthetic(nt, npts, layout=0, seed=5)
        src = bt.pos.reshape(nt * npts, 3).contiguous()
        g3 = bt.gps.reshape(nt * npts, 3)
        dst = torch.where(torch.isnan(g3), src + torch.nanmean(g3 - src, dim=0, keepdim=True), g3).contiguous()
        d = dst.reshape(nt, npts, 3)
        for b_ in range(nt):
            rows = rng.choice(npts, size=band_rows, replace=False)
            u = rng.normal(size=(band_rows, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
            d[b_, rows] += torch.as_tensor(u * (thr + rng.normal(size=(band_rows, 1)) * 10.0 ** rng.uniform(-9, -2, size=(band_rows, 1))), device="cuda")
        if wild:
            d[0, 7] = 0.0; d[min(1, nt - 1), 9, 1] = float("nan")
            d[min(2, nt - 1), 0] = 0.0; d[min(3, nt - 1), :40] = 0.0     # a set that STARTS with a wild row; one whose first 40 rows (three of the five probes) are wild
        offs = torch.arange(0, nt * npts + 1, npts, dtype=torch.int64, device="cuda")
        idx = torch.as_tensor(np.stack([np.stack([rng.permutation(npts)[:4] for _ in range(trials)]) for _ in range(nt)]).astype(np.int32)).cuda()
        res = {}
        for scr in (1, 0):
            B.context().set_option("k2b_screen", scr)
            res[scr] = [o.cpu().numpy() for o in B.sim3_ransac_batch(src, dst, offs, idx, thr, 4)]
        for a, b_ in zip(res[1], res[0]):
            np.testing.assert_array_equal(a, b_)
        return res[1]

    try:
        out = run(48, 271, 300, 4.0, 40)
        assert (out[5] > 150).all()                                      # n_inliers: the fits found the tracks
        run(48, 271, 300, 0.05, 0)
        run(48, 271, 300, 1e-4, 0)
        run(40, 271, 300, 4.0, 20, wild=True)
        run(1, 271, 1000, 4.0, 40)
        run(3, 1000, 400, 4.0, 100)
    finally:
        B.context().set_option("k2b_screen", 1)


def test_chip_wide_draws_match_numpy(B):
    """The chip-wide route of the draws (csrc/gsf_rng_tape.hip: tape -> transition tables -> composed walk -> replay -> trace) against
    NumPy: sample sets trial by trial and the generator state afterwards, for populations from 2 to 2040, k up to 64, entries at
    every kind of block position, several streams per call; the same cases with the tape cut short (the one-wave kernel must take
    over, nothing half-written) and a population above the bound the caller gave (that stream alone goes the one-wave way)."""
    import ctypes
    import torch
    from gps_optimize_slam_amd import _lib

    def numpy_side(seed, skip, n, trials, k):
        np.random.seed(seed)
        if skip: np.random.random(skip)
        st = B.mt19937_from_numpy()
        ref = np.stack([np.random.choice(n, k, replace=False) for _ in range(trials)]) if n >= k else None
        key, pos = np.random.get_state()[1:3]
        return st, ref, key.copy(), int(pos)

    cases = [((7,), (271,), 1000, 4, 0), ((11,), (271,), 700, 4, 311), ((3, 4, 5), (271, 150, 64), 400, 6, 17),
             ((21,), (2,), 20000, 1, 5), ((22,), (3,), 9000, 2, 0), ((23,), (65,), 700, 4, 1), ((24,), (129,), 300, 64, 2),
             ((25,), (2040,), 40, 4, 0), ((26,), (1730,), 60, 8, 623), ((30, 31, 32, 33), (300, 3, 300, 1000), 90, 4, 9)]
    try:
        for mode in (-1, 2):                                            # 2 = the tape ends at 90 % of the expected consumption
            B.context().set_option("tape_draws", mode)
            for seeds, ns, trials, k, skip in cases:
                sides = [numpy_side(s_, skip, n, trials, k) for s_, n in zip(seeds, ns)]
                st = torch.cat([x[0] for x in sides], dim=0).contiguous()
                idx = B.mt19937_choice_batch(st, list(ns), trials, k).cpu().numpy()
                got = st.cpu().numpy().view(np.uint32)
                for b_, (_, ref, key, pos) in enumerate(sides):
                    if ref is not None:
                        np.testing.assert_array_equal(idx[b_], ref, err_msg=f"mode {mode} case {seeds} stream {b_}")
                    np.testing.assert_array_equal(got[b_, :624], key, err_msg=f"state, mode {mode} case {seeds} stream {b_}")
                    assert int(got[b_, 624]) == pos
        # a bound smaller than one population (raw C ABI: the Python wrapper always passes the true maximum)
        B.context().set_option("tape_draws", -1)
        sides = [numpy_side(41, 0, 300, 200, 4), numpy_side(42, 0, 400, 200, 4)]
        st = torch.cat([x[0] for x in sides], dim=0).contiguous()
        npop = torch.tensor([300, 400], dtype=torch.int32, device="cuda")
        idx = torch.empty((2, 200, 4), dtype=torch.int32, device="cuda")
        vp = lambda t_: ctypes.c_void_p(t_.data_ptr())
        rc = _lib.load().gsf_mt19937_choice_bounded_batch_dev(B.context().handle, vp(st), vp(npop), 300, 2, 200, 4, vp(idx))
        assert rc == 0
        torch.cuda.synchronize()
        for b_, (_, ref, key, pos) in enumerate(sides):
            np.testing.assert_array_equal(idx[b_].cpu().numpy(), ref)
            got = st[b_].cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(got[:624], key); assert int(got[624]) == pos
    finally:
        B.context().set_option("tape_draws", -1)


@pytest.mark.parametrize("early_exit", [False, True])
@pytest.mark.parametrize("fit_rows", ["reference", "all"])
@pytest.mark.parametrize("nb", [24, 8])
def test_robust_pipeline_chain_vs_oracle(B, orc, nb, fit_rows, early_exit):
    """RANSAC -> final fit -> Sim3 of pose 0 -> EKF+RTS as ONE device chain with the draws generated on the device, against the
    oracle fed with NumPy's own draws for the same seeds: identical inlier masks / counts, R, t, s and fused poses inside the gate.
    24 streams are drawn one wave per stream, 8 by the chip-wide route (csrc/gsf_rng_tape.hip), the empty set among them by neither.
    early_exit: the planted outliers keep every trajectory from saturating, so the probe must hand ALL of them to the wide kernels and
    every generator still ends where NumPy's ends (trial_info: max_trials drawn, no GSF_SIM3_FLAG_SATURATED)."""
    N = 271
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=41)
    h = batch.host_traj_major()
    # outliers: a few GNSS fixes thrown far off so that the robust fit differs from the plain one
    rng = np.random.default_rng(3)
    for b in range(nb):
        rows = rng.choice(np.where(h["valid"][b] != 0)[0], size=9, replace=False)
        batch.gps[b, rows] += torch_from(rng.normal(size=(9, 3)) * 40.0)
    batch.valid[5, :] = 0                                               # no usable fix: the reference returns None before drawing
    batch.quat[7, 0] = 0.0                                              # pose-0 quaternion invalid
    h = batch.host_traj_major()
    cfg = B.CONFIG["sim3_ransac"]
    seeds = np.arange(100, 100 + nb)
    st = B.mt19937_seed(seeds)
    out, R, t, s, nin, mask, info = B.fuse_pipeline_robust_batch(batch, st, fit_rows=fit_rows, early_exit=early_exit, return_info=True)
    p, q, status = out.host_traj_major()
    R, t, s, nin, mask, info = R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy(), nin.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy()
    assert not ((status >> 8) & 256).any()                                # nobody saturates: every track holds fixes 40 m off
    plain = B.fuse_pipeline_batch(batch, fit_rows=fit_rows)[1].cpu().numpy()
    differs = 0
    for b in range(nb):
        ok = (h["valid"][b] != 0) & ~np.isnan(h["gps"][b]).any(axis=1)
        if fit_rows == "reference":                                         # the rows main_process_gui hands to its robust fit (ref :973-998)
            rows = orc.pick_sim3_rows(h["ts"][b], ok)
            ok = np.zeros(N, dtype=bool)
            if rows is not None:
                ok[rows] = True
        src, dst = h["pos"][b][ok], h["gps"][b][ok]
        np.random.seed(int(seeds[b]))
        if ok.sum() >= cfg["min_samples"]:
            draws = np.stack([np.random.choice(int(ok.sum()), cfg["min_samples"], replace=False) for _ in range(cfg["max_trials"])]).astype(np.int32)
            res = orc.compute_sim3_transform_robust(src, dst, cfg["min_samples"], cfg["residual_threshold"], cfg["max_trials"], cfg["min_inliers_needed"],
                                                    sample_idx=draws, return_mask=True)
        else:
            res = (None, None, None)
        key, pos = np.random.get_state()[1:3]
        got = st[b].cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got[:624], key); assert int(got[624]) == int(pos)
        assert info[b, 1] == (cfg["max_trials"] if ok.sum() >= cfg["min_samples"] else 0)
        if res[0] is None:
            assert (status[b] >> 8) & 1 and np.isnan(p[b]).all() and np.isnan(R[b]).all()
            continue
        Ro, to, so, mo = res
        full = np.zeros(N, dtype=bool); full[np.where(ok)[0]] = mo
        np.testing.assert_array_equal(mask[b].astype(bool), full, err_msg=f"inlier mask of trajectory {b}")
        assert nin[b] == mo.sum()
        np.testing.assert_allclose(R[b].reshape(3, 3), Ro, atol=2e-9, rtol=0)
        assert abs(s[b] - so) < 1e-11
        if b == 7:
            assert np.isnan(p[b]).all() and (status[b] & 16)
            continue
        sp, sq = orc.transform_trajectory(h["pos"][b][:1], h["quat"][b][:1], Ro, to, so)
        po, qo, sto = orc.apply_ekf_correction_aligned(h["ts"][b], h["pos"][b], h["quat"][b], h["gps"][b], h["valid"][b], sp[0], sq[0], return_status=True)
        assert np.abs(p[b] - po).max() < POS_TOL and np.abs(q[b] - qo).max() < Q_TOL, (b, np.abs(p[b] - po).max())
        assert (status[b] & 0xff) == sto
        differs += int(np.abs(R[b] - plain[b]).max() > 1e-6)
    assert differs >= nb // 2                                           # the planted outliers really separate the robust from the plain fit


def torch_from(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def test_two_wave_pipeline_kernels_are_bit_identical(B):
    """The helper-wave build of the fused pipeline (a second wave computes every chunk's variances during the fit; 128-thread
    blocks = duo_kernel 1) runs the same functions on the same operands as the one-wave kernel: identical bits, so the automatic
    choice by batch size cannot change results (shard invariance)."""
    for N, nb in ((65, 500), (271, 1001), (384, 203), (640, 256)):
        batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=31)
        batch.quat[7, N // 3] = 0.0                                     # one track on the generic (bad quaternion) path
        batch.quat[9, 0] = 0.0                                          # pose-0 quaternion invalid: the main wave leaves right after the fit
        batch.valid[11, :] = 0                                          # no usable fix at all: fit is None, same early exit
        res = {}
        modes = (0, 1)
        for duo in modes:
            B.context().set_option("duo_kernel", duo)
            try:
                out, R, t, s = B.fuse_pipeline_batch(batch)
                res[duo] = out.host_traj_major() + (R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy())
            finally:
                B.context().set_option("duo_kernel", -1)
        out, R, t, s = B.fuse_pipeline_batch(batch)                     # automatic choice
        res["auto"] = out.host_traj_major() + (R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy())
        for key in list(modes[1:]) + ["auto"]:
            for x0, x1 in zip(res[0], res[key]):
                np.testing.assert_array_equal(x0, x1, err_msg=f"N={N} B={nb} duo={key}")


def test_host_pointer_forms_equal_device_forms(B):
    """The host-array entry points added for a ctypes-only caller (fused pipeline, robust pipeline, the geodesy slice of
    load_gps_data, the fed-sample polynomial RANSAC) stage through the context's arena and run the SAME launches as the `_dev`
    forms: identical bits, and the generator states come back advanced identically."""
    import ctypes as C
    import torch
    from gps_optimize_slam_amd import _lib
    from gps_optimize_slam_amd.ekfgpsslam import CONFIG
    L, ctx = _lib.load(), B.context()
    h, hp = ctx.handle, _lib.hptr
    ctx.set_sim3_rows("reference", CONFIG)                               # the raw host-pointer calls below follow the context's row rule
    cfg = _lib.EkfConfig.from_config(CONFIG)
    nb, N = 37, 193
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=5)
    hb = batch.host_traj_major()
    # ---- plain pipeline
    out, R, t, s = B.fuse_pipeline_batch(batch)
    pd, qd, sd = out.host_traj_major()
    Rh, th, sh = np.empty((nb, 9)), np.empty((nb, 3)), np.empty(nb)
    ph, qh, sth = np.empty((nb, N, 3)), np.empty((nb, N, 4)), np.empty(nb, dtype=np.int32)
    _lib.check(L.gsf_fuse_pipeline_batch(h, 0, hp(hb["ts"]), hp(hb["pos"]), hp(hb["quat"]), hp(hb["gps"]), hp(hb["valid"]), C.byref(cfg), nb, N,
                                         hp(Rh), hp(th), hp(sh), hp(ph), hp(qh), hp(sth)))
    for a, b_ in ((ph, pd), (qh, qd), (sth, sd), (Rh, R.cpu().numpy()), (th, t.cpu().numpy()), (sh, s.cpu().numpy())):
        np.testing.assert_array_equal(a, b_)
    # ---- robust pipeline: per-trajectory legacy streams
    r = CONFIG["sim3_ransac"]
    st_dev = B.mt19937_seed(np.arange(100, 100 + nb))
    st_host = st_dev.cpu().numpy().copy()
    outr, Rr, tr, sr, nin, mask = B.fuse_pipeline_robust_batch(batch, st_dev, early_exit=False)      # (the option lives on the context: the host-pointer call below runs the same mode)
    pr, qr, str_ = outr.host_traj_major()
    ninh, maskh = np.empty(nb, dtype=np.int32), np.empty((nb, N), dtype=np.uint8)
    _lib.check(L.gsf_fuse_pipeline_robust_batch(h, hp(hb["ts"]), hp(hb["pos"]), hp(hb["quat"]), hp(hb["gps"]), hp(hb["valid"]), C.byref(cfg), nb, N,
                                                int(r["min_samples"]), float(r["residual_threshold"]), int(r["max_trials"]), int(r["min_inliers_needed"]),
                                                hp(st_host), hp(Rh), hp(th), hp(sh), hp(ph), hp(qh), hp(sth), hp(ninh), hp(maskh)))
    for a, b_ in ((ph, pr), (qh, qr), (sth, str_), (Rh, Rr.cpu().numpy()), (sh, sr.cpu().numpy()), (ninh, nin.cpu().numpy()), (maskh, mask.cpu().numpy()),
                  (st_host, st_dev.cpu().numpy())):
        np.testing.assert_array_equal(a, b_)
    # ---- geodesy slice of load_gps_data
    gb = B.GeodeticBatch.synthetic(11, 150, seed=3)
    offs = gb.gps_offsets.cpu().numpy(); llh = gb.gps_llh.cpu().numpy()
    utm_d = torch.empty_like(gb.gps_llh); z_d = torch.empty(11, dtype=torch.int32, device="cuda"); s_d = torch.empty(11, dtype=torch.int32, device="cuda")
    _lib.check(L.gsf_gps_rows_to_utm_batch_dev(h, B._p(gb.gps_llh), B._p(gb.gps_offsets), 11, B._p(utm_d), B._p(z_d), B._p(s_d)))
    utm_h, z_h, s_h = np.empty_like(llh), np.empty(11, dtype=np.int32), np.empty(11, dtype=np.int32)
    _lib.check(L.gsf_gps_rows_to_utm_batch(h, hp(llh), hp(offs), 11, hp(utm_h), hp(z_h), hp(s_h)))
    np.testing.assert_array_equal(utm_h, utm_d.cpu().numpy()); np.testing.assert_array_equal(z_h, z_d.cpu().numpy())
    np.testing.assert_array_equal(s_h, s_d.cpu().numpy())
    # ---- fed-sample polynomial RANSAC
    rng = np.random.default_rng(2)
    P, rows, trials, ms = 9, 120, 40, 6
    tt = np.sort(rng.uniform(0, 30, size=(P, rows)), axis=1).ravel(); yy = (0.3 * tt ** 2 - tt + rng.normal(size=tt.size) * 0.2)
    yy[rng.integers(0, yy.size, 60)] += 25.0
    po = np.arange(0, (P + 1) * rows, rows, dtype=np.int64)
    idx = np.stack([np.stack([rng.permutation(rows)[:ms] for _ in range(trials)]) for _ in range(P)]).astype(np.int32)
    m_d, ntr_d, nin_d, st_d = B.ransac_poly_batch(torch.as_tensor(tt).cuda(), torch.as_tensor(yy).cuda(), torch.as_tensor(po).cuda(), torch.as_tensor(idx).cuda(), 2, 1.0)
    m_h, ntr_h, nin_h, st_h = np.empty(tt.size, dtype=np.uint8), np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
    _lib.check(L.gsf_ransac_poly_batch(h, hp(tt), hp(yy), hp(po), P, hp(idx), trials, ms, 2, 1.0, 0.99, hp(m_h), hp(ntr_h), hp(nin_h), hp(st_h)))
    for a, b_ in ((m_h, m_d), (ntr_h, ntr_d), (nin_h, nin_d), (st_h, st_d)):
        np.testing.assert_array_equal(a, b_.cpu().numpy())
    # ---- ragged tracks (different lengths), the equal-window Umeyama and the ENU projection
    lens = np.array([3, 64, 65, 190, 1, 128, 77], dtype=np.int64)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pick = np.concatenate([np.arange(k * N, k * N + lens[k]) for k in range(len(lens))])
    fl = {k: np.ascontiguousarray(hb[k].reshape((nb * N,) + hb[k].shape[2:])[pick]) for k in ("ts", "pos", "quat", "gps", "valid")}
    nr, T = len(lens), int(ro[-1])
    dv = {k: torch.as_tensor(v).cuda() for k, v in fl.items()}
    dro = torch.as_tensor(ro).cuda()
    po_d, qo_d, st_d2, R_d, t_d, s_d2 = B.fuse_pipeline_ragged(dv["ts"], dv["pos"], dv["quat"], dv["gps"], dv["valid"], dro)
    Rr_, tr_, sr_ = np.empty((nr, 9)), np.empty((nr, 3)), np.empty(nr)
    pr_, qr_, sx_ = np.empty((T, 3)), np.empty((T, 4)), np.empty(nr, dtype=np.int32)
    _lib.check(L.gsf_fuse_pipeline_ragged(h, hp(fl["ts"]), hp(fl["pos"]), hp(fl["quat"]), hp(fl["gps"]), hp(fl["valid"]), hp(ro), C.byref(cfg), nr,
                                          hp(Rr_), hp(tr_), hp(sr_), hp(pr_), hp(qr_), hp(sx_)))
    for a, b_ in ((pr_, po_d), (qr_, qo_d), (sx_, st_d2), (Rr_, R_d), (tr_, t_d), (sr_, s_d2)):
        np.testing.assert_array_equal(a, b_.cpu().numpy())
    ip, iq = np.ascontiguousarray(hb["init_pos"][:nr]), np.ascontiguousarray(hb["init_quat"][:nr])
    po_d, qo_d, st_d2 = B.ekf_fuse_ragged(dv["ts"], dv["pos"], dv["quat"], dv["gps"], dv["valid"], dro, torch.as_tensor(ip).cuda(), torch.as_tensor(iq).cuda())
    _lib.check(L.gsf_ekf_fuse_ragged(h, hp(fl["ts"]), hp(fl["pos"]), hp(fl["quat"]), hp(fl["gps"]), hp(fl["valid"]), hp(ro), hp(ip), hp(iq), C.byref(cfg), nr,
                                     hp(pr_), hp(qr_), hp(sx_)))
    for a, b_ in ((pr_, po_d), (qr_, qo_d), (sx_, st_d2)):
        np.testing.assert_array_equal(a, b_.cpu().numpy())
    W = 50
    sw = np.ascontiguousarray(hb["pos"][:, :W]); dw = np.ascontiguousarray(np.nan_to_num(hb["gps"][:, :W]))
    Rw, tw, sw_, stw = B.sim3_umeyama_batch(torch.as_tensor(sw).cuda(), torch.as_tensor(dw).cuda())
    Rwh, twh, swh, stwh = np.empty((nb, 9)), np.empty((nb, 3)), np.empty(nb), np.empty(nb, dtype=np.int32)
    _lib.check(L.gsf_sim3_umeyama_windows(h, hp(sw), hp(dw), None, nb, W, hp(Rwh), hp(twh), hp(swh), hp(stwh)))
    for a, b_ in ((Rwh, Rw), (twh, tw), (swh, sw_), (stwh, stw)):
        np.testing.assert_array_equal(a, b_.cpu().numpy())
    lat, lon, alt = (np.ascontiguousarray(llh[:, k]) for k in range(3))
    ref = np.ascontiguousarray(np.stack([llh[offs[:-1]][:, 0], llh[offs[:-1]][:, 1], llh[offs[:-1]][:, 2]], axis=1))
    e_d, n_d, u_d = B.geodetic_to_enu_batch(torch.as_tensor(lat).cuda(), torch.as_tensor(lon).cuda(), torch.as_tensor(alt).cuda(), gb.gps_offsets, torch.as_tensor(ref).cuda())
    e_h, n_h, u_h = np.empty_like(lat), np.empty_like(lat), np.empty_like(lat)
    _lib.check(L.gsf_geodetic_to_enu_batch(h, hp(lat), hp(lon), hp(alt), hp(offs), hp(ref), 11, hp(e_h), hp(n_h), hp(u_h)))
    for a, b_ in ((e_h, e_d), (n_h, n_d), (u_h, u_d)):
        np.testing.assert_array_equal(a, b_.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("nb,N,probe", [(1000, 271, 64), (1000, 271, 3), (2500, 150, 64), (300, 1000, 16), (9, 271, 64), (9, 271, 2)])
def test_robust_early_exit_equals_the_full_chain_bit_for_bit(B, nb, N, probe):
    """gsf_set_option "ransac_early_exit": a trajectory stops at the first trial that counts every row of its fit (ref :413: only a STRICTLY
    larger count replaces the kept trial).  Against the chain that draws all max_trials, on the bench batch (1 000 x 271) and other
    shapes, with every 7th track given one fix 30 m off (it can never saturate: the wide kernels take its trials from where the probe
    stopped, carrying the arg-max key over) and every 11th a fix 3.9 m off (saturates late or never): R, t, s, n_inliers, inlier masks,
    fused poses, status words (but for the SATURATED bit) and the kept trial identical in every word; probe = 2 / 3 / 16 moves the
    hand-over point so that tracks saturating later are decided by the wide kernels with the probe's key merged in; 9 tracks: the
    few-sets form of K2b (hypotheses spread over the chip, keys merged by atomicMax)."""
    import torch
    bt = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=20250523)
    g = torch.Generator(device="cpu"); g.manual_seed(nb + N)
    rowmask = B.sim3_fit_rows_batch(bt.ts, bt.gps, bt.valid)[0].cpu()      # (the planted fixes sit among the rows the fit sees; they stay finite, so the choice of rows does not move)
    hit = torch.zeros(nb, dtype=torch.bool, device="cuda")
    for b in range(0, nb, 7):
        rows = torch.nonzero(rowmask[b] != 0).ravel()
        if rows.numel() > 8:
            bt.gps[b, int(rows[int(torch.randint(0, rows.numel(), (1,), generator=g))])] += 30.0; hit[b] = True
    for b in range(3, nb, 11):
        rows = torch.nonzero(rowmask[b] != 0).ravel()
        if rows.numel() > 8: bt.gps[b, int(rows[int(torch.randint(0, rows.numel(), (1,), generator=g))]), 0] += 3.9
    seeds = torch.arange(nb, dtype=torch.int64) + 1000
    ctx = B.context()
    st_f = B.mt19937_seed(seeds)
    full = B.fuse_pipeline_robust_batch(bt, st_f, early_exit=False, return_info=True)
    ctx.set_option("ransac_probe_trials", probe)
    try:
        st_e = B.mt19937_seed(seeds)
        ee = B.fuse_pipeline_robust_batch(bt, st_e, early_exit=True, return_info=True)
    finally:
        ctx.set_option("ransac_probe_trials", 64)
    SAT = 256 << 8
    (o, R, t, s, nin, mask, info), (oe, Re, te, se, nine, maske, infoe) = full, ee
    for a, b_ in ((o.pos, oe.pos), (o.quat, oe.quat), (R, Re), (t, te), (s, se)):
        assert torch.equal(torch.nan_to_num(a, nan=-1.0).view(torch.int64), torch.nan_to_num(b_, nan=-1.0).view(torch.int64))
    assert torch.equal(nin, nine) and torch.equal(mask, maske) and torch.equal(o.status, oe.status & ~SAT)
    assert torch.equal(info[:, 0], infoe[:, 0])                             # the same trial's inlier set was kept
    sat = (oe.status & SAT) != 0
    trials = B.CONFIG["sim3_ransac"]["max_trials"]
    assert not (o.status & SAT).any() and (info[:, 1][nin >= 0] == trials).all()
    # a saturated track drew only the probe's rounds, an unsaturated one everything -- and then its generator ends where the full chain's ends
    assert (infoe[sat, 1] <= min(probe, trials)).all() and (infoe[~sat, 1] == info[~sat, 1]).all()
    assert torch.equal(st_f[~sat], st_e[~sat])
    fitrows = B.sim3_fit_rows_batch(bt.ts, bt.gps, bt.valid)[1]
    assert torch.equal(sat, (nin == fitrows) & (info[:, 0] >= 0) & (info[:, 0] < probe))
    assert not sat[hit].any() and (nb < 100 or (sat.sum() > nb // 2))           # the 30 m fixes keep their tracks going; most clean tracks stop early
    print(f"[early exit {nb} x {N}, probe {probe}] saturated {int(sat.sum())}/{nb}; trials drawn by saturated tracks: "
          f"{torch.bincount(infoe[sat, 1].long()).nonzero().ravel().tolist()} -> {torch.bincount(infoe[sat, 1].long())[torch.bincount(infoe[sat, 1].long()) > 0].tolist()}")


@pytest.mark.gpu
def test_early_exit_keeps_its_flag_when_the_fit_then_fails(B):
    """A trajectory whose first trials count every row stops drawing -- also when the reference then returns None because there are fewer rows
    than min_inliers_needed (ref :416-418, after the loop): the same NaN outputs and n_inliers as the chain that draws every trial, and the
    SATURATED bit next to GSF_SIM3_NONE says that its generator stopped early (found by tests/campaigns/stress_run_chain.py: the bit used to be
    dropped on this branch, so a caller could not tell which generators had moved by fewer trials)."""
    import copy
    import torch
    cfg = copy.deepcopy(B.CONFIG)
    cfg["sim3_ransac"]["min_inliers_needed"] = 400                      # more than a 271-pose track can hold
    bt = B.TrajectoryBatch.synthetic(300, 271, layout=0, seed=31)
    seeds = torch.arange(300, dtype=torch.int64) + 5
    st_f, st_e = B.mt19937_seed(seeds), B.mt19937_seed(seeds)
    of, Rf, tf, sf, nf, mf, inf_f = B.fuse_pipeline_robust_batch(bt, st_f, cfg, early_exit=False, return_info=True)
    oe, Re, te, se, ne, me, inf_e = B.fuse_pipeline_robust_batch(bt, st_e, cfg, early_exit=True, return_info=True)
    assert torch.isnan(of.pos).all() and torch.isnan(oe.pos).all() and torch.isnan(Re).all()
    assert torch.equal(nf, ne) and torch.equal(mf, me) and torch.equal(inf_f[:, 0], inf_e[:, 0])
    sat = ((oe.status >> 8) & 256) != 0
    assert ((oe.status >> 8) & 1).all() and ((of.status >> 8) & 1).all() and torch.equal(of.status, oe.status & ~(256 << 8))
    assert sat.sum() > 250 and (inf_e[sat, 1] % 8 == 0).all() and (inf_e[sat, 1] <= 64).all() and (inf_f[:, 1] == cfg["sim3_ransac"]["max_trials"]).all()
    assert torch.equal(st_f[~sat], st_e[~sat]) and not torch.equal(st_f[sat], st_e[sat])


@contextlib.contextmanager
def block_kernel(B):
    """the workgroup-per-trajectory kernel behind the trajectory-major entry points (gsf_set_option "block_kernel" 1), restored afterwards"""
    ctx = B.context()
    ctx.set_option("block_kernel", 1)
    try:
        yield ctx
    finally:
        ctx.set_option("block_kernel", -1)


@pytest.mark.parametrize("rows", ["reference", "all"])
@pytest.mark.parametrize("N", [65, 129, 300, 640, 777, 1024])
def test_block_kernel_outage_stress_vs_oracle(B, orc, N, rows):
    """gsf_ekf_block.hip (one wave per 64-pose chunk, two-level scans through LDS) on the outage-stress tracks: up to four outages of 1..N/2
    poses (i.e. crossing up to eight chunk boundaries: the first-recovery records of barrier 4), NaN fixes, sharp-turn recoveries,
    outages at both ends, non-unit quaternions -- K4 against the dense oracle, status bits exact; the fused pipeline against the oracle's,
    under both row rules (the reference's choice ref :973-998 reaches this kernel as a row mask from a launch of sim3_rows_kernel: row bits
    of the status word exact, and a forced block_kernel = 1 must really run this kernel -- round 4 rerouted it silently)."""
    nb = 160
    ts, pos, quat, gps, valid, ip, iq = _random_outage_batch(nb, N, seed=500 + N)
    po, qo, sto = orc.fuse_batch(ts, pos, quat, gps, valid, ip, iq)
    pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, fit_rows=rows)
    with block_kernel(B):
        batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0)
        p, q, st = B.ekf_fuse_batch(batch).host_traj_major()
        out, R, t, s = B.fuse_pipeline_batch(batch, fit_rows=rows)
        pp, qp, stp = out.host_traj_major()
    np.testing.assert_array_equal(st, sto)
    assert np.abs(p - po).max() < POS_TOL and np.abs(q - qo).max() < Q_TOL
    ok = np.isfinite(pr).all(axis=(1, 2))
    assert (np.isfinite(pp).all(axis=(1, 2)) == ok).all() and ok.sum() >= nb // 3      # (short tracks lose their fit to the long outages: NaN rows on both sides)
    np.testing.assert_array_equal(stp[ok] & 0xff, str_[ok] & 0xff)
    rowbits = (32 | 64 | 128) << 8
    np.testing.assert_array_equal(stp & rowbits, str_ & rowbits)
    np.testing.assert_array_equal((stp >> 8) & 1, (str_ >> 8) & 1)
    assert np.abs(pp[ok] - pr[ok]).max() < POS_TOL and np.abs(qp[ok] - qr[ok]).max() < 1e-8
    np.testing.assert_allclose(R.cpu().numpy()[ok], Rr[ok], atol=1e-9, rtol=0)


def test_block_kernel_edge_cases_vs_oracle(B, orc, golden):
    """The block kernel on the edge cases of the golden EKF set that fit it (65..1024 poses) and on hand-made ones: an invalid quaternion in
    the middle of a track and at pose 0 (generic orientation path, barrier 2b), pose 0 without a usable fix (GNSS-side shift of the moments
    from a later chunk, barrier 0), fewer than three usable fixes (fit None -> NaN rows), all fixes missing, custom noise layouts."""
    import copy
    from gps_optimize_slam_amd.ekfgpsslam import CONFIG
    bt = B.TrajectoryBatch.synthetic(96, 271, layout=0, seed=9)
    h = bt.host_traj_major()
    ts, pos, quat, gps, valid = (h[k].copy() for k in ("ts", "pos", "quat", "gps", "valid"))
    quat[0, 100] = 0.0                                                   # zero quaternion mid-track: zero-motion branch (ref :84-86)
    quat[1, 0] = 0.0                                                     # ... at pose 0: SciPy raises in the pipeline (NaN rows), K4 treats it as zero motion
    quat[2, 64] = np.nan                                                 # NaN quaternion at a chunk boundary
    valid[3, :70] = 0; gps[3, :70] = np.nan                              # pose 0 and the whole first chunk without a fix: shift from chunk 1
    valid[4, 0] = 0                                                      # pose 0 masked but finite
    gps[5, 0] = np.nan                                                   # pose 0 valid but NaN
    valid[6, 2:] = 0; gps[6, 2:] = np.nan                                # two usable fixes: the fit is None
    valid[7, :] = 0; gps[7, :] = np.nan                                  # no fix at all
    valid[8, 200:] = 0; gps[8, 200:] = np.nan                            # ends in a long outage crossing a chunk boundary
    for cfg_over in (None, ([0.1, 0.2, 0.3], [0.1, 0.3, 0.7], [0.2, 0.25, 0.4]), ([0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3])):
        cfg = copy.deepcopy(CONFIG)
        if cfg_over:
            cfg["ekf"]["initial_cov_diag"][:3], cfg["ekf"]["process_noise_diag"][:3], cfg["ekf"]["meas_noise_diag"] = cfg_over
        po, qo, sto = orc.fuse_batch(ts, pos, quat, gps, valid, h["init_pos"], h["init_quat"], cfg)
        pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, cfg)
        with block_kernel(B):
            batch = B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, h["init_pos"], h["init_quat"], layout=0)
            p, q, st = B.ekf_fuse_batch(batch, config=cfg).host_traj_major()
            out, R, t, s = B.fuse_pipeline_batch(batch, config=cfg)
            pp, qp, stp = out.host_traj_major()
        np.testing.assert_array_equal(st, sto)
        assert np.abs(p - po).max() < POS_TOL and np.abs(q - qo).max() < Q_TOL
        ok = np.isfinite(pr).all(axis=(1, 2))
        assert not ok[1] and not ok[6] and not ok[7] and ok[[0, 2, 3, 4, 5, 8]].all()
        assert (np.isfinite(pp).all(axis=(1, 2)) == ok).all()
        np.testing.assert_array_equal(stp & 0xff, str_ & 0xff)
        np.testing.assert_array_equal((stp >> 8)[~ok] & 1, (str_ >> 8)[~ok] & 1)
        assert np.abs(pp[ok] - pr[ok]).max() < POS_TOL and np.abs(qp[ok] - qr[ok]).max() < 1e-8
    # the same bits whatever the batch size (the kernel choice never depends on B): rows of a sub-batch == rows of the batch
    with block_kernel(B):
        full = B.fuse_pipeline_batch(B.TrajectoryBatch.synthetic(700, 271, layout=0, seed=3))[0]
        part = B.fuse_pipeline_batch(B.TrajectoryBatch.synthetic(50, 271, layout=0, seed=3, traj0=300))[0]
        import torch
        assert torch.equal(full.pos[300:350], part.pos) and torch.equal(full.quat[300:350], part.quat)


@pytest.mark.parametrize("nb", [200, 700, 2500])
def test_pipeline_custom_noise_layouts_vs_oracle(B, orc, nb):
    """The wave kernels compile the choice of scans in for the default noise layout (x and y alike, z apart) and keep a generic
    build for every other layout (all three apart, all alike, y and z alike): both against the oracle, at batch sizes that pick
    the two-wave, the small-batch and the big-batch build."""
    import copy
    from gps_optimize_slam_amd.ekfgpsslam import CONFIG
    N = 193
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=17)
    h = batch.host_traj_major()
    for p0, qn, rn in (([0.1, 0.2, 0.3], [0.1, 0.3, 0.7], [0.2, 0.25, 0.4]),        # all three axes apart
                       ([0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]),         # all alike
                       ([0.3, 0.1, 0.1], [0.5, 0.1, 0.1], [0.4, 0.2, 0.2])):        # y and z alike
        cfg = copy.deepcopy(CONFIG)
        cfg["ekf"]["initial_cov_diag"][:3] = p0; cfg["ekf"]["process_noise_diag"][:3] = qn; cfg["ekf"]["meas_noise_diag"] = rn
        out, R, t, s = B.fuse_pipeline_batch(batch, config=cfg)
        p, q, st = out.host_traj_major()
        sel = slice(0, nb, max(1, nb // 40))
        pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(h["ts"][sel], h["pos"][sel], h["quat"][sel], h["gps"][sel], h["valid"][sel], cfg)
        assert np.abs(p[sel] - pr).max() < POS_TOL and np.abs(q[sel] - qr).max() < Q_TOL
        np.testing.assert_array_equal(st[sel] & 0xff, str_ & 0xff)
        k4 = B.ekf_fuse_batch(batch, config=cfg)
        p4, q4, st4 = k4.host_traj_major()
        po, qo, sto = orc.fuse_batch(h["ts"][sel], h["pos"][sel], h["quat"][sel], h["gps"][sel], h["valid"][sel], h["init_pos"][sel], h["init_quat"][sel], cfg)
        assert np.abs(p4[sel] - po).max() < POS_TOL and np.abs(q4[sel] - qo).max() < Q_TOL
        np.testing.assert_array_equal(st4[sel], sto)


def test_pipeline_fit_degenerate_and_mirrored_tracks_vs_oracle(B, orc):
    """The fused pipeline's fit takes the polar-iteration route where it applies and the SVD otherwise: exactly planar SLAM tracks
    (singular H: SVD route), GNSS mirrored through a plane (a true reflection: the :441-442 branch with well separated sigma3), a
    straight line (rank 1), two valid fixes only (None), all against the oracle's SVD-based fit."""
    nb, N = 64, 150
    batch = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=23)
    h = batch.host_traj_major()
    pos, gps, valid = h["pos"].copy(), h["gps"].copy(), h["valid"].copy()
    pos[0:8, :, 1] = 0.0                                                   # exactly planar SLAM side
    gps[8:16, :, 2] = 2.0 * np.nanmean(gps[8:16, :, 2], axis=1, keepdims=True) - gps[8:16, :, 2]   # altitude mirrored
    pos[16:20, :, 0] = pos[16:20, :, 2] * 0.5; pos[16:20, :, 1] = pos[16:20, :, 2] * 0.25         # straight line
    valid[20:24, 2:] = 0                                                   # two usable fixes
    pos[24:28] *= 1e-4                                                     # tiny track: scale >> 1
    hb = B.TrajectoryBatch.from_host(h["ts"], pos, h["quat"], gps, valid, h["init_pos"], h["init_quat"], layout=0)
    out, R, t, s = B.fuse_pipeline_batch(hb)
    p, q, st = out.host_traj_major()
    pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(h["ts"], pos, h["quat"], gps, valid)
    ok = np.isfinite(pr).all(axis=(1, 2))
    assert (np.isfinite(p).all(axis=(1, 2)) == ok).all() and not ok[20:24].any() and ok[:20].sum() >= 12
    np.testing.assert_array_equal(st & 0xff, str_ & 0xff)
    np.testing.assert_array_equal((st >> 8)[~ok], (str_ >> 8)[~ok])
    # rank-deficient sets leave the rotation about the track free: compare what the fit determines (the fused poses agree where the
    # oracle's own answer is stable), everything else to the usual tolerances
    stable = ok.copy(); stable[16:20] = False; stable[0:8] = False
    assert np.abs(p[stable] - pr[stable]).max() < POS_TOL and np.abs(q[stable] - qr[stable]).max() < 1e-8
    assert np.abs(s.cpu().numpy()[stable] - sr[stable]).max() < 1e-9
    Rg = R.cpu().numpy()[ok].reshape(-1, 3, 3)
    np.testing.assert_allclose(np.einsum("bij,bkj->bik", Rg, Rg), np.broadcast_to(np.eye(3), Rg.shape), atol=1e-11)
    assert np.abs(np.linalg.det(Rg) - 1.0).max() < 1e-11


@pytest.mark.gpu
def test_repeated_launches_return_the_same_bits(B):
    """No launch-to-launch variation anywhere on the path: the fused pipeline (small and big-batch builds, both row rules), K4 in both layouts,
    the robust chain from the same generator states and the C4 window fit, each launched several times on the same inputs (with other work in
    between, so that the workspaces and the caches are not in the state the first launch found) -- every output word identical."""
    import torch
    def bits(*ts):
        return [t.clone().view(torch.int64) if t.dtype == torch.float64 else t.clone() for t in ts]
    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    noise = torch.rand(1 << 24, device="cuda", dtype=torch.float64)
    for nb, N in ((1000, 271), (4096, 300)):
        bt = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=5)
        btt = B.TrajectoryBatch.synthetic(nb, N, layout=1, seed=5)
        for rows in ("reference", "all"):
            first = None
            for rep in range(4):
                out, R, t, s = B.fuse_pipeline_batch(bt, fit_rows=rows)
                o2 = B.ekf_fuse_batch(bt)
                o3 = B.ekf_fuse_batch(btt)
                got = bits(out.pos, out.quat, out.status, R, t, s, o2.pos, o2.quat, o2.status, o3.pos, o3.quat, o3.status)
                if first is None: first = got
                assert same(first, got), (nb, N, rows, rep)
                noise.mul_(1.0000001)                                     # 128 MB of unrelated traffic between the launches
    bt = B.TrajectoryBatch.synthetic(256, 271, layout=0, seed=6)
    seeds = torch.arange(256, dtype=torch.int64) + 77
    first = None
    for rep in range(3):
        out, R, t, s, nin, mask = B.fuse_pipeline_robust_batch(bt, B.mt19937_seed(seeds))
        got = bits(out.pos, out.quat, out.status, R, t, s, nin, mask)
        if first is None: first = got
        assert same(first, got), rep
        if rep == 0: B.context().trim()                                   # the second launch regrows every workspace
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    src = torch.randn(20000, 50, 3, dtype=torch.float64, device="cuda", generator=g)
    dst = 1.1 * src.flip(-1) + 0.01 * torch.randn(20000, 50, 3, dtype=torch.float64, device="cuda", generator=g)
    first = None
    for rep in range(3):
        got = bits(*B.sim3_umeyama_batch(src, dst))
        if first is None: first = got
        assert same(first, got), rep
        noise.mul_(1.0000001)


@pytest.mark.gpu
def test_random_reference_tracks_on_every_route(B, golden):
    """K4 on 64 random outage / sharp-turn / NaN-fix tracks against the REFERENCE's own outputs (ekf_random_tracks.npz, generated by
    apply_ekf_correction itself) -- every route: wave per trajectory (small build; big-batch build on 40 stacked copies), time-major through
    the transposes, lane per trajectory, workgroup per trajectory."""
    g = golden("ekf_random_tracks.npz")
    args = [g[k] for k in ("ts", "pos", "quat")] + [g["aligned"], g["valid"].astype(np.uint8), g["sp0"], g["sq0"]]
    for name, layout, opt, copies in (("wave", 0, None, 1), ("big-batch build", 0, None, 40), ("time-major via the wave kernel", 1, None, 1),
                                      ("lane", 1, ("lane_min_traj", 0), 1), ("block", 0, ("block_kernel", 1), 1)):
        a = [np.concatenate([x] * copies) for x in args]
        batch = B.TrajectoryBatch.from_host(*a, layout=layout)
        if opt: B.context().set_option(*opt)
        try:
            p, q, st = B.ekf_fuse_batch(batch).host_traj_major()
        finally:
            if opt: B.context().set_option(opt[0], 32768 if opt[0] == "lane_min_traj" else -1)
        nb = g["ts"].shape[0]
        for c in range(0, copies, max(1, copies - 1)):                       # first and last copy
            np.testing.assert_allclose(p[c * nb:(c + 1) * nb], g["out_pos"], atol=POS_TOL, rtol=0, err_msg=name)
            np.testing.assert_allclose(q[c * nb:(c + 1) * nb], g["out_quat"], atol=Q_TOL, rtol=0, err_msg=name)
        assert (st[:nb] & 1).any() and (st[:nb] & 2).any() and (st[:nb] & 4).any() and (st[:nb] & 8).any(), name
