"""GPU tier of the pose-query entries (gsf_pose_query[_dev] / gsf_georef_points[_dev], batch.query_poses_ragged / georef_points_ragged /
query_fused / georef_fused, ekfgpsslam.interpolate_trajectory) against the long-double yardstick (tests/pose_query_ref.py) on the batch of
pose_query_ref.build_cases: the smallest shapes at which the kernel can go wrong (wave = 64 queries, window = 64 poses, block = 256).
Flags, indices, pose flags and track states are exact, NaN patterns identical, values inside bounds computed from the inputs; the two routes
of the kernel, the host and the device entry, and clean and dirty workspaces give the same bits."""
import ctypes as C

import numpy as np
import pytest

import pose_query_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def cases():
    c = ref.build_cases()
    want_q = ref.query(c["ts"], c["pos"], c["quat"], c["offsets"], c["q_t"], c["q_offsets"], c["pose_flags"], c["run_status"], ref.MAX_GAP)
    want_g = ref.georef(c["ts"], c["pos"], c["quat"], c["offsets"], c["q_t"], c["x"], c["q_offsets"], c["ext_q"], c["ext_t"], c["scale"],
                        c["pose_flags"], c["run_status"], ref.MAX_GAP)
    return c, want_q, want_g


KEYS = ("ts", "pos", "quat", "offsets", "q_t", "q_offsets", "pose_flags", "run_status", "ext_q", "ext_t", "scale", "x")


def _dev(c):
    import torch
    return {k: torch.as_tensor(c[k]).cuda() for k in KEYS}


def _poses(B, d, q_t=None):
    return B.query_poses_ragged(d["ts"], d["pos"], d["quat"], d["offsets"], d["q_t"] if q_t is None else q_t, d["q_offsets"], pose_flags=d["pose_flags"],
                                run_status=d["run_status"], max_gap=ref.MAX_GAP)


def _points(B, d, q_t=None, x=None, ext=True, **kw):
    e = dict(ext_q=d["ext_q"], ext_t=d["ext_t"], scale=d["scale"]) if ext else {}
    return B.georef_points_ragged(d["ts"], d["pos"], d["quat"], d["offsets"], d["q_t"] if q_t is None else q_t, d["x"] if x is None else x, d["q_offsets"],
                                  pose_flags=d["pose_flags"], run_status=d["run_status"], max_gap=ref.MAX_GAP, **e, **kw)


def _host(r, names):
    return {k: getattr(r, k).cpu().numpy() for k in names}


POSE_OUT = ("pos", "quat", "flags", "index", "pose_flags", "track_state")
POINT_OUT = ("xyz", "flags", "index", "pose_flags", "track_state")


def _same_bits(a, b, names, what):
    for k in names:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _exact_fields(got, want):
    for k in ("flags", "index", "pose_flags", "track_state"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- 1. against the yardstick
def test_poses_against_the_yardstick(B, cases):
    """max |pos - yardstick| / bound and max |quat - yardstick| are printed before they are asserted (the figures DESIGN 7e records)"""
    c, want, _ = cases
    got = _host(_poses(B, _dev(c)), POSE_OUT)
    _exact_fields(got, want)
    assert ref.same_nan_pattern(got["pos"], want["pos"]) and ref.same_nan_pattern(got["quat"], want["quat"])
    gi, gj = ref.bracket_rows(c["offsets"], c["q_offsets"], want["index"], want["flags"])
    exc_p, worst_p = ref.max_excess(got["pos"], want["pos"], ref.pos_bound(c["pos"], gi, gj))
    exc_q, worst_q = ref.max_excess(got["quat"], want["quat"], ref.QUAT_BOUND)
    print(f"pose query: max |pos - yardstick| = {worst_p:.3e} m (excess over the bound {exc_p:.3e}), max |quat - yardstick| = {worst_q:.3e} "
          f"= {worst_q / ref.EPS:.2f} x 2^-52 (bound 10)")
    assert exc_p <= 0 and exc_q <= 0
    ex = (want["flags"] & ref.Q_EXACT) != 0                             # an exact hit: the stored pose bit for bit, NaN position included
    assert ex.sum() > 20
    assert got["pos"][ex].tobytes() == c["pos"][gi[ex]].tobytes() and got["quat"][ex].tobytes() == c["quat"][gi[ex]].tobytes()


def test_points_against_the_yardstick(B, cases):
    c, _, want = cases
    got = _host(_points(B, _dev(c)), POINT_OUT)
    _exact_fields(got, want)
    assert ref.same_nan_pattern(got["xyz"], want["xyz"])
    gi, gj = ref.bracket_rows(c["offsets"], c["q_offsets"], want["index"], want["flags"])
    tb = np.repeat(np.arange(c["B"]), np.diff(c["q_offsets"]))
    exc, worst = ref.max_excess(got["xyz"], want["xyz"], ref.point_bound(c["pos"], gi, gj, c["x"], c["scale"][tb], c["ext_t"][tb]))
    bound = ref.point_bound(c["pos"], gi, gj, c["x"], c["scale"][tb], c["ext_t"][tb])
    fin = np.isfinite(got["xyz"])
    used = float(np.max(np.asarray(np.abs(got["xyz"].astype(ref.LD) - want["xyz"]), float)[fin] / bound[fin]))
    print(f"georef: max |xyz - yardstick| = {worst:.3e} m (excess over the bound {exc:.3e}; at most {used:.2f} of the bound is used)")
    assert exc <= 0
    assert np.isfinite(got["xyz"]).sum() > 2000


# ---------------------------------------------------------------------------------------------------------------- 2. the same bits
def test_shuffled_queries_give_the_sorted_run_bit_for_bit(B, cases):
    """Shuffled inside each track, a wave's queries span the whole track: the general route.  Time-sorted they take the window route wherever a
    wave lies inside one track.  Un-shuffled, every output must be the sorted run's."""
    import torch
    c, _, _ = cases
    d = _dev(c)
    rng = np.random.default_rng(5)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(c["q_offsets"][:-1], c["q_offsets"][1:])])
    inv = np.argsort(perm)
    qs, xs = torch.as_tensor(c["q_t"][perm]).cuda(), torch.as_tensor(np.ascontiguousarray(c["x"][perm])).cuda()
    a, b = _host(_poses(B, d), POSE_OUT), _host(_poses(B, d, q_t=qs), POSE_OUT)
    for k in POSE_OUT[:-1]:
        b[k] = np.ascontiguousarray(b[k][inv])
    _same_bits(a, b, POSE_OUT, "poses")
    a, b = _host(_points(B, d), POINT_OUT), _host(_points(B, d, q_t=qs, x=xs), POINT_OUT)
    for k in POINT_OUT[:-1]:
        b[k] = np.ascontiguousarray(b[k][inv])
    _same_bits(a, b, POINT_OUT, "points")


def test_host_entries_and_dirty_workspaces(B, cases):
    """gsf_pose_query / gsf_georef_points (host arrays) return the device entries' bytes; with every workspace of the context filled with
    another word (the staging arena of the host entries is one) nothing changes; optional outputs may be NULL"""
    from gps_optimize_slam_amd import _lib
    c, _, _ = cases
    d = _dev(c)
    dev_q, dev_g = _host(_poses(B, d), POSE_OUT), _host(_points(B, d), POINT_OUT)
    L, ctx, hp, M, nb = _lib.load(), B.context(), _lib.hptr, c["M"], c["B"]

    def host_route(optional=True):
        q = dict(pos=np.full((M, 3), 3.0), quat=np.full((M, 4), 3.0), flags=np.full(M, 9, np.uint8), index=np.full(M, 9, np.int32),
                 pose_flags=np.full(M, 9, np.uint8), track_state=np.full(nb, 9, np.int32))
        g = dict(xyz=np.full((M, 3), 3.0), flags=np.full(M, 9, np.uint8), index=np.full(M, 9, np.int32), pose_flags=np.full(M, 9, np.uint8),
                 track_state=np.full(nb, 9, np.int32))
        head = [hp(c["ts"]), hp(c["pos"]), hp(c["quat"]), hp(c["offsets"]), hp(c["run_status"]), hp(c["pose_flags"]), nb, hp(c["q_t"]), hp(c["q_offsets"]), M,
                ref.MAX_GAP]
        opt = lambda o: (hp(o["index"]), hp(o["pose_flags"])) if optional else (None, None)
        _lib.check(L.gsf_pose_query(ctx.handle, *head, hp(q["pos"]), hp(q["quat"]), hp(q["flags"]), *opt(q), hp(q["track_state"])))
        _lib.check(L.gsf_georef_points(ctx.handle, *head, hp(c["x"]), hp(c["ext_q"]), hp(c["ext_t"]), hp(c["scale"]), hp(g["xyz"]), hp(g["flags"]), *opt(g),
                                       hp(g["track_state"])))
        return q, g

    q, g = host_route()
    _same_bits(dev_q, q, POSE_OUT, "host poses"); _same_bits(dev_g, g, POINT_OUT, "host points")
    q, g = host_route(optional=False)
    _same_bits(dev_q, q, ("pos", "quat", "flags", "track_state"), "host poses, no optional outputs")
    _same_bits(dev_g, g, ("xyz", "flags", "track_state"), "host points, no optional outputs")
    assert (q["index"] == 9).all() and (g["pose_flags"] == 9).all()
    try:
        for word in (0xA5, 0x00):
            ctx.set_option("poison_workspaces", word)
            q, g = host_route()
            _same_bits(dev_q, q, POSE_OUT, word); _same_bits(dev_g, g, POINT_OUT, word)
            _same_bits(dev_q, _host(_poses(B, d), POSE_OUT), POSE_OUT, word); _same_bits(dev_g, _host(_points(B, d), POINT_OUT), POINT_OUT, word)
    finally:
        ctx.set_option("poison_workspaces", -1)
    # B == 0 and M == 0 are no-ops
    _lib.check(L.gsf_pose_query(ctx.handle, *([None] * 6), 0, None, None, 5, 0.0, *([None] * 6)))
    _lib.check(L.gsf_georef_points_dev(ctx.handle, *([None] * 6), 3, None, None, 0, 0.0, *([None] * 9)))


def test_points_at_the_sensor_origin_are_the_positions(B, cases):
    """NULL extrinsics and x = 0: out_xyz is out_pos of the pose entry bit for bit (where the pose's quaternion can be normalised)"""
    import torch
    c, _, _ = cases
    d = _dev(c)
    p = _host(_poses(B, d), POSE_OUT)
    g = _host(_points(B, d, x=torch.zeros_like(d["x"]), ext=False), POINT_OUT)
    ok = (g["flags"] & ref.Q_BAD_QUAT) == 0
    assert ok.sum() > c["M"] - 10 and g["xyz"][ok].tobytes() == p["pos"][ok].tobytes()
    np.testing.assert_array_equal(g["flags"][ok], p["flags"][ok])
    np.testing.assert_array_equal(g["index"], p["index"])
    assert np.isnan(g["xyz"][~ok]).all()
    np.testing.assert_array_equal(g["track_state"], p["track_state"])   # without ext_q there is no dead extrinsic


def test_wgs84_rows_are_the_existing_inverse(B, cases):
    import torch
    c, _, _ = cases
    d = _dev(c)
    zone = torch.full((c["B"],), 37, dtype=torch.int32).cuda()
    south = torch.ones((c["B"],), dtype=torch.int32).cuda()
    r = _points(B, d, zone=zone, south=south)
    want = B.utm_to_wgs84_ragged(r.xyz, d["q_offsets"], zone, south, d["run_status"])
    assert r.lonlatalt.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    ok = torch.isfinite(r.xyz).all(dim=1)
    assert torch.isfinite(r.lonlatalt[ok]).all() and int(ok.sum()) > 500
    assert _points(B, d).lonlatalt is None


# ---------------------------------------------------------------------------------------------------------------- 3. on a fused run
def test_query_fused_on_a_ragged_run(B, golden):
    """three tracks of different lengths, one of them failed: queries at the SLAM stamps return the fused poses bit for bit with GSF_Q_EXACT,
    the failed track's queries get GSF_Q_TRACK; the run's pose flags come through; wgs84=True needs a projector"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    from gps_optimize_slam_amd import _lib
    from test_sim3_rows import case_cfg, cases as row_cases
    g, _ = row_cases(golden)
    members = [("all_valid", 300), ("longer_than_180s", 2000), ("too_few_valid", 250)]
    cfg = case_cfg(E.CONFIG, g["all_valid_par"])
    cfg["gps_filtering_ransac"] = dict(cfg["gps_filtering_ransac"], enabled=False)
    tracks = [(g[f"{n}_ts"][:k], g[f"{n}_pos"][:k], g[f"{n}_quat"][:k]) for n, k in members]
    logs = [np.column_stack((g[f"{n}_gps_t"], g[f"{n}_gps_p"])) for n, _ in members]
    rb = B.RaggedGeodeticBatch.from_host(tracks, logs)
    r = B.run_fusion_ragged(rb, B.mt19937_seed([int(g[f"{n}_seed"]) for n, _ in members]), cfg, projected=True, want_cov=True)
    rs = r.run_status.cpu().numpy()
    assert rs[0] == 0 and rs[1] == 0 and rs[2] != 0
    q = B.query_fused(rb, r, rb.ts, rb.slam_offsets)
    so = rb.slam_offsets.cpu().numpy()
    fl, idx = q.flags.cpu().numpy(), q.index.cpu().numpy()
    ok = slice(0, so[2])
    ts = rb.ts.cpu().numpy()
    last_of_equal = np.r_[ts[1:] != ts[:-1], True]                      # (a repeated stamp answers with its last pose)
    sel = np.flatnonzero(last_of_equal[ok])
    assert len(sel) > 2000 and (fl[ok] == _lib.Q_EXACT).all()
    assert q.pos.cpu().numpy()[sel].tobytes() == r.fused.pos.cpu().numpy()[sel].tobytes()
    assert q.quat.cpu().numpy()[sel].tobytes() == r.fused.quat.cpu().numpy()[sel].tobytes()
    np.testing.assert_array_equal(idx[sel], np.r_[np.arange(so[1]), np.arange(so[2] - so[1])][sel])
    np.testing.assert_array_equal(q.pose_flags.cpu().numpy()[sel], r.cov.flags.cpu().numpy()[sel])
    assert (fl[so[2]:] == _lib.Q_TRACK).all() and torch.isnan(q.pos[so[2]:]).all() and (idx[so[2]:] == -1).all()
    np.testing.assert_array_equal(q.track_state.cpu().numpy(), [0, 0, _lib.QT_SKIPPED])
    # midpoints of the first track, as points at the sensor origin: the positions of the pose query
    mid = torch.as_tensor(0.5 * (ts[:so[1] - 1] + ts[1:so[1]])).cuda()
    qoff = torch.tensor([0, mid.numel(), mid.numel(), mid.numel()]).cuda()
    pq = B.query_fused(rb, r, mid, qoff)
    gq = B.georef_fused(rb, r, mid, torch.zeros((mid.numel(), 3), dtype=torch.float64).cuda(), qoff)
    assert gq.lonlatalt is None and gq.xyz.cpu().numpy().tobytes() == pq.pos.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="projected"):
        B.georef_fused(rb, r, mid, torch.zeros((mid.numel(), 3), dtype=torch.float64).cuda(), qoff, wgs84=True)


def test_interpolate_trajectory_on_the_bundled_track(B, golden):
    """the single-track form on the 271-pose fixture: its own stamps give the track back, midpoints the yardstick"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    k = golden("kat_bundled.npz")
    ts, pos, quat = k["ts"], k["kat4_pos"], k["kat4_quat"]
    assert len(ts) == 271 and (np.diff(ts) > 0).all()
    p, q, fl = E.interpolate_trajectory(ts, pos, quat, ts)
    assert (fl == ref.Q_EXACT).all() and p.tobytes() == np.ascontiguousarray(pos).tobytes() and q.tobytes() == np.ascontiguousarray(quat).tobytes()
    mid = 0.5 * (ts[:-1] + ts[1:])
    p, q, fl = E.interpolate_trajectory(ts, pos, quat, mid)
    off, qoff = np.array([0, 271]), np.array([0, 270])
    want = ref.query(ts, pos, quat, off, mid, qoff)
    np.testing.assert_array_equal(fl, want["flags"])
    assert (fl == 0).all()
    gi, gj = ref.bracket_rows(off, qoff, want["index"], want["flags"])
    assert ref.max_excess(p, want["pos"], ref.pos_bound(pos, gi, gj))[0] <= 0 and ref.max_excess(q, want["quat"], ref.QUAT_BOUND)[0] <= 0
    x = np.random.default_rng(2).normal(size=(270, 3)) * 30.0
    xyz, fl = E.georeference_points(ts, pos, quat, mid, x, ext_quat=[0.1, -0.2, 0.3, 0.9], ext_trans=[0.5, -0.25, 1.5], scale=1.25)
    wg = ref.georef(ts, pos, quat, off, mid, x, qoff, np.array([[0.1, -0.2, 0.3, 0.9]]), np.array([[0.5, -0.25, 1.5]]), np.array([1.25]))
    np.testing.assert_array_equal(fl, wg["flags"])
    bound = ref.point_bound(pos, gi, gj, x, np.full(270, 1.25), np.tile([0.5, -0.25, 1.5], (270, 1)))
    assert ref.max_excess(xyz, wg["xyz"], bound)[0] <= 0
    with pytest.raises(ValueError):
        E.georeference_points(ts, pos, quat, mid, x, ext_quat=[0.0, 0.0, 0.0, 0.0])
