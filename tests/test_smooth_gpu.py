"""GPU tier of the whole-track RTS smoother (gsf_ekf_smooth_ragged_dev / batch.ekf_smooth_ragged): the kernel against the reference's own
smoother on the 88 tracks of tests/golden/ekf_smooth_tracks.npz, against the NumPy restatement that tests/test_smooth_host.py pins to that
file, against properties that need no yardstick, against the pose and covariance kernels, and under dirty buffers, other batch orders,
NULL optional outputs and skipped runs.

Gates, the project's existing GPU gates for these quantities: positions 1e-6 m, variances 1e-10 relative, quaternions
1e-9.  Derived, not tuned: positions of UTM size carry 1e-9 m per rounding and a chunk's scans a few dozen of them; the variance scans
round at about 1e-14 over the stated noise range; the smallest real mistake -- a span off by one pose, A not squared, the g of the wrong
row, a lost carry between chunks -- moves a pose by more than 1e-3 m or a variance by more than 1e-3 relative.  Flags, span starts, status
words and everything called "the same" are compared exactly."""
import copy
import ctypes as C

import numpy as np
import pytest

import hygiene
from test_cov_gpu import AXES_DIFFER, file_batch, planted_cov_tracks, small_dirt, words
from test_smooth_host import (BAD_QUAT, GNSS_USED, IN_OUTAGE, RTS_APPLIED, SHARP_TURN, SMOOTHED, SPAN_START, restate, smooth_tracks, var_err)

pytestmark = pytest.mark.gpu

POS_TOL, VAR_TOL, QUAT_TOL = 1e-6, 1e-10, 1e-9
LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129]
UTM = np.array([4.5e5, 5.4e6, 110.0])


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def flat(tracks):
    """tracks [(ts, pos, quat, aligned, valid, ip, iq)] -> flat host arrays (ts, pos, quat, aligned, valid, offsets, init_pos, init_quat)"""
    offs = np.zeros(len(tracks) + 1, np.int64); offs[1:] = np.cumsum([len(t[0]) for t in tracks])
    cat = lambda k, shape: np.concatenate([np.asarray(t[k], np.float64).reshape(shape) for t in tracks]) if tracks else np.empty(shape).reshape(shape)
    return (cat(0, (-1,)), cat(1, (-1, 3)), cat(2, (-1, 4)), cat(3, (-1, 3)), np.concatenate([np.asarray(t[4]).astype(np.uint8) for t in tracks]), offs,
            np.array([t[5] for t in tracks], np.float64).reshape(-1, 3), np.array([t[6] for t in tracks], np.float64).reshape(-1, 4))


def run(B, arrays, cfg, **kw):
    import torch
    r = B.ekf_smooth_ragged(*[dev(x) for x in arrays], config=cfg, **kw)
    torch.cuda.synchronize()
    return r


def host(r):
    h = lambda t: None if t is None else t.cpu().numpy()
    return dict(pos=h(r.pos), quat=h(r.quat), cov=h(r.cov), pos_filt=h(r.pos_filt), cov_filt=h(r.cov_filt), flags=h(r.flags), status=h(r.status))


def full_cfg(part):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = copy.deepcopy(E.CONFIG)
    for sec, kv in part.items():
        cfg[sec].update(kv)
    return cfg


def quat_err(got, want):
    """largest component difference up to the common sign of a quaternion"""
    return float(np.minimum(np.abs(got - want).max(axis=1), np.abs(got + want).max(axis=1)).max(initial=0.0))


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_track(out, sl, w, what):
    """one track of a launch against its restatement: positions, variances, quaternion within the gates; flags and span starts exact"""
    ep = max(np.abs(out["pos"][sl] - w["xs"]).max(initial=0.0), np.abs(out["pos_filt"][sl] - w["xf"]).max(initial=0.0))
    ev = max(var_err(out["cov"][sl], w["Ps"]), var_err(out["cov_filt"][sl], w["Pf"]))
    eq = quat_err(out["quat"][sl], w["quat"])
    assert ep < POS_TOL and ev < VAR_TOL and eq < QUAT_TOL, (what, ep, ev, eq)
    np.testing.assert_array_equal(out["flags"][sl], w["flags"], err_msg=str(what))
    assert np.flatnonzero(out["flags"][sl] & SPAN_START).tolist() == w["starts"], what
    return ep, ev, eq


def check_structure(out, what):
    """what needs no yardstick: rows without SMOOTHED hold the filter's bytes; the smoothed variance never exceeds the filtered one and is
    strictly smaller on axes 0-2 of SMOOTHED rows whose gain towards the later fix is above zero -- the filtered variance is positive there
    (A = Pf / Pp > 0 exactly when Pf > 0)"""
    sm = (out["flags"] & SMOOTHED) != 0
    assert same(out["pos"][~sm], out["pos_filt"][~sm]) and same(out["cov"][~sm], out["cov_filt"][~sm]), what
    assert (out["cov"] <= out["cov_filt"]).all(), what
    live = out["cov_filt"][:, :3] > 0
    assert (out["cov"][:, :3][sm[:, None] & live] < out["cov_filt"][:, :3][sm[:, None] & live]).all(), what
    assert same(out["cov"][:, 3:], out["cov_filt"][:, 3:]), what         # the quaternion axes are never smoothed
    assert sm.any() and (~sm).any(), what


# ------------------------------------------------------------------------------------------------ (a) the reference's smoother
@pytest.fixture(scope="module")
def golden_runs(B, golden):
    """the 88 golden tracks as ragged batches in file order, one launch per config; their restatements, made once"""
    tracks, g = smooth_tracks(golden)
    runs = []
    for ci in sorted(set(int(c) for c in g["cfg_index"])):
        ids = [t for t in range(len(tracks)) if int(g["cfg_index"][t]) == ci]
        cfg = full_cfg(tracks[ids[0]][8])
        arrays = flat([tracks[t][1:8] for t in ids])
        runs.append((ids, arrays, cfg, host(run(B, arrays, cfg, want_filtered=True))))
    return tracks, g, runs, {t: restate(*tracks[t][1:]) for t in range(len(tracks))}


def test_golden_parity(golden_runs):
    tracks, g, runs, want = golden_runs
    off = g["offsets"]
    worst = {"pos": 0.0, "var": 0.0, "restated_pos": 0.0, "restated_var": 0.0, "quat": 0.0}
    poses = 0
    for ids, arrays, cfg, out in runs:
        offs = arrays[5]
        poses += int(offs[-1])
        for k, t in enumerate(ids):
            name = tracks[t][0]
            sl, gl = slice(offs[k], offs[k + 1]), slice(off[t], off[t + 1])
            ef, es = np.abs(out["pos_filt"][sl] - g["filt_pos"][gl]).max(), np.abs(out["pos"][sl] - g["smooth_pos"][gl]).max()
            ev = var_err(out["cov"][sl][:, :3], g["smooth_var"][gl])
            worst["pos"], worst["var"] = max(worst["pos"], ef, es), max(worst["var"], ev)
            assert ef < POS_TOL and es < POS_TOL and ev < VAR_TOL, (name, ef, es, ev)
            assert np.flatnonzero(out["flags"][sl] & SPAN_START).tolist() == [int(a) for b, a in g["span_starts"] if b == t], name
            ep, ev2, eq = check_track(out, sl, want[t], name)
            worst["restated_pos"], worst["restated_var"], worst["quat"] = max(worst["restated_pos"], ep), max(worst["restated_var"], ev2), max(worst["quat"], eq)
            assert out["status"][k] == want[t]["status"], (name, out["status"][k], want[t]["status"])
        check_structure(out, f"config of {tracks[ids[0]][0]}")
    assert poses == off[-1] and poses > 10000
    print("largest deviation from the reference: positions %.2e m, variances %.2e relative; from the restatement: positions %.2e m, "
          "variances %.2e relative, quaternions %.2e" % (worst["pos"], worst["var"], worst["restated_pos"], worst["restated_var"], worst["quat"]))


# ------------------------------------------------------------------------------------------------ (b) the smallest shapes that can go wrong
def with_init(t):
    """(ts, quat, aligned, valid, pos) of test_cov_gpu's planted tracks -> (ts, pos, quat, aligned, valid, init_pos, init_quat)"""
    ts, quat, aligned, valid, pos = t
    ip = aligned[0] if not np.isnan(aligned[0]).any() else pos[0] * 1.03 + UTM
    return ts, pos, quat, aligned, valid, ip, quat[0] / np.linalg.norm(quat[0])


@pytest.fixture(scope="module")
def planted(B):
    """16 planted tracks per length (an empty track for length 0), both configs: one launch and one set of restatements each, made once"""
    tracks = []
    for N in LENGTHS:
        if N == 0:
            tracks.append((np.empty(0), np.empty((0, 3)), np.empty((0, 4)), np.empty((0, 3)), np.empty(0, bool), np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])))
        else:
            tracks += [with_init(t) for t in planted_cov_tracks(N, 100 + N, with_pos=True)]
    cfgs = {"default": full_cfg({}), "axes-differ": full_cfg(AXES_DIFFER)}
    arrays = flat(tracks)
    out = {name: host(run(B, arrays, cfg, want_filtered=True)) for name, cfg in cfgs.items()}
    want = {name: [restate(*t, cfg) if len(t[0]) else None for t in tracks] for name, cfg in cfgs.items()}
    return tracks, arrays, cfgs, out, want


@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_planted_lengths_against_the_restatement(planted, config):
    tracks, arrays, cfgs, out, want = planted
    offs, o = arrays[5], out[config]
    worst = [0.0, 0.0, 0.0]
    seen = set()
    for k, (t, w) in enumerate(zip(tracks, want[config])):
        sl = slice(offs[k], offs[k + 1])
        if w is None:
            assert offs[k] == offs[k + 1] and o["status"][k] == 0       # an empty track: no rows, status 0
            continue
        for rate, thr in w["rates"]:
            assert not (0.9 * thr <= rate <= 1.1 * thr)                  # no planted decision hangs on an ulp
        what = (config, len(t[0]), k)
        worst = [max(a, b) for a, b in zip(worst, check_track(o, sl, w, what))]
        assert o["status"][k] == w["status"], (what, o["status"][k], w["status"])
        seen |= {int(v) for v in np.unique(o["flags"][sl])} | {("start-lane", s % 64) for s in w["starts"][1:]}
    check_structure(o, config)
    print(f"{config}: largest deviation from the restatement: positions {worst[0]:.2e} m, variances {worst[1]:.2e} relative, quaternions {worst[2]:.2e}")
    assert {SPAN_START | SMOOTHED, GNSS_USED | SMOOTHED, GNSS_USED | SPAN_START | SMOOTHED, IN_OUTAGE | SMOOTHED, IN_OUTAGE | SHARP_TURN, GNSS_USED,
            IN_OUTAGE} <= seen, seen


# ------------------------------------------------------------------------------------------------ (c) the pose and covariance kernels
def test_filter_is_the_pose_kernels(B, planted):
    """the quaternion is ekf_fuse_ragged's; the filtered position is ekf_fuse_ragged's wherever its per-outage RTS rewrote nothing (the rows
    the covariance entry does not flag SMOOTHED); the status words agree but for RTS_APPLIED, which means another thing here"""
    import torch
    tracks, arrays, cfgs, out, want = planted
    d = [dev(x) for x in arrays]
    po, qo, st = B.ekf_fuse_ragged(*d, config=cfgs["default"])
    cov = B.ekf_covariance_ragged(d[0], d[2], d[3], d[4], d[5], config=cfgs["default"])
    torch.cuda.synchronize()
    o = out["default"]
    assert np.abs(o["quat"] - qo.cpu().numpy()).max() < QUAT_TOL
    untouched = (cov.flags.cpu().numpy() & SMOOTHED) == 0
    assert untouched.sum() > 5000 and (~untouched).sum() > 100
    assert np.abs(o["pos_filt"][untouched] - po.cpu().numpy()[untouched]).max() < 1e-7
    np.testing.assert_array_equal(o["status"] & ~RTS_APPLIED, st.cpu().numpy() & ~RTS_APPLIED)
    assert (o["status"] & BAD_QUAT == 0).all()
    np.testing.assert_array_equal(o["flags"] & (GNSS_USED | IN_OUTAGE | SHARP_TURN), cov.flags.cpu().numpy() & (GNSS_USED | IN_OUTAGE | SHARP_TURN))
    assert var_err(o["cov_filt"], cov.filtered.cpu().numpy()) < 1e-14    # the same variance_chunk(), the same sum of dt


# ------------------------------------------------------------------------------------------------ (d) the same bytes
def test_a_track_alone_in_the_batch_and_in_reversed_order(B, planted):
    tracks, arrays, cfgs, out, want = planted
    offs, o = arrays[5], out["default"]
    rev = list(range(len(tracks)))[::-1]
    r = host(run(B, flat([tracks[k] for k in rev]), cfgs["default"], want_filtered=True))
    roffs = np.zeros(len(tracks) + 1, np.int64); roffs[1:] = np.cumsum([len(tracks[k][0]) for k in rev])
    for j, k in enumerate(rev):
        a, b = slice(offs[k], offs[k + 1]), slice(roffs[j], roffs[j + 1])
        for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags"):
            assert same(o[name][a], r[name][b]), (name, k)
        assert o["status"][k] == r["status"][j]
    for k in (1, 20, 40, 70, 100, len(tracks) - 1):                     # lengths 1, 2, 63, 65, 129, 129
        alone = host(run(B, flat([tracks[k]]), cfgs["default"], want_filtered=True))
        a = slice(offs[k], offs[k + 1])
        for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags"):
            assert same(o[name][a], alone[name]), (name, k)
        assert o["status"][k] == alone["status"][0]


def test_optional_outputs_null_or_present(B, planted):
    import torch
    from gps_optimize_slam_amd import _lib
    tracks, arrays, cfgs, out, want = planted
    o = out["default"]
    bare = host(run(B, arrays, cfgs["default"]))                        # pos_filt, cov_filt = NULL
    assert bare["pos_filt"] is None and bare["cov_filt"] is None
    for name in ("pos", "quat", "cov", "flags", "status"):
        assert same(o[name], bare[name]), name
    d = [dev(x) for x in arrays]
    P, nb = int(arrays[5][-1]), len(tracks)
    c = _lib.EkfConfig.from_config(cfgs["default"])
    f = dict(dtype=torch.float64, device="cuda")
    pos, quat, cov = torch.full((P, 3), float("nan"), **f), torch.full((P, 4), float("nan"), **f), torch.full((P, 7), float("nan"), **f)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_ekf_smooth_ragged_dev(B.context().handle, *[p(x) for x in d], None, C.byref(c), nb, p(pos), p(quat), p(cov),
                                                     None, None, None, None))       # every optional output NULL
    torch.cuda.synchronize()
    assert same(pos.cpu().numpy(), o["pos"]) and same(quat.cpu().numpy(), o["quat"]) and same(cov.cpu().numpy(), o["cov"])


def test_outputs_do_not_depend_on_stale_buffers(B, monkeypatch, planted):
    """outputs prefilled with two byte patterns, workspaces poisoned and not: the same bytes -- every row of every non-empty track is written,
    and what the forward pass parks in cov_out leaves nothing behind"""
    tracks, arrays, cfgs, out, want = planted
    d = [dev(x) for x in arrays]
    res = hygiene.same_bytes_under_dirt(monkeypatch, B.context(), lambda: B.ekf_smooth_ragged(*d, config=cfgs["default"], want_filtered=True),
                                        small_dirt(B), rows_of=arrays[5])
    o = out["default"]
    assert same(res.cov.cpu().numpy(), o["cov"]) and same(res.pos.cpu().numpy(), o["pos"])
    assert np.isfinite(o["cov"]).all() and (o["cov"] >= 0).all() and not np.signbit(o["cov"]).any()      # no tag bit survives


# ------------------------------------------------------------------------------------------------ (e) skipped runs
def test_skipped_runs_get_nan_rows_and_their_inputs_are_not_read(B, planted):
    tracks, arrays, cfgs, out, want = planted
    offs, o = arrays[5], out["default"]
    nb = len(tracks)
    rs = np.zeros(nb, np.int32)
    skipped = [3, 40, 41, nb - 1]
    rs[skipped] = [8, 1, 256, 4]
    poisoned = [x.copy() for x in arrays]
    rows = np.zeros(int(offs[-1]), bool)
    for k in skipped:
        rows[offs[k]:offs[k + 1]] = True
        poisoned[6][k], poisoned[7][k] = np.nan, np.nan
    for j in (0, 1, 2, 3):
        poisoned[j][rows] = np.nan
    poisoned[4][rows] = 1
    r = host(run(B, poisoned, cfgs["default"], run_status=dev(rs), want_filtered=True))
    for name in ("pos", "quat", "cov", "pos_filt", "cov_filt"):
        assert np.isnan(r[name][rows]).all() and same(r[name][~rows], o[name][~rows]), name
    assert (r["flags"][rows] == 0).all() and same(r["flags"][~rows], o["flags"][~rows])
    assert (r["status"][skipped] == 0).all() and (np.delete(r["status"], skipped) == np.delete(o["status"], skipped)).all()


# ------------------------------------------------------------------------------------------------ (f) on a whole run
def test_smooth_fused_on_a_run(B, golden, tmp_path):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    rb = file_batch(B, golden, tmp_path)
    r = B.run_fusion_ragged(rb, B.mt19937_seed([3, 4, 5, 6]), E.CONFIG)
    st = B.smooth_fused(rb, r)
    g = B.gate_fused(rb, r, [float("inf")])                             # a gate that rejects nothing
    gated = B.smooth_fused(rb, r, valid=g.valid(0))
    torch.cuda.synchronize()
    for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags", "status", "err_stats2", "errors2"):
        assert torch.equal(words(getattr(st, name)), words(getattr(gated, name))), name
    rs, so = r.run_status.cpu().numpy(), rb.slam_offsets.cpu().numpy()
    stats = st.err_stats2.cpu().numpy()
    assert stats.shape == (2, 4, 4) and st.errors2.shape == (2, int(so[-1]))
    pos, flags = st.pos.cpu().numpy(), st.flags.cpu().numpy()
    for b in range(4):
        sl = slice(so[b], so[b + 1])
        if rs[b] != 0:
            assert np.isnan(pos[sl]).all() and (flags[sl] == 0).all() and int(st.status[b]) == 0
            continue
        assert np.isfinite(pos[sl]).all() and (flags[sl] & SMOOTHED).any()
        # step 6 of the fused track as the run itself reports it, and a finite RMSE of the smoothed one over the same fixes
        np.testing.assert_allclose(stats[0, b], r.err_stats[0, 2, b].cpu().numpy(), rtol=1e-9)
        assert stats[1, b, 0] == stats[0, b, 0] > 0 and np.isfinite(stats[1, b]).all() and stats[1, b, 3] > 0
    assert torch.equal(words(st.correction()), words(st.pos - st.pos_filt))


# ------------------------------------------------------------------------------------------------ (g) the single-track entries
def test_single_track_entries(B, golden, golden_runs):
    """ekfgpsslam.ekf_smooth_aligned equals the batch entry's rows; smooth_trajectory makes apply_ekf_correction's alignment call first"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    tracks, g, runs, want = golden_runs
    ids, arrays, cfg, out = runs[0]
    k = [tracks[t][0] for t in ids].index("gentle_across_two_boundaries")
    t = tracks[ids[k]]
    one = E.ekf_smooth_aligned(*t[1:8], cfg)
    sl = slice(arrays[5][k], arrays[5][k + 1])
    for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags"):
        assert same(one[name], out[name][sl]), name
    assert one["status"] == out["status"][k]
    kb = golden("kat_bundled.npz")                                      # the bundled drive: fixes at the SLAM stamps, all valid
    slam = {"timestamps": kb["ts"], "positions": kb["pos"], "quaternions": kb["quat"]}
    s = E.smooth_trajectory(slam, {"timestamps": kb["ts"], "positions": kb["gt"]}, kb["kat2_pos"], kb["kat2_quat"], E.CONFIG)
    direct = E.ekf_smooth_aligned(kb["ts"], kb["pos"], kb["quat"], kb["kat3_aligned"], kb["kat3_valid"], kb["kat2_pos"][0], kb["kat2_quat"][0], E.CONFIG)
    assert np.abs(s["pos"] - direct["pos"]).max() < POS_TOL and (s["flags"] == direct["flags"]).all() and s["status"] == direct["status"]
    n = len(kb["ts"])
    assert s["pos"].shape == (n, 3) and (s["flags"][:-1] & SMOOTHED).all() and not s["flags"][-1] & SMOOTHED
    assert (s["cov"][:-1, :3] < s["cov_filt"][:-1, :3]).all() and np.abs(s["pos"] - s["pos_filt"]).max() > 1e-3
