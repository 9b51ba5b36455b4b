"""GPU tier of per-fix GNSS noise (gsf_ekf_smooth_weighted_dev / batch.ekf_smooth_weighted_ragged, gsf_fix_var_at_poses_dev /
batch.fix_var_at_poses_ragged): the kernel against the unweighted smoother where the variances are the config's, against the per-pose
restatement of tests/weighted_ref.py at the chunk edges, against the 50-digit yardstick at both ends of the stated range, and the rules
that need no yardstick -- a bad variance is a missing fix, what is not read is not read, a track's bytes do not depend on its neighbours,
on stale buffers, on the stream or on which optional outputs are asked for.

Gates: those of tests/test_smooth_gpu.py and their derivation -- positions 1e-6 m, variances and nis 1e-10 relative, quaternions 1e-9;
kernel against kernel 1e-7 m and 1e-14 relative (test_filter_is_the_pose_kernels).  tests/test_weighted_host.py measured what the
restatement itself loses against the yardstick at the ends of the range (positions 1.9e-9 m, variances 2.6e-15, nis 4.9e-13): nothing that
asks for a wider gate.  On the one track whose steps alternate between 1e14 s and repeated stamps the smoothed variance is held to the
bound in u and Pf derived there (weighted_ref.ps_within_bound); that track returns NaN if the kernel's scan loses either rescale.  Flags, span starts, status words and everything called "the same" are compared exactly."""
import copy
import ctypes as C

import numpy as np
import pytest

import hygiene
import weighted_ref as W
from test_cov_gpu import AXES_DIFFER, file_batch, planted_cov_tracks, small_dirt, words
from test_smooth_gpu import check_structure, check_track, dev, flat, full_cfg, host, quat_err, same, with_init
from test_smooth_host import GNSS_USED, IN_OUTAGE, SHARP_TURN, SMOOTHED, SPAN_START, var_err
from test_weighted_host import rmse, yard_errors

pytestmark = pytest.mark.gpu

POS_TOL, VAR_TOL, QUAT_TOL = 1e-6, 1e-10, 1e-9
LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129]
BAD_SIGMA = W.BAD_SIGMA
NAMES = ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags", "nis")


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def runw(B, arrays, mv, cfg, **kw):
    """one launch of the weighted entry on host arrays (flat()'s order) -> host dict with nis"""
    import torch
    kw.setdefault("want_filtered", True); kw.setdefault("want_nis", True)
    d = [dev(x) for x in arrays]
    r = B.ekf_smooth_weighted_ragged(*d[:5], dev(mv), *d[5:], config=cfg, **kw)
    torch.cuda.synchronize()
    o = host(r)
    o["nis"] = None if r.nis is None else r.nis.cpu().numpy()
    return o


def empty_track():
    return (np.empty(0), np.empty((0, 3)), np.empty((0, 4)), np.empty((0, 3)), np.empty(0, bool), np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]))


def base_rows(arrays):
    """the rows that would take an update but for their variances: not a track's first row, mask set, fix free of NaN"""
    ts, pos, quat, aligned, valid, offs = arrays[:6]
    base = (valid != 0) & ~np.isnan(aligned).any(1)
    base[offs[:-1][offs[:-1] < len(base)]] = False
    return base


@pytest.fixture(scope="module")
def planted(B):
    """16 planted tracks per length (one empty track for length 0) with per-row variances drawn per track from the five kinds, and bad
    variances planted on two kinds of track: in the middle of a run of fixes, and next to an outage.  Both configs: one launch and one set
    of restatements each, made once."""
    tracks, mvs = [], []
    for N in LENGTHS:
        if N == 0:
            tracks.append(empty_track()); mvs.append(np.empty((0, 3)))
            continue
        for kind, t in enumerate(planted_cov_tracks(N, 100 + N, with_pos=True)):
            t = with_init(t)
            rng = np.random.default_rng(9000 + 100 * N + kind)
            mv = W.variances(W.VAR_KINDS[(kind + N) % len(W.VAR_KINDS)], N, full_cfg({})["ekf"]["meas_noise_diag"], rng)
            if N >= 63 and kind == 0:
                mv[N // 2, 1] = np.nan                                  # a bad variance between two used fixes
                mv[N // 4] = np.inf                                     # "no information": no fix, no bit
            if N >= 63 and kind == 8:
                mv[N // 2 + 1] = 0.0                                    # ... and one that lengthens an outage
            tracks.append(t); mvs.append(mv)
    cfgs = {"default": full_cfg({}), "axes-differ": full_cfg(AXES_DIFFER)}
    arrays, mv = flat(tracks), np.concatenate(mvs)
    out = {name: runw(B, arrays, mv, cfg) for name, cfg in cfgs.items()}
    want = {name: [W.weighted_restate(*t[:5], m, *t[5:], cfg) if len(t[0]) else None for t, m in zip(tracks, mvs)] for name, cfg in cfgs.items()}
    return tracks, mvs, arrays, mv, cfgs, out, want


# ------------------------------------------------------------------------------------------------ 1. constant variances: the unweighted smoother
def test_constant_variances_are_the_unweighted_smoother(B, planted):
    import torch
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    for name, cfg in cfgs.items():
        const = np.tile(np.array(cfg["ekf"]["meas_noise_diag"], float), (len(mv), 1))
        o = runw(B, arrays, const, cfg)
        r = B.ekf_smooth_ragged(*[dev(x) for x in arrays], config=cfg, want_filtered=True)
        torch.cuda.synchronize()
        u = host(r)
        np.testing.assert_array_equal(o["flags"], u["flags"])
        np.testing.assert_array_equal(o["status"], u["status"])
        assert (o["flags"] & BAD_SIGMA == 0).all()
        ep = max(np.abs(o["pos"] - u["pos"]).max(), np.abs(o["pos_filt"] - u["pos_filt"]).max())
        ev = max(var_err(o["cov"], u["cov"]), var_err(o["cov_filt"], u["cov_filt"]))
        eq = quat_err(o["quat"], u["quat"])
        print(f"{name}: weighted entry with the config's R against ekf_smooth_ragged: positions {ep:.2e} m, variances {ev:.2e} relative, quaternions {eq:.2e}; "
              f"bytes equal: " + ", ".join(f"{k} {same(o[k], u[k])}" for k in ("pos", "quat", "cov", "pos_filt", "cov_filt")))
        assert ep < 1e-7 and ev < 1e-14 and eq < QUAT_TOL, (name, ep, ev, eq)


# ------------------------------------------------------------------------------------------------ 2. the chunk edges against the restatement
def nis_err(got, want):
    used = ~np.isnan(want)
    assert (np.isnan(got) == ~used).all()
    return float(np.max(np.abs(got[used] - want[used]) / want[used], initial=0.0))


@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_planted_lengths_against_the_restatement(planted, config):
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    offs, o = arrays[5], out[config]
    worst = [0.0, 0.0, 0.0, 0.0]
    seen, bad_alone, bad_beside = set(), 0, 0
    for k, (t, w) in enumerate(zip(tracks, want[config])):
        sl = slice(offs[k], offs[k + 1])
        if w is None:
            assert offs[k] == offs[k + 1] and o["status"][k] == 0       # an empty track: no rows, status 0
            continue
        for rate, thr in w["rates"]:
            assert not (0.9 * thr <= rate <= 1.1 * thr)                  # no planted decision hangs on an ulp
        what = (config, len(t[0]), k)
        en = nis_err(o["nis"][sl], w["nis"])
        assert en < VAR_TOL, (what, en)
        worst = [max(a, b) for a, b in zip(worst, check_track(o, sl, w, what) + (en,))]
        assert o["status"][k] == w["status"], (what, o["status"][k], w["status"])
        f = o["flags"][sl]
        seen |= {int(v) for v in np.unique(f)}
        np.testing.assert_array_equal((f & BAD_SIGMA) != 0, w["bad"])
        for i in np.flatnonzero(w["bad"]):
            nb = [int(f[j]) for j in (i - 1, i + 1) if 0 <= j < len(f)]
            beside = any((v & IN_OUTAGE) and not (v & BAD_SIGMA) for v in nb)
            bad_beside += beside; bad_alone += not beside
            assert f[i] & IN_OUTAGE and not f[i] & GNSS_USED
    check_structure(o, config)
    print(f"{config}: largest deviation from the restatement: positions {worst[0]:.2e} m, variances {worst[1]:.2e} relative, quaternions {worst[2]:.2e}, "
          f"nis {worst[3]:.2e} relative")
    strip = {v & ~(SPAN_START | BAD_SIGMA) for v in seen}
    assert {GNSS_USED | SMOOTHED, IN_OUTAGE | SMOOTHED, IN_OUTAGE | SHARP_TURN} <= strip, seen
    assert any(v & BAD_SIGMA for v in seen) and bad_alone > 0 and bad_beside > 0, (seen, bad_alone, bad_beside)


# ------------------------------------------------------------------------------------------------ 3. the range's ends
@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_both_ends_of_the_range_against_the_yardstick(B, config):
    cfg = full_cfg({} if config == "default" else AXES_DIFFER)
    yt = W.yardstick_tracks() + [W.long_short_track()]                  # ... and the track whose scans overflow without the rescales
    tracks, mvs = [t[1:8] for t in yt], [t[8] for t in yt]
    arrays = flat(tracks)
    o = runw(B, arrays, np.concatenate(mvs), cfg)
    offs = arrays[5]
    worst = [0.0, 0.0, 0.0]
    for k, (t, m) in enumerate(zip(tracks, mvs)):
        sl = slice(offs[k], offs[k + 1])
        w = W.weighted_restate(*t[:5], m, *t[5:], cfg)
        y = W.yardstick(w, t[3], m, t[5], cfg)
        got = dict(xf=o["pos_filt"][sl], xs=o["pos"][sl], Pf=o["cov_filt"][sl], Ps=o["cov"][sl], nis=o["nis"][sl])
        if yt[k][0] == "long_short_steps":                              # Ps = Pf + d cancels to 1e-15 of Pf there: the bound of weighted_ref.ps_within_bound
            ok, c_ps, ratio = W.ps_within_bound(got["Ps"][:, :3], y, VAR_TOL)
            print(f"{config}: long and short steps on the device: Ps: largest Pf / Ps {ratio:.2e}, worst |dPs| / (u Pf) {c_ps:.2f} (gate {8 * W.PS_C:.1f})")
            assert np.isfinite(got["Pf"]).all() and ok, (yt[k][0], c_ps)
            e = yard_errors(dict(got, Ps=np.column_stack((y["Ps"], got["Ps"][:, 3:]))), y)
        else:
            e = yard_errors(got, y)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] < POS_TOL and e[1] < VAR_TOL and e[2] < VAR_TOL, (yt[k][0], e)
        np.testing.assert_array_equal(o["flags"][sl], w["flags"], err_msg=yt[k][0])
        assert np.isfinite(o["cov"][sl]).all() and (o["cov"][sl] >= 0).all()
    print(f"{config}: device against the 50-digit yardstick at the ends of the range: positions {worst[0]:.2e} m, variances {worst[1]:.2e}, nis {worst[2]:.2e} relative")


# ------------------------------------------------------------------------------------------------ 4. a bad variance is a missing fix
def planted_bad_rows(arrays, rng):
    """rows that are otherwise available: mid-track, at lanes 0 and 63 of a chunk, next to outages (which lengthens them), between two
    outages (which merges them) and inside runs of fixes (which opens one)"""
    offs = arrays[5]
    base = base_rows(arrays)
    pick = np.zeros(len(base), bool)
    for b in range(len(offs) - 1):
        n = offs[b + 1] - offs[b]
        rows = [n // 2, 63, 64, 127, 128, 1, n - 1] + list(rng.integers(1, max(n, 2), 6))
        av = base[offs[b]:offs[b + 1]]
        for i in range(1, n - 1):                                       # a fix next to an outage, and a lone run of fixes between two
            if av[i] and (not av[i - 1] or not av[i + 1]) and rng.random() < 0.5:
                rows.append(i)
        gone = np.flatnonzero(~av[1:]) + 1                              # every short run of fixes between two outages, whole: the two become one
        for lo, hi in zip(gone[:-1], gone[1:]):
            if 1 < hi - lo <= 6:
                rows += list(range(lo + 1, hi))
        for i in rows:
            if 0 < i < n:
                pick[offs[b] + i] = True
    return pick & base


def outage_runs(flags):
    """[(first, end)] of the runs of IN_OUTAGE rows of one track"""
    m = np.concatenate(([False], (flags & IN_OUTAGE) != 0, [False]))
    edges = np.flatnonzero(m[1:] != m[:-1])
    return list(zip(edges[0::2].tolist(), edges[1::2].tolist()))


@pytest.mark.parametrize("how", ["bad", "all-inf"])
def test_a_bad_variance_is_a_missing_fix(B, planted, how):
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    cfg = cfgs["axes-differ"]
    rng = np.random.default_rng(77)
    clean = np.where(np.isfinite(mv) & (mv > 0), mv, 0.04)              # every planted variance usable
    rows = planted_bad_rows(arrays, rng)
    offs = arrays[5]
    lanes = {int(i - offs[np.searchsorted(offs, i, side="right") - 1]) % 64 for i in np.flatnonzero(rows)}
    assert rows.sum() > 300 and {0, 63} <= lanes
    planted_mv = clean.copy()
    if how == "all-inf":
        planted_mv[rows] = np.inf
    else:
        values = [np.nan, 0.0, -1.0, np.nextafter(1e-8, 0), np.nextafter(1e8, np.inf), -np.inf, 1e9, 1e-300]
        for j, i in enumerate(np.flatnonzero(rows)):
            if j % 3 == 0:
                planted_mv[i, j % 2] = np.inf                           # +inf on one axis (or two): bad, not "no information"
                planted_mv[i, 2] = np.inf if j % 2 else planted_mv[i, 2]
            else:
                planted_mv[i, int(rng.integers(0, 3))] = values[j % len(values)]
    got = runw(B, arrays, planted_mv, cfg)
    masked = [x.copy() for x in arrays]
    masked[4][rows] = 0                                                 # the same rows with their mask bytes cleared instead
    ref = runw(B, masked, clean, cfg)
    base = runw(B, arrays, clean, cfg)
    for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "nis"):
        assert same(got[name], ref[name]), (how, name)
    np.testing.assert_array_equal(got["status"], ref["status"])
    np.testing.assert_array_equal(got["flags"] & np.uint8(255 - BAD_SIGMA), ref["flags"])
    np.testing.assert_array_equal((got["flags"] & BAD_SIGMA) != 0, rows if how == "bad" else np.zeros_like(rows))
    assert (ref["flags"] & BAD_SIGMA == 0).all()
    # the planted rows did open, lengthen and merge outages: every outage of the masked launch against the clean launch's outages inside it
    kinds = {"opened": 0, "lengthened": 0, "merged": 0}
    for b in range(len(offs) - 1):
        before, after = outage_runs(base["flags"][offs[b]:offs[b + 1]]), outage_runs(ref["flags"][offs[b]:offs[b + 1]])
        for lo, hi in after:
            inside = [(a, c) for a, c in before if lo <= a and c <= hi]
            kinds["opened"] += not inside
            kinds["lengthened"] += len(inside) == 1 and inside[0] != (lo, hi)
            kinds["merged"] += len(inside) >= 2
    print(f"{how}: outages of the launch with the planted rows: {kinds}")
    assert all(v > 0 for v in kinds.values()), kinds
    assert not same(base["pos"], got["pos"]) and ((base["flags"] ^ ref["flags"]) & (SMOOTHED | SHARP_TURN | SPAN_START)).any()
    assert (base["status"] != ref["status"]).any()


# ------------------------------------------------------------------------------------------------ 5. what is not read
def test_what_is_not_read(B, planted):
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    offs, cfg, o = arrays[5], cfgs["default"], out["default"]
    nb = len(tracks)
    unread = ~base_rows(arrays)                                         # row 0 of every track, masked-out rows, rows whose fix holds a NaN
    assert unread.sum() > 500 and (arrays[4][unread] != 0).any() and (arrays[4][unread] == 0).any()
    for pattern in (np.frombuffer(b"\xff" * 8, np.float64)[0], np.nan, -np.inf, 0.0):
        dirty = mv.copy()
        dirty[unread] = pattern
        r = runw(B, arrays, dirty, cfg)
        for name in NAMES:
            assert same(r[name], o[name]), (name, pattern)
        np.testing.assert_array_equal(r["status"], o["status"])
    # skipped runs: NaN rows (nis included), zero flags, status 0, and nothing of theirs is read
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
    dirty = mv.copy()
    dirty[rows] = np.frombuffer(b"\xff" * 8, np.float64)[0]
    r = runw(B, poisoned, dirty, cfg, run_status=dev(rs))
    for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "nis"):
        assert np.isnan(r[name][rows]).all() and same(r[name][~rows], o[name][~rows]), name
    assert (r["flags"][rows] == 0).all() and same(r["flags"][~rows], o["flags"][~rows])
    assert (r["status"][skipped] == 0).all() and (np.delete(r["status"], skipped) == np.delete(o["status"], skipped)).all()


# ------------------------------------------------------------------------------------------------ 6. batch independence and hygiene
def test_a_track_alone_in_the_batch_and_in_reversed_order(B, planted):
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    offs, o, cfg = arrays[5], out["default"], cfgs["default"]
    rev = list(range(len(tracks)))[::-1]
    r = runw(B, flat([tracks[k] for k in rev]), np.concatenate([mvs[k] for k in rev]), cfg)
    roffs = np.zeros(len(tracks) + 1, np.int64); roffs[1:] = np.cumsum([len(tracks[k][0]) for k in rev])
    for j, k in enumerate(rev):
        a, b = slice(offs[k], offs[k + 1]), slice(roffs[j], roffs[j + 1])
        for name in NAMES:
            assert same(o[name][a], r[name][b]), (name, k)
        assert o["status"][k] == r["status"][j]
    for k in (1, 20, 40, 49, 57, 70, 100, len(tracks) - 1):             # lengths 1, 2, 63, 64 (bad rows planted), 64, 65, 129, 129
        alone = runw(B, flat([tracks[k]]), mvs[k], cfg)
        a = slice(offs[k], offs[k + 1])
        for name in NAMES:
            assert same(o[name][a], alone[name]), (name, k)
        assert o["status"][k] == alone["status"][0]


def test_optional_outputs_null_or_present(B, planted):
    import torch
    from gps_optimize_slam_amd import _lib
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    o, cfg = out["default"], cfgs["default"]
    for kw in (dict(want_filtered=False), dict(want_nis=False), dict(want_filtered=False, want_nis=False)):
        bare = runw(B, arrays, mv, cfg, **kw)
        assert (bare["pos_filt"] is None) == (not kw.get("want_filtered", True)) and (bare["nis"] is None) == (not kw.get("want_nis", True))
        for name in NAMES + ("status",):
            if bare[name] is not None:
                assert same(o[name], bare[name]), (kw, name)
    d, dmv = [dev(x) for x in arrays], dev(mv)
    P, nb = int(arrays[5][-1]), len(tracks)
    c = _lib.EkfConfig.from_config(cfg)
    f = dict(dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    opt = dict(pos_filt=(P, 3), cov_filt=(P, 7), flags=(P,), status=(nb,), nis=(P,))
    kinds = dict(flags=torch.uint8, status=torch.int32)
    for leave_out in list(opt) + ["all"]:                               # each optional output NULL in turn, then all of them
        pos, quat, cov = torch.full((P, 3), float("nan"), **f), torch.full((P, 4), float("nan"), **f), torch.full((P, 7), float("nan"), **f)
        o_t = {k: None if leave_out in (k, "all") else torch.zeros(s, dtype=kinds.get(k, torch.float64), device="cuda") for k, s in opt.items()}
        _lib.check(_lib.load().gsf_ekf_smooth_weighted_dev(B.context().handle, *[p(x) for x in d[:5]], p(dmv), *[p(x) for x in d[5:]], None, C.byref(c),
                                                           nb, p(pos), p(quat), p(cov), p(o_t["pos_filt"]), p(o_t["cov_filt"]), p(o_t["flags"]),
                                                           p(o_t["status"]), p(o_t["nis"])))
        torch.cuda.synchronize()
        assert same(pos.cpu().numpy(), o["pos"]) and same(quat.cpu().numpy(), o["quat"]) and same(cov.cpu().numpy(), o["cov"]), leave_out
        for k, t in o_t.items():
            if t is not None:
                assert same(t.cpu().numpy(), o[k]), (leave_out, k)


def test_outputs_do_not_depend_on_stale_buffers(B, monkeypatch, planted):
    """outputs prefilled with two byte patterns behind guard bytes, workspaces poisoned and not: the same bytes -- every row of every
    non-empty track is written, nis included, and what the forward pass parks in cov_out leaves nothing behind"""
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    d = [dev(x) for x in arrays]
    dmv = dev(mv)
    res = hygiene.same_bytes_under_dirt(monkeypatch, B.context(),
                                        lambda: B.ekf_smooth_weighted_ragged(*d[:5], dmv, *d[5:], config=cfgs["default"], want_filtered=True, want_nis=True),
                                        small_dirt(B), rows_of=arrays[5])
    o = out["default"]
    assert same(res.cov.cpu().numpy(), o["cov"]) and same(res.pos.cpu().numpy(), o["pos"]) and same(res.nis.cpu().numpy(), o["nis"])
    assert np.isfinite(o["cov"]).all() and (o["cov"] >= 0).all() and not np.signbit(o["cov"]).any()      # no tag bit survives


def test_side_stream_gives_the_same_bytes(B, planted):
    import torch
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    o = out["default"]
    ctx0 = B.context()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
        busy = a @ a                                                    # keeps the stream busy while the inputs and the call are queued behind it
        up = lambda x: torch.as_tensor(np.ascontiguousarray(x)).pin_memory().to("cuda", non_blocking=True)
        d2 = [up(x) for x in arrays]
        assert B.context() is not ctx0
        got = B.ekf_smooth_weighted_ragged(*d2[:5], up(mv), *d2[5:], config=cfgs["default"], want_filtered=True, want_nis=True)
        s.synchronize()
    for name, t in (("pos", got.pos), ("quat", got.quat), ("cov", got.cov), ("pos_filt", got.pos_filt), ("cov_filt", got.cov_filt), ("flags", got.flags),
                    ("nis", got.nis), ("status", got.status)):
        assert same(t.cpu().numpy(), o[name]), name
    del busy


# ------------------------------------------------------------------------------------------------ 7. variances onto SLAM stamps
@pytest.mark.parametrize("masks", ["none", "keep", "keep+valid", "valid"])
def test_fix_var_at_poses_bit_for_bit(B, monkeypatch, masks):
    import torch
    c = W.bracket_case()
    keep = c["keep"] if "keep" in masks else None
    valid = c["valid"] if "valid" in masks else None
    want = W.fix_var_at_poses_ref(c["ts"], c["slam_offsets"], c["gps_t"], c["gps_offsets"], c["fix_var"], keep, valid)
    args = [dev(c[k]) for k in ("ts", "slam_offsets", "gps_t", "gps_offsets", "fix_var")]
    kw = dict(keep=None if keep is None else dev(keep), valid=None if valid is None else dev(valid))
    for sentinel in (0, -1):                                            # the output behind guard bytes, pre-filled with two patterns
        alloc = hygiene.GuardedAllocator(sentinel)
        with alloc.installed(monkeypatch):
            got = B.fix_var_at_poses_ragged(*args, **kw)
        torch.cuda.synchronize()
        alloc.assert_guards_intact()
        assert alloc.find(got) is not None
        assert same(got.cpu().numpy(), want), (masks, sentinel)
    if masks == "none":                                                 # offsets that do not end at the rows given are refused, not clamped
        short = dev(c["slam_offsets"][:-1].copy()), dev(c["gps_offsets"][:-1].copy())
        with pytest.raises(ValueError):
            B.fix_var_at_poses_ragged(args[0], short[0], args[2], short[1], args[4])
        with pytest.raises(ValueError):
            B.fix_var_at_poses_ragged(args[0][:-1].contiguous(), args[1], args[2], args[3], args[4])


# ------------------------------------------------------------------------------------------------ 8. composition
def test_smooth_weighted_fused_is_its_steps_and_leaves_the_run_alone(B, golden, tmp_path):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    rb = file_batch(B, golden, tmp_path)
    seeds = [3, 4, 5, 6]
    r = B.run_fusion_ragged(rb, B.mt19937_seed(seeds), E.CONFIG)
    T = int(rb.gps_t.numel())
    rng = np.random.default_rng(5)
    codes = torch.as_tensor(rng.choice([1, 2, 4, 5, 9], T, p=[0.2, 0.1, 0.5, 0.15, 0.05])).cuda()
    fix_var = B.quality_to_var(codes, {4: (4e-4, 4e-4, 1.6e-3), 5: (0.25, 0.25, 1.0), 2: (1.0, 1.0, 4.0), 1: (9.0, 9.0, 36.0)})      # 9: not in the table, +inf
    st = B.smooth_weighted_fused(rb, r, fix_var)
    # the steps by hand
    ts, offsets = rb.ts.reshape(-1), rb.slam_offsets
    pv = B.fix_var_at_poses_ragged(ts, offsets, rb.gps_t, rb.gps_offsets, fix_var, keep=r.gps_keep, valid=r.valid.reshape(-1))
    ip, iq = B._fused_init_pose(rb, r)
    by_hand = B.ekf_smooth_weighted_ragged(ts, rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), r.aligned.reshape(-1, 3), r.valid.reshape(-1).contiguous(), pv,
                                           offsets, ip, iq, config=None, run_status=r.run_status, want_filtered=True, want_nis=True)
    rows = B._step6_rows(ts, offsets, (rb.pos.reshape(-1, 3), r.sim3_pos.reshape(-1, 3), by_hand.pos_filt, by_hand.pos), r.aligned.reshape(-1, 3),
                         r.valid.reshape(-1).contiguous(), 5.0)
    again = B.run_fusion_ragged(rb, B.mt19937_seed(seeds), E.CONFIG)    # the same context, after the weighted calls
    torch.cuda.synchronize()
    assert isinstance(st, B.WeightedTrack) and torch.equal(words(st.pose_var), words(pv))
    for name in ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags", "status", "nis"):
        assert torch.equal(words(getattr(st, name)), words(getattr(by_hand, name))), name
    assert torch.equal(words(st.err_stats4), words(torch.stack([x[0] for x in rows]))) and torch.equal(words(st.errors4), words(torch.stack([x[1] for x in rows])))
    assert tuple(st.err_stats4.shape) == (4, 4, 4) and tuple(st.errors4.shape) == (4, int(ts.numel()))
    ran = (r.run_status == 0).cpu().numpy()
    np.testing.assert_allclose(st.err_stats4[1].cpu().numpy()[ran], r.err_stats[0, 1].cpu().numpy()[ran], rtol=1e-9)      # Sim3: the run's own step 6
    for name in ("aligned", "valid", "sim3_pos", "gps_keep", "run_status", "err_stats", "R", "t", "s"):
        assert torch.equal(words(getattr(r, name)), words(getattr(again, name))), name
    assert torch.equal(words(r.fused.buf), words(again.fused.buf)) and torch.equal(r.fused.status, again.fused.status)
    rs, so = r.run_status.cpu().numpy(), offsets.cpu().numpy()
    flags, nis, pvh = st.flags.cpu().numpy(), st.nis.cpu().numpy(), st.pose_var.cpu().numpy()
    m = st.mean_nis().cpu().numpy()
    for b in range(4):
        sl = slice(so[b], so[b + 1])
        if rs[b] != 0:
            assert np.isnan(st.pos.cpu().numpy()[sl]).all() and (flags[sl] == 0).all() and np.isnan(nis[sl]).all() and np.isnan(m[b])
            continue
        used = (flags[sl] & GNSS_USED) != 0
        assert used.any() and (flags[sl] & SMOOTHED).any() and np.isfinite(nis[sl][used]).all() and np.isfinite(pvh[sl][used]).all()
        assert abs(m[b] - nis[sl][used].mean()) <= 1e-12 * abs(m[b])
        assert np.isinf(pvh[sl]).all(1).sum() > 0                       # code 9 and the poses outside the kept fixes: no information
    assert not (flags & BAD_SIGMA).any()                                 # every variance of the table is usable


def test_single_track_entry(B, planted):
    from gps_optimize_slam_amd import ekfgpsslam as E
    tracks, mvs, arrays, mv, cfgs, out, want = planted
    k = 100                                                              # 129 poses
    one = E.ekf_smooth_aligned_weighted(*tracks[k][:5], mvs[k], *tracks[k][5:], cfgs["default"])
    sl = slice(arrays[5][k], arrays[5][k + 1])
    for name in NAMES:
        assert same(one[name], out["default"][name][sl]), name
    assert one["status"] == out["default"]["status"][k]


# ------------------------------------------------------------------------------------------------ 9. why per-fix variances, on the device
def test_per_fix_variances_beat_the_unweighted_smoother_on_the_device(B):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    ts, pos, quat, aligned, valid, ip, iq, mv, truth = W.motivation_track()
    cfg = copy.deepcopy(E.CONFIG)
    cfg["gps_filtering_ransac"] = dict(cfg["gps_filtering_ransac"], enabled=False)
    rb = B.RaggedGeodeticBatch.from_host([(ts, pos, quat)], [np.column_stack((ts, aligned))])      # the fixes as a log of projected rows
    r = B.run_fusion_ragged(rb, B.mt19937_seed([9]), cfg, projected=True)
    assert int(r.run_status[0]) == 0
    plain = B.smooth_fused(rb, r, config=cfg)
    weighted = B.smooth_weighted_fused(rb, r, dev(mv), config=cfg)
    torch.cuda.synchronize()
    used = (weighted.flags.cpu().numpy() & GNSS_USED) != 0
    assert used.sum() > 200 and not (weighted.flags.cpu().numpy() & BAD_SIGMA).any()
    a, b = rmse(weighted.pos.cpu().numpy(), truth), rmse(plain.pos.cpu().numpy(), truth)
    print(f"RMSE against the truth on the device: per-fix variances {a:.4f} m, the default R {b:.4f} m; mean nis {float(weighted.mean_nis()[0]):.2f}")
    assert a < b
