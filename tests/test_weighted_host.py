"""CPU tier of per-fix GNSS noise (gsf_ekf_smooth_weighted_dev, gsf_fix_var_at_poses_dev): the SPECIFICATION, pinned before any GPU runs.

1. tests/weighted_ref.weighted_restate is test_smooth_host.restate with R a per-row array.  With meas_var[i] = meas_noise_diag on every
   row it must return restate's arrays byte for byte, flags and status exactly, on every track of tests/golden/ekf_smooth_tracks.npz --
   which ties the new restatement to the goldens generated from the reference.
2. The rules of gsf_weighted_core.hpp -- usable variance, row kind, avail, BAD_SIGMA against all-inf, the bracket rule -- compiled with g++
   -ffp-contract=off as a stand-alone program (tests/host_harness_weighted.cpp), run plain and under -fsanitize=address,undefined, against
   the restatement bit for bit.
3. The yardstick: the same recurrences in 50 digits (mpmath) on tracks of 2, 65 and 129 poses whose variances jump between both ends of
   the stated range (1e-8, 1e8) inside a chunk and across a chunk boundary, under the default config and AXES_DIFFER.

Gates: the project's existing ones for these quantities and their derivation (head of tests/test_smooth_gpu.py) -- positions 1e-6 m,
variances (and nis) 1e-10 relative, quaternions 1e-9.  Measured here, restatement against the yardstick over the ten (track, config) pairs:
positions 1.9e-9 m (two ulp of a UTM northing), filtered variances 5.0e-16, smoothed variances 2.6e-15, nis 4.9e-13, all relative.  A jump
of sixteen orders of magnitude in r under even steps costs the restatement no more digits than a constant r does (restate against the
reference: 8.2e-15), so no gate is widened there.
4. The track the kernel's rescaled scan exists for (weighted_ref.long_short_track): r at both ends AND steps of 1e14 s followed by repeated
   stamps.  A NumPy emulation of the staged scan (weighted_ref.scan_variances) leaves the doubles without the two rescales and returns the
   yardstick's variances with them.  There the smoothed variance Ps = Pf + d cancels to 1e-15 of Pf (largest Pf / Ps 9.09e14), so it is
   held to |dPs| <= 1e-10 Ps + 8 C u Pf per row, u = 2^-53, C = 0.55 from the restatement's measured worst 0.51 (weighted_ref.PS_C); Pf,
   positions and nis stay at the ordinary gates (measured: Pf exact, positions 1.4e-14 m, nis 4.0e-14).
The device is held to the same yardstick at the same gates and bounds (tests/test_weighted_gpu.py), never to itself."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import weighted_ref as W
from test_cov_gpu import AXES_DIFFER
from test_smooth_host import restate, smooth_tracks, var_err

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POS_TOL, VAR_TOL = 1e-6, 1e-10


def full_cfg(part):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = copy.deepcopy(E.CONFIG)
    for sec, kv in part.items():
        cfg[sec].update(kv)
    return cfg


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------ 1. against the unweighted restatement
def test_constant_variances_are_the_unweighted_restatement_on_every_golden_track(golden):
    tracks, g = smooth_tracks(golden)
    assert len(tracks) == 88
    for t in tracks:
        name, ts, pos, quat, aligned, valid, ip, iq, cfg = t
        want = restate(ts, pos, quat, aligned, valid, ip, iq, cfg)
        mv = np.tile(np.array(cfg["ekf"]["meas_noise_diag"], float), (len(ts), 1))
        mv[0] = np.nan                                                  # row 0 is not read
        got = W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)
        for key in ("xf", "g", "quat", "Pf", "Pp", "avail", "reached", "e", "d", "xs", "Ps", "flags"):
            assert same(got[key], want[key]), (name, key)
        assert got["starts"] == want["starts"] and got["status"] == want["status"] and not got["bad"].any(), name
        used = (got["flags"] & W.GNSS_USED) != 0
        assert np.isnan(got["nis"][~used]).all() and np.isfinite(got["nis"][used]).all() and (got["nis"][used] >= 0).all(), name


# ------------------------------------------------------------------------------------------------ 2. the host harness
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request):
    """tests/host_harness_weighted.cpp as a stand-alone program: plain, and under AddressSanitizer + UndefinedBehaviorSanitizer"""
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, "host_harness_weighted_" + request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HERE, "host_harness_weighted.cpp")])

    def run(mode, payload, tmp_path):
        fin, fout = tmp_path / f"{mode}.in", tmp_path / f"{mode}.out"
        fin.write_bytes(payload)
        p = subprocess.run([exe, mode, str(fin), str(fout)], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return fout.read_bytes()
    return run


def below(v):
    return float(np.nextafter(v, -np.inf))


def above(v):
    return float(np.nextafter(v, np.inf))


def test_usable_variance_avail_and_bad_sigma_rules(harness, tmp_path):
    inf, nan = np.inf, np.nan
    ok = 0.04
    singles = [nan, 0.0, -0.0, -1.0, below(1e-8), 1e-8, above(1e-8), below(1e8), 1e8, above(1e8), inf, -inf, 5e-324, 1.7976931348623157e308, ok]
    rows = []
    for base in (0.0, 1.0):
        for v in singles:                                               # the value on one axis, on each axis in turn, and on all three
            rows += [[base, v, ok, ok], [base, ok, v, ok], [base, ok, ok, v], [base, v, v, v]]
        rows += [[base, inf, inf, 1e8], [base, inf, nan, inf], [base, inf, inf, -inf], [base, 1e-8, 1e8, 1e-8], [base, 1e8, 1e-8, 1e8]]
    rows = np.array(rows, float)
    out = np.frombuffer(harness("rows", np.int64(len(rows)).tobytes() + rows.tobytes(), tmp_path), np.int32).reshape(-1, 6)
    assert len(out) == len(rows)
    seen = set()
    for r, o in zip(rows, out):
        kind = W.row_kind(r[1:])
        want = [int(W.usable(v)) for v in r[1:]] + [kind, int(r[0] != 0 and kind == W.USABLE), int(r[0] != 0 and kind == W.BAD)]
        assert o.tolist() == want, (r, o, want)
        seen.add((int(r[0]), kind))
    assert seen == {(b, k) for b in (0, 1) for k in (W.USABLE, W.BAD, W.NO_INFO)}
    # the ends of the range are inside it; one ulp outside is not; all-inf is no information, inf on one axis is a bad row
    assert W.usable(1e-8) and W.usable(1e8) and not W.usable(below(1e-8)) and not W.usable(above(1e8))
    assert W.row_kind([inf, inf, inf]) == W.NO_INFO and W.row_kind([inf, ok, ok]) == W.BAD and W.row_kind([nan, nan, nan]) == W.BAD


def bracket_payload(c, keep, valid):
    P, B, T = len(c["ts"]), len(c["slam_offsets"]) - 1, len(c["gps_t"])
    parts = [np.array([P, B, T, keep is not None, valid is not None], np.int64), c["ts"], c["slam_offsets"], c["gps_t"], c["gps_offsets"]]
    if keep is not None:
        parts.append(keep)
    parts.append(c["fix_var"])
    if valid is not None:
        parts.append(valid)
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.mark.parametrize("masks", ["none", "keep", "keep+valid", "valid"])
def test_bracket_rule_bit_for_bit(harness, tmp_path, masks):
    c = W.bracket_case()
    keep = c["keep"] if "keep" in masks else None
    valid = c["valid"] if "valid" in masks else None
    want = W.fix_var_at_poses_ref(c["ts"], c["slam_offsets"], c["gps_t"], c["gps_offsets"], c["fix_var"], keep, valid)
    got = np.frombuffer(harness("bracket", bracket_payload(c, keep, valid), tmp_path), np.float64).reshape(-1, 3)
    assert same(got, want), np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(1))
    # the cases are all there: no bracket, a bracket, a NaN carried through
    assert np.isinf(want).all(1).any() and np.isfinite(want).all(1).any() and np.isnan(want).any()
    if valid is not None:
        assert np.isinf(want[valid == 0]).all()


def test_bracket_rule_by_hand():
    """the restatement itself, on the cases the definition names"""
    t = np.arange(7.0)
    fv = np.column_stack((np.arange(1.0, 8.0), 10.0 - np.arange(7.0), np.ones(7)))
    so, go = np.array([0, 6]), np.array([0, 7])
    keep = np.array([0, 1, 1, 0, 1, 0, 0], np.uint8)
    ts = np.array([0.5, 1.0, 1.5, 3.0, 4.0, 4.5])
    out = W.fix_var_at_poses_ref(ts, so, t, go, fv, keep)
    assert np.isinf(out[0]).all() and np.isinf(out[5]).all()             # before the first / after the last KEPT fix
    assert out[1].tolist() == fv[1].tolist() and out[4].tolist() == fv[4].tolist()      # on a kept fix's stamp: that fix's own
    assert out[2].tolist() == [3.0, 9.0, 1.0]                            # the larger of fixes 1 and 2 per axis
    assert out[3].tolist() == [5.0, 8.0, 1.0]                            # on a removed fix's stamp: its kept neighbours 2 and 4
    rep = W.fix_var_at_poses_ref(np.array([1.0]), np.array([0, 1]), np.array([0.0, 1.0, 1.0, 1.0, 2.0]), np.array([0, 5]),
                                 np.column_stack((np.array([9.0, 2.0, 7.0, 3.0, 9.0]),) * 3))
    assert rep[0].tolist() == [3.0, 3.0, 3.0]                            # repeated stamps: the larger of the last and the first of them


# ------------------------------------------------------------------------------------------------ 3. the yardstick
@pytest.fixture(scope="module")
def yard():
    return W.yardstick_tracks()


def yard_errors(w, y):
    """largest deviation of a result (restatement's keys) from the yardstick: positions (m), variances, nis (relative)"""
    ep = max(np.abs(w["xf"] - y["xf"]).max(), np.abs(w["xs"] - y["xs"]).max())
    ev = max(var_err(w["Pf"][:, :3], y["Pf"]), var_err(w["Ps"][:, :3], y["Ps"]))
    used = ~np.isnan(y["nis"])
    assert (np.isnan(w["nis"]) == ~used).all()
    en = float(np.max(np.abs(w["nis"][used] - y["nis"][used]) / y["nis"][used], initial=0.0))
    return ep, ev, en


@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_restatement_against_the_50_digit_yardstick_at_the_ends_of_the_range(yard, config):
    cfg = full_cfg({} if config == "default" else AXES_DIFFER)
    worst = [0.0, 0.0, 0.0]
    for name, ts, pos, quat, aligned, valid, ip, iq, mv in yard:
        used = mv[1:][valid[1:] & ~np.isnan(aligned[1:]).any(1)]
        assert set(np.unique(used)) <= {W.VAR_MIN, W.VAR_MAX} and (len(ts) == 2 or len(np.unique(used)) == 2)   # both ends, nothing between
        if len(ts) > 64:
            assert (mv[63] != mv[64]).all() and (mv[62] != mv[63]).all()                # a jump inside a chunk and across its boundary
        w = W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)
        assert not w["bad"].any() and w["avail"].any()
        y = W.yardstick(w, aligned, mv, ip, cfg)
        e = yard_errors(w, y)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] < POS_TOL and e[1] < VAR_TOL and e[2] < VAR_TOL, (name, e)
        # corrections, where nothing of UTM size is added; d = Ps - Pf is held relative to the row's own Pf, the larger of the two it is made of
        assert np.abs(w["e"] - y["e"]).max() < POS_TOL and np.abs(w["xr"] - y["xr"]).max() < POS_TOL, name
        assert (np.abs(w["d"] - y["d"]) <= VAR_TOL * y["Pf"]).all(), name
    print(f"{config}: restatement against the yardstick: positions {worst[0]:.2e} m, variances {worst[1]:.2e}, nis {worst[2]:.2e} relative")


@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_long_and_short_steps_need_the_rescaled_scan(yard, config):
    """r at both ends of the range AND steps of 1e14 s followed by repeated stamps: the product of a chunk's scaled steps leaves the doubles
    (variance_scan as it stands returns NaN), the two rescales of variance_scan<6, true> keep it in range, and the result is the yardstick's"""
    cfg = full_cfg({} if config == "default" else AXES_DIFFER)
    name, ts, pos, quat, aligned, valid, ip, iq, mv = W.long_short_track()
    P0, Q = (np.array(cfg["ekf"][k], float)[:3] for k in ("initial_cov_diag", "process_noise_diag"))
    assert (Q * np.diff(ts).max() <= 1e14).all() and set(np.unique(mv)) == {W.VAR_MIN, W.VAR_MAX}      # inside the stated domain
    w = W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)
    assert w["avail"][1:].all() and not w["bad"].any()
    y = W.yardstick(w, aligned, mv, ip, cfg)
    for c in range(3):
        plain = W.scan_variances(w["dt"], w["avail"], mv[:, c], Q[c], P0[c], rescale=False)
        scaled = W.scan_variances(w["dt"], w["avail"], mv[:, c], Q[c], P0[c], rescale=True)
        assert not np.isfinite(plain[:64]).all() and not np.isfinite(plain[64:]).all(), c      # both chunks overflow without the rescales
        assert var_err(scaled, y["Pf"][:, c]) < VAR_TOL, c
    # ... and on a track with even steps the rescales change no bit
    _, ts2, pos2, quat2, al2, va2, ip2, iq2, mv2 = yard[3]
    w2 = W.weighted_restate(ts2, pos2, quat2, al2, va2, mv2, ip2, iq2, cfg)
    for c in range(3):
        a, b = (W.scan_variances(w2["dt"], w2["avail"], mv2[:, c], Q[c], P0[c], rescale=k) for k in (False, True))
        assert same(a, b) and var_err(a, w2["Pf"][:, c]) < VAR_TOL, c
    ep = max(np.abs(w["xf"] - y["xf"]).max(), np.abs(w["xs"] - y["xs"]).max())
    used = ~np.isnan(y["nis"])
    en = float(np.max(np.abs(w["nis"][used] - y["nis"][used]) / y["nis"][used]))
    ok, c_ps, ratio = W.ps_within_bound(w["Ps"][:, :3], y, VAR_TOL)
    print(f"{config}: long and short steps, restatement against the yardstick: positions {ep:.2e} m, Pf {var_err(w['Pf'][:, :3], y['Pf']):.2e}, nis {en:.2e} relative; "
          f"Ps: largest Pf / Ps {ratio:.2e}, worst |dPs| / (u Pf) {c_ps:.2f} (C = {W.PS_C}, gate 8 C)")
    assert ep < POS_TOL and var_err(w["Pf"][:, :3], y["Pf"]) < VAR_TOL and en < VAR_TOL
    assert c_ps <= W.PS_C and ok and ratio > 1e14


# ------------------------------------------------------------------------------------------------ 4. why per-fix variances
def rmse(a, b):
    return float(np.sqrt(np.mean(np.sum((a - b) ** 2, axis=1))))


def test_per_fix_variances_beat_every_constant_on_a_planted_track():
    ts, pos, quat, aligned, valid, ip, iq, mv, truth = W.motivation_track()
    cfg = full_cfg({})
    weighted = rmse(W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)["xs"], truth)
    good = mv[:, 0].min()
    figures = {}
    for name, R in (("the default R", cfg["ekf"]["meas_noise_diag"]), ("the mean variance", [float(mv[:, 0].mean())] * 3), ("the good fixes' variance", [good] * 3)):
        c = copy.deepcopy(cfg)
        c["ekf"]["meas_noise_diag"] = [float(v) for v in R]
        figures[name] = rmse(restate(ts, pos, quat, aligned, valid, ip, iq, c)["xs"], truth)
    print(f"RMSE against the truth, smoothed: per-fix variances {weighted:.4f} m; " + "; ".join(f"{k} {v:.4f} m" for k, v in figures.items()))
    for name, v in figures.items():
        assert weighted < v, (name, weighted, v)


# ------------------------------------------------------------------------------------------------ 5. the library's surface
def test_library_exports_the_entries_as_declared():
    from gps_optimize_slam_amd import _lib
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    L = C.CDLL(_lib.library_path())                                     # loads without a device
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsf.h")).read(), flags=re.S)
    kinds = {"gsf_ctx *": C.c_void_p, "const double *": C.c_void_p, "double *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p,
             "const int64_t *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t *": C.c_void_p, "int64_t": C.c_int64,
             "const gsf_ekf_config *": C.POINTER(_lib.EkfConfig)}
    want = {"gsf_ekf_smooth_weighted_dev": ["ctx", "ts", "pos", "quat", "gps", "valid", "meas_var", "offsets", "init_pos", "init_quat", "run_status", "cfg",
                                            "B", "pos_out", "quat_out", "cov_out", "pos_filt", "cov_filt", "pose_flags", "status", "nis"],
            "gsf_fix_var_at_poses_dev": ["ctx", "ts", "slam_offsets", "gps_t", "gps_offsets", "gps_keep", "fix_var", "valid", "B", "P", "pose_var"]}
    for name, names in want.items():
        assert hasattr(L, name) and not hasattr(L, name[:-4]) and name[:-4] not in _lib.SIGNATURES      # device forms only
        m = re.search(r"GSF_API int " + name + r"\s*\(([^;]*)\);", src)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        assert [re.search(r"(\w+)$", p).group(1) for p in params] == names
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [kinds[re.sub(r"\w+$", "", p).strip()] for p in params], name
    assert re.search(r"#define\s+GSF_POSE_BAD_SIGMA\s+32\b", src) and _lib.POSE_BAD_SIGMA == 32 == W.BAD_SIGMA
    core = open(os.path.join(ROOT, "gps_optimize_slam_amd", "csrc", "gsf_weighted_core.hpp")).read()
    assert re.search(r"POSE_BAD_SIGMA\s*=\s*32\b", core) and re.search(r"WVAR_MIN\s*=\s*1e-8,\s*WVAR_MAX\s*=\s*1e8\b", core)


def test_weighted_track_places_its_pieces():
    import torch
    from gps_optimize_slam_amd import _lib, batch
    rng = np.random.default_rng(0)
    t = lambda *shape: torch.as_tensor(rng.uniform(0.1, 1, shape))
    pos, quat, cov, pf, cf = t(5, 3), t(5, 4), t(5, 7), t(5, 3), t(5, 7)
    flags = torch.tensor([16, 1, 2 | 32, 1, 2], dtype=torch.uint8)
    nis = torch.tensor([float("nan"), 2.0, float("nan"), 4.0, float("nan")], dtype=torch.float64)
    wt = batch.WeightedTrack(pos, quat, cov, pf, cf, flags, torch.zeros(3, dtype=torch.int32), torch.tensor([0, 3, 3, 5]), nis)
    assert isinstance(wt, batch.SmoothedTrack) and torch.equal(wt.correction(), pos - pf) and tuple(wt.dense().shape) == (5, 7, 7)
    assert wt.bad_sigma.tolist() == [False, False, True, False, False] and wt.nis is nis
    m = wt.mean_nis()
    assert m[0].item() == 2.0 and np.isnan(m[1].item()) and m[2].item() == 4.0      # per track over its used rows; none: NaN
    with pytest.raises(ValueError):
        batch.WeightedTrack(pos, quat, cov, None, None, flags, wt.status, wt.offsets).mean_nis()
    # the lookup from a quality code to a variance triple
    v = batch.quality_to_var(torch.tensor([4, 5, 1, 9]), {4: (4e-4, 4e-4, 1.6e-3), 5: (0.25, 0.25, 1.0), 1: (9.0, 9.0, 36.0)})
    assert v.dtype == torch.float64 and v[0].tolist() == [4e-4, 4e-4, 1.6e-3] and v[2].tolist() == [9.0, 9.0, 36.0] and torch.isinf(v[3]).all()
    assert batch.quality_to_var(torch.tensor([7.0]), {}, default=2.0).tolist() == [[2.0, 2.0, 2.0]]
    with pytest.raises(ValueError):
        batch.quality_to_var(torch.tensor([1]), {1: (1.0, 2.0)})


def test_read_gnss_quality(tmp_path):
    from gps_optimize_slam_amd import batch
    rng = np.random.default_rng(1)
    a = np.column_stack((np.arange(5.0), rng.uniform(40, 41, (5, 3)), rng.integers(4, 20, 5), rng.integers(1, 6, 5)))
    b = np.column_stack((np.arange(3.0), rng.uniform(40, 41, (3, 3)), rng.integers(4, 20, 3), rng.integers(1, 6, 3)))
    pa, pb, pc, pd = (str(tmp_path / n) for n in ("a.txt", "b.txt", "c.txt", "d.txt"))
    np.savetxt(pa, a, fmt="%.18e"); np.savetxt(pb, b, fmt="%.18e", delimiter=",")
    np.savetxt(pc, a[:, :4], fmt="%.18e"); np.savetxt(pd, a[:, :5], fmt="%.18e")
    q = batch.read_gnss_quality([pa, pb])
    assert q.shape == (8, 2) and same(q, np.concatenate((a[:, 4:], b[:, 4:])))
    assert same(batch._read_gnss_file(pa), a[:, :4])                    # the loader itself still reads four columns
    with pytest.raises(ValueError, match="c.txt"):
        batch.read_gnss_quality([pa, pc])
    with pytest.raises(ValueError, match="d.txt"):
        batch.read_gnss_quality([pa, pd])
    pe = str(tmp_path / "empty.txt")
    open(pe, "w").close()
    for reader in (batch.read_gnss_quality, lambda paths: [batch._read_gnss_file(q_) for q_ in paths]):      # an empty file: refused by both, by name
        with pytest.raises(ValueError, match="empty.txt"):
            reader([pa, pe])
    with pytest.raises(ValueError, match="missing.txt"):
        batch.read_gnss_quality([str(tmp_path / "missing.txt")])
