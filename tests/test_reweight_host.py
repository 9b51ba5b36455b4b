"""CPU tier of robust smoothing (gsf_ekf_smooth_reweighted_dev): the SPECIFICATION, pinned before any GPU runs.

1. tests/reweight_ref.reweight_restate against weighted_ref.weighted_restate: rounds = 0 returns its bytes (law A); every solve of a call
   with rounds = R is weighted_restate on min(meas_var / w, 1e8), w the weights of the call with rounds = R - 1 (law B: by construction,
   checked all the same); the stop at a fixed point.
2. A 50-digit yardstick (mpmath): the filter and smoother recurrences AND the weight rule across all solves, rounded once at the end, on
   motivation_track(0, 129) with planted outliers (both losses, c2 = 7.81, 4 rounds) and on weighted_ref.yardstick_tracks() (Cauchy).
   Gates, the project's own: positions 1e-6 m; variances, nis and weights 1e-10 relative.  Measured here, restatement against yardstick:
   positions 1.9e-9 m (two ulp of a UTM northing; 1.5e-14 m relative to init_pos), variances 2.7e-14, nis 4.5e-13, weights 3.9e-14.
   The residual is formed relative to init_pos: from UTM positions the weights carry 4.4e-10 after four rounds, outside the gate.
3. gsf_reweight_core.hpp compiled with g++ -ffp-contract=off as a stand-alone program (tests/host_harness_reweight.cpp), run plain and
   under -fsanitize=address,undefined, against the restatement bit for bit: u2 = 0, = c2, one ulp either side, +inf, the largest and
   smallest doubles; a weight that underflows to 0; v / w just under, on and over 1e8; both losses; the fixed-point rule.
4. The exported symbol and its parameter list against the header.
5. The Huber objective does not rise from one round to the next (one-span track); the motivation: reweighted RMSE < the weighted
   smoother's on three seeds."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reweight_ref as R
import weighted_ref as W
from test_cov_gpu import AXES_DIFFER
from test_weighted_host import above, below, full_cfg, rmse, same

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POS_TOL, VAR_TOL = 1e-6, 1e-10
C2 = 7.81
SHARED = ("xf", "g", "quat", "Pf", "Pp", "avail", "reached", "e", "d", "xs", "Ps", "flags", "nis", "bad", "xr")


@pytest.fixture(scope="module")
def planted():
    """motivation_track(0, 129) with planted outliers, and the calls on it that several tests share: {(loss, rounds): result}"""
    t = R.motivation(0, 129)
    cfg = full_cfg({})
    calls = {(loss, k): R.reweight_restate(*t[:5], t[7], t[5], t[6], cfg, loss, C2, k) for loss in (R.HUBER, R.CAUCHY) for k in (0, 1, 2, 3, 4)}
    return t, cfg, calls


# ------------------------------------------------------------------------------------------------ 1. the two laws, the stop
def test_law_a_rounds_zero_is_the_weighted_restatement(planted):
    t, cfg, calls = planted
    ts, pos, quat, aligned, valid, ip, iq, mv = t[:8]
    want = W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)
    for loss in (R.HUBER, R.CAUCHY):
        got = calls[(loss, 0)]
        for key in SHARED:
            assert same(got[key], want[key]), (loss, key)
        assert got["starts"] == want["starts"] and got["status"] == want["status"] and got["rounds_used"] == 0
        used = (got["flags"] & W.GNSS_USED) != 0
        assert np.isnan(got["weight"][~used]).all() and ((got["weight"][used] > 0) & (got["weight"][used] <= 1)).all()
        assert (got["weight"][used] < 1).any() and got["w_change"] == np.max(1.0 - got["weight"][used])
    # without variances: the config's R on every row, which is the unweighted restatement (test_weighted_host ties those two)
    const = np.tile(np.array(cfg["ekf"]["meas_noise_diag"], float), (len(ts), 1))
    a = R.reweight_restate(ts, pos, quat, aligned, valid, None, ip, iq, cfg, R.HUBER, C2, 0)
    b = W.weighted_restate(ts, pos, quat, aligned, valid, const, ip, iq, cfg)
    for key in SHARED:
        assert same(a[key], b[key]), key


@pytest.mark.parametrize("rounds", [1, 3])
def test_law_b_a_round_is_the_weighted_restatement_on_the_effective_variances(planted, rounds):
    t, cfg, calls = planted
    ts, pos, quat, aligned, valid, ip, iq, mv = t[:8]
    for loss in (R.HUBER, R.CAUCHY):
        w = calls[(loss, rounds - 1)]["weight"]
        with np.errstate(invalid="ignore"):
            fed = np.where(np.isnan(w)[:, None], mv, np.minimum(mv / w[:, None], 1e8))
        want = W.weighted_restate(ts, pos, quat, aligned, valid, fed, ip, iq, cfg)
        got = calls[(loss, rounds)]
        assert got["rounds_used"] == rounds
        for key in SHARED:
            assert same(got[key], want[key]), (loss, key)
        assert got["starts"] == want["starts"] and got["status"] == want["status"]
        assert not same(got["xs"], calls[(loss, rounds - 1)]["xs"])      # the round did move the track


def test_the_stop_at_a_fixed_point():
    ts, pos, quat, aligned, valid, ip, iq, mv, truth = W.motivation_track(0, 129)      # no outlier planted
    cfg = full_cfg({})
    for loss in (R.HUBER, R.CAUCHY):                                      # a threshold nothing reaches: Huber stops at once, Cauchy moves every weight
        r = R.reweight_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg, loss, 1e6, 5)
        used = (r["flags"] & W.GNSS_USED) != 0
        if loss == R.HUBER:
            assert r["rounds_used"] == 0 and r["w_change"] == 0.0 and (r["weight"][used] == 1.0).all() and len(r["history"]) == 1
        else:
            # ... by a few 1e-6 at most, so the weights reach a fixed point of their own bits before the rounds run out
            assert 1 <= r["rounds_used"] < 5 and r["w_change"] == 0.0 and (r["weight"][used] < 1.0).any() and (r["weight"][used] > 1.0 - 1e-3).all()
            assert len(r["history"]) == r["rounds_used"] + 1 and same(r["history"][-1]["w"], r["history"][-1]["w_used"])
    # a track without a used row: nothing to weigh
    none = R.reweight_restate(ts, pos, quat, aligned, np.zeros_like(valid), mv, ip, iq, cfg, R.HUBER, C2, 5)
    assert none["rounds_used"] == 0 and none["w_change"] == 0.0 and np.isnan(none["weight"]).all()
    # outliers planted: every round is used, and the weights of the planted rows fall
    t = R.motivation(0, 129)
    r = R.reweight_restate(*t[:5], t[7], t[5], t[6], cfg, R.HUBER, C2, 4)
    assert r["rounds_used"] == 4 and r["w_change"] > 0.0 and len(r["history"]) == 5
    rows = t[9]
    assert np.nanmedian(r["weight"][rows]) < 0.05 and np.nanmedian(r["weight"][~rows]) == 1.0
    # a weight of 0 and the cap: r_eff = 1e8, inside the usable range
    assert R.effective_var(np.array([[1e-8, 1.0, 1e8]]), np.array([0.0])).tolist() == [[1e8, 1e8, 1e8]]
    assert R.effective_var(np.array([[np.nan, 0.0, np.inf]]), np.array([np.nan]))[0].tolist()[1:] == [0.0, np.inf]


# ------------------------------------------------------------------------------------------------ 2. the yardstick
def result_keys(r):
    return dict(xf=r["xf"], xs=r["xs"], Pf=r["Pf"], Ps=r["Ps"], nis=r["nis"], weight=r["weight"])


def hold_to_yardstick(r, aligned, ip, cfg, loss, what):
    y = R.yardstick(r, aligned, ip, cfg, loss, C2)
    e = R.yard_errors(result_keys(r), y)
    rel = float(np.abs(r["xr"] - y["xr"]).max())
    assert e[0] < POS_TOL and e[1] < VAR_TOL and e[2] < VAR_TOL and e[3] < VAR_TOL and rel < POS_TOL, (what, e, rel)
    return e + (rel,)


def test_restatement_against_the_50_digit_yardstick_with_planted_outliers(planted):
    t, cfg, calls = planted
    for loss in (R.HUBER, R.CAUCHY):
        r = calls[(loss, 4)]
        assert r["rounds_used"] == 4
        e = hold_to_yardstick(r, t[3], t[5], cfg, loss, loss)
        print(f"loss {loss}, 4 rounds, restatement against the yardstick: positions {e[0]:.2e} m ({e[4]:.2e} m relative to init_pos), variances {e[1]:.2e}, "
              f"nis {e[2]:.2e}, weights {e[3]:.2e} relative")


@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_restatement_against_the_yardstick_at_the_ends_of_the_range(config):
    cfg = full_cfg({} if config == "default" else AXES_DIFFER)
    worst = [0.0] * 5
    for name, ts, pos, quat, aligned, valid, ip, iq, mv in W.yardstick_tracks():
        r = R.reweight_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg, R.CAUCHY, C2, 4)
        assert r["rounds_used"] >= 1 or len(ts) == 2, name
        worst = [max(a, b) for a, b in zip(worst, hold_to_yardstick(r, aligned, ip, cfg, R.CAUCHY, name))]
    print(f"{config}: Cauchy at the ends of the range, restatement against the yardstick: positions {worst[0]:.2e} m, variances {worst[1]:.2e}, "
          f"nis {worst[2]:.2e}, weights {worst[3]:.2e} relative")


# ------------------------------------------------------------------------------------------------ 3. the host harness
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request):
    """tests/host_harness_reweight.cpp as a stand-alone program: plain, and under AddressSanitizer + UndefinedBehaviorSanitizer"""
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, "host_harness_reweight_" + request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HERE, "host_harness_reweight.cpp")])

    def run(mode, rows, tmp_path, dtype=np.float64):
        rows = np.ascontiguousarray(rows, np.float64)
        fin, fout = tmp_path / f"{mode}.in", tmp_path / f"{mode}.out"
        fin.write_bytes(np.int64(len(rows)).tobytes() + rows.tobytes())
        p = subprocess.run([exe, mode, str(fin), str(fout)], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return np.frombuffer(fout.read_bytes(), dtype)
    return run


BIG, TINY = 1.7976931348623157e308, 5e-324


def test_weight_rule_bit_for_bit(harness, tmp_path):
    rows = []
    for loss in (R.HUBER, R.CAUCHY):
        for c2 in (C2, 1.0, 1e-300, 1e300, above(0.0) * 4):
            for u2 in (0.0, c2, below(c2), above(c2), np.inf, BIG, TINY, 2.0 * c2, 1e10 * c2, np.nan, 1.0, 1e5):
                rows.append([loss, c2, u2])
    rows = np.array(rows)
    got = harness("weights", rows, tmp_path)
    want = np.concatenate([R.weight_of(int(l), np.array([u]), c) for l, c, u in rows])
    assert same(got, want), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    w = {(int(l), c, u): v for (l, c, u), v in zip(rows.tolist(), got.tolist()) if not np.isnan(u)}
    for loss in (R.HUBER, R.CAUCHY):
        assert w[(loss, C2, 0.0)] == 1.0 and w[(loss, C2, np.inf)] == 0.0 and not np.signbit(w[(loss, C2, np.inf)])
        assert w[(loss, 1e-300, BIG)] == 0.0                             # a weight that underflows to 0
        assert all(0.0 <= v <= 1.0 for v in w.values())
    # Huber: 1 up to and on the threshold, below 1 one ulp over it -- by one rounding: no jump at the threshold
    assert w[(R.HUBER, C2, C2)] == 1.0 and w[(R.HUBER, C2, below(C2))] == 1.0 and 1.0 - 2.0 ** -52 <= w[(R.HUBER, C2, above(C2))] <= 1.0
    assert w[(R.CAUCHY, C2, C2)] == 0.5 and abs(w[(R.CAUCHY, C2, below(C2))] - 0.5) < 1e-15 and abs(w[(R.CAUCHY, C2, above(C2))] - 0.5) < 1e-15


def test_effective_variance_bit_for_bit(harness, tmp_path):
    rows = []
    for v in (1e-8, 0.0025, 9.0, 1e8, below(1e8)):
        for w in (1.0, 0.5, 3e-3, TINY, 0.0, below(1.0), v / 1e8, below(v / 1e8), above(v / 1e8), 1e-300):
            rows.append([v, w])
    rows += [[0.5e8, 0.5], [below(0.5e8), 0.5], [above(0.5e8), 0.5]]     # v / w just under 1e8, on it and over it
    rows = np.array(rows)
    got = harness("vars", rows, tmp_path)
    want = R.effective_var(rows[:, :1], rows[:, 1])[:, 0]
    assert same(got, want)
    assert got[-3] == 1e8 and got[-2] == below(1e8) and got[-1] == 1e8
    rule = rows[:, 1] <= 1.0                                             # the weights the rule can give
    assert ((got >= rows[:, 0]) & (got <= 1e8) & (got >= 1e-8))[rule].all()      # usable in, usable out: no row changes its availability
    assert same(got[rows[:, 1] == 1.0], rows[rows[:, 1] == 1.0, 0])     # a weight of 1 returns the given variance's bits


def test_residual_and_u2_bit_for_bit(harness, tmp_path):
    rng = np.random.default_rng(4)
    n = 400
    zr, xr = rng.normal(0, 300.0, (n, 3)), rng.normal(0, 300.0, (n, 3))
    e = np.where(rng.random((n, 1)) < 0.3, 0.0, rng.normal(0, 0.5, (n, 3)))
    v = 10.0 ** rng.uniform(-8, 8, (n, 3))
    zr[:3] = xr[:3] + e[:3]                                              # a residual of (nearly) 0
    zr[3], v[3] = 1e200, 1e-8                                            # u2 = +inf
    zr[4] = np.inf
    loss = rng.integers(0, 2, n).astype(float)
    rows = np.column_stack((loss, np.full(n, C2), zr, xr, e, v))
    got = harness("rows", rows, tmp_path).reshape(n, 5)
    res = zr - (xr + e)
    with np.errstate(invalid="ignore", over="ignore"):
        u2 = R.u2_of(res, v)
        w = np.where(loss == R.CAUCHY, R.weight_of(R.CAUCHY, u2, C2), R.weight_of(R.HUBER, u2, C2))
    assert same(got[:, :3], res) and same(got[:, 3], u2) and same(got[:, 4], w)
    assert np.isinf(u2[3]) and w[3] == 0.0 and (w[:3] == 1.0).all()


def test_fixed_point_rule_and_argument_checks(harness, tmp_path):
    nan2 = np.frombuffer(np.uint64(0x7ff8000000000001).tobytes(), np.float64)[0]
    pairs = np.array([[1.0, 1.0], [1.0, below(1.0)], [0.0, -0.0], [0.5, 0.5], [np.nan, np.nan], [np.nan, nan2], [0.0, 0.0], [TINY, 0.0]])
    got = harness("fixed", pairs, tmp_path, np.int32)
    assert got.tolist() == R.same_bits(pairs[:, 0], pairs[:, 1]).astype(int).tolist() == [1, 0, 0, 1, 1, 0, 1, 0]
    args = np.array([[0, C2, 0], [1, C2, 32], [0, C2, 33], [0, C2, -1], [2, C2, 5], [-1, C2, 5], [0, 0.0, 5], [0, -1.0, 5], [0, np.inf, 5], [0, np.nan, 5],
                     [1, TINY, 5], [1, BIG, 5]], float)
    assert harness("args", args, tmp_path, np.int32).tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ 4. the library's surface
def test_library_exports_the_entry_as_declared():
    from gps_optimize_slam_amd import _lib
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    L = C.CDLL(_lib.library_path())                                     # loads without a device
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsf.h")).read(), flags=re.S)
    kinds = {"gsf_ctx *": C.c_void_p, "const double *": C.c_void_p, "double *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p,
             "const int64_t *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t *": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32,
             "double": C.c_double, "const gsf_ekf_config *": C.POINTER(_lib.EkfConfig)}
    name = "gsf_ekf_smooth_reweighted_dev"
    names = ["ctx", "ts", "pos", "quat", "gps", "valid", "meas_var", "offsets", "init_pos", "init_quat", "run_status", "cfg", "B", "loss", "c2", "rounds",
             "pos_out", "quat_out", "cov_out", "pos_filt", "cov_filt", "pose_flags", "status", "nis", "weight", "rounds_used", "w_change"]
    assert hasattr(L, name) and not hasattr(L, name[:-4]) and name[:-4] not in _lib.SIGNATURES      # device form only
    m = re.search(r"GSF_API int " + name + r"\s*\(([^;]*)\);", src)
    assert m, name
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == names
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [kinds[re.sub(r"\w+$", "", p).strip()] for p in params]
    assert re.search(r"#define\s+GSF_REWEIGHT_HUBER\s+0\b", src) and re.search(r"#define\s+GSF_REWEIGHT_CAUCHY\s+1\b", src)
    assert (_lib.REWEIGHT_HUBER, _lib.REWEIGHT_CAUCHY, _lib.REWEIGHT_MAX_ROUNDS) == (R.HUBER, R.CAUCHY, R.MAX_ROUNDS) == (0, 1, 32)
    assert re.search(r"#define\s+GSF_ABI_VERSION\s+1\b", src)
    core = open(os.path.join(ROOT, "gps_optimize_slam_amd", "csrc", "gsf_reweight_core.hpp")).read()
    assert re.search(r"REWEIGHT_HUBER\s*=\s*0,\s*REWEIGHT_CAUCHY\s*=\s*1\b", core) and re.search(r"REWEIGHT_MAX_ROUNDS\s*=\s*32\b", core)


def test_reweighted_track_places_its_pieces():
    import torch
    from gps_optimize_slam_amd import batch
    rng = np.random.default_rng(0)
    t = lambda *shape: torch.as_tensor(rng.uniform(0.1, 1, shape))
    nan = float("nan")
    weight = torch.tensor([nan, 1.0, 0.25, nan, 0.0], dtype=torch.float64)
    mv = torch.tensor([[1.0, 2.0, 4.0]] * 4 + [[1e-8, 1.0, 1e8]], dtype=torch.float64)
    rt = batch.ReweightedTrack(t(5, 3), t(5, 4), t(5, 7), None, None, torch.tensor([16, 1, 1, 2, 1], dtype=torch.uint8), torch.zeros(2, dtype=torch.int32),
                               torch.tensor([0, 3, 5]), None, weight, torch.tensor([2, 0], dtype=torch.int32), torch.tensor([0.1, 0.0]), mv)
    assert isinstance(rt, batch.WeightedTrack)
    assert rt.downweighted().tolist() == [False, False, True, False, True] and rt.downweighted(below=0.2).tolist() == [False, False, False, False, True]
    assert rt.effective_var().tolist() == [[1.0, 2.0, 4.0], [1.0, 2.0, 4.0], [4.0, 8.0, 16.0], [1.0, 2.0, 4.0], [1e8, 1e8, 1e8]]
    for kw in (dict(loss="tukey"), dict(c2=0.0), dict(c2=float("inf")), dict(c2=float("nan")), dict(rounds=33), dict(rounds=-1), dict(rounds=2.5)):
        with pytest.raises(ValueError):                                  # refused before anything is touched
            batch.ekf_smooth_reweighted_ragged(*[None] * 8, **kw)


# ------------------------------------------------------------------------------------------------ 5. the objective, the motivation
def test_the_huber_objective_does_not_rise():
    cfg = R.one_span(full_cfg({}))
    for seed in range(3):
        t = R.motivation(seed, 271)
        r = R.reweight_restate(*t[:5], t[7], t[5], t[6], cfg, R.HUBER, C2, 8)
        J = [R.objective(h["sol"], t[3], t[5], r["given"], cfg, C2) for h in r["history"]]
        assert len(J) == 9
        for a, b in zip(J[:-1], J[1:]):
            assert b <= a * (1.0 + 1e-12), (seed, J)
        assert J[-1] < 0.1 * J[0]
        print(f"seed {seed}: Huber objective over the rounds: " + " ".join(f"{v:.6g}" for v in J))


def test_reweighting_beats_the_weighted_smoother_on_planted_outliers():
    cfg = full_cfg({})
    for seed in range(3):
        ts, pos, quat, aligned, valid, ip, iq, mv, truth, rows = R.motivation(seed, 271)
        plain = rmse(W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)["xs"], truth)
        figures = {name: rmse(R.reweight_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg, loss, C2, 8)["xs"], truth) for name, loss in R.LOSSES.items()}
        clean = rmse(W.weighted_restate(*W.motivation_track(seed, 271)[:5], mv, ip, iq, cfg)["xs"], truth)
        print(f"seed {seed}: RMSE against the truth, smoothed: weighted {plain:.3f} m, Huber rounds {figures['huber']:.3f} m, Cauchy rounds {figures['cauchy']:.4f} m; "
              f"the same track without the {int(rows.sum())} outliers {clean:.4f} m")
        for name, v in figures.items():
            assert v < plain, (seed, name, v, plain)
