"""CPU tier of the GNSS outage study (gsf_outage_study_dev; definitions in include/gsf.h).

tests/outage_study_ref.py restates the study the long way round: mask bytes cleared, the filter run pose by pose, the smoother as the
reference's backward recurrence -- no closed form.  Here its fused positions are pinned to the oracle's apply_ekf_correction on the same
cleared bytes (1e-6 m, the project's gate; both are float64 evaluations of the same recursion, so the difference is rounding at UTM
magnitudes, around 1e-9 m).  The GSF_HD helpers of gsf_outage_core.hpp -- window -> [a, b), the flag word, the closed form -- are compiled
into a stand-alone program with g++ and checked there against per-pose loops on all 2^10 availability patterns x all windows and against
the backward recurrence, once more under the address and undefined-behaviour sanitizers.  The bindings are checked without a device, and
on tracks drawn from the filter's own model the recovery NIS is consistent and the smoother takes drift back.
tests/test_outage_study.py compares the kernels with the same restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import noise_sweep_ref as NR
import outage_study_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = ("ts", "pos", "quat", "aligned", "valid", "init_pos", "init_quat")


# ------------------------------------------------------------------------------------------------ 1. restatement == oracle on cleared bytes
def test_restatement_agrees_with_the_oracle_on_cleared_mask_bytes(golden):
    """17 fixture tracks x the fixed scenario list.  On [a, b) the restatement's fused positions are the oracle's to 1e-6 m; before a the
    modified run IS the unmodified run, bit for bit, in the oracle and in the restatement.  (After the recovery the two runs differ --
    the recovery's gain saw a larger predicted variance -- and the difference decays over the following updates; the study reports
    nothing there.)"""
    from oracle import oracle as orc
    cases, _, _ = NR.fixture_cases(golden)
    assert len(cases) == 17
    worst, seen, n_scen, worst_after = 0.0, 0, 0, 0.0
    for c in cases:
        tr = [c[k] for k in KEYS]
        scen, tags = R.scenario_list(c["ts"], c["aligned"], c["valid"])
        base = orc.apply_ekf_correction_aligned(*tr, c["cfg"])[0]
        for (s, L), tag, r in zip(scen, tags, R.study(tr, scen, c["cfg"])):
            seen |= r["flags"]
            assert "empty" not in tag or r["flags"] == R.OS_EMPTY, (c["name"], tag, r["flags"])     # (a timed window of a very short track may be empty too)
            if r["flags"] & R.OS_EMPTY:
                assert (r["row"] == 0).all() and (r["seg"] == -1).all()
                continue
            n_scen += 1
            a, b = r["seg"]
            w0, w1 = r["W"]
            cleared = np.asarray(c["valid"]).astype(np.uint8).copy()
            cleared[w0:w1] = 0
            po = orc.apply_ekf_correction_aligned(tr[0], tr[1], tr[2], tr[3], cleared, tr[5], tr[6], c["cfg"])[0]
            worst = max(worst, float(np.abs(po[a:b] - r["p_fu"][a:b]).max()))
            assert np.array_equal(po[:a], base[:a]), (c["name"], tag)
            if b + 1 < len(po):
                worst_after = max(worst_after, float(np.abs(po[b + 1:] - base[b + 1:]).max()))
            # the flags describe what the oracle did: smoothed rows moved away from dead reckoning, sharp / unrecovered ones did not
            if r["flags"] & (R.OS_SHARP_TURN | R.OS_NO_RECOVERY):
                assert np.array_equal(r["p_fu"][a:b], r["p_dr"][a:b])
            assert r["row"][2] == b - a and a <= w0 < w1 <= b and bool(r["flags"] & R.OS_MERGED) == ((a, b) != (w0, w1))
            assert bool(r["flags"] & R.OS_FROM_START) == (a == 0) and bool(r["flags"] & R.OS_NO_RECOVERY) == (b == len(po))
    print(f"restatement vs oracle on cleared mask bytes, {n_scen} scenarios over {len(cases)} tracks: worst |dp| on [a, b) {worst:.2e} m; "
          f"modified vs unmodified run after the recovery: up to {worst_after:.2e} m")
    assert worst <= 1e-6
    want = R.OS_EMPTY | R.OS_NO_RECOVERY | R.OS_SMOOTHED | R.OS_SHARP_TURN | R.OS_MERGED | R.OS_FROM_START
    assert seen & want == want, seen


def test_unsorted_and_empty_tracks(golden):
    cases, _, _ = NR.fixture_cases(golden)
    c = next(c for c in cases if len(c["ts"]) >= 65)
    tr = [np.array(c[k], copy=True) for k in KEYS]
    tr[0][10], tr[0][11] = tr[0][11], tr[0][10]
    r = R.scenario(*tr, c["cfg"], 1.0, 2.0)
    assert r["flags"] == R.OS_UNSORTED and np.isnan(r["row"]).all() and (r["seg"] == -1).all()
    tr[0][10:12] = np.nan
    assert R.scenario(*tr, c["cfg"], 1.0, 2.0)["flags"] == R.OS_UNSORTED
    e = R.scenario(np.empty(0), np.empty((0, 3)), np.empty((0, 4)), np.empty((0, 3)), np.empty(0, bool), np.zeros(3), np.array([0, 0, 0, 1.0]),
                   c["cfg"], 0.0, 1.0)
    assert e["flags"] == R.OS_EMPTY and (e["row"] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the kernel's host/device helpers
def _build_and_run(flags, tag):
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, f"host_harness_outage{tag}")
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(HERE, "host_harness_outage.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout.strip())
    assert p.returncode == 0 and p.stdout.startswith("OK"), (p.stdout, p.stderr)


def test_core_helpers_against_per_pose_loops():
    _build_and_run(["-O2"], "")


def test_core_helpers_under_sanitizers():
    """the same stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into python)"""
    _build_and_run(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "_san")


# ------------------------------------------------------------------------------------------------ 3. the surface, without a device
def test_outage_scenarios_ordering():
    from gps_optimize_slam_amd import batch as GB
    sc = GB.outage_scenarios([0.0, 5.0, 10.0], [2.0, 8.0])
    assert sc.shape == (6, 2) and sc.dtype == np.float64
    np.testing.assert_array_equal(sc, [[0, 2], [5, 2], [10, 2], [0, 8], [5, 8], [10, 8]])      # length-major
    np.testing.assert_array_equal(GB.outage_scenarios(3.0, [1.0]), [[3.0, 1.0]])
    for bad in (([], [1.0]), ([0.0], []), (np.zeros(65), np.ones(64))):
        with pytest.raises(ValueError):
            GB.outage_scenarios(*bad)


def test_argument_errors():
    import torch
    from gps_optimize_slam_amd import batch as GB
    P = 5
    f = lambda *s: torch.zeros(s, dtype=torch.float64)
    args = lambda: [f(P), f(P, 3), f(P, 4), f(P, 3), torch.zeros(P, dtype=torch.uint8), torch.tensor([0, P]), f(1, 3), f(1, 4)]
    sc = np.array([[0.0, 1.0]])
    bad = []
    a = args(); a[1] = f(P, 2); bad.append((a, sc, {}))                                       # pos shape
    a = args(); a[4] = torch.zeros(P, dtype=torch.bool); bad.append((a, sc, {}))               # valid dtype
    a = args(); a[6] = f(2, 3); bad.append((a, sc, {}))                                       # init_pos rows
    bad.append((args(), np.zeros((3, 3)), {}))                                                 # scenarios shape
    bad.append((args(), np.zeros((0, 2)), {}))                                                 # K = 0
    bad.append((args(), np.zeros((4097, 2)), {}))                                              # K too large
    bad.append((args(), sc, dict(trace=1)))                                                    # trace names no scenario
    bad.append((args(), sc, dict(trace=-1)))
    bad.append((args(), sc, dict(truth=f(P, 3))))                                              # truth without truth_valid
    bad.append((args(), sc, dict(truth=f(P, 2), truth_valid=torch.zeros(P, dtype=torch.uint8))))
    bad.append((args(), sc, dict(run_status=torch.zeros(1, dtype=torch.int64))))
    for a, s, kw in bad:
        with pytest.raises((ValueError, TypeError)):
            GB.outage_study_ragged(*a, s, **kw)

    class Run:                                                                                  # a result without a ground-truth leg
        gt_aligned = gt_valid = None
    with pytest.raises(ValueError):
        GB.outage_study_fused(None, Run(), sc, truth="gt")
    with pytest.raises(ValueError):
        GB.outage_study_fused(None, Run(), sc, truth="other")


def test_curve_pools_the_usable_rows():
    """OutageStudy.curve() on hand-made rows (CPU tensors): per length, over the rows without EMPTY | UNSORTED | SKIPPED and with |E| > 0;
    NaN rows of a skipped track do not leak into any figure"""
    import torch
    from gps_optimize_slam_amd import batch as GB
    scen = torch.tensor([[0.0, 2.0], [5.0, 2.0], [0.0, 8.0]], dtype=torch.float64)
    st = torch.zeros((3, 3, 13), dtype=torch.float64)
    fl = torch.zeros((3, 3), dtype=torch.int32)
    st[0, 0, [0, 3, 4, 5, 6, 7, 8, 12]] = torch.tensor([4.0, 2.0, 10.0, 16.0, 3.0, 4.0, 1.5, 2.0], dtype=torch.float64); fl[0, 0] = R.OS_SMOOTHED
    st[0, 1, [0, 3, 4, 5, 6, 7, 8, 12]] = torch.tensor([2.0, 4.0, 20.0, 8.0, 2.5, 8.0, 2.5, 4.0], dtype=torch.float64); fl[0, 1] = R.OS_SHARP_TURN
    st[0, 2, [0, 3, 4, 5, 6, 7, 8]] = torch.tensor([5.0, 8.0, 40.0, 45.0, 4.0, 45.0, 4.0], dtype=torch.float64); fl[0, 2] = R.OS_NO_RECOVERY
    st[0, 2, 11:] = float("nan")
    st[1] = float("nan"); fl[1] = R.OS_SKIPPED
    fl[2] = R.OS_EMPTY                                                   # rows of zeros
    st[2, 1, 0] = 0.0
    cv = GB.OutageStudy(stats=st, flags=fl, scenarios=scen).curve()
    assert cv["length"].tolist() == [2.0, 8.0] and cv["rows"].tolist() == [2.0, 1.0]
    np.testing.assert_allclose(cv["rms_dr"].numpy(), [np.sqrt(24.0 / 6.0), 3.0])
    np.testing.assert_allclose(cv["rms_fused"].numpy(), [np.sqrt(12.0 / 6.0), 3.0])
    assert cv["max_dr"].tolist() == [3.0, 4.0] and cv["max_fused"].tolist() == [2.5, 4.0]
    assert cv["mean_gap"].tolist() == [3.0, 8.0] and cv["mean_dist"].tolist() == [15.0, 40.0]
    assert cv["mean_recovery_nis"][0].item() == 3.0 and np.isnan(cv["mean_recovery_nis"][1].item())
    assert cv["share_smoothed"].tolist() == [0.5, 0.0] and cv["share_sharp"].tolist() == [0.5, 0.0]


def test_entry_is_declared_bound_and_exported():
    from gps_optimize_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    m = re.search(r"GSF_API int gsf_outage_study_dev\(([^;]*)\);", hdr)
    assert m, "gsf_outage_study_dev is not declared in include/gsf.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["gsf_outage_study_dev"]
    assert res is C.c_int and len(args) == len(params) == 23
    for p, a in zip(params, args):
        want = C.POINTER(_lib.EkfConfig) if "gsf_ekf_config" in p else (C.c_void_p if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}[p.split()[0]])
        assert a is want, (p, a)
    assert "gsf_outage_study(" not in hdr                                   # device form only
    names = ("EMPTY", "NO_RECOVERY", "SMOOTHED", "SHARP_TURN", "MERGED", "FROM_START", "UNSORTED", "SKIPPED")
    for k, name in enumerate(names):
        assert re.search(rf"#define GSF_OS_{name} {1 << k}\b", hdr), name
        assert getattr(_lib, f"OS_{name}") == getattr(R, f"OS_{name}") == 1 << k
    core = open(os.path.join(ROOT, "gps_optimize_slam_amd", "csrc", "gsf_outage_core.hpp")).read()
    for k, name in enumerate(names):
        assert re.search(rf"\bOS_{name} = {1 << k}\b", core), name
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    assert hasattr(C.CDLL(_lib.library_path()), "gsf_outage_study_dev")


# ------------------------------------------------------------------------------------------------ 4. planted sanity
def test_planted_recovery_nis_is_consistent_and_smoothing_helps():
    """noise_sweep_ref.planted_batch, seeds 0-7: tracks drawn from the filter's own model.  Windows of 6, 12 and 9 poses starting at poses
    14, 30 and 48 of every track.  A consistent filter has a recovery NIS of mean 3 and variance 6 (chi-square, 3 degrees of freedom), so
    the pooled mean over M recoveries lies within 3 +- 4 sqrt(6 / M); and the smoother must take drift back: pooled rms_fused < rms_dr."""
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    nis, sq_dr, sq_fu, nE = [], 0.0, 0.0, 0
    for seed in range(8):
        for tr in NR.planted_batch(cfg, seed):
            scen = np.array([R.pose_window(tr[0], i0, cnt) for i0, cnt in ((14, 6), (30, 12), (48, 9))])
            for r in R.study(tr, scen, cfg):
                assert not r["flags"] & (R.OS_EMPTY | R.OS_NO_RECOVERY | R.OS_UNSORTED)
                nis.append(r["row"][12]); sq_dr += r["row"][5]; sq_fu += r["row"][7]; nE += int(r["row"][0])
    M = len(nis)
    mean, tol = float(np.mean(nis)), 4.0 * np.sqrt(6.0 / M)
    rms_dr, rms_fu = np.sqrt(sq_dr / nE), np.sqrt(sq_fu / nE)
    print(f"planted: {M} recoveries, mean NIS {mean:.3f} (3 +- {tol:.3f}); pooled rms over {nE} poses: dead-reckoned {rms_dr:.3f} m, fused {rms_fu:.3f} m")
    assert M == 384 and abs(mean - 3.0) <= tol
    assert rms_fu < rms_dr
