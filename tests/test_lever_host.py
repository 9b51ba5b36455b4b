"""CPU tier of the antenna lever arm (gsf_lever_fit_dev / gsf_lever_apply_dev; definitions in include/gsf.h).

tests/lever_ref.py restates the feature row by row in NumPy and, with the same code in 50 digits, provides the yardstick of the same
iteration.  gsf_lever_core.hpp -- row rule, the 49 sums of a round, the normal equations, the scaled Cholesky, the rotation update, the
flags, the apply -- is compiled with g++ into a stand-alone program (tests/host_harness_lever.cpp), once plain and once under the address
and undefined-behaviour sanitizers, and run on the cases of the GPU tier under every switch combination: flags, counts and the first usable
row must be the restatement's, flagged tracks return their starting bytes, the apply under fed (R, l) is the restatement's bits, and the
program's fits are held to the yardstick under the bounds and gates of tests/lever_ref.py.  The restatement itself is held to the same
yardstick, and its worst ratio is the figure the gates are derived from.  The struct and the flag values are checked against the header,
and the feature does what it is for: the yardstick recovers a planted lever arm, and the oracle's filter fed de-levered fixes lies closer
to the true camera track than fed the raw ones.  tests/test_lever_gpu.py compares the kernels with the same restatement."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lever_ref as V

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L_FED, SIGN_FED = np.array([-0.3, 0.2, -1.1]), -1.0


# ------------------------------------------------------------------------------------------------ 1. the header, compiled for the host
def _hex(v):
    v = float(v)
    return "nan" if v != v else v.hex()


def _case_file(path, cname):
    tracks, cfg = V.gpu_tracks(), V.configs()[cname]
    with open(path, "w") as f:
        f.write(f"{len(tracks)} " + " ".join(_hex(v) for v in [cfg["sigma_fix"], *cfg["sigma_prior"], cfg["sigma_rot"], cfg["ratio_max"], cfg["pivot_min"],
                                                                 cfg["weak_ratio"], cfg["conv_tol"]])
                + f" {cfg['min_rows']} {cfg['iters']} {cfg['fit_scale']} {cfg['fit_rotation']}\n")
        for tr in tracks:
            n = len(tr["valid"])
            f.write(f"{n} {tr['run_status']} " + " ".join(_hex(v) for v in [*tr["R"].reshape(9), *tr["t"], tr["s"], *tr["l0"], *L_FED, SIGN_FED]) + "\n")
            for i in range(n):
                f.write(" ".join(_hex(v) for v in [*tr["pos"][i], *tr["quat"][i], *tr["gps"][i]]) + f" {int(tr['valid'][i])}\n")


def _build(flags, tag):
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, f"host_harness_lever{tag}")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HERE, "host_harness_lever.cpp")])
    return exe


def _run(exe, cname, tag):
    path = os.path.join(HERE, "_build", f"lever_cases_{cname}{tag}.txt")
    _case_file(path, cname)
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), (p.stdout[-400:], p.stderr[-2000:])
    return [l.split() for l in p.stdout.splitlines()]


def _f(tok):
    return float.fromhex(tok) if "nan" not in tok else float("nan")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def check_fit(name, cname, ref, got, worst):
    """one track's outputs `got` = dict(flags, n_rows, n_bad_quat, R (9,), t, s, l, l_cov (9,), rms_before, rms_after, last_step) against the
    restatement's `ref` and the yardstick: what both tiers ask of a fit.  Updates worst (ratios to the bounds with C = 1)."""
    tr, cfg = V.track(name), V.configs()[cname]
    assert (got["flags"], got["n_rows"], got["n_bad_quat"]) == (ref["flags"], ref["n_rows"], ref["n_bad_quat"]), (name, cname, got["flags"], ref["flags"])
    if ref["flags"] & V.KEPT:                                               # the starting values, byte for byte
        assert _same_bits(got["R"], tr["R"].reshape(9)) and _same_bits(got["t"], tr["t"]) and _same_bits(got["s"], tr["s"]) and _same_bits(got["l"], tr["l0"]), (name, cname)
        assert _same_bits(got["l_cov"], np.diag(np.array(cfg["sigma_prior"]) ** 2).reshape(9)), (name, cname)
        assert _same_bits(got["rms_after"], got["rms_before"]) and math.isnan(got["last_step"]), (name, cname)
        if ref["n_rows"] >= 1:
            assert abs(got["rms_before"] - ref["rms_before"]) <= 1e-9 * max(ref["rms_before"], 1.0), (name, cname)
        else:
            assert math.isnan(got["rms_before"])
        return
    have_y = (name, cname) in V.YARDSTICK_CASES
    y = V.track_yardstick(name, cname) if have_y else ref
    # without a yardstick of its own (the other switch combinations): the restatement, which lies within the gate of the exact iterate
    # itself -- hence twice the gate
    factor = 1.0 if have_y else 2.0
    for key, v in V.ratios(y, tr, got["R"], got["t"], got["s"], got["l"], got["l_cov"]).items():
        if have_y:
            worst[key] = max(worst[key], v)
        assert v <= factor * V.GATE[key], (name, cname, key, v)
    b = V.bounds(y, tr)
    assert got["rms_after"] <= got["rms_before"] * (1.0 + V.GATE["l"]), (name, cname)
    # an RMS of residuals moves by no more than the residuals do: the bounds of l, s (times the extent) and t together
    tol = factor * (V.GATE["l"] * b["l"] + V.GATE["s"] * b["s"] / abs(y["s"]) * y["E"] + V.GATE["R"] * b["R"] * y["E"] + V.GATE["t"] * b["t"])
    assert abs(got["rms_after"] - y["rms_after"]) <= tol and abs(got["rms_before"] - y["rms_before"]) <= tol, (name, cname)
    assert got["last_step"] <= cfg["conv_tol"] or got["flags"] & V.NOT_CONVERGED


def _compare(lines, cname):
    tracks, ref = V.gpu_tracks(), V.reference(cname)
    F = {int(l[1]): l for l in lines if l[0] == "F"}
    A = {(int(l[1]), int(l[2])): l for l in lines if l[0] == "A"}
    Z = {(int(l[1]), int(l[2])): l for l in lines if l[0] == "Z"}
    assert len(F) == len(tracks) and len(A) == len(Z) == sum(len(t["valid"]) for t in tracks)
    worst, n_fit, n_rows = dict(l=0.0, s=0.0, R=0.0, t=0.0, cov=0.0), 0, 0
    for b, (tr, rf) in enumerate(zip(tracks, ref)):
        l = F[b]
        v = [_f(t) for t in l[6:]]
        got = dict(flags=int(l[2]), n_rows=int(l[3]), n_bad_quat=int(l[4]), R=np.array(v[0:9]), t=np.array(v[9:12]), s=v[12], l=np.array(v[13:16]),
                   l_cov=np.array(v[16:25]), rms_before=v[25], rms_after=v[26], last_step=v[27])
        assert int(l[5]) == rf["first"], tr["name"]
        check_fit(tr["name"], cname, rf, got, worst)
        n_fit += not rf["flags"] & V.KEPT
        # the apply under the fed (R, l): the restatement's bits; under l = 0: the fix's own bytes (a bad quaternion: a NaN row all the same)
        want, wfl = V.apply_track(tr["quat"], tr["gps"], tr["R"], L_FED, SIGN_FED)
        for i in range(len(tr["valid"])):
            a, z = A[(b, i)], Z[(b, i)]
            assert int(a[3]) == int(z[3]) == wfl[i], (tr["name"], i)
            assert _same_bits([_f(t) for t in a[4:7]], want[i]), (tr["name"], i, a[4:7], want[i].tolist())
            assert _same_bits([_f(t) for t in z[4:7]], tr["gps"][i] if not wfl[i] else [np.nan] * 3), (tr["name"], i)
            n_rows += 1
    return n_fit, n_rows, worst


@pytest.fixture(scope="module")
def plain_exe():
    return _build(["-O2"], "")


@pytest.mark.parametrize("cname", list(V.configs()))
def test_core_header_against_the_restatement(plain_exe, cname):
    """flags, counts, first usable row exactly; flagged tracks return their starting bytes; apply rows to the last bit; fits inside the gates"""
    n_fit, n_rows, worst = _compare(_run(plain_exe, cname, ""), cname)
    print(f"{cname}: {n_fit} fitted tracks, {n_rows} apply rows equal; worst ratio to the bounds (C = 1) l {worst['l']:.3f} s {worst['s']:.3f} R {worst['R']:.3f} "
          f"t {worst['t']:.3f} l_cov {worst['cov']:.3f} (gates {V.GATE['l']:.2f} / {V.GATE['s']:.2f} / {V.GATE['R']:.2f} / {V.GATE['t']:.2f})")
    assert n_fit >= 11 and n_rows > 2000


def test_core_header_under_sanitizers():
    """the same stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into python)"""
    exe = _build(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "_san")
    for cname in ("s1r1", "s0r0", "rot_free"):
        _compare(_run(exe, cname, "_san"), cname)


# ------------------------------------------------------------------------------------------------ 2. the restatement against the yardstick
@pytest.mark.parametrize("name,cname", V.YARDSTICK_CASES)
def test_restatement_against_the_yardstick(name, cname):
    """the float64 iteration against the same iteration in 50 digits: inside the gates, and no worse than the figures the gates come from"""
    ref = V.reference(cname)[[t["name"] for t in V.gpu_tracks()].index(name)]
    y = V.track_yardstick(name, cname)
    assert not ref["flags"] & V.KEPT and y["flags"] == ref["flags"] and y["n_rows"] == ref["n_rows"]
    r = V.ratios(y, V.track(name), ref["R"], ref["t"], ref["s"], ref["l"], ref["l_cov"])
    print(f"{name} {cname}: kappa {y['kappa']:.3g}, E {y['E']:.1f} m; ratios to the bounds (C = 1) l {r['l']:.4f} s {r['s']:.4f} R {r['R']:.4f} t {r['t']:.4f} l_cov {r['cov']:.4f}")
    for key, v in r.items():
        assert v <= V.MEASURED_WORST[key], (key, v)                        # the module's figures are the measured ones


def test_yardstick_recovers_the_planted_lever_arm():
    """no noise, all three axes observable, sigma_prior = 1e3: the iteration in 50 digits lands on the planted l.  What is left under the
    defaults is the rotation prior's pull (sigma_rot = 0.05 rad about a start that the lever arm itself bent) and four rounds of convergence.
    With sigma_rot = inf and 8 rounds only the prior's own shrinkage remains, weight (sigma_fix / 1e3)^2 against the data's information:
    |l| l_cov / 1e3^2 per axis -- that figure is the bound (twice it, plus 1e-10 m for the float64 rows of the generator)."""
    tr = V.track("len271_L3_noiseless")
    y = V.yardstick(tr, V.config(sigma_prior=(1e3,) * 3))
    e = float(np.abs(y["l"] - tr["l_true"]).max())
    y8 = V.yardstick(tr, V.config(sigma_prior=(1e3,) * 3, sigma_rot=math.inf, iters=8))
    e8 = float(np.abs(y8["l"] - tr["l_true"]).max())
    shrink = float(np.abs(tr["l_true"]).max() * np.abs(y8["l_cov"]).max() / 1e6)
    print(f"planted l {tr['l_true']}: residual {e:.3e} m under the defaults' rotation prior and 4 rounds; {e8:.3e} m with sigma_rot = inf and 8 rounds "
          f"(the prior's shrinkage: {shrink:.3e} m); s {y8['s']:.12f} against the planted {tr['s_true']}")
    assert y["flags"] == 0 and y8["flags"] == 0
    assert e < 0.02                                                         # 2 % of |l|: the rotation prior's pull, see above
    assert e8 <= 2 * shrink + 1e-10 and abs(y8["s"] - tr["s_true"]) < 1e-10


def test_cases_hold_what_the_gpu_tier_needs():
    names = [t["name"] for t in V.gpu_tracks()]
    assert sorted({len(t["valid"]) for t in V.gpu_tracks()}) == [0, 1, 2, 7, 8, 63, 64, 65, 72, 130, 271] and len(names) == 20
    for cname, cfg in V.configs().items():
        for tr, f in zip(V.gpu_tracks(), V.reference(cname)):
            assert V.clear_of_switches(f, cfg), (cname, tr["name"])
    r = {c: dict(zip(names, V.reference(c))) for c in V.configs()}
    d = r["s1r1"]
    assert all(not d[n]["flags"] & V.KEPT for n in V.FITTED)
    assert d["len7_few"]["flags"] & V.KEPT == V.FEW and d["len7_few"]["n_rows"] == 7 and d["len8_min_rows"]["n_rows"] == 8
    assert d["len0"]["flags"] & V.FEW and math.isnan(d["len0"]["rms_before"]) and d["len65_all_masked"]["n_rows"] == 0
    assert d["len130_standstill"]["flags"] & V.KEPT == V.VAR0
    assert d["len65_run_failed"]["flags"] & V.KEPT == V.TRACK and d["len65_run_failed"]["n_rows"] == 0
    assert d["len130_scale_jump"]["flags"] & V.KEPT == V.SCALE
    assert d["len130_bad_quats"]["n_bad_quat"] == 3 and d["len130_bad_quats"]["n_rows"] == 127
    assert d["len130_masked"]["first"] == 3 and d["len130_masked"]["n_rows"] == 110
    assert abs(V.track("len271_south")["gps"][0, 1] - 1e7) < 5e6 and V.track("len271_south")["gps"][0, 1] > 5e6
    # observability: a straight track observes nothing, a yaw-only L everything but the yaw axis, the wiggling L all three
    assert d["len271_straight"]["flags"] == V.WEAK and d["len130_yaw_L"]["flags"] == V.WEAK_Z and d["len271_L3"]["flags"] == 0
    assert d["len72_bend"]["flags"] == V.WEAK
    assert np.abs(d["len271_straight"]["l"]).max() <= V.GATE["l"] * V.bounds(d["len271_straight"], None)["l"]      # l stays at l0 = 0
    s = r["rot_free"]["len271_straight"]
    assert s["flags"] & V.KEPT == V.SINGULAR and s["min_pivot"] < 1e-12 and _same_bits(s["R"], V.track("len271_straight")["R"])
    for c in ("s1r0", "s0r0"):
        assert _same_bits(r[c]["len271_L3"]["R"], V.track("len271_L3")["R"])                                      # a pinned rotation is the start's bytes
    for c in ("s0r1", "s0r0"):
        assert r[c]["len271_L3"]["s"] == V.track("len271_L3")["s"]
    for n in ("len271_L3", "len271_south", "len130_masked", "len65"):                                                # the fit does what it is for
        assert d[n]["rms_after"] < d[n]["rms_before"] and np.abs(d[n]["l"] - V.track(n)["l_true"]).max() < 0.15, n


# ------------------------------------------------------------------------------------------------ 3. the surface, without a device
def test_struct_layout_and_flag_values(tmp_path):
    from gps_optimize_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    core = open(os.path.join(ROOT, "gps_optimize_slam_amd", "csrc", "gsf_lever_core.hpp")).read()
    cls, cname = _lib.LeverConfig, "gsf_lever_config"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsf.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {l.split()[0]: int(l.split()[1]) for l in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"] == C.sizeof(cls) == 9 * 8 + 4 * 4
    assert [f for f, _ in cls._fields_] == ["sigma_fix", "sigma_prior", "sigma_rot", "ratio_max", "pivot_min", "weak_ratio", "conv_tol", "min_rows", "iters",
                                             "fit_scale", "fit_rotation"]
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    for k, name in enumerate(("FEW", "VAR0", "SINGULAR", "SCALE", "WEAK_X", "WEAK_Y", "WEAK_Z", "NOT_CONVERGED", "TRACK")):
        assert re.search(rf"#define GSF_LEVER_{name} {1 << k}\b", hdr), name
        assert getattr(_lib, f"LEVER_{name}") == getattr(V, name) == 1 << k
        assert re.search(rf"\bLEVER_{name} = {1 << k}\b", core), name
    assert re.search(r"#define GSF_LVP_BAD_QUAT 1\b", hdr) and _lib.LVP_BAD_QUAT == V.LVP_BAD_QUAT == 1 and re.search(r"\bLVP_BAD_QUAT = 1\b", core)
    assert _lib.LEVER_KEPT == V.KEPT
    from gps_optimize_slam_amd import batch as GB
    c = GB._lever_config(0.5, (1.0, 1.0, 1.0), 0.05, True, True, 4, 8, 2.0, 1e-10, 0.5, 1e-6)                        # the Python defaults are the cases'
    for k, v in V.DEFAULTS.items():
        assert (tuple(getattr(c, k)) if k == "sigma_prior" else getattr(c, k)) == v, k


def test_entries_are_declared_bound_and_exported():
    from gps_optimize_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    for name, n_args in (("gsf_lever_fit_dev", 24), ("gsf_lever_apply_dev", 10)):
        m = re.search(rf"GSF_API int {name}\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in include/gsf.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params) == n_args
        for p, a in zip(params, args):
            want = C.POINTER(_lib.LeverConfig) if "gsf_lever_config" in p else (C.c_void_p if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}[p.split()[0]])
            assert a is want, (name, p, a)
        assert f"{name[:-4]}(" not in hdr                                    # device forms only
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    L = C.CDLL(_lib.library_path())
    assert hasattr(L, "gsf_lever_fit_dev") and hasattr(L, "gsf_lever_apply_dev")


def test_argument_errors():
    import torch
    from gps_optimize_slam_amd import batch as GB, ekfgpsslam as E
    P = 5
    f = lambda *s: torch.zeros(s, dtype=torch.float64)
    args = lambda: [f(P, 3), f(P, 4), f(P, 3), torch.zeros(P, dtype=torch.uint8), torch.tensor([0, P]), f(1, 9), f(1, 3), f(1)]
    for kw in (dict(sigma_fix=0.0), dict(sigma_fix=float("inf")), dict(sigma_prior=(1.0, 0.0, 1.0)), dict(sigma_prior=(1.0, 1.0)), dict(sigma_rot=-1.0),
               dict(iters=0), dict(iters=9), dict(min_rows=0), dict(ratio_max=0.5), dict(pivot_min=-1.0), dict(sigma_prior=float("nan"))):
        with pytest.raises(ValueError):                                      # (checked before anything that needs a device)
            GB.lever_fit_ragged(*args(), **kw)
    with pytest.raises(ValueError):
        GB.lever_apply_ragged(f(P, 4), f(P, 3), torch.tensor([0, P]), f(1, 9), f(1, 3), sign=0)
    with pytest.raises(ValueError):
        E.remove_lever_arm(np.zeros((3, 4)), np.zeros((3, 3)), np.eye(3), np.zeros(3), sign=2)
    with pytest.raises(ValueError):
        E.estimate_lever_arm({"positions": np.zeros((3, 3)), "quaternions": np.zeros((3, 4))}, np.zeros((3, 3)), np.ones(3, bool), np.eye(3), np.zeros(3), 1.0, iters=0)
    assert tuple(GB._lever_config(0.5, 2.0, float("inf"), False, True, 4, 8, 2.0, 1e-10, 0.5, 1e-6).sigma_prior) == (2.0, 2.0, 2.0)


# ------------------------------------------------------------------------------------------------ 4. it does what it is for
def motivation_by_hand(tr, fit):
    """the oracle's filter on the planted L with 0.1 m noise, fed the raw fixes under the plain Sim3 and the de-levered fixes under the
    fitted one -> RMSE of the two fused camera tracks against the TRUE camera positions"""
    from oracle import oracle as orc
    import local_align_ref as LR
    def fused(Rm, t, s, gps):
        p0 = s * tr["pos"][0] @ np.asarray(Rm).reshape(3, 3).T + t
        q0, _ = V.quat_unit_rows(tr["quat"][:1])
        q0 = LR._quat_mul(LR._quat_from_matrix(np.asarray(Rm).reshape(9)), tuple(q0[0]))
        po, _ = orc.apply_ekf_correction_aligned(tr["ts"], tr["pos"], tr["quat"], gps, tr["valid"], p0, np.array(q0))
        return po
    rmse = lambda p: float(np.sqrt(((p - tr["cam"]) ** 2).sum(1).mean()))
    gc, _ = V.apply_track(tr["quat"], tr["gps"], fit["R"], fit["l"], -1.0)
    return rmse(fused(tr["R"], tr["t"], tr["s"], tr["gps"])), rmse(fused(fit["R"], fit["t"], fit["s"], gc))


def test_oracle_filter_is_closer_to_the_camera_on_de_levered_fixes():
    tr = V.motivation_track()
    fit = V.fit_track(tr)
    assert fit["flags"] == 0
    plain, lever = motivation_by_hand(tr, fit)
    print(f"planted L, 0.1 m noise: fitted l {np.round(fit['l'], 3)} (planted {tr['l_true']}), rms {fit['rms_before']:.3f} -> {fit['rms_after']:.3f} m; oracle filter "
          f"against the true camera track: RMSE {plain:.3f} m on the raw fixes, {lever:.3f} m on the de-levered ones (ratio {lever / plain:.3f})")
    assert fit["rms_after"] < fit["rms_before"]
    assert lever < plain
