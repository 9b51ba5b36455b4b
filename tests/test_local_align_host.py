"""CPU tier of the local Sim3 alignment (gsf_sim3_local_fit_dev / gsf_sim3_local_apply_dev; definitions in include/gsf.h).

tests/local_align_ref.py restates the feature pose by pose and knot by knot in NumPy.  gsf_local_core.hpp -- grid, window bounds, row rule,
the knot's closed form and validity, neighbour tables, weight, blend -- is compiled with g++ into a stand-alone program
(tests/host_harness_local.cpp), once plain and once under the address and undefined-behaviour sanitizers, and run on the cases of the GPU
tier: every index and flag must be the restatement's, the blended rows under fed knots must be its bits, and the program's knots are
held to the 50-digit yardsticks under the bounds of a shifted reduction.  The restatement's own knots are held to tests/sim3_ref.py's
yardstick (mode 1) and to the mode-0 bound written down in tests/local_align_ref.py.  The struct and the flag values are checked against
the header, and on a drifting track the feature does what it is for: the locally aligned track lies closer to the fixes than the globally
aligned one, and the oracle's filter fed the local track dead-reckons a 30 s outage with a smaller end error.
tests/test_local_align.py compares the kernels with the same restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import local_align_ref as R
import sim3_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KMAX = 8


# ------------------------------------------------------------------------------------------------ 1. the header, compiled for the host
def _hex(v):
    v = float(v)
    return "nan" if v != v else v.hex()


def _case_file(path, mode, Kmax):
    tracks, ref = R.gpu_tracks(), R.reference(mode, Kmax)
    with open(path, "w") as f:
        f.write(f"{len(tracks)} {Kmax} {mode} {R.MIN_ROWS} {_hex(R.SPACING)} {_hex(R.HALF_WINDOW)} {_hex(R.ROT_OPEN)} {_hex(R.RATIO_MAX)}\n")
        for tr, (fit, _) in zip(tracks, ref):
            f.write(f"{len(tr['ts'])} " + " ".join(_hex(v) for v in list(tr["R"].reshape(9)) + list(tr["t"]) + [tr["s"]]) + f" {fit['K']} {fit['status']}\n")
            for kn in fit["knots"]:
                f.write(f"{kn['flags']} " + " ".join(_hex(v) for v in list(np.asarray(kn["R"]).reshape(9)) + list(kn["t"]) + [kn["s"]]) + "\n")
            for i in range(len(tr["ts"])):
                row = [tr["ts"][i], *tr["pos"][i], *tr["quat"][i], *tr["gps"][i]]
                f.write(" ".join(_hex(v) for v in row) + f" {int(tr['valid'][i])}\n")


def _build(flags, tag):
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, f"host_harness_local{tag}")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HERE, "host_harness_local.cpp")])
    return exe


def _run(exe, mode, Kmax, tag):
    path = os.path.join(HERE, "_build", f"local_cases_{mode}_{Kmax}{tag}.txt")
    _case_file(path, mode, Kmax)
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), (p.stdout[-400:], p.stderr[-2000:])
    return [l.split() for l in p.stdout.splitlines()]


def _f(tok):
    return float.fromhex(tok) if "nan" not in tok else float("nan")


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def _compare(lines, mode, Kmax):
    """every line of the program against the restatement -> counts for the log"""
    tracks, ref = R.gpu_tracks(), R.reference(mode, Kmax)
    T = {int(l[1]): l for l in lines if l[0] == "T"}
    W = {(int(l[1]), int(l[2])): l for l in lines if l[0] == "W"}
    P = {(int(l[1]), int(l[2])): l for l in lines if l[0] == "P"}
    assert len(T) == len(tracks) and len(P) == sum(len(t["ts"]) for t in tracks)
    worst = dict(R=0.0, s=0.0, img=0.0, s0=0.0)
    n_knots = n_bits = 0
    for b, (tr, (fit, bl)) in enumerate(zip(tracks, ref)):
        assert (int(T[b][2]), int(T[b][3])) == (fit["status"], fit["K"]), tr["name"]
        ok = R.usable(tr["gps"], tr["valid"]) if len(tr["ts"]) else None
        for k, kn in enumerate(fit["knots"]):
            l = W[(b, k)]
            inwin = np.flatnonzero(R.window(tr["ts"], R.tau(float(tr["ts"][0]), R.SPACING, k), R.HALF_WINDOW))
            lo, hi = (int(inwin[0]), int(inwin[-1]) + 1) if inwin.size else (int(l[3]), int(l[3]))
            assert inwin.size == hi - lo                                     # (sorted stamps: a window is a run of rows)
            assert (int(l[3]), int(l[4])) == (lo, hi), (tr["name"], k)
            rows = np.flatnonzero(kn["rows"])
            assert int(l[5]) == (int(rows[0]) if rows.size else -1), (tr["name"], k)
            assert (int(l[6]), int(l[7])) == (kn["n"], kn["flags"]), (tr["name"], k, l[6:8])
            n_knots += 1
            if kn["flags"] & R.KNOT_INVALID:
                assert all("nan" in t for t in l[8:21]), (tr["name"], k)
                continue
            Rk, tk, sk = np.array([_f(t) for t in l[8:17]]).reshape(3, 3), np.array([_f(t) for t in l[17:20]]), _f(l[20])
            src, fix = tr["pos"][kn["rows"]], tr["gps"][kn["rows"]]
            if mode == R.LOC_SIM3 and not kn["flags"] & R.KNOT_ROT_FALLBACK:      # the program's knot against the 50-digit closed form, shifted bounds
                y = SR.yardstick(src, fix)
                assert y.cls == "determined" and y.status == 0, (tr["name"], k, y.cls)
                for key, v in SR.ratios(y, src, fix, None, Rk, tk, sk, shifted=True).items():
                    worst[key] = max(worst[key], v)
                    assert v <= SR.gate_of(key), (tr["name"], k, key, v)
            else:
                y0 = R.scale_yardstick(src, fix, tr["R"])
                v = abs(sk - y0.s) / (y0.b0_shift * y0.s)
                worst["s0"] = max(worst["s0"], v)
                assert v <= R.C_S0, (tr["name"], k, v)
                assert _same_bits(Rk, tr["R"]), (tr["name"], k)              # mode 0: the global rotation itself
        for i in range(len(tr["ts"])):
            l = P[(b, i)]
            if fit["status"]:
                assert int(l[6]) == R.LP_TRACK and all("nan" in t for t in l[8:16])
                continue
            got = (int(l[3]), int(l[4]), int(l[5]), int(l[6]))
            assert got == (int(bl["cell"][i]), int(bl["L"][i]), int(bl["Rr"][i]), int(bl["flags"][i])), (tr["name"], i, got)
            vals = np.array([_f(t) for t in l[7:16]])
            want = np.concatenate([[bl["w"][i]], bl["pos"][i], bl["quat"][i], [bl["scale"][i]]])
            assert _same_bits(vals, want), (tr["name"], i, vals.tolist(), want.tolist())
            n_bits += 1
    return n_knots, n_bits, worst


@pytest.fixture(scope="module")
def plain_exe():
    return _build(["-O2"], "")


@pytest.mark.parametrize("mode,Kmax", [(R.LOC_SCALE, KMAX), (R.LOC_SIM3, KMAX), (R.LOC_SCALE, KMAX - 1)])
def test_core_header_against_the_restatement(plain_exe, mode, Kmax):
    """indices and flags exactly, blended rows to the last bit (fed knots: the restatement's), the program's own knots inside the gates"""
    n_knots, n_bits, worst = _compare(_run(plain_exe, mode, Kmax, ""), mode, Kmax)
    print(f"mode {mode}, Kmax {Kmax}: {n_knots} knots and {n_bits} blended poses equal; worst ratio to the shifted bounds R {worst['R']:.2f} "
          f"s {worst['s']:.2f} image {worst['img']:.2f} (gates {SR.C_R:.0f} / {SR.C_S:.0f} / {SR.C_IMG:.0f}), mode-0 scale {worst['s0']:.2f} (gate {R.C_S0:.1f})")
    assert n_knots > 40 and (n_bits > 1500 or Kmax < KMAX)


def test_core_header_under_sanitizers():
    """the same stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into python)"""
    exe = _build(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "_san")
    for mode in (R.LOC_SCALE, R.LOC_SIM3):
        _compare(_run(exe, mode, KMAX, "_san"), mode, KMAX)


# ------------------------------------------------------------------------------------------------ 2. the restatement against the yardsticks
def test_restatement_knots_against_the_yardstick():
    """every valid knot of the shared cases: mode 1 inside C x bound of tests/sim3_ref.py, the mode-0 scale inside C_S0 x b0; the worst
    mode-0 ratio printed here is the figure in the header of tests/local_align_ref.py (C_S0 = 8 x it)"""
    worst, at = dict(R=0.0, s=0.0, img=0.0), None
    worst0, n0, n1 = 0.0, 0, 0
    for tr, mode in R.host_cases():
        fit = R.reference(mode, KMAX)[[t["name"] for t in R.gpu_tracks()].index(tr["name"])][0]
        assert R.clear_of_switches(fit, mode, s_global=tr["s"]), (tr["name"], mode)
        for k, kn in enumerate(fit["knots"]):
            if kn["flags"] & R.KNOT_INVALID:
                continue
            src, fix = tr["pos"][kn["rows"]], tr["gps"][kn["rows"]]
            if mode == R.LOC_SIM3 and not kn["flags"] & R.KNOT_ROT_FALLBACK:
                y = SR.yardstick(src, fix)
                assert y.cls == "determined" and y.status == 0
                for key, v in SR.ratios(y, src, fix, None, kn["R"], kn["t"], kn["s"]).items():
                    worst[key] = max(worst[key], v)
                    assert v <= SR.gate_of(key), (tr["name"], k, key, v)
                n1 += 1
            else:
                y0 = R.scale_yardstick(src, fix, tr["R"])
                v = abs(kn["s"] - y0.s) / (y0.b0 * y0.s)
                if v > worst0:
                    worst0, at = v, (tr["name"], k)
                assert v <= R.C_S0, (tr["name"], k, v)
                n0 += 1
    print(f"{n1} mode-1 knots: worst ratio R {worst['R']:.2f} s {worst['s']:.2f} image {worst['img']:.2f}; {n0} mode-0 scales: worst ratio {worst0:.2f} at {at}")
    assert n0 > 60 and n1 > 50
    assert worst0 <= R.MEASURED_WORST_S0                                     # the header's figure is the measured one


def test_cases_hold_what_the_gpu_tier_needs():
    names = [t["name"] for t in R.gpu_tracks()]
    assert sorted({len(t["ts"]) for t in R.gpu_tracks()}) == [0, 1, 2, 3, 63, 64, 65, 130, 271]
    r0, r1, r7 = R.reference(R.LOC_SCALE, KMAX), R.reference(R.LOC_SIM3, KMAX), R.reference(R.LOC_SCALE, KMAX - 1)
    by = lambda ref, name: ref[names.index(name)]
    # a row exactly on either bound is inside, its neighbour one ulp further out is not
    tr, (fit, _) = R.track("len130_on_the_bound"), by(r0, "len130_on_the_bound")
    rows = fit["knots"][1]["rows"]
    assert rows[8] and rows[72] and not rows[7] and not rows[73]
    assert tr["ts"][8] - 4.0 == -R.HALF_WINDOW and tr["ts"][72] - 4.0 == R.HALF_WINDOW
    sizes = {kn["n"] for f, _ in r0 for kn in f["knots"]}
    assert {63, 64, 65} <= sizes                                            # windows on both sides of the wave boundary
    assert all(kn["flags"] == R.KNOT_FEW for kn in by(r0, "len65_no_usable_row")[0]["knots"])
    assert (by(r0, "len65_no_usable_row")[1]["flags"] == R.LP_GLOBAL).all()
    f, b = by(r0, "len271_usable_rows_stop")
    assert [kn["flags"] & R.KNOT_INVALID != 0 for kn in f["knots"]] == [False, False, False, True, True, True, False, False]
    assert (b["flags"] & R.LP_BRIDGED).any() and set(zip(b["L"][b["flags"] == R.LP_BRIDGED], b["Rr"][b["flags"] == R.LP_BRIDGED])) == {(2, 6)}
    f, b = by(r0, "len271_last_third")
    held = b["flags"] == R.LP_HELD
    assert held.any() and (b["L"][held] == -1).all() and (b["Rr"][held] == 4).all()
    assert all(kn["flags"] == R.KNOT_ROT_FALLBACK for kn in by(r1, "len271_straight")[0]["knots"])
    assert all(kn["flags"] == 0 for kn in by(r1, "len271_curved")[0]["knots"])
    assert by(r0, "len130_zero_quat")[1]["flags"][41] & R.LP_BAD_QUAT and np.isnan(by(r0, "len130_zero_quat")[1]["quat"][41]).all()
    assert by(r0, "len65_unsorted")[0]["status"] == R.LOC_UNSORTED and by(r0, "len0")[0]["status"] == R.LOC_EMPTY
    assert by(r0, "len271_curved")[0]["K"] == KMAX and by(r7, "len271_curved")[0]["status"] == R.LOC_TOO_MANY and by(r7, "len130")[0]["status"] == 0
    assert by(r0, "len130_standstill")[0]["knots"][2]["flags"] == R.KNOT_VAR0 and by(r0, "len130_scale_jump")[0]["knots"][2]["flags"] == R.KNOT_SCALE
    assert R.track("len271_unix_south")["ts"][0] == 1.3e9 and abs(R.track("len271_unix_south")["gps"][0, 1] - SR.OFFSET_S[1]) < 500.0
    s = [kn["s"] for kn in by(r0, "len271_drifting")[0]["knots"]]
    assert 0.89 < s[-1] / s[0] < 0.93 and all(a > b_ for a, b_ in zip(s, s[1:]))      # the planted 10 % drift is what the knots see


# ------------------------------------------------------------------------------------------------ 3. the surface, without a device
def test_struct_layout_and_flag_values(tmp_path):
    from gps_optimize_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    core = open(os.path.join(ROOT, "gps_optimize_slam_amd", "csrc", "gsf_local_core.hpp")).read()
    cls, cname = _lib.LocalConfig, "gsf_local_config"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsf.h"', 'int main(void) {', f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {l.split()[0]: int(l.split()[1]) for l in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"] == C.sizeof(cls) == 40
    assert [f for f, _ in cls._fields_] == ["mode", "min_rows", "spacing", "half_window", "rot_open", "ratio_max"]
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    groups = (("LOC", ("EMPTY", "UNSORTED", "TOO_MANY", "SKIPPED")), ("KNOT", ("FEW", "VAR0", "SCALE", "ROT_FALLBACK")),
              ("LP", ("BRIDGED", "HELD", "GLOBAL", "BAD_QUAT", "TRACK")))
    for prefix, names in groups:
        for k, name in enumerate(names):
            assert re.search(rf"#define GSF_{prefix}_{name} {1 << k}\b", hdr), (prefix, name)
            assert getattr(_lib, f"{prefix}_{name}") == getattr(R, f"{prefix}_{name}") == 1 << k
            assert re.search(rf"\b{prefix}_{name} = {1 << k}\b", core), (prefix, name)
    for k, name in enumerate(("SCALE", "SIM3")):
        assert re.search(rf"#define GSF_LOC_{name} {k}\b", hdr) and getattr(_lib, f"LOC_{name}") == getattr(R, f"LOC_{name}") == k
    assert _lib.LOC_KMAX == R.LOC_KMAX == 4096 and re.search(r"\bLOC_KMAX = 4096\b", core)


def test_entries_are_declared_bound_and_exported():
    from gps_optimize_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    for name, n_args in (("gsf_sim3_local_fit_dev", 20), ("gsf_sim3_local_apply_dev", 21)):
        m = re.search(rf"GSF_API int {name}\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in include/gsf.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params) == n_args
        for p, a in zip(params, args):
            want = C.POINTER(_lib.LocalConfig) if "gsf_local_config" in p else (C.c_void_p if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}[p.split()[0]])
            assert a is want, (name, p, a)
        assert f"{name[:-4]}(" not in hdr                                    # device forms only
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    L = C.CDLL(_lib.library_path())
    assert hasattr(L, "gsf_sim3_local_fit_dev") and hasattr(L, "gsf_sim3_local_apply_dev")


def test_argument_errors():
    import torch
    from gps_optimize_slam_amd import batch as GB, ekfgpsslam as E
    P = 5
    f = lambda *s: torch.zeros(s, dtype=torch.float64)
    args = lambda: [f(P), f(P, 3), f(P, 4), f(P, 3), torch.zeros(P, dtype=torch.uint8), torch.tensor([0, P]), f(1, 9), f(1, 3), f(1)]
    for kw in (dict(mode="both"), dict(spacing=0.0), dict(spacing=float("nan")), dict(half_window=-1.0), dict(min_rows=1), dict(mode="sim3", min_rows=2),
               dict(ratio_max=0.5), dict(rot_open=-1.0), dict(max_knots=0), dict(max_knots=5000)):
        with pytest.raises(ValueError):                                      # (checked before anything that needs a device)
            GB.local_align_ragged(*args(), **kw)
    assert GB._local_config("scale", 8, 30.0, 30.0, 1e-3, 2.0).mode == 0 and GB._local_config("sim3", 8, 30.0, 30.0, 1e-3, 2.0).mode == 1
    with pytest.raises(ValueError):
        E.align_trajectory_local({"timestamps": np.zeros(3), "positions": np.zeros((3, 3)), "quaternions": np.zeros((3, 4))}, np.zeros((3, 3)),
                                 np.ones(3, bool), np.eye(3), np.zeros(3), 1.0, mode="neither")


# ------------------------------------------------------------------------------------------------ 4. it does what it is for
def test_local_alignment_follows_a_drifting_scale():
    """the restatement on the drifting case (271 poses, the scale falls by 10 % end to end): closer to the fixes than the global fit"""
    tr = R.track("len271_drifting")
    _, bl = R.reference(R.LOC_SCALE, KMAX)[[t["name"] for t in R.gpu_tracks()].index("len271_drifting")]
    glob = tr["s"] * tr["pos"] @ tr["R"].T + tr["t"]
    rmse = lambda p: float(np.sqrt(((p - tr["gps"]) ** 2).sum(1).mean()))
    print(f"drifting case: RMSE against the fixes {rmse(glob):.3f} m under the global Sim3, {rmse(bl['pos']):.3f} m locally aligned (ratio {rmse(bl['pos']) / rmse(glob):.3f})")
    assert rmse(bl["pos"]) < rmse(glob)


def test_oracle_filter_bridges_an_outage_better_on_the_local_track():
    """the oracle's apply_ekf_correction on a 90 s drifting track whose last 30 s have no fix: fed the locally aligned track as its motion
    source it ends closer to the withheld fix than fed the original track (whose increments carry no scale at all)"""
    from oracle import oracle as orc
    tr = R.motivation_track()
    n = len(tr["ts"])
    valid = tr["valid"].copy()
    valid[tr["ts"] > tr["ts"][-1] - 30.0] = 0
    fit = R.fit_track(tr["ts"], tr["pos"], tr["gps"], valid, tr["R"], tr["s"], mode=R.LOC_SCALE)
    Rk, tk, sk, _, _, fl = R.knot_arrays(fit, fit["K"])
    bl = R.blend_track(tr["ts"], tr["pos"], tr["quat"], tr["R"], tr["t"], tr["s"], Rk, tk, sk, fl, fit["K"], fit["status"])
    assert (bl["flags"][valid == 0] == R.LP_HELD).all()                      # the outage is bridged under the last knot that had fixes
    g0 = R.blend_track(tr["ts"][:1], tr["pos"][:1], tr["quat"][:1], tr["R"], tr["t"], tr["s"], Rk[:0], tk[:0], sk[:0], fl[:0], 0, 0)
    po, _ = orc.apply_ekf_correction_aligned(tr["ts"], tr["pos"], tr["quat"], tr["gps"], valid, g0["pos"][0], g0["quat"][0])
    pl, _ = orc.apply_ekf_correction_aligned(tr["ts"], bl["pos"], bl["quat"], tr["gps"], valid, bl["pos"][0], bl["quat"][0])
    e_o, e_l = float(np.linalg.norm(po[-1] - tr["gps"][-1])), float(np.linalg.norm(pl[-1] - tr["gps"][-1]))
    print(f"30 s outage at the end of {n} poses: end error {e_o:.2f} m on the original track, {e_l:.2f} m on the locally aligned one (ratio {e_l / e_o:.3f})")
    assert e_l < e_o
