"""CPU tier of the pose-query entries (gsf_pose_query[_dev], gsf_georef_points[_dev]): the yardstick (tests/pose_query_ref.py) pinned to the
reference's quaternion_nlerp, the GSF_HD helpers the kernel calls (gsf_query_core.hpp, compiled with g++ as in test_cov_host.py) against the
yardstick on random tracks and on the edge cases of the GPU tier, the library's surface, and the Python wrappers' argument checks.
tests/test_pose_query.py compares the kernel with the same yardstick."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pose_query_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hq():
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libhost_harness_query.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_harness_query.cpp")])
    L = C.CDLL(so)
    L.hq_count_le.restype, L.hq_count_le.argtypes = C.c_int64, [f64p, C.c_int64, C.c_double]
    L.hq_count_le_i64.restype, L.hq_count_le_i64.argtypes = C.c_int64, [i64p, C.c_int64, C.c_int64]
    L.hq_track_unsorted.restype, L.hq_track_unsorted.argtypes = C.c_int, [f64p, C.c_int64]
    L.hq_query.restype = None
    L.hq_query.argtypes = [f64p, f64p, f64p, C.c_int64, C.c_int32, f64p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                           f64p, f64p, u8p, i32p]
    return L


def run_helpers(hq, c, points):
    """the whole batch through the harness, track by track -> the arrays the entries return (pose_flags are the kernel's own two loads)"""
    M = c["M"]
    a, q = np.full((M, 3), 7.0), np.full((M, 4), 7.0)
    flags, index = np.zeros(M, np.uint8), np.zeros(M, np.int32)
    state = ref.track_states(c["ts"], c["offsets"], c["run_status"], c["ext_q"] if points else None)
    for b in range(c["B"]):
        lo, hi, ql, qh = c["offsets"][b], c["offsets"][b + 1], c["q_offsets"][b], c["q_offsets"][b + 1]
        if qh == ql:
            continue
        pad = lambda v, cols: np.ascontiguousarray(v if len(v) else np.zeros((1, cols) if cols > 1 else 1))
        tau = np.ascontiguousarray(c["q_t"][ql:qh])
        ao, qo = np.empty((qh - ql, 3)), np.empty((qh - ql, 4))
        fo, io = np.empty(qh - ql, np.uint8), np.empty(qh - ql, np.int32)
        x = np.ascontiguousarray(c["x"][ql:qh]) if points else None
        eq = np.ascontiguousarray(c["ext_q"][b]) if points else None
        et = np.ascontiguousarray(c["ext_t"][b]) if points else None
        hq.hq_query(pad(c["ts"][lo:hi], 1), pad(c["pos"][lo:hi], 3), pad(c["quat"][lo:hi], 4), hi - lo, int(state[b]), tau, qh - ql, ref.MAX_GAP,
                    _ptr(x), _ptr(eq), _ptr(et), float(c["scale"][b]) if points else 1.0, ao, qo, fo, io)
        a[ql:qh], q[ql:qh], flags[ql:qh], index[ql:qh] = ao, qo, fo, io
    return a, q, flags, index, state


@pytest.fixture(scope="module")
def cases():
    c = ref.build_cases()
    want_q = ref.query(c["ts"], c["pos"], c["quat"], c["offsets"], c["q_t"], c["q_offsets"], c["pose_flags"], c["run_status"], ref.MAX_GAP)
    want_g = ref.georef(c["ts"], c["pos"], c["quat"], c["offsets"], c["q_t"], c["x"], c["q_offsets"], c["ext_q"], c["ext_t"], c["scale"],
                        c["pose_flags"], c["run_status"], ref.MAX_GAP)
    return c, want_q, want_g


# ------------------------------------------------------------------------------------------------ 1. the yardstick against the reference
def test_restated_nlerp_equals_the_reference(golden):
    g = golden("helper_cases.npz")
    for a, b, w, out in zip(g["nl_a"], g["nl_b"], g["nl_w"], g["nl_out"]):
        got = np.asarray(ref.nlerp(a, b, w), dtype=np.float64)
        assert np.abs(got - out).max() <= 10 * ref.EPS, (a, b, w)


def test_float64_formula_sits_well_inside_the_bounds():
    """plain float64 NumPy against the long-double restatement on UTM-sized coordinates: the margin the bounds leave (a factor >= 4)"""
    rng = np.random.default_rng(3)
    ts, pos, quat = ref.make_track(400, rng)
    tau = ref.inner_queries(ts, 4000, rng)
    off, qoff = np.array([0, 400]), np.array([0, 4000])
    want = ref.query(ts, pos, quat, off, tau, qoff)
    i = want["index"]
    w = (tau - ts[i]) / (ts[i + 1] - ts[i])
    p = pos[i] + w[:, None] * (pos[i + 1] - pos[i])
    gi, gj = ref.bracket_rows(off, qoff, want["index"], want["flags"])
    assert (np.abs(p.astype(ref.LD) - want["pos"]) * 4 <= ref.pos_bound(pos, gi, gj)).all()


# ------------------------------------------------------------------------------------------------ 2. the kernel's host/device helpers
def test_searches(hq):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 63, 64, 65, 130, 1000):
        t = np.sort(rng.uniform(0, 10, n))
        if n >= 3:
            t[n // 2] = t[n // 2 - 1]                                   # a repeated stamp
        taus = np.r_[t, t[:-1] + 0.5 * np.diff(t), t[0] - 1, t[-1] + 1, np.nextafter(t, -np.inf), np.nextafter(t, np.inf)]
        for tau in taus:
            assert hq.hq_count_le(t, n, float(tau)) == np.searchsorted(t, tau, side="right"), (n, tau)
    offs = np.array([0, 0, 5, 5, 5, 9, 12, 12], dtype=np.int64)       # empty tracks: a query belongs to the LAST track that starts at or before it
    for m in range(12):
        b = hq.hq_count_le_i64(offs, len(offs), m) - 1
        assert offs[b] <= m < offs[b + 1], m
    assert hq.hq_track_unsorted(np.array([1.0, 2.0, 2.0, 3.0]), 4) == 0
    assert hq.hq_track_unsorted(np.array([1.0, 2.0, 1.5, 3.0]), 4) == 1
    assert hq.hq_track_unsorted(np.array([np.nan, 2.0]), 2) == 1 and hq.hq_track_unsorted(np.array([1.0, np.nan, 3.0]), 3) == 1
    assert hq.hq_track_unsorted(np.array([1.0]), 1) == 0 and hq.hq_track_unsorted(np.array([np.nan]), 1) == 1


@pytest.mark.parametrize("points", [False, True])
def test_helpers_agree_with_the_yardstick(hq, cases, points):
    c, want_q, want_g = cases
    want = want_g if points else want_q
    a, q, flags, index, state = run_helpers(hq, c, points)
    np.testing.assert_array_equal(state, want["track_state"])
    np.testing.assert_array_equal(flags, want["flags"])
    np.testing.assert_array_equal(index, want["index"])
    gi, gj = ref.bracket_rows(c["offsets"], c["q_offsets"], want["index"], want["flags"])
    if points:
        tb = np.repeat(np.arange(c["B"]), np.diff(c["q_offsets"]))
        bound = ref.point_bound(c["pos"], gi, gj, c["x"], c["scale"][tb], c["ext_t"][tb])
        assert ref.same_nan_pattern(a, want["xyz"])
        exc, worst = ref.max_excess(a, want["xyz"], bound)
        assert exc <= 0, (exc, worst)
    else:
        assert ref.same_nan_pattern(a, want["pos"]) and ref.same_nan_pattern(q, want["quat"])
        exc, worst = ref.max_excess(a, want["pos"], ref.pos_bound(c["pos"], gi, gj))
        assert exc <= 0, (exc, worst)
        exc, worst = ref.max_excess(q, want["quat"], ref.QUAT_BOUND)
        assert exc <= 0, (exc, worst)
        ex = (want["flags"] & ref.Q_EXACT) != 0                         # an exact hit is the stored pose, bit for bit
        assert a[ex].tobytes() == c["pos"][gi[ex]].tobytes() and q[ex].tobytes() == c["quat"][gi[ex]].tobytes()


def test_edge_cases_are_in_the_batch(cases):
    """what the issue lists is really there, as the yardstick sees it (so neither tier can pass by the generator having dropped a case)"""
    c, want, want_g = cases
    n, st, fl = c["notes"], want["track_state"], want["flags"]
    assert st[n["n0"]] == ref.QT_EMPTY and st[n["unsorted"]] == ref.QT_UNSORTED and st[n["nan_stamp"]] == ref.QT_UNSORTED
    assert st[n["skipped"]] == ref.QT_SKIPPED and want_g["track_state"][n["dead_extrinsic"]] == ref.QT_BAD_EXTRINSIC and st[n["dead_extrinsic"]] == 0
    for bit in (ref.Q_EXACT, ref.Q_BEFORE, ref.Q_AFTER, ref.Q_GAP, ref.Q_NAN, ref.Q_TRACK):
        assert (fl == bit).any(), bit
    assert (want_g["flags"] == (ref.Q_EXACT | ref.Q_BAD_QUAT)).any()
    q0 = c["q_offsets"]
    rep = slice(q0[n["repeated"]], q0[n["repeated"] + 1])
    hit = (c["q_t"][rep] == c["ts"][c["offsets"][n["repeated"]] + 4])
    assert hit.any() and (want["index"][rep][hit] == 6).all() and (fl[rep][hit] == ref.Q_EXACT).all()     # the last of the three equals
    sp, so = slice(q0[n["special"]], q0[n["special"] + 1]), c["offsets"][n["special"]]
    idx = want["index"][sp]
    assert ((idx == 1) & (fl[sp] == ref.Q_EXACT)).any() and np.isfinite(np.asarray(want["pos"][sp][(idx == 1) & (fl[sp] == ref.Q_EXACT)], float)).all()
    assert ((idx == 1) & (fl[sp] == 0)).any() and np.isnan(np.asarray(want["pos"][sp][(idx == 1) & (fl[sp] == 0)], float)).all()
    tiny = (idx == 8) & (fl[sp] == 0)                                   # the blend's norm is below 1e-9: q_i below a weight of 0.5, q_j above
    got = np.asarray(want["quat"][sp][tiny], float)
    assert len(got) >= 2 and {tuple(g) for g in got} == {tuple(c["quat"][so + 8]), tuple(c["quat"][so + 9])}
    assert (np.diff(c["q_offsets"]) % 64 != 0).any() and c["M"] < 3000
    packed = slice(q0[n["n130"]], q0[n["n130"]] + 257)
    assert set(np.unique(want["index"][packed])) <= {40, 41, 42} and len(np.unique(want["index"][q0[n["n130"]] + 257:q0[n["n130"] + 1]])) > 40


# ------------------------------------------------------------------------------------------------ 3. the library's surface
NAMES_QUERY = ["ctx", "ts", "pos", "quat", "offsets", "run_status", "pose_flags", "B", "q_t", "q_offsets", "M", "max_gap"]
NAMES_OUT = ["q_flags", "q_index", "q_pose_flags", "track_state"]
WANT = {
    "gsf_pose_query_dev": NAMES_QUERY + ["out_pos", "out_quat"] + NAMES_OUT,
    "gsf_pose_query": NAMES_QUERY + ["out_pos", "out_quat"] + NAMES_OUT,
    "gsf_georef_points_dev": NAMES_QUERY + ["x", "ext_q", "ext_t", "scale", "out_xyz"] + NAMES_OUT,
    "gsf_georef_points": NAMES_QUERY + ["x", "ext_q", "ext_t", "scale", "out_xyz"] + NAMES_OUT,
}


def test_library_exports_the_entries_as_declared():
    from gps_optimize_slam_amd import _lib
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    L = C.CDLL(_lib.library_path())                                     # loads without a device
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsf.h")).read(), flags=re.S)
    kinds = {"gsf_ctx *": C.c_void_p, "const double *": C.c_void_p, "double *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p,
             "const int64_t *": C.c_void_p, "const int32_t *": C.c_void_p, "int32_t *": C.c_void_p, "int64_t": C.c_int64, "double": C.c_double}
    for name, want_names in WANT.items():
        assert hasattr(L, name), name
        m = re.search(r"GSF_API int " + name + r"\s*\(([^;]*)\);", src)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        assert [re.search(r"(\w+)$", p).group(1) for p in params] == want_names, name
        types = [kinds[re.sub(r"\w+$", "", p).strip()] for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == types, name
    for macro, v in (("GSF_QT_EMPTY", 1), ("GSF_QT_UNSORTED", 2), ("GSF_QT_SKIPPED", 4), ("GSF_QT_BAD_EXTRINSIC", 8), ("GSF_Q_EXACT", 1),
                     ("GSF_Q_BEFORE", 2), ("GSF_Q_AFTER", 4), ("GSF_Q_GAP", 8), ("GSF_Q_NAN", 16), ("GSF_Q_TRACK", 32), ("GSF_Q_BAD_QUAT", 64)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(v) + r"\b", src), macro
        assert getattr(_lib, macro[4:]) == v and getattr(ref, macro[4:]) == v, macro
    core = open(os.path.join(ROOT, "gps_optimize_slam_amd", "csrc", "gsf_query_core.hpp")).read()
    for macro in ("QT_EMPTY = 1", "QT_UNSORTED = 2", "QT_SKIPPED = 4", "QT_BAD_EXTRINSIC = 8", "Q_EXACT = 1", "Q_BEFORE = 2", "Q_AFTER = 4", "Q_GAP = 8",
                  "Q_NAN = 16", "Q_TRACK = 32", "Q_BAD_QUAT = 64"):
        assert macro in core, macro


# ------------------------------------------------------------------------------------------------ 4. the wrappers' argument checks
def test_wrappers_refuse_bad_arguments():
    import torch
    from gps_optimize_slam_amd import batch
    from gps_optimize_slam_amd import ekfgpsslam as E
    ts, pos, quat = torch.zeros(4, dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 4), dtype=torch.float64)
    off, qt, qoff = torch.tensor([0, 4]), torch.zeros(2, dtype=torch.float64), torch.tensor([0, 2])
    for bad in (dict(ts=ts.float()), dict(pos=pos[:, :2]), dict(quat=quat[:3]), dict(offsets=off.int()), dict(q_t=qt.reshape(2, 1)), dict(q_offsets=torch.tensor([0, 1, 2]))):
        kw = dict(ts=ts, pos=pos, quat=quat, offsets=off, q_t=qt, q_offsets=qoff)
        kw.update(bad)
        with pytest.raises(ValueError):
            batch.query_poses_ragged(**kw)
    with pytest.raises(ValueError):
        batch.georef_points_ragged(ts, pos, quat, off, qt, torch.zeros((2, 2), dtype=torch.float64), qoff)

    class Run:                                                          # a projected=True run: no projector (ref :1096)
        zone = south = None
    with pytest.raises(ValueError, match="projected"):
        batch.georef_fused(None, Run(), qt, torch.zeros((2, 3), dtype=torch.float64), qoff, wgs84=True)
    n = np.zeros
    with pytest.raises(ValueError):
        E.interpolate_trajectory(n(4), n((4, 2)), n((4, 4)), n(2))
    with pytest.raises(ValueError):
        E.interpolate_trajectory(n(4), n((4, 3)), n((3, 4)), n(2))
    with pytest.raises(ValueError):
        E.georeference_points(n(4), n((4, 3)), n((4, 4)), n(2), n((3, 3)))
    with pytest.raises(ValueError):
        E.georeference_points(n(4), n((4, 3)), n((4, 4)), n(2), n((2, 3)), ext_quat=n(3))
