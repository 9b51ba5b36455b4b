"""GPU tier of the antenna lever arm (gsf_lever_fit_dev / gsf_lever_apply_dev; definitions in include/gsf.h).

One ragged batch (tests/lever_ref.py: 20 tracks of 0, 1, 2, 7, 8, 63, 64, 65, 72, 130 and 271 poses -- a straight track with a constant
quaternion, a yaw-only L, Ls with a roll / pitch wiggle, a 0.2 rad bend, a standstill, zero-norm / NaN / tiny quaternions, masked rows
and NaN fixes, southern-hemisphere UTM, a failed run, a scale the caller has wrong by 3) through every combination of fit_scale /
fit_rotation and once without a rotation prior.  Counts and flags must be the restatement's; fitted tracks lie inside the gates of the
50-digit yardstick of the same iteration (the bounds of tests/lever_ref.py, never the device's own figures); flagged tracks return their
starting bytes.  The apply entry returns the fix's bytes under l = 0 and NaN rows with their flag for bad quaternions.  Masked-out rows
are not read, a track alone gives the bytes it gives inside the batch, outputs do not depend on what memory held or on the stream,
refuse_lever is the composition done by hand, a whole run is unchanged by the new calls, and on the planted L the fused camera track
lies closer to the true camera positions through lever_fit_fused -> refuse_lever than from the plain run."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import hygiene
import lever_ref as V
from test_cov_gpu import file_batch, small_dirt
from test_lever_host import check_fit

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OUT_FIELDS = ("R", "t", "s", "l", "l_cov", "n_rows", "n_bad_quat", "rms_before", "rms_after", "last_step", "flags")


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).cuda()          # (a copy: the shared arrays are read-only)


def h(t):
    return t.cpu().numpy()


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def batch(B):
    """the host arrays of the batch and their device copies: (host dict, device dict, names)"""
    hst = V.pack(V.gpu_tracks())
    return hst, {k: dev(v) for k, v in hst.items()}, [t["name"] for t in V.gpu_tracks()]


def kwargs_of(cfg):
    return {k: cfg[k] for k in ("sigma_fix", "sigma_prior", "sigma_rot", "ratio_max", "pivot_min", "weak_ratio", "conv_tol", "min_rows", "iters")} | dict(
        fit_scale=bool(cfg["fit_scale"]), fit_rotation=bool(cfg["fit_rotation"]))


def fit(B, d, cname="s1r1"):
    import torch
    lv = B.lever_fit_ragged(d["pos"], d["quat"], d["gps"], d["valid"], d["offsets"], d["R"], d["t"], d["s"], l0=d["l0"], run_status=d["run_status"],
                            **kwargs_of(V.configs()[cname]))
    torch.cuda.synchronize()
    return lv


def raw_fit(B, d, cname, fill):
    """gsf_lever_fit_dev itself on outputs pre-filled with the byte `fill` -> the eleven output tensors in OUT_FIELDS' order"""
    import torch
    from gps_optimize_slam_amd import _lib
    nb = int(d["offsets"].numel()) - 1
    mk = lambda shape, dt: torch.full(shape, fill, dtype=torch.uint8, device="cuda").repeat_interleave(8 if dt == torch.float64 else 4, dim=-1).view(dt)
    f, i = torch.float64, torch.int32
    out = [mk((nb, 9), f), mk((nb, 3), f), mk((nb,), f), mk((nb, 3), f), mk((nb, 9), f), mk((nb,), i), mk((nb,), i), mk((nb,), f), mk((nb,), f), mk((nb,), f), mk((nb,), i)]
    k = kwargs_of(V.configs()[cname])
    cfg = B._lever_config(k["sigma_fix"], k["sigma_prior"], k["sigma_rot"], k["fit_scale"], k["fit_rotation"], k["iters"], k["min_rows"], k["ratio_max"],
                          k["pivot_min"], k["weak_ratio"], k["conv_tol"])
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_lever_fit_dev(B.context().handle, p(d["pos"]), p(d["quat"]), p(d["gps"]), p(d["valid"]), p(d["offsets"]), nb, p(d["R"]), p(d["t"]),
                                             p(d["s"]), p(d["l0"]), p(d["run_status"]), C.byref(cfg), *[p(t) for t in out]))
    torch.cuda.synchronize()
    return out


def raw_apply(B, d, R, l, sign, fill):
    """gsf_lever_apply_dev itself on pre-filled outputs -> xyz_out, pose_flags"""
    import torch
    from gps_optimize_slam_amd import _lib
    nb, P = int(d["offsets"].numel()) - 1, int(d["gps"].shape[0])
    mk = lambda shape, dt: torch.full(shape, fill, dtype=torch.uint8, device="cuda").repeat_interleave(8 if dt == torch.float64 else 4, dim=-1).view(dt)
    out = [mk((P, 3), torch.float64), mk((P,), torch.int32)]
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_lever_apply_dev(B.context().handle, p(d["quat"]), p(d["gps"]), p(d["offsets"]), nb, p(R), p(l), float(sign), *[p(t) for t in out]))
    torch.cuda.synchronize()
    return out


def got_of(lv, b):
    return dict(flags=int(lv.flags[b]), n_rows=int(lv.n_rows[b]), n_bad_quat=int(lv.n_bad_quat[b]), R=h(lv.R[b]), t=h(lv.t[b]), s=float(lv.s[b]), l=h(lv.l[b]),
                l_cov=h(lv.l_cov[b]).reshape(9), rms_before=float(lv.rms_before[b]), rms_after=float(lv.rms_after[b]), last_step=float(lv.last_step[b]))


# ------------------------------------------------------------------------------------------------ 1. the fit
@pytest.mark.parametrize("cname", list(V.configs()))
def test_fit_against_the_restatement_and_the_yardstick(B, batch, cname):
    """integers and flags exactly, flagged tracks the starting bytes, fitted tracks inside the gates of tests/lever_ref.py (check_fit of the
    CPU tier: the same bounds, the same gates), rms_after <= rms_before (1 + gate)"""
    hst, d, names = batch
    lv = fit(B, d, cname)
    worst, n_fit = dict(l=0.0, s=0.0, R=0.0, t=0.0, cov=0.0), 0
    for b, (name, ref) in enumerate(zip(names, V.reference(cname))):
        check_fit(name, cname, ref, got_of(lv, b), worst)
        n_fit += not ref["flags"] & V.KEPT
    print(f"{cname}: {n_fit} fitted tracks; worst ratio to the bounds (C = 1) l {worst['l']:.4f} s {worst['s']:.4f} R {worst['R']:.4f} t {worst['t']:.4f} "
          f"l_cov {worst['cov']:.3f} (gates {V.GATE['l']:.2f} / {V.GATE['s']:.2f} / {V.GATE['R']:.2f} / {V.GATE['t']:.2f} / {V.GATE['cov']:.1f})")
    assert n_fit >= 11
    fl = dict(zip(names, h(lv.flags)))
    if cname == "s1r1":
        assert fl["len271_straight"] == V.WEAK and fl["len130_yaw_L"] == V.WEAK_Z and fl["len271_L3"] == 0      # observability, axis by axis
        y = V.track_yardstick("len271_straight")
        assert np.abs(h(lv.l)[names.index("len271_straight")] - V.track("len271_straight")["l0"]).max() <= V.GATE["l"] * V.bounds(y, None)["l"]
        ob = h(lv.observed)
        assert not ob[names.index("len271_straight")].any() and ob[names.index("len130_yaw_L")].tolist() == [True, True, False] and ob[names.index("len271_L3")].all()
        np.testing.assert_array_equal(h(lv.sigma), np.sqrt(np.diagonal(h(lv.l_cov), axis1=1, axis2=2)))
        assert h(lv.fitted).tolist() == [not r["flags"] & V.KEPT for r in V.reference(cname)]
        assert len(lv.table().splitlines()) == len(names) + 1
    if cname == "rot_free":
        assert fl["len271_straight"] & V.KEPT == V.SINGULAR


# ------------------------------------------------------------------------------------------------ 2. the apply
def test_apply_against_the_restatement(B, batch):
    """l = 0: the fix's bytes (a bad quaternion: a NaN row and its flag all the same).  A fed l: the restatement's flags, NaN fixes stay NaN,
    rows within 2 u |fix| + 16 u |l| of it -- the shift R (M l) is a dozen operations on numbers of size |l| that the device contracts
    differently (each within u |l| of the exact value), and the sum with the fix rounds once more at the fix's size"""
    import torch
    hst, d, names = batch
    nb = len(names)
    zero = torch.zeros((nb, 3), dtype=torch.float64, device="cuda")
    out0, fl0 = B.lever_apply_ragged(d["quat"], d["gps"], d["offsets"], d["R"], zero, sign=-1)
    l_fed = V.track("len271_L3")["l_true"]
    lfed = dev(np.tile(l_fed, (nb, 1)))
    out1, fl1 = B.lever_apply_ragged(d["quat"], d["gps"], d["offsets"], d["R"], lfed, sign=-1)
    back, _ = B.lever_apply_ragged(d["quat"], out1, d["offsets"], d["R"], lfed, sign=1)
    torch.cuda.synchronize()
    out0, fl0, out1, fl1, back = h(out0), h(fl0), h(out1), h(fl1), h(back)
    off = hst["offsets"]
    n_bad = 0
    for b, tr in enumerate(V.gpu_tracks()):
        sl = slice(off[b], off[b + 1])
        want, wfl = V.apply_track(tr["quat"], tr["gps"], tr["R"], l_fed, -1.0)
        np.testing.assert_array_equal(fl0[sl], wfl); np.testing.assert_array_equal(fl1[sl], wfl)
        bad = wfl != 0
        n_bad += int(bad.sum())
        assert np.isnan(out0[sl][bad]).all() and np.isnan(out1[sl][bad]).all()
        np.testing.assert_array_equal(words(out0[sl][~bad]), words(tr["gps"][~bad]), err_msg=tr["name"])
        assert (np.isnan(out1[sl]) == np.isnan(want)).all(), tr["name"]
        if len(want):
            with np.errstate(invalid="ignore"):
                tol = 2 * U * np.abs(tr["gps"]).max(1) + 16 * U * np.abs(l_fed).max()
                err = np.abs(out1[sl] - want).max(1)
                assert (np.isnan(err) | (err <= tol)).all(), (tr["name"], float(np.nanmax(err / tol)))
                rt = np.abs(back[sl] - tr["gps"]).max(1)                    # camera -> antenna again: the fix, to the same tolerance twice
                assert (np.isnan(rt) | (rt <= 2 * tol)).all(), tr["name"]
    assert n_bad == 3


# ------------------------------------------------------------------------------------------------ 3. rows that are not read; a track alone
def test_masked_rows_are_not_read_and_a_track_alone_is_its_rows_in_the_batch(B, batch):
    import torch
    hst, d, names = batch
    lv = fit(B, d)
    # other values in every masked-out row, and in every row of the failed run: no output byte changes
    dirty = {k: v.clone() for k, v in d.items()}
    masked = dirty["valid"] == 0
    off = hst["offsets"]
    b = names.index("len65_run_failed")
    masked[off[b]:off[b + 1]] = True
    assert int(masked.sum()) >= 65 + 65 + 13
    dirty["pos"][masked] = 1e9; dirty["gps"][masked] = -3e8; dirty["quat"][masked] = float("nan")
    lw = fit(B, dirty)
    for f in OUT_FIELDS:
        np.testing.assert_array_equal(words(h(getattr(lw, f))), words(h(getattr(lv, f))), err_msg=f)
    # a batch of one track gives the bytes that track has inside the big batch, fit and apply
    lfed = dev(np.tile(V.track("len271_L3")["l_true"], (len(names), 1)))
    out, fl = B.lever_apply_ragged(d["quat"], d["gps"], d["offsets"], d["R"], lfed, sign=-1)
    for name in ("len271_L3", "len130_bad_quats", "len130_masked", "len65", "len64", "len63", "len8_min_rows", "len1", "len130_scale_jump", "len271_straight"):
        b = names.index(name)
        one = {k: dev(v) for k, v in V.pack([V.gpu_tracks()[b]]).items()}
        lb = fit(B, one)
        for f in OUT_FIELDS:
            np.testing.assert_array_equal(words(h(getattr(lb, f))[0]), words(h(getattr(lv, f))[b]), err_msg=f"{name} {f}")
        o1, f1 = B.lever_apply_ragged(one["quat"], one["gps"], one["offsets"], one["R"], lfed[:1].contiguous(), sign=-1)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(words(h(o1)), words(h(out)[off[b]:off[b + 1]]), err_msg=name)
        np.testing.assert_array_equal(h(f1), h(fl)[off[b]:off[b + 1]])


# ------------------------------------------------------------------------------------------------ 4. hygiene
@pytest.mark.parametrize("cname", ["s1r1", "rot_free"])
def test_outputs_do_not_depend_on_stale_buffers_or_the_stream(B, batch, monkeypatch, cname):
    import torch
    hst, d, names = batch
    # outputs pre-filled with 0xFF and with 0xAA bytes: the same bytes from both entries (every byte of every output is written)
    a, b = raw_fit(B, d, cname, 0xFF), raw_fit(B, d, cname, 0xAA)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(words(h(x).reshape(-1)), words(h(y).reshape(-1)))
    pa, pb = raw_apply(B, d, a[0], a[3], -1, 0xFF), raw_apply(B, d, a[0], a[3], -1, 0xAA)
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(words(h(x)), words(h(y)))
    # guard bytes around every output, workspaces poisoned after a foreign call: the same bytes
    def call():
        lv = B.lever_fit_ragged(d["pos"], d["quat"], d["gps"], d["valid"], d["offsets"], d["R"], d["t"], d["s"], l0=d["l0"], run_status=d["run_status"],
                                **kwargs_of(V.configs()[cname]))
        lv.gps_camera, lv.pose_flags = B.lever_apply_ragged(d["quat"], d["gps"], d["offsets"], lv.R, lv.l, sign=-1)
        return lv
    lv = hygiene.same_bytes_under_dirt(monkeypatch, B.context(), call, small_dirt(B))
    for f, want in zip(OUT_FIELDS, a):
        np.testing.assert_array_equal(words(h(getattr(lv, f)).reshape(-1)), words(h(want).reshape(-1)), err_msg=f)
    np.testing.assert_array_equal(words(h(lv.gps_camera)), words(h(pa[0])))
    np.testing.assert_array_equal(h(lv.pose_flags), h(pa[1]))
    # a side stream (its own context): the same bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ls = call()
    side.synchronize()
    for f in OUT_FIELDS + ("gps_camera", "pose_flags"):
        np.testing.assert_array_equal(words(h(getattr(ls, f)).reshape(-1)), words(h(getattr(lv, f)).reshape(-1)), err_msg=f)


def test_argument_errors_of_the_entries(B, batch):
    from gps_optimize_slam_amd import _lib
    hst, d, names = batch
    p = lambda t: C.c_void_p(t.data_ptr())
    L, hd = _lib.load(), B.context().handle
    ok = B._lever_config(0.5, 1.0, 0.05, True, True, 4, 8, 2.0, 1e-10, 0.5, 1e-6)
    assert L.gsf_lever_fit_dev(hd, *[None] * 4, p(d["offsets"]), 0, *[None] * 5, C.byref(ok), *[None] * 11) == 0       # B = 0: nothing to do
    for field, value in (("iters", 0), ("iters", 9), ("min_rows", 0), ("sigma_fix", 0.0), ("sigma_rot", -1.0), ("ratio_max", 0.5)):
        bad = B._lever_config(0.5, 1.0, 0.05, True, True, 4, 8, 2.0, 1e-10, 0.5, 1e-6)
        setattr(bad, field, value)
        assert L.gsf_lever_fit_dev(hd, *[None] * 4, p(d["offsets"]), 0, *[None] * 5, C.byref(bad), *[None] * 11) != 0, field
    assert L.gsf_lever_apply_dev(hd, None, None, p(d["offsets"]), 0, None, None, -1.0, None, None) == 0
    assert L.gsf_lever_apply_dev(hd, None, None, p(d["offsets"]), 0, None, None, 0.5, None, None) != 0
    assert L.gsf_lever_apply_dev(hd, None, None, p(d["offsets"]), 1, None, None, 1.0, None, None) != 0                 # NULL arrays


# ------------------------------------------------------------------------------------------------ 5. composition and what it is for
def _run_of(B, one):
    import torch
    rb = types.SimpleNamespace(ts=one["ts"], pos=one["pos"], quat=one["quat"], slam_offsets=one["offsets"])
    r = B.RunResult(aligned=one["gps"], valid=one["valid"], run_status=torch.zeros(1, dtype=torch.int32, device="cuda"), R=one["R"], t=one["t"], s=one["s"])
    return rb, r


def test_refuse_lever_is_the_composition_by_hand_and_moves_the_track_to_the_camera(B):
    """refuse_lever == lever_apply_ragged, apply_sim3_batch row 0, ekf_fuse_ragged by hand, byte for byte; the single-track wrappers return
    the batch entries' bytes; on the planted L with 0.1 m noise the fused camera track lies closer to the TRUE camera positions through
    lever_fit_fused -> refuse_lever than from the plain run, and rms_after < rms_before"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    tr = V.motivation_track()
    one = {k: dev(v) for k, v in V.pack([tr]).items()}
    rb, r = _run_of(B, one)
    lv = B.lever_fit_fused(rb, r)
    out = B.refuse_lever(rb, r, lv, want_cov=True)
    gc, lf = B.lever_apply_ragged(one["quat"], one["gps"], one["offsets"], lv.R, lv.l, sign=-1)
    first = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    ip, iq, _ = B.apply_sim3_batch(one["pos"][:1].contiguous(), one["quat"][:1].contiguous(), first, lv.R, lv.t, lv.s)
    po, qo, st = B.ekf_fuse_ragged(one["ts"], one["pos"], one["quat"], gc, one["valid"], one["offsets"], ip, iq)
    ip0, iq0, _ = B.apply_sim3_batch(one["pos"][:1].contiguous(), one["quat"][:1].contiguous(), first, one["R"], one["t"], one["s"])
    pp, _, _ = B.ekf_fuse_ragged(one["ts"], one["pos"], one["quat"], one["gps"], one["valid"], one["offsets"], ip0, iq0)     # the plain run's filter
    torch.cuda.synchronize()
    for got, want in ((out.pos, po), (out.quat, qo), (out.status, st), (out.gps_camera, gc), (out.lever_flags, lf), (out.init_pos, ip), (out.init_quat, iq)):
        np.testing.assert_array_equal(words(h(got)), words(h(want)))
    assert tuple(out.err_stats3.shape) == (3, 1, 4) and tuple(out.errors3.shape) == (3, 271) and out.cov is not None
    assert int(lv.flags[0]) == 0
    rmse = lambda p: float(np.sqrt(((h(p) - tr["cam"]) ** 2).sum(1).mean()))
    e_plain, e_lever = rmse(pp), rmse(out.pos)
    print(f"planted L, 0.1 m noise: l {np.round(h(lv.l)[0], 3)} +- {np.round(h(lv.sigma)[0], 3)} (planted {tr['l_true']}); rms {float(lv.rms_before[0]):.3f} -> "
          f"{float(lv.rms_after[0]):.3f} m; fused camera track against the true camera positions: RMSE {e_plain:.3f} m plain, {e_lever:.3f} m through refuse_lever; "
          f"step 6 against the de-levered fixes raw / Sim3 / fused: {h(out.err_stats3)[:, 0, 3].round(3).tolist()}")
    assert float(lv.rms_after[0]) < float(lv.rms_before[0])
    assert e_lever < e_plain
    # the single-track wrappers
    slam = {"timestamps": tr["ts"], "positions": tr["pos"], "quaternions": tr["quat"]}
    w = E.estimate_lever_arm(slam, tr["gps"], tr["valid"], tr["R"], tr["t"], tr["s"])
    np.testing.assert_array_equal(words(w["l"]), words(h(lv.l)[0]))
    np.testing.assert_array_equal(words(w["R"].reshape(9)), words(h(lv.R)[0]))
    assert w["fitted"] and w["observed"].all() and w["flags"] == 0 and w["n_rows"] == 271
    g2, f2 = E.remove_lever_arm(tr["quat"], tr["gps"], w["R"], w["l"])
    np.testing.assert_array_equal(words(g2), words(h(gc)))
    assert not f2.any()


def test_a_whole_run_is_unchanged_by_the_lever_arm(B, golden, tmp_path):
    """run_fusion_ragged on the bundled track's files, lever_fit_fused and refuse_lever on its result, the run again: the same fused bytes;
    the stopped track is flagged and keeps its starting values"""
    import torch
    from gps_optimize_slam_amd import _lib, ekfgpsslam as E
    rb = file_batch(B, golden, tmp_path)
    seeds = lambda: B.mt19937_seed([3, 4, 5, 6])
    r = B.run_fusion_ragged(rb, seeds(), E.CONFIG)
    before = (h(r.fused.pos).copy(), h(r.fused.quat).copy(), h(r.run_status).copy())
    lv = B.lever_fit_fused(rb, r)
    out = B.refuse_lever(rb, r, lv)
    torch.cuda.synchronize()
    fl = h(lv.flags)
    assert before[2][2] != 0 and fl[2] & _lib.LEVER_TRACK and not (fl[[0, 1, 3]] & _lib.LEVER_TRACK).any()
    np.testing.assert_array_equal(words(h(lv.R)[2]), words(h(r.R)[2]))
    print(lv.table())
    for b in (0, 1, 3):
        assert np.isfinite(h(out.err_stats3)[:, b]).all(), b
    r2 = B.run_fusion_ragged(rb, seeds(), E.CONFIG)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(words(h(r2.fused.pos)), words(before[0]))
    np.testing.assert_array_equal(words(h(r2.fused.quat)), words(before[1]))
    np.testing.assert_array_equal(h(r2.run_status), before[2])
