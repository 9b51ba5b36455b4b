"""GPU tier of the local Sim3 alignment (gsf_sim3_local_fit_dev / gsf_sim3_local_apply_dev; definitions in include/gsf.h).

One ragged batch (tests/local_align_ref.py: tracks of 0, 1, 2, 3, 63, 64, 65, 130 and 271 poses at 10 Hz under spacing 4 s, half-window
3.2 s, min_rows 8 -- windows of 63 / 64 / 65 rows, rows exactly on a window's bounds, a track without a usable row, knots that lose
their rows in the middle and at the start, a straight and a curved track, a zero-norm quaternion, a decreasing stamp, Unix stamps with
southern-hemisphere fixes, a standstill, a scale jump, a drifting scale) through both modes and a knot stride one below the longest grid.
The fit's counts, flags and statuses must be the restatement's; its knots lie inside the C x bound gates of the 50-digit yardsticks with
the bounds of a reduction shifted by the window's first usable row.  The blend under fed knots gives gsf_apply_sim3_batch_dev's bytes
where every knot is the global transform, and the restatement's flags and rows under its knots.  fit -> apply is local_align_ragged byte
for byte, a track alone gives the bytes it gives inside the batch, outputs do not depend on what memory held or on the stream, and the
locally aligned track composes with the existing fuse entry."""
import ctypes as C
import types

import numpy as np
import pytest

import hygiene
import local_align_ref as R
import sim3_ref as SR
from test_cov_gpu import file_batch, small_dirt

pytestmark = pytest.mark.gpu

KMAX = 8
U = 2.0 ** -53
MODES = {R.LOC_SCALE: "scale", R.LOC_SIM3: "sim3"}
GRID = dict(spacing=R.SPACING, half_window=R.HALF_WINDOW, min_rows=R.MIN_ROWS)


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
    hst = R.pack(R.gpu_tracks())
    return hst, {k: dev(v) for k, v in hst.items()}, [t["name"] for t in R.gpu_tracks()]


def align(B, d, mode, **kw):
    import torch
    la = B.local_align_ragged(d["ts"], d["pos"], d["quat"], d["gps"], d["valid"], d["offsets"], d["R"], d["t"], d["s"], mode=MODES[mode], **GRID, **kw)
    torch.cuda.synchronize()
    return la


def raw_fit(B, d, mode, Kmax, fill):
    """gsf_sim3_local_fit_dev itself on outputs pre-filled with the byte `fill` -> the eight output tensors"""
    import torch
    from gps_optimize_slam_amd import _lib
    nb = int(d["offsets"].numel()) - 1
    mk = lambda shape, dt: torch.full(shape, fill, dtype=torch.uint8, device="cuda").repeat_interleave(8 if dt == torch.float64 else 4, dim=-1).view(dt)
    out = [mk((nb, Kmax * 9), torch.float64), mk((nb, Kmax * 3), torch.float64), mk((nb, Kmax), torch.float64), mk((nb, Kmax), torch.int32),
           mk((nb, Kmax), torch.float64), mk((nb, Kmax), torch.int32), mk((nb,), torch.int32), mk((nb,), torch.int32)]
    cfg = B._local_config(MODES[mode], R.MIN_ROWS, R.SPACING, R.HALF_WINDOW, R.ROT_OPEN, R.RATIO_MAX)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_sim3_local_fit_dev(B.context().handle, p(d["ts"]), p(d["pos"]), p(d["gps"]), p(d["valid"]), p(d["offsets"]), nb, p(d["R"]),
                                                  p(d["t"]), p(d["s"]), C.byref(cfg), Kmax, *[p(t) for t in out]))
    torch.cuda.synchronize()
    return out


def raw_apply(B, d, Kmax, knots, fill):
    """gsf_sim3_local_apply_dev itself under knots = (R, t, s, flags, n_knots, track_status) on pre-filled outputs -> pos, quat, scale, flags"""
    import torch
    from gps_optimize_slam_amd import _lib
    nb, P = int(d["offsets"].numel()) - 1, int(d["ts"].numel())
    mk = lambda shape, dt: torch.full(shape, fill, dtype=torch.uint8, device="cuda").repeat_interleave(8 if dt == torch.float64 else 4, dim=-1).view(dt)
    out = [mk((P, 3), torch.float64), mk((P, 4), torch.float64), mk((P,), torch.float64), mk((P,), torch.int32)]
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_sim3_local_apply_dev(B.context().handle, p(d["ts"]), p(d["pos"]), p(d["quat"]), p(d["offsets"]), nb, p(d["R"]), p(d["t"]),
                                                    p(d["s"]), R.SPACING, Kmax, *[p(t) for t in knots], *[p(t) for t in out]))
    torch.cuda.synchronize()
    return out


def ref_knots(mode, Kmax):
    """the restatement's knot arrays of the whole batch, (B,Kmax,.) as the entry lays them out"""
    ref = R.reference(mode, Kmax)
    arr = [R.knot_arrays(f, Kmax) for f, _ in ref]
    stack = lambda k: np.stack([a[k] for a in arr])
    return (stack(0), stack(1), stack(2), stack(3), stack(4), stack(5), np.array([f["K"] for f, _ in ref], np.int32),
            np.array([f["status"] for f, _ in ref], np.int32))


# ------------------------------------------------------------------------------------------------ 1. the fit
@pytest.mark.parametrize("mode,Kmax", [(R.LOC_SCALE, KMAX), (R.LOC_SIM3, KMAX), (R.LOC_SIM3, KMAX - 1)])
def test_fit_against_the_restatement(B, batch, mode, Kmax):
    hst, d, names = batch
    la = align(B, d, mode, max_knots=Kmax)
    kR, kt, ks, kn, krms, kfl, nk, st = ref_knots(mode, Kmax)
    np.testing.assert_array_equal(h(la.n_knots), nk)
    np.testing.assert_array_equal(h(la.track_status), st)
    np.testing.assert_array_equal(h(la.knot_n), kn)
    np.testing.assert_array_equal(h(la.knot_flags), kfl)
    gR, gt, gs, grms = h(la.knot_R).reshape(-1, Kmax, 9), h(la.knot_t), h(la.knot_s), h(la.knot_rms)
    invalid = (kfl & R.KNOT_INVALID) != 0
    beyond = np.arange(Kmax)[None, :] >= nk[:, None]
    nan_rows = invalid | beyond                                             # invalid knots and the slots beyond n_knots: NaN, all of it
    assert np.isnan(gR[nan_rows]).all() and np.isnan(gt[nan_rows]).all() and np.isnan(gs[nan_rows]).all() and np.isnan(grms[nan_rows]).all()
    assert np.isfinite(gR[~nan_rows]).all() and np.isfinite(gt[~nan_rows]).all() and np.isfinite(gs[~nan_rows]).all()
    assert (h(la.knot_n)[beyond] == 0).all() and (h(la.knot_flags)[beyond] == 0).all()
    worst = dict(R=0.0, s=0.0, img=0.0, s0=0.0, img0=0.0, rms=0.0)
    checked = 0
    for b, (tr, (fit, _)) in enumerate(zip(R.gpu_tracks(), R.reference(mode, Kmax))):
        for k, knot in enumerate(fit["knots"]):
            if knot["flags"] & R.KNOT_INVALID:
                continue
            src, fix = tr["pos"][knot["rows"]], tr["gps"][knot["rows"]]
            kind, y = R.knot_yardstick(tr["name"], mode, k, Kmax)
            Rk, tk, sk = gR[b, k].reshape(3, 3), gt[b, k], float(gs[b, k])
            if kind == "sim3":
                assert y.cls == "determined" and y.status == 0
                for key, v in SR.ratios(y, src, fix, None, Rk, tk, sk, shifted=True).items():
                    worst[key] = max(worst[key], v)
                    assert v <= SR.gate_of(key), (tr["name"], k, key, v)
                bimg = y.bimg_shift
            else:
                np.testing.assert_array_equal(words(Rk), words(tr["R"]), err_msg=f"{tr['name']} knot {k}: mode 0 keeps the global rotation")
                v = abs(sk - y.s) / (y.b0_shift * y.s)
                worst["s0"] = max(worst["s0"], v)
                assert v <= R.C_S0, (tr["name"], k, "s0", v)
                img, want = sk * src @ Rk.T + tk, y.s * src @ Rk.T + y.t
                v = float(np.abs(img - want).max()) / y.bimg_shift
                worst["img0"] = max(worst["img0"], v)
                assert v <= SR.C_IMG, (tr["name"], k, "img0", v)
                bimg = y.bimg_shift
            v = abs(float(grms[b, k]) - knot["rms"]) / bimg                 # an RMS of residuals moves by no more than the largest image error
            worst["rms"] = max(worst["rms"], v)
            assert v <= 2 * SR.C_IMG, (tr["name"], k, "rms", v)              # (kernel and restatement each within C_IMG x bimg of the exact images)
            checked += 1
    print(f"mode {mode}, Kmax {Kmax}: {checked} valid knots; worst ratio to the shifted bounds R {worst['R']:.2f} s {worst['s']:.2f} image {worst['img']:.2f} "
          f"(gates {SR.C_R:.0f} / {SR.C_S:.0f} / {SR.C_IMG:.0f}); mode-0 scale {worst['s0']:.2f} (gate {R.C_S0:.0f}) image {worst['img0']:.2f}; rms {worst['rms']:.2f}")
    assert checked > (60 if Kmax == KMAX else 20)


# ------------------------------------------------------------------------------------------------ 2. the blend under fed knots
def test_apply_with_every_knot_the_global_transform(B, batch):
    """pos_out / quat_out are gsf_apply_sim3_batch_dev's bytes and scale_at is s to the bit, on every track (fed status 0: the unsorted one too)"""
    import torch
    hst, d, names = batch
    nb = len(names)
    kR = d["R"][:, None, :].expand(nb, KMAX, 9).contiguous()
    kt = d["t"][:, None, :].expand(nb, KMAX, 3).contiguous()
    ks = d["s"][:, None].expand(nb, KMAX).contiguous()
    zero = torch.zeros((nb, KMAX), dtype=torch.int32, device="cuda")
    full = torch.full((nb,), KMAX, dtype=torch.int32, device="cuda")
    po, qo, sc, fl = B.local_apply_ragged(d["ts"], d["pos"], d["quat"], d["offsets"], d["R"], d["t"], d["s"], R.SPACING, kR, kt, ks, zero, full, zero[:, 0].contiguous())
    p3, q3, _ = B.apply_sim3_batch(d["pos"], d["quat"], d["offsets"], d["R"], d["t"], d["s"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(words(h(po)), words(h(p3)))
    np.testing.assert_array_equal(words(h(qo)), words(h(q3)))
    n = np.diff(hst["offsets"])
    np.testing.assert_array_equal(words(h(sc)), words(np.repeat(hst["s"], n)))
    assert (h(fl) & ~(R.LP_BRIDGED | R.LP_BAD_QUAT) == 0).all()


@pytest.mark.parametrize("mode", [R.LOC_SCALE, R.LOC_SIM3])
def test_apply_with_the_restatements_knots(B, batch, mode):
    """pose flags exactly; rows inside gates computed from the two knots involved.  Kernel and restatement evaluate the same ~12 operations
    per coordinate (T_L, T_Rr, the blend) with different contractions: each rounds by at most u times the largest intermediate, so the
    coordinates differ by no more than ~12 u x that magnitude; the gate is C_IMG x 4 u x it, the image gate's form.  Unit quaternions pass
    ~40 roundings (normalise, matrix to quaternion, product, nlerp), the matrix step amplifying by up to 2: 256 u.  scale_at: 4 u s."""
    import torch
    hst, d, names = batch
    kR, kt, ks, _, _, kfl, nk, st = ref_knots(mode, KMAX)
    po, qo, sc, fl = B.local_apply_ragged(d["ts"], d["pos"], d["quat"], d["offsets"], d["R"], d["t"], d["s"], R.SPACING, dev(kR), dev(kt), dev(ks),
                                          dev(kfl), dev(nk), dev(st))
    torch.cuda.synchronize()
    po, qo, sc, fl = h(po), h(qo), h(sc), h(fl)
    off = hst["offsets"]
    worst = [0.0, 0.0, 0.0]
    seen = 0
    for b, (tr, (fit, bl)) in enumerate(zip(R.gpu_tracks(), R.reference(mode, KMAX))):
        sl = slice(off[b], off[b + 1])
        np.testing.assert_array_equal(fl[sl], bl["flags"], err_msg=tr["name"])
        seen |= int(np.bitwise_or.reduce(bl["flags"])) if len(bl["flags"]) else 0
        if fit["status"]:
            assert np.isnan(po[sl]).all() and np.isnan(qo[sl]).all() and np.isnan(sc[sl]).all()
            continue
        for i in range(len(tr["ts"])):
            L, Rr = int(bl["L"][i]), int(bl["Rr"][i])
            ks_ = [k for k in (L, Rr) if k >= 0]
            Rs = [kR[b, k] for k in ks_] or [tr["R"].reshape(9)]
            ts_ = [kt[b, k] for k in ks_] or [tr["t"]]
            ss = [ks[b, k] for k in ks_] or [tr["s"]]
            mag = max([float(np.abs(t_).max()) for t_ in ts_] + [float(s_ * np.abs(tr["pos"][i]).sum()) for s_ in ss] + [float(np.abs(bl["pos"][i]).max())])
            v = float(np.abs(po[off[b] + i] - bl["pos"][i]).max()) / (4 * U * mag)
            worst[0] = max(worst[0], v)
            assert v <= SR.C_IMG, (tr["name"], i, v)
            if np.isnan(bl["quat"][i]).any():
                assert np.isnan(qo[off[b] + i]).all()
            else:
                v = float(np.abs(qo[off[b] + i] - bl["quat"][i]).max()) / U
                worst[1] = max(worst[1], v)
                assert v <= 256, (tr["name"], i, v)
            v = abs(sc[off[b] + i] - bl["scale"][i]) / (U * max(ss))
            worst[2] = max(worst[2], v)
            assert v <= 4, (tr["name"], i, v)
    print(f"mode {mode}: worst position ratio {worst[0]:.2f} (gate {SR.C_IMG:.0f}), quaternion {worst[1]:.0f} u (gate 256), scale_at {worst[2]:.1f} u (gate 4)")
    assert seen & R.LP_BRIDGED and seen & R.LP_HELD and seen & R.LP_GLOBAL and seen & R.LP_BAD_QUAT and seen & R.LP_TRACK


# ------------------------------------------------------------------------------------------------ 3. one entry is the two entries; a track alone
@pytest.mark.parametrize("mode", [R.LOC_SCALE, R.LOC_SIM3])
def test_fit_then_apply_is_local_align_ragged(B, batch, mode):
    hst, d, names = batch
    la = align(B, d, mode)
    assert int(la.knot_s.shape[1]) == KMAX                                  # the stride local_align_ragged works out: the longest grid
    kR, kt, ks, kn, krms, kfl, nk, st = raw_fit(B, d, mode, KMAX, 0xAA)
    for got, want in ((kR, la.knot_R), (kt, la.knot_t), (ks, la.knot_s), (kn, la.knot_n), (krms, la.knot_rms), (kfl, la.knot_flags), (nk, la.n_knots),
                      (st, la.track_status)):
        np.testing.assert_array_equal(words(h(got).reshape(-1)), words(h(want).reshape(-1)))
    po, qo, sc, fl = raw_apply(B, d, KMAX, (kR, kt, ks, kfl, nk, st), 0xAA)
    for got, want in ((po, la.pos), (qo, la.quat), (sc, la.scale_at), (fl, la.pose_flags)):
        np.testing.assert_array_equal(words(h(got)), words(h(want)))
    # a batch of one track gives the bytes that track has inside the big batch (its own stride: the first K_b slots)
    off = hst["offsets"]
    for name in ("len271_curved", "len271_usable_rows_stop", "len130_zero_quat", "len64", "len1"):
        b = names.index(name)
        one = {k: dev(v) for k, v in R.pack([R.gpu_tracks()[b]]).items()}
        lb = align(B, one, mode)
        K = int(lb.n_knots[0])
        assert K == int(la.n_knots[b]) and int(lb.knot_s.shape[1]) == K
        for f in ("knot_R", "knot_t", "knot_s", "knot_n", "knot_rms", "knot_flags"):
            np.testing.assert_array_equal(words(h(getattr(lb, f))[0, :K]), words(h(getattr(la, f))[b, :K]), err_msg=f"{name} {f}")
        for f in ("pos", "quat", "scale_at", "pose_flags"):
            np.testing.assert_array_equal(words(h(getattr(lb, f))), words(h(getattr(la, f))[off[b]:off[b + 1]]), err_msg=f"{name} {f}")
    c = la.scale_curve(names.index("len271_drifting"))
    assert len(c[0]) == KMAX and c[2].all() and c[0][1] - c[0][0] == R.SPACING
    hi, lo = la.drift(names.index("len271_drifting"))
    assert lo < 0.97 < 1.03 < hi                                            # the planted 10 % drift straddles the global scale


# ------------------------------------------------------------------------------------------------ 4. hygiene
@pytest.mark.parametrize("mode", [R.LOC_SCALE, R.LOC_SIM3])
def test_outputs_do_not_depend_on_stale_buffers_or_the_stream(B, batch, monkeypatch, mode):
    import torch
    hst, d, names = batch
    # outputs pre-filled with NaN bytes and with 0xAA bytes: the same bytes from both entries (every byte of every output is written --
    # the knot slots beyond n_knots[b] included, which the header says are NaN-filled; rows outside offsets do not exist)
    a, b = raw_fit(B, d, mode, KMAX, 0xFF), raw_fit(B, d, mode, KMAX, 0xAA)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(words(h(x).reshape(-1)), words(h(y).reshape(-1)))
    knots = (a[0], a[1], a[2], a[5], a[6], a[7])
    pa, pb = raw_apply(B, d, KMAX, knots, 0xFF), raw_apply(B, d, KMAX, knots, 0xAA)
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(words(h(x)), words(h(y)))
    nk = h(a[6])
    beyond = np.arange(KMAX)[None, :] >= nk[:, None]
    assert beyond.any() and np.isnan(h(a[2])[beyond]).all() and np.isnan(h(a[0]).reshape(-1, KMAX, 9)[beyond]).all() and (h(a[3])[beyond] == 0).all()
    # guard bytes around every output, workspaces poisoned with two words after a foreign call: the same bytes (the neighbour tables live
    # in the kernel workspace)
    call = lambda: B.local_align_ragged(d["ts"], d["pos"], d["quat"], d["gps"], d["valid"], d["offsets"], d["R"], d["t"], d["s"], mode=MODES[mode],
                                        max_knots=KMAX, **GRID)
    la = hygiene.same_bytes_under_dirt(monkeypatch, B.context(), call, small_dirt(B))
    for got, want in ((la.pos, pa[0]), (la.quat, pa[1]), (la.scale_at, pa[2]), (la.pose_flags, pa[3]), (la.knot_s, a[2]), (la.knot_flags, a[5])):
        np.testing.assert_array_equal(words(h(got).reshape(-1)), words(h(want).reshape(-1)))
    # a side stream (its own context): the same bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ls = call()
    side.synchronize()
    for f in ("knot_R", "knot_t", "knot_s", "knot_n", "knot_rms", "knot_flags", "n_knots", "track_status", "pos", "quat", "scale_at", "pose_flags"):
        np.testing.assert_array_equal(words(h(getattr(ls, f)).reshape(-1)), words(h(getattr(la, f)).reshape(-1)), err_msg=f)


def test_skipped_runs_pass_through_and_argument_errors(B, batch):
    import torch
    from gps_optimize_slam_amd import _lib
    hst, d, names = batch
    rs = np.zeros(len(names), np.int32)
    b = names.index("len271_curved")
    rs[b] = 8
    la = align(B, d, R.LOC_SCALE, run_status=dev(rs))
    base = align(B, d, R.LOC_SCALE)
    off = hst["offsets"]
    assert int(la.track_status[b]) == R.LOC_SKIPPED and int(la.n_knots[b]) == 0
    assert np.isnan(h(la.pos)[off[b]:off[b + 1]]).all() and (h(la.pose_flags)[off[b]:off[b + 1]] == R.LP_TRACK).all() and np.isnan(h(la.knot_s)[b]).all()
    keep = np.ones(int(off[-1]), bool); keep[off[b]:off[b + 1]] = False
    np.testing.assert_array_equal(words(h(la.pos)[keep]), words(h(base.pos)[keep]))
    p = lambda t: C.c_void_p(t.data_ptr())
    L, hd = _lib.load(), B.context().handle
    cfg = B._local_config("scale", 8, 4.0, 3.2, 1e-3, 2.0)
    assert L.gsf_sim3_local_fit_dev(hd, *[None] * 4, p(d["offsets"]), 0, None, None, None, C.byref(cfg), 4, *[None] * 8) == 0       # B = 0: nothing to do
    for Kmax in (0, 4097):
        assert L.gsf_sim3_local_fit_dev(hd, *[None] * 4, p(d["offsets"]), 0, None, None, None, C.byref(cfg), Kmax, *[None] * 8) != 0
    bad = B._local_config("scale", 8, 4.0, 3.2, 1e-3, 2.0)
    bad.min_rows = 1
    assert L.gsf_sim3_local_fit_dev(hd, *[None] * 4, p(d["offsets"]), 0, None, None, None, C.byref(bad), 4, *[None] * 8) != 0
    assert L.gsf_sim3_local_apply_dev(hd, *[None] * 3, p(d["offsets"]), 0, None, None, None, 0.0, 4, *[None] * 10) != 0      # spacing 0
    assert L.gsf_sim3_local_apply_dev(hd, *[None] * 3, p(d["offsets"]), 0, None, None, None, 4.0, 4, *[None] * 10) == 0


# ------------------------------------------------------------------------------------------------ 5. composition
def test_refuse_local_is_the_existing_fuse_entry_on_the_local_track(B, batch):
    """refuse_local on the drifting case == ekf_fuse_ragged called by hand on la.pos / la.quat, byte for byte; the local track goes into
    the sweep, outage and gate entries as their track; the single-track wrapper returns the batch entry's bytes"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    tr = R.track("len271_drifting")
    one = {k: dev(v) for k, v in R.pack([tr]).items()}
    rb = types.SimpleNamespace(ts=one["ts"], pos=one["pos"], quat=one["quat"], slam_offsets=one["offsets"])
    r = B.RunResult(aligned=one["gps"], valid=one["valid"], run_status=torch.zeros(1, dtype=torch.int32, device="cuda"), R=one["R"], t=one["t"], s=one["s"])
    la = B.local_align_fused(rb, r, **GRID)
    out = B.refuse_local(rb, r, la, want_cov=True)
    po, qo, st = B.ekf_fuse_ragged(one["ts"], la.pos, la.quat, one["gps"], one["valid"], one["offsets"], la.pos[:1].contiguous(), la.quat[:1].contiguous())
    torch.cuda.synchronize()
    for got, want in ((out.pos, po), (out.quat, qo), (out.status, st)):
        np.testing.assert_array_equal(words(h(got)), words(h(want)))
    assert tuple(out.err_stats3.shape) == (3, 1, 4) and tuple(out.errors3.shape) == (3, 271) and out.cov is not None
    rmse = h(out.err_stats3)[:, 0, 3]
    print(f"drifting case, step 6 RMSE raw / local-aligned / fused: {rmse[0]:.3f} / {rmse[1]:.3f} / {rmse[2]:.3f} m")
    assert np.isfinite(rmse).all() and rmse[1] < rmse[0]
    # straight into the other entries as their track
    ip, iq = la.pos[:1].contiguous(), la.quat[:1].contiguous()
    args = (one["ts"], la.pos, la.quat, one["gps"], one["valid"], one["offsets"], ip, iq)
    g = B.innovation_gate_ragged(*args, [np.inf])
    assert torch.equal(g.valid_out[0], one["valid"])
    sw = B.ekf_noise_sweep_ragged(*args, B.noise_candidates(E.CONFIG, (1.0,), (1.0, 4.0))[0])
    os_ = B.outage_study_ragged(*args, B.outage_scenarios([10.0], [5.0]))
    torch.cuda.synchronize()
    assert np.isfinite(h(sw.stats)).any() and np.isfinite(h(os_.stats)).any()
    # the single-track wrapper
    slam = {"timestamps": tr["ts"], "positions": tr["pos"], "quaternions": tr["quat"]}
    w = E.align_trajectory_local(slam, tr["gps"], tr["valid"], tr["R"], tr["t"], tr["s"], **GRID)
    np.testing.assert_array_equal(words(w["positions"]), words(h(la.pos)))
    np.testing.assert_array_equal(words(w["quaternions"]), words(h(la.quat)))
    assert w["knot_valid"].all() and w["knot_R"].shape == (KMAX, 3, 3)
    bad = dict(slam, timestamps=tr["ts"][::-1].copy())
    with pytest.raises(ValueError):
        E.align_trajectory_local(bad, tr["gps"], tr["valid"], tr["R"], tr["t"], tr["s"], **GRID)


def test_a_whole_run_is_unchanged_by_the_local_alignment(B, golden, tmp_path):
    """run_fusion_ragged on the bundled track's files, local_align_fused and refuse_local on its result, the run again: the same fused
    bytes; the stopped track passes through as NaN rows"""
    import torch
    from gps_optimize_slam_amd import _lib, ekfgpsslam as E
    rb = file_batch(B, golden, tmp_path)
    seeds = lambda: B.mt19937_seed([3, 4, 5, 6])
    r = B.run_fusion_ragged(rb, seeds(), E.CONFIG)
    before = (h(r.fused.pos).copy(), h(r.fused.quat).copy(), h(r.run_status).copy())
    for mode in ("scale", "sim3"):
        la = B.local_align_fused(rb, r, spacing=5.0, half_window=5.0, min_rows=8, mode=mode)
        out = B.refuse_local(rb, r, la)
    torch.cuda.synchronize()
    st, so = h(la.track_status), h(rb.slam_offsets)
    assert before[2][2] != 0 and st[2] == _lib.LOC_SKIPPED and (st[[0, 1, 3]] == 0).all()
    assert np.isnan(h(la.pos)[so[2]:so[3]]).all()
    for b in (0, 1, 3):
        assert np.isfinite(h(la.pos)[so[b]:so[b + 1]]).all() and np.isfinite(h(out.err_stats3)[:, b]).all(), b
    r2 = B.run_fusion_ragged(rb, seeds(), E.CONFIG)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(words(h(r2.fused.pos)), words(before[0]))
    np.testing.assert_array_equal(words(h(r2.fused.quat)), words(before[1]))
    np.testing.assert_array_equal(h(r2.run_status), before[2])
