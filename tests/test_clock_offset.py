"""The clock-offset search on the device (gsf_clock_offset_search[_dev], batch.estimate_clock_offset) against the composition of the CPU
oracle's restatements (tests/clock_offset_ref.py): J, NaN pattern, row counts and arg-min on ragged batches that cross every path of the
kernel; a planted offset; the status bits; R, t, s against the existing device entries; host route == device route bit for bit, also on
poisoned workspaces, with guard rows; search -> shift -> whole run on the bundled KITTI-04 files."""
import ctypes as C

import numpy as np
import pytest

import clock_offset_ref as ref
from test_gpu_parity import POS_TOL

pytestmark = pytest.mark.gpu

GAP = 5.0


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def _flat(tracks):
    """list of dict(ts, pos, gps_t, gps_p[, keep]) -> host arrays ts, pos, so, gps_t, gps_p, go, keep (uint8, all ones where a track has none)"""
    so = np.zeros(len(tracks) + 1, dtype=np.int64); so[1:] = np.cumsum([len(t["ts"]) for t in tracks])
    go = np.zeros(len(tracks) + 1, dtype=np.int64); go[1:] = np.cumsum([len(t["gps_t"]) for t in tracks])
    cat = lambda k, cols: np.ascontiguousarray(np.concatenate([np.asarray(t[k], dtype=np.float64).reshape(-1, cols) for t in tracks]).reshape((-1, cols) if cols > 1 else -1))
    keep = np.concatenate([np.asarray(t.get("keep", np.ones(len(t["gps_t"]))), dtype=np.uint8) for t in tracks])
    return cat("ts", 1), cat("pos", 3), so, cat("gps_t", 1), cat("gps_p", 3), go, np.ascontiguousarray(keep)


def _dev(arrs):
    import torch
    return tuple(torch.as_tensor(a).cuda() for a in arrs)


def _ragged_cases():
    """every pose count x every fix count of the issue's lists, plus the log variants and an empty track"""
    tracks = [ref.make_track(n, ng) for n in (1, 5, 63, 64, 65, 130) for ng in (1, 2, 3, 4, 65, 130)]
    rng = np.random.default_rng(17)
    gap = ref.make_track(130, 65)                                        # a hole of 7 s in the log: two segments, the second one short of the end
    sel = (gap["gps_t"] < 4.0) | (gap["gps_t"] > 11.0)
    gap["gps_t"], gap["gps_p"] = gap["gps_t"][sel], gap["gps_p"][sel]
    uns = ref.make_track(65, 65)                                         # shuffled, with five stamps repeated (another position: the first one must win)
    dup = np.r_[np.arange(65), [3, 3, 20, 40, 64]]
    p = np.r_[uns["gps_p"], uns["gps_p"][[3, 3, 20, 40, 64]] + 5.0]
    order = rng.permutation(len(dup))
    uns["gps_t"], uns["gps_p"] = uns["gps_t"][dup][order], p[order]
    msk = ref.make_track(130, 130)                                       # NaN-marked rows (the loader's mark, and a lone NaN northing) + a keep mask
    msk["gps_p"][[0, 7, 8, 50], :2] = np.nan
    msk["gps_p"][60, 1] = np.nan
    msk["keep"] = (rng.uniform(size=130) > 0.2).astype(np.uint8)
    empty = ref.make_track(0, 65)
    return tracks + [gap, uns, msk, empty]


GRIDS = {1: (0.30, 0.05), 2: (0.28, 0.05), 3: (0.25, 0.05), 65: (-24.0, 0.75)}     # K -> (tau0, dtau); the last one runs out of overlap on both sides


# ---------------------------------------------------------------------------------------------------------------- 1. J against the yardstick
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("K", [1, 2, 3, 65])
def test_J_rows_and_argmin_against_the_oracle_composition(B, orc, K, mode):
    import torch
    tracks = _ragged_cases()
    Bn = len(tracks)
    tau0, dtau = GRIDS[K]
    tau0s = tau0 + 0.01 * (np.arange(Bn) % 3)                            # a per-track start
    h = _flat(tracks)
    d = _dev(h)
    r = B.estimate_clock_offset(d, tau0=tau0s, dtau=dtau, K=K, fit_rows="reference" if mode else "all")
    torch.cuda.synchronize()
    J, nr, bk = r.J.cpu().numpy(), r.n_rows.cpu().numpy(), r.best_k.cpu().numpy()
    assert J.shape == (Bn, K) and r.tau.cpu().numpy().tobytes() == (tau0s[:, None] + np.arange(K)[None, :] * dtau).tobytes()
    worst, seen_nan, seen_fit = 0.0, 0, 0
    for b, t in enumerate(tracks):
        Jo, nro, tau = ref.sweep(orc, t["ts"], t["pos"], t["gps_t"], t["gps_p"], t.get("keep"), tau0s[b], dtau, K, max_gap=GAP, mode=mode,
                                 min_samples=4 if mode else 0)          # (fit_rows="all" sets the rule's min_samples to 0: the fit's own 3 rows decide)
        what = (b, len(t["ts"]), len(t["gps_t"]))
        np.testing.assert_array_equal(np.isnan(J[b]), np.isnan(Jo), err_msg=str(what))
        np.testing.assert_array_equal(nr[b], nro, err_msg=str(what))
        fin = np.isfinite(Jo)
        seen_nan += int((~fin).sum()); seen_fit += int(fin.sum())
        if fin.any():
            worst = max(worst, float(np.abs(J[b][fin] - Jo[fin]).max()))
        ko, tbo, tro, sto = ref.pick(Jo, tau, dtau)
        if ko < 0:
            assert bk[b] == -1 and int(r.status[b]) == ref.CLK_NONE and np.isnan(float(r.tau_best[b])) and np.isnan(float(r.tau_refined[b])), what
            assert torch.isnan(r.R[b]).all() and torch.isnan(r.t[b]).all() and torch.isnan(r.s[b]), what
        else:
            if ref.margin(Jo) > 2 * POS_TOL:
                assert bk[b] == ko and int(r.status[b]) == sto, (what, bk[b], ko)
            assert float(r.tau_best[b]) == tau[bk[b]], what           # bit for bit numpy's tau0 + k * dtau
    print(f"K {K} mode {mode}: max |J - yardstick| = {worst:.3g} m over {seen_fit} fits, {seen_nan} NaN candidates")
    assert worst < POS_TOL
    assert seen_fit > 0 and seen_nan > 0
    assert bk[-1] == -1 and np.isnan(J[-1]).all() and (nr[-1] == 0).all()                      # the empty track


# ---------------------------------------------------------------------------------------------------------------- 2. planted offset
@pytest.fixture(scope="module")
def planted(B):
    import torch
    tracks = [ref.make_track(n, ng) for n, ng in ref.PLANTED_SHAPES]
    d = _dev(_flat(tracks))
    r = B.estimate_clock_offset(d[:6], tau0=-1.0, dtau=0.05, K=41)
    torch.cuda.synchronize()
    return tracks, d, r


def test_planted_offset_and_parabola(planted):
    tracks, d, r = planted
    tau = r.tau.cpu().numpy()
    J = r.J.cpu().numpy()
    for b in range(len(tracks)):
        k = int(r.best_k[b])
        assert k == int(np.argmin(np.abs(tau[b] - ref.TAU_TRUE))) and int(r.status[b]) == 0, (b, k)
        assert float(r.tau_best[b]) == tau[b, k]
        a, m, c = J[b, k - 1] ** 2, J[b, k] ** 2, J[b, k + 1] ** 2
        assert (a - 2 * m + c) / a > 1e-3                                # the parabola is well conditioned on these shapes
        want = ref.parabola(J[b], tau[b], 0.05, k)
        print(f"track {b}: tau_best {tau[b, k]:.2f} tau_refined {float(r.tau_refined[b]):.6f} J {J[b, k]:.3g} m")
        assert abs(float(r.tau_refined[b]) - want) <= 1e-9 * 0.05, (b, float(r.tau_refined[b]), want)
        assert abs(float(r.tau_refined[b]) - ref.TAU_TRUE) < 1e-3


# ---------------------------------------------------------------------------------------------------------------- 3. status bits
def test_status_bits(B):
    import torch
    tracks = [ref.make_track(130, 65), ref.make_track(130, 65, straight=True), ref.make_track(130, 1)]
    d = _dev(_flat(tracks))
    r = B.estimate_clock_offset(d[:6], tau0=-1.0, dtau=0.05, K=21, flat_threshold=1e-3)        # the grid ends at 0.0, short of 0.30
    torch.cuda.synchronize()
    st = r.status.cpu().numpy()
    J = r.J.cpu().numpy()
    print("J spread of the straight track:", np.nanmax(J[1]) - np.nanmin(J[1]))
    assert st[0] == ref.CLK_AT_EDGE and int(r.best_k[0]) == 20
    assert st[1] & ref.CLK_FLAT and np.nanmax(J[1]) - np.nanmin(J[1]) < 1e-3
    assert st[2] == ref.CLK_NONE and int(r.best_k[2]) == -1 and np.isnan(J[2]).all()
    r0 = B.estimate_clock_offset(d[:6], tau0=-1.0, dtau=0.05, K=21)                              # flat_threshold 0 never sets the bit
    assert not (r0.status.cpu().numpy() & ref.CLK_FLAT).any()


# ---------------------------------------------------------------------------------------------------------------- 4. R, t, s of best_k
def test_fit_of_the_best_candidate_equals_the_existing_entries(B, planted):
    import torch
    from gps_optimize_slam_amd import _lib
    tracks, d, r = planted
    ts, pos, so, gps_t, utm, go = d[:6]
    Bn = len(tracks)
    shifted = gps_t + torch.repeat_interleave(r.tau_best, go[1:] - go[:-1])
    aligned = torch.empty((ts.numel(), 3), dtype=torch.float64, device="cuda")
    valid = torch.empty((ts.numel(),), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.load().gsf_time_align_batch_dev(B.context().handle, p(ts), p(so), p(shifted), p(utm), p(go), Bn, 130, GAP, p(aligned), p(valid), None))
    mask, n_rows, st = B.sim3_fit_rows_batch(ts, aligned, valid, offsets=so)
    R, t, s, fst = B.sim3_umeyama_batch(pos, aligned, so, mask)
    torch.cuda.synchronize()
    assert (fst == 0).all()
    k = r.best_k.long()
    assert torch.equal(n_rows, r.n_rows[torch.arange(Bn, device="cuda"), k])
    np.testing.assert_allclose(r.R.cpu().numpy(), R.cpu().numpy(), atol=1e-10, rtol=0)
    np.testing.assert_allclose(r.s.cpu().numpy(), s.cpu().numpy(), atol=1e-11, rtol=0)
    for b, tr in enumerate(tracks):
        a = float(r.s[b]) * tr["pos"] @ r.R[b].cpu().numpy().reshape(3, 3).T + r.t[b].cpu().numpy()
        o = float(s[b]) * tr["pos"] @ R[b].cpu().numpy().reshape(3, 3).T + t[b].cpu().numpy()
        np.testing.assert_allclose(a, o, atol=POS_TOL, rtol=0)


# ---------------------------------------------------------------------------------------------------------------- 5. host route == device route
def test_host_route_device_route_poison_and_guards(B):
    import torch
    from gps_optimize_slam_amd import _lib
    tracks = _ragged_cases()
    Bn, K = len(tracks), 5
    h = _flat(tracks)
    d = _dev(h)
    tau0 = np.full(Bn, 0.2)
    L, ctx = _lib.load(), B.context()
    ctx.set_sim3_rows("reference", B.CONFIG)
    SENT = -7.25

    def dev_route():
        o = dict(J=torch.full((Bn + 2, K), SENT, dtype=torch.float64, device="cuda"), nr=torch.full((Bn + 2, K), -9, dtype=torch.int32, device="cuda"),
                 bk=torch.empty((Bn,), dtype=torch.int32, device="cuda"), tb=torch.empty((Bn,), dtype=torch.float64, device="cuda"),
                 tr=torch.empty((Bn,), dtype=torch.float64, device="cuda"), R=torch.empty((Bn, 9), dtype=torch.float64, device="cuda"),
                 t=torch.empty((Bn, 3), dtype=torch.float64, device="cuda"), s=torch.empty((Bn,), dtype=torch.float64, device="cuda"),
                 st=torch.empty((Bn,), dtype=torch.int32, device="cuda"))
        t0 = torch.as_tensor(tau0).cuda()
        p = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(L.gsf_clock_offset_search_dev(ctx.handle, p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), p(d[6]), p(d[5]), Bn, 130, p(t0), 0.05, K, GAP, 0, 0.0,
                                                 p(o["J"][1]), p(o["nr"][1]), p(o["bk"]), p(o["tb"]), p(o["tr"]), p(o["R"]), p(o["t"]), p(o["s"]), p(o["st"])))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    a = dev_route()
    for k in ("J", "nr"):                                                # nothing outside [B][K]
        assert (a[k][0] == (SENT if k == "J" else -9)).all() and (a[k][-1] == (SENT if k == "J" else -9)).all()
    # host arrays
    hp = _lib.hptr
    ho = dict(J=np.full((Bn, K), SENT), nr=np.full((Bn, K), -9, dtype=np.int32), bk=np.zeros(Bn, dtype=np.int32), tb=np.zeros(Bn), tr=np.zeros(Bn),
              R=np.zeros((Bn, 9)), t=np.zeros((Bn, 3)), s=np.zeros(Bn), st=np.zeros(Bn, dtype=np.int32))
    _lib.check(L.gsf_clock_offset_search(ctx.handle, hp(h[0]), hp(h[1]), hp(h[2]), hp(h[3]), hp(h[4]), hp(h[6]), hp(h[5]), Bn, hp(tau0), 0.05, K, GAP, 0, 0.0,
                                         hp(ho["J"]), hp(ho["nr"]), hp(ho["bk"]), hp(ho["tb"]), hp(ho["tr"]), hp(ho["R"]), hp(ho["t"]), hp(ho["s"]), hp(ho["st"])))
    for k in ho:
        got = a[k][1:-1] if k in ("J", "nr") else a[k]
        assert got.tobytes() == ho[k].tobytes(), k
    assert np.isfinite(ho["J"]).any() and np.isnan(ho["J"]).any()
    # the same call on workspaces filled with another word: the same bits
    try:
        for word in (0xA5, 0x00):
            ctx.set_option("poison_workspaces", word)
            b = dev_route()
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (k, word)
    finally:
        ctx.set_option("poison_workspaces", -1)


def test_logs_beyond_the_lds_staging_use_the_scratch_slab(B, orc):
    """max_fixes > 2 560 stages the logs in the context's scratch slab (one row per resident workgroup): the same numbers as the LDS route,
    on dirty scratch as well"""
    import torch
    tracks = [ref.make_track(65, 130), ref.make_track(130, 65), ref.make_track(5, 4)]
    d = _dev(_flat(tracks))
    arrs = d[:6]
    r_lds = B.estimate_clock_offset(arrs, tau0=0.2, dtau=0.05, K=5)

    class Big:                                                           # the batch form: max_fixes is the caller's
        pass
    b = Big()
    b.ts, b.pos, b.slam_offsets, b.gps_t, b.gps_offsets, b.max_fixes = arrs[0], arrs[1], arrs[2], arrs[3], arrs[5], 2561

    class Run:
        gps_utm, gps_keep = arrs[4], None
    ctx = B.context()
    try:
        ctx.set_option("poison_workspaces", 0x5A)
        r_slab = B.estimate_clock_offset(b, tau0=0.2, dtau=0.05, K=5, run=Run)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("poison_workspaces", -1)
    for k in ("J", "n_rows", "best_k", "tau_best", "tau_refined", "R", "t", "s", "status"):
        assert getattr(r_lds, k).cpu().numpy().tobytes() == getattr(r_slab, k).cpu().numpy().tobytes(), k
    assert torch.isfinite(r_lds.J).all()


# ---------------------------------------------------------------------------------------------------------------- 6. end to end, KITTI 04
def test_search_shift_run_on_the_bundled_kitti04_files(B, golden):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    g, k = golden("c1_kitti04gps.npz"), golden("kat_bundled.npz")
    log = np.column_stack((g["gps_t_raw"], g["lat"], g["lon"], g["alt"]))
    copies = 2
    rb = B.RaggedGeodeticBatch.from_host([(k["ts"], k["pos"], k["quat"])] * copies, [log] * copies)
    r = B.run_fusion_ragged(rb, B.mt19937_seed([0] * copies), E.CONFIG)
    assert (r.run_status == 0).all()
    est = B.estimate_clock_offset(rb, tau0=-1.0, dtau=0.05, K=41, run=r, flat_threshold=1e-3)
    torch.cuda.synchronize()
    J = est.J.cpu().numpy()
    print(f"KITTI 04: J spread {np.nanmax(J[0]) - np.nanmin(J[0]):.4g} m (min {np.nanmin(J[0]):.4g} m at tau {float(est.tau_best[0]):+.2f} s, refined "
          f"{float(est.tau_refined[0]):+.4f} s, status {int(est.status[0])})")
    assert (est.best_k >= 0).all() and torch.isfinite(est.tau_refined).all() and J.tobytes() == np.repeat(J[:1], copies, axis=0).tobytes()
    # a zero shift changes nothing: the whole run again, bit for bit
    r0 = B.run_fusion_ragged(rb.with_clock_offset(0.0 * est.tau_refined), B.mt19937_seed([0] * copies), E.CONFIG)
    torch.cuda.synchronize()
    for name in ("R", "t", "s", "n_inliers", "gps_utm", "gps_keep", "aligned", "valid", "sim3_pos", "err_stats", "run_status"):
        x, y = getattr(r, name), getattr(r0, name)
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name
    assert r.fused.pos.cpu().numpy().tobytes() == r0.fused.pos.cpu().numpy().tobytes()
    assert r.fused.quat.cpu().numpy().tobytes() == r0.fused.quat.cpu().numpy().tobytes()
    # the run with the estimated offset completes
    r1 = B.run_fusion_ragged(rb.with_clock_offset(est.tau_refined), B.mt19937_seed([0] * copies), E.CONFIG)
    torch.cuda.synchronize()
    assert (r1.run_status == 0).all() and torch.isfinite(r1.fused.pos).all()
