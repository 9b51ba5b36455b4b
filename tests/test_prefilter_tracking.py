"""GPS pre-filter on high-rate and long logs: scikit-learn's sample_without_replacement takes its TRACKING-SELECTION route once
min_samples / n <= 0.01 (n >= 100 min_samples rows: a 15 s window of a 40 Hz receiver, a global fit over 600 fixes).  The device sampler
(gsf_mt19937_sample_without_replacement_batch_dev, mt_draw_tracking in the chain) against live scikit-learn, the chain's windows and whole
filter against RANSACRegressor / the oracle, the chain's options, and whole runs on 50 Hz logs."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_run_chain import _oracle_run
from test_run_ragged import _oracle_run_gt, _synthetic_case, _log

pytestmark = pytest.mark.gpu


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


def np_state(st_row):
    a = st_row.cpu().numpy().view(np.uint32)
    return a[:624].copy(), int(a[624])


def _tracking_census(n, k, trials, key, pos):
    """restatement of scikit-learn's tracking selection on a copy of the generator: (duplicate rejections, trials that span a regeneration)"""
    rs = np.random.RandomState()
    rs.set_state(("MT19937", key.copy(), pos, 0, 0.0))
    dups = spans = 0
    for _ in range(trials):
        p0 = rs.get_state()[2]
        sel = set()
        for _ in range(k):
            j = rs.randint(n)
            while j in sel:
                dups += 1
                j = rs.randint(n)
            sel.add(j)
        p1 = rs.get_state()[2]
        spans += int(p1 < p0)                                            # the stream regenerated inside the trial
    return dups, spans


# ------------------------------------------------------------------------------------------------------------- 1. the sampler
def test_sampler_vs_live_sklearn(B):
    """batch.sample_without_replacement_batch over seeds, k = 1 .. 16 and 64, n in {k, 100k-1, 100k, 100k+1, 750, 14 000, 2^20, 2^31-1},
    1 .. 200 trials, several streams per call: every set (in draw order) and every final state equal to live scikit-learn's; streams with
    n < k untouched.  The grid must have exercised duplicate rejections and trials that straddle a regeneration."""
    import torch
    from sklearn.utils.random import sample_without_replacement
    rng = np.random.default_rng(3)
    dups = spans = tracking = 0
    for k in list(range(1, 17)) + [64]:
        ns = [k, 100 * k - 1, 100 * k, 100 * k + 1, 750, 14000, 2 ** 20, 2 ** 31 - 1, max(k - 1, 0)]
        for trials in (1, int(rng.integers(2, 40)), 200 if k in (1, 2, 6, 16, 64) else 7):
            seeds = rng.integers(0, 2 ** 31, len(ns))
            st = B.mt19937_seed(seeds)
            st0 = st.clone()
            idx = B.sample_without_replacement_batch(st, ns, trials, k).cpu().numpy()
            for b, n in enumerate(ns):
                if n < k:
                    assert torch.equal(st[b], st0[b]) and (idx[b] == 0).all(), (k, n)
                    continue
                rs = np.random.RandomState(int(seeds[b]))
                if k / n <= 0.01:
                    tracking += trials
                    d, s = _tracking_census(n, k, trials, *rs.get_state()[1:3])
                    dups += d; spans += s
                want = np.stack([sample_without_replacement(n, k, random_state=rs) for _ in range(trials)])
                np.testing.assert_array_equal(idx[b], want, err_msg=f"k={k} n={n} trials={trials}")
                key, pos = np_state(st[b])
                rk, rp = rs.get_state()[1:3]
                np.testing.assert_array_equal(key, rk, err_msg=f"k={k} n={n}"); assert pos == rp, (k, n)
    assert tracking > 1000 and dups >= 20 and spans >= 1, (tracking, dups, spans)


# ------------------------------------------------------------------------------------------------------------- 2. one window
def _window(rng, n, deg, share, rate):
    t = np.arange(n) / rate + rng.uniform(0, 0.01)                      # track-relative stamps (see test_gps_ransac_problems_vs_live_sklearn)
    base = np.column_stack((3.0 * t + 0.02 * t * t, -2.0 * t + 0.001 * t ** 3 if deg == 3 else -2.0 * t, 0.3 * t))
    p = base + np.array([450000.0, 5430000.0, 110.0]) + rng.normal(0, 0.4, (n, 3))
    bad = rng.random(n) < share
    p[bad, rng.integers(0, 3)] += rng.choice([-1, 1], bad.sum()) * rng.uniform(12, 300, bad.sum())
    return t, p


def test_one_window_vs_ransacregressor(B):
    """gsf_gps_prefilter_chain on ONE window of n >= 100 min_samples rows (log_status 0; it was 2 before the tracking route): kept rows and
    the generator afterwards equal to make_pipeline(PolynomialFeatures(d), RANSACRegressor(...)) per axis run live on the same seed --
    windows held in registers (min_samples 4, 400 .. 512 rows) and read from memory (600 .. 5 000 rows), degree 1 .. 3, 0 .. 45 % outliers."""
    from sklearn.linear_model import RANSACRegressor
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import PolynomialFeatures
    from gps_optimize_slam_amd import _lib
    L, h = _lib.load(), B.context().handle
    rng = np.random.default_rng(41)
    for case in range(24):
        in_regs = case % 3 == 0
        ms = 4 if in_regs else int(rng.integers(4, 7))
        n = int(rng.integers(400, 513)) if in_regs else int(rng.integers(max(600, 100 * ms), 5001))
        deg = int(rng.integers(1, 4)); share = float(rng.uniform(0, 0.45)); thr = float(rng.choice([2.0, 10.0]))
        trials = int(rng.choice([50, 100]))
        t, p = _window(rng, n, deg, share, max(n / 60.0, float(rng.uniform(20, 80))))   # (at most 60 s: well-conditioned cubic fits)
        np.random.seed(case)
        ref = np.ones(n, bool)
        try:
            for ax in range(3):
                m = make_pipeline(PolynomialFeatures(degree=deg), RANSACRegressor(min_samples=ms, residual_threshold=thr, max_trials=trials))
                m.fit(t.reshape(-1, 1), p[:, ax]); ref &= m[-1].inlier_mask_
        except ValueError:
            ref = None
        rk, rp = np.random.get_state()[1:3]
        np.random.seed(case)
        key, pos_ = np.random.get_state()[1:3]
        state = np.concatenate([key.astype(np.uint32), np.array([pos_], dtype=np.uint32)])
        keep, ws, ls = np.zeros(n, np.uint8), np.zeros(1, np.int32), np.full(1, -1, np.int32)
        wr, off, wo = np.array([0, n], np.int32), np.array([0, n], np.int64), np.array([0, 1], np.int64)
        tt, pp = np.ascontiguousarray(t), np.ascontiguousarray(p)
        _lib.check(L.gsf_gps_prefilter_chain(h, tt.ctypes.data, pp.ctypes.data, off.ctypes.data, 1, wr.ctypes.data, wo.ctypes.data, n, trials, ms, deg,
                                             thr, 0.99, state.ctypes.data, keep.ctypes.data, ws.ctypes.data, ls.ctypes.data))
        assert ls[0] == 0, (case, n, ms)
        if ref is None:
            assert ws[0] == 1 and not keep.any(), case
        else:
            assert ws[0] == 0, case
            np.testing.assert_array_equal(keep.astype(bool), ref, err_msg=f"case {case}: n={n} ms={ms} deg={deg}")
        np.testing.assert_array_equal(state[:624], rk, err_msg=str(case)); assert int(state[624]) == rp, case


# ------------------------------------------------------------------------------------------------------------- 3. whole filter
def _logs_mixed(rng, count):
    """sliding-window logs at 20 .. 80 Hz whose 15 s windows straddle 100 x min_samples = 600 rows (both sampler routes in one log),
    and global-mode logs of 1 000 .. 14 000 fixes"""
    logs = []
    for b in range(count):
        sliding = b % 4 != 3
        rate = float(rng.uniform(20, 80)) if sliding else float(rng.uniform(10, 50))
        n = int(rng.integers(300, 3000)) if sliding else int(rng.integers(1000, 14001))
        dt = 1.0 / rate * (1.0 + 0.3 * np.sin(np.arange(n) / 97.0))     # the rate drifts: window lengths cross 600 rows within a log
        t = np.cumsum(dt)
        p = np.column_stack((3.0 * t + 0.01 * t * t, -2.0 * t, 100 + 0.1 * t)) + np.array([450000.0, 5430000.0, 0.0]) + rng.normal(0, 0.4, (n, 3))
        bad = rng.random(n) < rng.uniform(0, 0.3)
        p[bad, b % 3] += rng.choice([-1, 1], bad.sum()) * rng.uniform(15, 200, bad.sum())
        logs.append((t, p, sliding))
    return logs


def test_whole_filter_vs_the_oracle(B, orc):
    """filter_gps_outliers_ransac as a whole: gsf_gps_prefilter_auto_dev (windows walked on the device) and the drop-in
    ekfgpsslam.filter_gps_outliers_ransac against the oracle, which calls scikit-learn's sampler live: kept rows, final generator state,
    log_status 0 -- on logs that take both sampler routes."""
    import torch
    from gps_optimize_slam_amd import _lib
    from gps_optimize_slam_amd import ekfgpsslam as E
    L, h = _lib.load(), B.context().handle
    logs = _logs_mixed(np.random.default_rng(8), 24)
    both = 0
    for sliding in (True, False):
        sel = [(t, p) for t, p, s in logs if s == sliding]
        f = dict(E.CONFIG["gps_filtering_ransac"], use_sliding_window=sliding)
        nl = len(sel)
        offs = np.zeros(nl + 1, dtype=np.int64); offs[1:] = np.cumsum([len(t) for t, _ in sel])
        T = torch.as_tensor(np.concatenate([t for t, _ in sel])).cuda(); P = torch.as_tensor(np.concatenate([p for _, p in sel])).cuda()
        O = torch.as_tensor(offs).cuda()
        mx = int(max(len(t) for t, _ in sel))
        seeds = np.arange(nl) + 31
        st = B.mt19937_seed(seeds)
        keep = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda"); ls = torch.full((nl,), -1, dtype=torch.int32, device="cuda")
        pc = _lib.PrefilterConfig.from_config(f)
        _lib.check(L.gsf_gps_prefilter_auto_dev(h, B._p(T), B._p(P), B._p(O), nl, mx, C.byref(pc), B._p(st), B._p(keep), B._p(ls), None))
        keep, ls = keep.cpu().numpy().astype(bool), ls.cpu().numpy()
        for b, (t, p) in enumerate(sel):
            assert ls[b] == 0, (sliding, b)
            if sliding:
                ranges, _ = E._prefilter_windows(t, f, 6)
                lens = [r1 - r0 for r0, r1 in ranges]
                both += int(min(lens) < 600 <= max(lens))
            np.random.seed(int(seeds[b]))
            ft, _ = orc.filter_gps_outliers_ransac(t, p, f)
            rk, rp = np.random.get_state()[1:3]
            np.testing.assert_array_equal(keep[offs[b]:offs[b + 1]], np.isin(t, ft), err_msg=f"sliding={sliding} log {b}")
            key, pos = np_state(st[b])
            np.testing.assert_array_equal(key, rk, err_msg=str(b)); assert pos == rp, (sliding, b)
            # the drop-in (its chain call, no host-drawn route) from the same seed
            np.random.seed(int(seeds[b]))
            dt_, _ = E.filter_gps_outliers_ransac(t, p, f)
            np.testing.assert_array_equal(dt_, ft, err_msg=f"drop-in sliding={sliding} log {b}")
            dk, dp = np.random.get_state()[1:3]
            np.testing.assert_array_equal(dk, rk); assert dp == rp
    assert both >= 5, both


# ------------------------------------------------------------------------------------------------------------- 4. options
def test_options_change_no_output_on_tracking_windows(B):
    """prefilter_speculate / prefilter_first_batch / prefilter_miss_batch on tracking windows with ~50 % outliers and max_trials >= 200
    (many batches, the first or miss batch beyond 32 trials: their doubling is clamped at the 64 models the chain holds): every word equal."""
    import torch
    from gps_optimize_slam_amd import _lib
    from gps_optimize_slam_amd import ekfgpsslam as E
    L, ctx = _lib.load(), B.context()
    rng = np.random.default_rng(12)
    logs = []
    for b in range(32):
        # 27 .. 34 Hz: 15 s windows of 400 .. 512 rows (min_samples 4: tracking selection on rows held in registers, speculative pass
        # included; min_samples 6: permutation); 45 .. 60 Hz: 675 .. 900 rows (tracking selection on rows read from memory)
        rate = float(rng.uniform(27, 34)) if b % 2 else float(rng.uniform(45, 60))
        n = int(rng.integers(800, 2500))
        t = np.arange(n) / rate
        p = np.column_stack((3.0 * t, -2.0 * t + 0.02 * t * t, 100 + 0.1 * t)) + rng.normal(0, 0.3, (n, 3))
        bad = rng.random(n) < 0.5
        p[bad] += rng.choice([-1, 1], (bad.sum(), 3)) * rng.uniform(15, 300, (bad.sum(), 3))
        logs.append((t, p))
    offs = np.zeros(len(logs) + 1, dtype=np.int64); offs[1:] = np.cumsum([len(t) for t, _ in logs])
    T = torch.as_tensor(np.concatenate([t for t, _ in logs])).cuda(); P = torch.as_tensor(np.concatenate([p for _, p in logs])).cuda()
    O = torch.as_tensor(offs).cuda()
    mx, nl = int(max(len(t) for t, _ in logs)), len(logs)
    outs = {}
    try:
        for ms in (4, 6):
            f = dict(E.CONFIG["gps_filtering_ransac"], min_samples=ms, max_trials=300, residual_threshold_meters=3.0)
            pc = _lib.PrefilterConfig.from_config(f)
            for spec in (0, 1):
                for fb in (1, 2, 5, 48, 64):
                    for mb in (1, 4, 7):
                        if spec == 0 and mb != 4:
                            continue
                        ctx.set_option("prefilter_speculate", spec); ctx.set_option("prefilter_first_batch", fb); ctx.set_option("prefilter_miss_batch", mb)
                        st = B.mt19937_seed(np.arange(nl) + 5)
                        keep = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda"); ls = torch.empty(nl, dtype=torch.int32, device="cuda")
                        info = torch.empty((nl, 2), dtype=torch.int32, device="cuda")
                        _lib.check(L.gsf_gps_prefilter_auto_dev(ctx.handle, B._p(T), B._p(P), B._p(O), nl, mx, C.byref(pc), B._p(st), B._p(keep), B._p(ls), B._p(info)))
                        outs[(ms, spec, fb, mb)] = (keep, ls, info, st)
    finally:
        ctx.set_option("prefilter_speculate", 1); ctx.set_option("prefilter_first_batch", 1); ctx.set_option("prefilter_miss_batch", 4)
    for ms in (4, 6):
        ref = outs[(ms, 0, 1, 4)]
        assert (ref[1] == 0).all() and (ref[2][:, 0] > 0).all()
        for key, cur in outs.items():
            if key[0] == ms:
                for a, b_ in zip(ref, cur):
                    assert torch.equal(a, b_), key


# ------------------------------------------------------------------------------------------------------------- 5. whole runs
def _track_with_rate(orc, n, seed, rate, rng, sigma=0.3, outliers=True):
    tt, pp, qq, uu = _synthetic_case(orc, n, seed)
    tg = tt[0] + np.arange(int((tt[-1] - tt[0]) * rate) + 1) / rate
    ug = np.column_stack([np.interp(tg, tt, uu[:, c]) for c in range(3)])
    log = _log(orc, tg, ug, rng, sigma, 0.003)
    if outliers:
        m = len(log)
        for r_ in rng.choice(m, size=max(1, m // 200), replace=False):
            log[r_, 1] += 60.0 / 111200.0 * rng.choice([-1, 1]); log[r_, 2] += 60.0 / 73000.0 * rng.choice([-1, 1])
    return (tt, pp, qq), log


def _check_run(o, r, b, p, q, keep, rs, go, k=1.0):
    assert rs[b] == o["status"], (b, rs[b], o["status"])
    np.testing.assert_array_equal(keep[go[b]:go[b + 1]], o["keep"] if "keep" in o else o["primary"]["keep"], err_msg=str(b))
    if o["status"] == 0:
        assert int(r.n_inliers[b]) == o["n_inliers"], b
        np.testing.assert_allclose(r.R[b].cpu().numpy().reshape(3, 3), o["R"], atol=2e-9 * k, rtol=0)
        assert abs(float(r.s[b]) - o["s"]) < 1e-11 * k
        assert np.abs(p - o["pos"]).max() < 1e-6 * k and np.abs(q - o["quat"]).max() < 1e-8 * k, (b, np.abs(p - o["pos"]).max())


def test_whole_runs_on_50_hz_logs(B, orc):
    """run_fusion_batch on 50 Hz logs (15 s windows of 750 fixes: tracking selection) and run_fusion_ragged with a 50 Hz ground-truth log
    under ground_truth_gps_filtering: no track flagged UNHANDLED / GT_UNHANDLED, every word against the oracle's compositions with the gates
    of test_run_chain / test_run_ragged."""
    from gps_optimize_slam_amd import _lib
    from gps_optimize_slam_amd import ekfgpsslam as E
    rng = np.random.default_rng(50)
    nb, N = 12, 271
    tracks, logs = zip(*[_track_with_rate(orc, N, b, 50.0, rng) for b in range(nb)])
    ts, pos, quat = (np.stack([tr[i] for tr in tracks]) for i in range(3))
    cfg = copy.deepcopy(E.CONFIG)
    gb = B.GeodeticBatch.from_host(ts, pos, quat, list(logs))
    seeds = np.arange(nb) + 70
    st = B.mt19937_seed(seeds)
    r = B.run_fusion_batch(gb, st, cfg, early_exit=False)
    p, q, _ = r.fused.host_traj_major()
    rs, keep, go = r.run_status.cpu().numpy(), r.gps_keep.cpu().numpy().astype(bool), gb.gps_offsets.cpu().numpy()
    assert not (rs & _lib.RUN_PREFILTER_UNHANDLED).any(), rs
    for b in range(nb):
        o = _oracle_run(orc, ts[b], pos[b], quat[b], logs[b], cfg, int(seeds[b]))
        key, ppos = np.random.get_state()[1:3]
        gk, gp = np_state(st[b])
        np.testing.assert_array_equal(gk, key, err_msg=str(b)); assert gp == int(ppos), b
        assert o["status"] == 0 and o["keep"].sum() < len(o["keep"]), b
        fr, al = o["fit_rows"], o["aligned"]
        sv = np.linalg.svd((pos[b][fr] - pos[b][fr].mean(0)).T @ (al[fr] - al[fr].mean(0)), compute_uv=False)
        _check_run(o, r, b, p[b], q[b], keep, rs, go, k=max(1.0, float(sv[0] / max(sv[1] + sv[2], 1e-300)) / 100.0))   # (test_run_ragged's gates)
    # ragged, 50 Hz ground truth through its enabled filter
    cfg["ground_truth_gps_filtering"]["enabled"] = True
    rng = np.random.default_rng(51)
    tr2, lg2, gt2 = [], [], []
    for b in range(8):
        n = int(rng.integers(150, 500))
        (tt, pp, qq), log = _track_with_rate(orc, n, 20 + b, 10.0, rng)
        _, gt = _track_with_rate(orc, n, 20 + b, 50.0, rng, sigma=0.15)
        tr2.append((tt, pp, qq)); lg2.append(log); gt2.append(gt)
    rb = B.RaggedGeodeticBatch.from_host(tr2, lg2, gt2)
    seeds = np.arange(8) + 300
    st = B.mt19937_seed(seeds)
    r = B.run_fusion_ragged(rb, st, cfg, early_exit=False)
    rs = r.run_status.cpu().numpy()
    assert not (rs & (_lib.RUN_PREFILTER_UNHANDLED | _lib.RUN_GT_UNHANDLED)).any(), rs
    so, go, to = (x.cpu().numpy() for x in (rb.slam_offsets, rb.gps_offsets, rb.gt_offsets))
    p, q = r.fused.pos.cpu().numpy(), r.fused.quat.cpu().numpy()
    keep, gkeep = r.gps_keep.cpu().numpy().astype(bool), r.gt_keep.cpu().numpy().astype(bool)
    stats = r.err_stats.cpu().numpy()
    for b in range(8):
        ts_, pos_, quat_ = tr2[b]
        o = _oracle_run_gt(orc, ts_, pos_, quat_, lg2[b], gt2[b], cfg, int(seeds[b]))
        key, ppos = np.random.get_state()[1:3]
        gk, gp = np_state(st[b])
        np.testing.assert_array_equal(gk, key, err_msg=str(b)); assert gp == int(ppos), b
        assert o["status"] == 0, b
        np.testing.assert_array_equal(gkeep[to[b]:to[b + 1]], o["gt"]["keep"], err_msg=str(b))
        sl = slice(so[b], so[b + 1])
        _check_run(o, r, b, p[sl], q[sl], keep, rs, go, k=max(1.0, o["amp"] / 100.0))
        for row in range(3):
            e = o["errs_gt"][row]
            assert int(stats[1, row, b, 0]) == e["count"]
            if e["count"]:
                np.testing.assert_allclose(stats[1, row, b, 1:], [e["mean"], e["median"], e["rmse"]], rtol=1e-12, atol=1e-6)


def test_mixed_rates_batch_equals_one_track_per_call(B, orc):
    """10 Hz, 50 Hz and thinned logs in one batch: every output word equal to the same tracks run one per call."""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    rng = np.random.default_rng(60)
    tracks, logs = [], []
    for b in range(9):
        (tt, pp, qq), log = _track_with_rate(orc, 271, 40 + b, (10.0, 50.0, 50.0)[b % 3], rng)
        if b % 3 == 2:
            log = log[np.sort(rng.choice(len(log), size=len(log) // 3, replace=False))]   # thinned: windows on both sides of 600 rows
        tracks.append((tt, pp, qq)); logs.append(log)
    cfg = copy.deepcopy(E.CONFIG)
    seeds = np.arange(9) + 11
    rb = B.RaggedGeodeticBatch.from_host(tracks, logs)
    st = B.mt19937_seed(seeds)
    r = B.run_fusion_ragged(rb, st, cfg, early_exit=True)
    so = rb.slam_offsets.cpu().numpy(); go = rb.gps_offsets.cpu().numpy()
    assert (r.run_status == 0).all(), r.run_status
    for b in range(9):
        rb1 = B.RaggedGeodeticBatch.from_host([tracks[b]], [logs[b]])
        st1 = B.mt19937_seed(seeds[b:b + 1])
        r1 = B.run_fusion_ragged(rb1, st1, cfg, early_exit=True)
        sl, gl = slice(so[b], so[b + 1]), slice(go[b], go[b + 1])
        for a, c in ((r.fused.pos[sl], r1.fused.pos), (r.fused.quat[sl], r1.fused.quat), (r.R[b], r1.R[0]), (r.t[b], r1.t[0]), (r.s[b:b + 1], r1.s),
                     (r.err_stats[:, :, b], r1.err_stats[:, :, 0]), (r.sim3_pos[sl], r1.sim3_pos)):
            assert torch.equal(torch.nan_to_num(a, nan=-1.0).view(torch.int64), torch.nan_to_num(c, nan=-1.0).view(torch.int64)), b
        assert torch.equal(r.gps_keep[gl], r1.gps_keep) and torch.equal(st[b], st1[0]) and int(r.n_inliers[b]) == int(r1.n_inliers[0]), b
        assert torch.equal(r.fused.status[b:b + 1], r1.fused.status) and torch.equal(r.run_status[b:b + 1], r1.run_status), b


# ------------------------------------------------------------------------------------------------------------- 6. still flagged
def test_unsorted_stamps_still_flagged(B):
    """a sliding-window log with unsorted stamps keeps log_status 3 and its generator untouched, next to a 50 Hz log that is filtered"""
    import torch
    from gps_optimize_slam_amd import _lib
    from gps_optimize_slam_amd import ekfgpsslam as E
    L, h = _lib.load(), B.context().handle
    rng = np.random.default_rng(2)
    t0 = np.arange(2000) / 50.0
    t1 = t0.copy(); t1[700], t1[701] = t1[701], t1[700]
    logs = [(t0, rng.normal(0, 0.3, (2000, 3)) + t0[:, None]), (t1, rng.normal(0, 0.3, (2000, 3)) + t1[:, None])]
    offs = np.array([0, 2000, 4000], dtype=np.int64)
    T = torch.as_tensor(np.concatenate([t for t, _ in logs])).cuda(); P = torch.as_tensor(np.concatenate([p for _, p in logs])).cuda()
    O = torch.as_tensor(offs).cuda()
    st = B.mt19937_seed([1, 2]); st0 = st.clone()
    keep = torch.empty(4000, dtype=torch.uint8, device="cuda"); ls = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    pc = _lib.PrefilterConfig.from_config(E.CONFIG["gps_filtering_ransac"])
    _lib.check(L.gsf_gps_prefilter_auto_dev(h, B._p(T), B._p(P), B._p(O), 2, 2000, C.byref(pc), B._p(st), B._p(keep), B._p(ls), None))
    assert ls.tolist() == [0, 3]
    assert not torch.equal(st[0], st0[0]) and torch.equal(st[1], st0[1])
