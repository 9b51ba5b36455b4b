"""GPU tier of the pre-filter's polynomial fit: the kernels of csrc/gsf_gpsfilter.hip against the 50-digit yardstick of
tests/prefilter_fit_ref.py, through the C ABI (contract: include/gsf.h, DESIGN.md "Domain of the pre-filter's fit").

The entries return masks, not models, so the fit is READ THROUGH THE MASK: one fed sample per problem (max_trials = 1), and at every probe
stamp a ladder of extra rows on that same stamp whose targets are exact(t) +- thr + e_k.  A ladder row is an inlier iff the device's
prediction error err(t) lies on the right side of e_k, so the mask brackets err(t) to one ladder step; every determined case must bracket it
inside C_GATE x b(t).  Shift invariance is exact: logs on a 2^-20 s grid return the same bytes with 0, 130, 2^20 and 1.3e9 s added to every
stamp, on all four entries, and those bytes are the exact replay's.  Logs of a receiver that repeats its stamps go through the chain against
the exact replay under the rank rule, and against scikit-learn live."""
import ctypes as C

import numpy as np
import pytest

import prefilter_fit_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def _d(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the fit, read through the mask
FINE = (0.25, 0.5, 1.0, 2.0, 4.0)                    # rungs below the gate, in units of b(t): what the device's error is REPORTED to (not asserted)


def _ladder(c):
    """rows appended to case c: [(probe row, side, e' (mp: the stored target minus exact minus side thr), is the gate's rung)], stamps, targets,
    and how many of the three wanted probes (first row, last row, the sample's first row) the ladder cannot read"""
    mp = R._mp()
    thr = c["thr"]
    # the mask reads an error only while |e' - err| < 2 thr, and the ladder ends at 1e-3 thr: a probe whose gate lies beyond that (the far end
    # of a window for a degree-8 sample bunched at the other end: Lambda ~ 1e9) cannot be read here and stays with the CPU tier
    readable = lambda i: R.C_GATE * c["bound"][i] <= 1e-3 * thr
    wanted = {c["probes"][0], c["probes"][-1], int(c["idx"][0])}
    probes = sorted(i for i in wanted if readable(i))
    dropped = len(wanted) - len(probes)
    if not probes:
        probes = [i for i in sorted(c["probes"], key=lambda j: c["bound"][j])[:1] if readable(i)]
    meta, ts, ys = [], [], []
    for i in probes:
        E, b = c["exact"][i], c["bound"][i]
        g = R.C_GATE * b
        rungs = [(f * b, False) for f in FINE if f * b < g] + [(g, True)]
        e = 2 * g
        while e <= 1e-3 * thr:
            rungs.append((e, False)); e *= 2
        for mag, gate in rungs:
            for sign in (-1.0, 1.0):
                for side in (-1.0, 1.0):
                    y = float(E + side * thr + sign * mag)
                    ep = mp.mpf(y) - E - side * thr
                    if gate:                                             # the gate's own rung: the stored target may not lie outside C_GATE b(t)
                        while abs(ep) > g:
                            y = float(np.nextafter(y, float(E + side * thr)))
                            ep = mp.mpf(y) - E - side * thr
                    meta.append((i, side, float(ep), gate))
                    ts.append(c["t"][i]); ys.append(y)
    return meta, np.array(ts), np.array(ys), dropped


def _bracket(meta, inl):
    """{probe: [lo, hi]} of err = device prediction - exact: y = exact + side thr + e' is an inlier iff side (e' - err) <= 0"""
    out = {}
    for (i, side, ep, _), m in zip(meta, inl):
        lo, hi = out.setdefault(i, [-np.inf, np.inf])
        if (side > 0) == bool(m):                                        # side +, inlier: err >= e';  side -, outlier: err > e'
            out[i][0] = max(lo, ep)
        else:                                                            # side +, outlier: err < e';  side -, inlier: err <= e'
            out[i][1] = min(hi, ep)
    return out


def test_fit_read_through_the_mask_fed_sample_kernels(B):
    """ransac_poly_kernel (scratch form: degree <= 3, <= 16 samples) and ransac_poly_wide_kernel (degree 4, 5, 8; up to 64 samples): every
    determined case of cases() inside C_GATE b(t), every rank-open case at the exact polynomial of degree (distinct stamps - 1)."""
    cs = R.cases()
    groups = {}
    for ci, c in enumerate(cs):
        groups.setdefault((c["degree"], c["ms"], c["thr"]), []).append(ci)
    worst = {"fast": (0.0, ""), "wide": (0.0, ""), "open": (0.0, "")}
    unread, dropped = [], {}
    for (deg, ms, thr), members in sorted(groups.items()):
        T, Y, offs, idx, metas = [], [], [0], [], []
        for ci in members:
            c = cs[ci]
            meta, lt, ly, nd = _ladder(c)
            if nd:
                dropped[c["name"]] = nd
            T += [c["t"], lt]; Y += [c["y"], ly]
            offs.append(offs[-1] + len(c["t"]) + len(lt)); idx.append(c["idx"]); metas.append(meta)
        mask, ntr, nin, st = B.ransac_poly_batch(_d(np.concatenate(T)), _d(np.concatenate(Y)), _d(np.array(offs, dtype=np.int64)),
                                                 _d(np.stack(idx).astype(np.int32).reshape(len(members), 1, ms)), deg, thr)
        mask, st = mask.cpu().numpy(), st.cpu().numpy()
        assert (st == 0).all(), (deg, ms, st.tolist())
        for k, ci in enumerate(members):
            c = cs[ci]
            n = len(c["t"])
            br = _bracket(metas[k], mask[offs[k] + n:offs[k + 1]])
            if not br:
                unread.append(c["name"])
            for i, (lo, hi) in br.items():
                g = R.C_GATE * c["bound"][i]
                assert -g <= lo <= hi <= g, (c["name"], c["route"], i, lo, hi, g, "the device's prediction error leaves C_GATE x b(t)")
                key = "open" if c["klass"] != "determined" else c["route"]
                r = max(abs(lo), abs(hi)) / c["bound"][i]
                if r > worst[key][0]:
                    worst[key] = (r, c["name"])
    print("device prediction error bracketed to (units of b(t), gate %.2f):" % R.C_GATE, {k: (round(v[0], 2), v[1]) for k, v in worst.items()})
    print(f"probes left out of the ladder (gate beyond 1e-3 thr), {sum(dropped.values())} in {len(dropped)} cases:", dropped)
    print("no probe readable through the mask (gate beyond 1e-3 thr at every probe):", unread)
    assert all(n.startswith("wide-d8") and "bunched" in n for n in dropped), dropped   # only degree-8 samples bunched at one end of their window
    assert all(n.startswith("wide-d8") and "bunched" in n for n in unread) and len(unread) <= 1
    assert worst["fast"][0] > 0 and worst["wide"][0] > 0 and worst["open"][0] > 0


# ------------------------------------------------------------------------------------------------ the chain entries
def _chain(B, logs, seeds, degree, ms, thr, trials, width):
    """gsf_gps_prefilter_chain (host arrays, host-listed windows) for several logs: keep [per log], win_status [per log], state (nl, 625)"""
    from gps_optimize_slam_amd import _lib
    L, h = _lib.load(), B.context().handle
    wins = [R.windows(t, width, 0.5, ms) if width else [(0, len(t))] for t, _ in logs]
    offs = np.zeros(len(logs) + 1, dtype=np.int64); offs[1:] = np.cumsum([len(t) for t, _ in logs])
    wo = np.zeros(len(logs) + 1, dtype=np.int64); wo[1:] = np.cumsum([len(w) for w in wins])
    wr = np.ascontiguousarray(np.array([r for w in wins for r in w], dtype=np.int32).reshape(-1, 2))
    tt = np.ascontiguousarray(np.concatenate([t for t, _ in logs])); pp = np.ascontiguousarray(np.concatenate([p for _, p in logs]))
    state = np.ascontiguousarray(np.stack([R.seed_state(s) for s in seeds]))
    keep, ws, ls = np.zeros(len(tt), np.uint8), np.full(len(wr), -1, np.int32), np.full(len(logs), -1, np.int32)
    _lib.check(L.gsf_gps_prefilter_chain(h, tt.ctypes.data, pp.ctypes.data, offs.ctypes.data, len(logs), wr.ctypes.data, wo.ctypes.data,
                                         int(max(b - a for a, b in wr)), trials, ms, degree, thr, 0.99, state.ctypes.data, keep.ctypes.data,
                                         ws.ctypes.data, ls.ctypes.data))
    assert (ls == 0).all(), ls.tolist()
    return ([keep[offs[b]:offs[b + 1]] for b in range(len(logs))], [ws[wo[b]:wo[b + 1]] for b in range(len(logs))], state)


def _auto(B, logs, seeds, cfg):
    """gsf_gps_prefilter_auto_dev (windows walked on the device): keep [per log], state (nl, 625)"""
    import torch
    from gps_optimize_slam_amd import _lib
    L, h = _lib.load(), B.context().handle
    offs = np.zeros(len(logs) + 1, dtype=np.int64); offs[1:] = np.cumsum([len(t) for t, _ in logs])
    T, P, O = _d(np.concatenate([t for t, _ in logs])), _d(np.concatenate([p for _, p in logs])), _d(offs)
    st = B.mt19937_seed(np.array(seeds))
    keep = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda"); ls = torch.full((len(logs),), -1, dtype=torch.int32, device="cuda")
    pc = _lib.PrefilterConfig.from_config(cfg)
    _lib.check(L.gsf_gps_prefilter_auto_dev(h, B._p(T), B._p(P), B._p(O), len(logs), int(max(len(t) for t, _ in logs)), C.byref(pc), B._p(st),
                                            B._p(keep), B._p(ls), None))
    assert (ls.cpu().numpy() == 0).all()
    keep = keep.cpu().numpy()
    return [keep[offs[b]:offs[b + 1]] for b in range(len(logs))], st.cpu().numpy().view(np.uint32)


CFG = {"enabled": True, "use_sliding_window": True, "window_duration_seconds": 15.0, "window_step_factor": 0.5, "polynomial_degree": 2,
       "min_samples": 6, "residual_threshold_meters": 10.0, "max_trials": 50}


@pytest.fixture(scope="module")
def dyadic():
    """six 30 s logs on the 2^-20 s grid whose exact replay (CONFIG's pre-filter: 15 s windows, degree 2, 6 samples) keeps clear of every decision"""
    return R.usable_seeds(lambda s: R.dyadic_log(s, n=240, width=30.0), lambda log, s: R.replay_log(*log, s, 2, 6, 10.0, 50, width=15.0), 6)


@pytest.mark.parametrize("ms", [6, 12])
def test_chain_register_forms_against_the_exact_replay(B, ms):
    """gps_prefilter_chain_kernel with host-listed windows -- fit_subset_regs<3,8> at 6 samples, <3,16> at 12 -- draws its own samples: keep
    mask, window status and generator state are the exact replay's, on Unix-sized stamps (1.3e9 s added)."""
    picked = R.usable_seeds(lambda s: R.dyadic_log(s, n=240, width=30.0), lambda log, s: R.replay_log(*log, s, 2, ms, 10.0, 50, width=15.0), 4, first_seed=40)
    logs = [(log[0] + 1.3e9, log[1]) for _, log, _ in picked]
    keep, ws, state = _chain(B, logs, [s for s, _, _ in picked], 2, ms, 10.0, 50, 15.0)
    for b, (seed, _, r) in enumerate(picked):
        np.testing.assert_array_equal(keep[b], r["keep"], err_msg=f"seed {seed}")
        np.testing.assert_array_equal(ws[b], r["win_status"], err_msg=f"seed {seed}")
        np.testing.assert_array_equal(state[b], r["state"], err_msg=f"seed {seed}")


# ------------------------------------------------------------------------------------------------ 2. shift invariance, exact
@pytest.mark.parametrize("degree,ms", [(2, 6), (4, 10)])
def test_shift_invariance_fed_sample_entry(B, dyadic, degree, ms):
    """ransac_poly_batch (degree 2 from 6 samples: ransac_poly_kernel; degree 4 from 10: the wide kernel): the northing of every log with 50
    fed sample sets, stamps + 0 / 130 / 2^20 / 1.3e9 s: mask, n_trials, inlier count and status are the same bytes, and the exact replay's"""
    rng = np.random.default_rng(5)
    n = 240
    idx = np.stack([np.stack([rng.choice(n, ms, replace=False) for _ in range(50)]) for _ in dyadic]).astype(np.int32)
    offs = np.arange(len(dyadic) + 1, dtype=np.int64) * n
    Y = np.concatenate([log[1][:, 1] for _, log, _ in dyadic])
    outs = []
    for shift in R.SHIFTS:
        T = np.concatenate([log[0] + shift for _, log, _ in dyadic])
        outs.append([o.cpu().numpy() for o in B.ransac_poly_batch(_d(T), _d(Y), _d(offs), _d(idx), degree, 10.0)])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)
    replayed = 0
    for k, (seed, log, _) in enumerate(dyadic):
        r = R.replay_fed(log[0], log[1][:, 1], list(idx[k]), degree, 10.0)
        replayed += int(R.usable(r))
        if R.usable(r):
            np.testing.assert_array_equal(outs[0][0][k * n:(k + 1) * n], r["mask"].astype(np.uint8), err_msg=str(seed))
            assert (outs[0][1][k], outs[0][2][k], outs[0][3][k]) == (r["n_trials"], r["n_inliers"], r["status"]), seed
    assert replayed >= len(dyadic) - 1                                  # (fed sets drawn here, not by the seed: at most one replay may come close to a decision)


def test_shift_invariance_chain_and_auto_entries(B, dyadic):
    """gps_prefilter_chain (host-listed windows) and gps_prefilter_auto (windows walked on the device): keep mask, window status and the
    625-word generator state are the same bytes under the four shifts, equal between the two entries, and the exact replay's"""
    seeds = [s for s, _, _ in dyadic]
    first = None
    for shift in R.SHIFTS:
        logs = [(log[0] + shift, log[1]) for _, log, _ in dyadic]
        keep, ws, state = _chain(B, logs, seeds, 2, 6, 10.0, 50, 15.0)
        keep_a, state_a = _auto(B, logs, seeds, CFG)
        got = (np.concatenate(keep).tobytes(), np.concatenate(ws).tobytes(), state.tobytes())
        assert (np.concatenate(keep_a).tobytes(), state_a.tobytes()) == (got[0], got[2]), shift
        if first is None:
            first = got
            for b, (seed, _, r) in enumerate(dyadic):
                np.testing.assert_array_equal(keep[b], r["keep"], err_msg=f"seed {seed}")
                np.testing.assert_array_equal(ws[b], r["win_status"], err_msg=f"seed {seed}")
                np.testing.assert_array_equal(state[b], r["state"], err_msg=f"seed {seed}")
        assert got == first, shift


def _near_miss_log(seed):
    """a clean log (no spikes) with two fixes 11 m off in northing, one in each half: just outside the 10 m threshold"""
    t, p = R.dyadic_log(seed, n=240, width=30.0, spikes=0.0)
    for k, at in enumerate((5.0, 25.0)):
        p[int(np.argmin(np.abs(t - at))), 1] += 11.0 * (1.0 if (seed + k) % 2 else -1.0)
    return t, p


def test_shift_invariance_speculative_pass(B):
    """the chain's speculative pass (one trial per axis, accepted when it counts every row of the window): on clean windows it decides the
    axis, and on a window with ONE fix just outside the threshold a model that is metres off takes that fix in and ends the axis early --
    a model that under-counts only falls back to the sequential walk, which is why the spiked logs above cannot see this pass.  Same bytes
    under the four shifts, and the exact replay's."""
    picked = R.usable_seeds(_near_miss_log, lambda log, s: R.replay_log(*log, s, 2, 6, 10.0, 50, width=15.0), 8, first_seed=300)
    assert sum(int(n == 1) for _, _, r in picked for n in r["n_trials"]) >= 20          # axes that one trial decides: the pass is used
    assert sum(int(n > 1) for _, _, r in picked for n in r["n_trials"]) >= 8           # ... and axes it must hand over
    seeds = [s for s, _, _ in picked]
    for shift in R.SHIFTS:
        keep, ws, state = _chain(B, [(log[0] + shift, log[1]) for _, log, _ in picked], seeds, 2, 6, 10.0, 50, 15.0)
        for b, (seed, _, r) in enumerate(picked):
            np.testing.assert_array_equal(keep[b], r["keep"], err_msg=f"seed {seed} shift {shift}")
            np.testing.assert_array_equal(ws[b], r["win_status"], err_msg=f"seed {seed} shift {shift}")
            np.testing.assert_array_equal(state[b], r["state"], err_msg=f"seed {seed} shift {shift}")


def test_shift_invariance_whole_run_entry(B, dyadic):
    """run_fusion_batch with the pre-filter enabled, from projected logs, SLAM stamps shifted alike.  Under the four shifts: run_status is 0,
    the fixes that survive the pre-filter (gps_keep) are the same bytes and the exact replay's, and the 625-word generator state and the
    fit's trial_info are the same bytes.  early_exit=False: the robust fit after the pre-filter then draws all its max_trials sample sets
    from the same generator, a count that depends only on the rows time alignment marks valid -- so the state differs between shifts iff
    the pre-filter's own consumption (its n_trials per window and axis) does, also where the final mask would hide that."""
    from gps_optimize_slam_amd import ekfgpsslam as E
    import copy
    cfg = copy.deepcopy(E.CONFIG)
    cfg["gps_filtering_ransac"] = dict(CFG)
    N = 120
    sec = np.arange(N) * 0.25
    seeds = [s for s, _, _ in dyadic]
    first = None
    for shift in R.SHIFTS:
        ts, pos, quat, logs = [], [], [], []
        for _, (t, p), _ in dyadic:
            clean = np.column_stack((4.5e5 + 9.0 * sec, 5.4e6 - 4.0 * sec + 0.1 * sec * sec, 110.0 + 0.1 * sec))
            ts.append(sec + shift); pos.append((clean - clean[0]) / 1.02); quat.append(np.tile([0.0, 0.0, 0.0, 1.0], (N, 1)))
            logs.append(np.column_stack((t + shift, p)))
        gb = B.GeodeticBatch.from_host(np.stack(ts), np.stack(pos), np.stack(quat), logs)
        st = B.mt19937_seed(np.array(seeds))
        st0 = st.cpu().numpy().copy()
        r = B.run_fusion_batch(gb, st, cfg, early_exit=False, projected=True)
        got = dict(run_status=r.run_status.cpu().numpy(), keep=r.gps_keep.cpu().numpy(), state=st.cpu().numpy().view(np.uint32).copy(),
                   trial_info=r.trial_info.cpu().numpy(), valid=r.valid.cpu().numpy())
        assert (got["run_status"] == 0).all(), (shift, got["run_status"].tolist())
        assert (got["state"] != st0.view(np.uint32)).any(axis=1).all(), shift      # every log's generator was drawn from
        if first is None:
            first = got
            np.testing.assert_array_equal(got["keep"], np.concatenate([rr["keep"] for _, _, rr in dyadic]))
        for k, v in got.items():
            np.testing.assert_array_equal(v, first[k], err_msg=f"{k} at shift {shift}")


# ------------------------------------------------------------------------------------------------ 3. repeated stamps
MOVED_BY_MINIMUM_NORM = {(210, 16), (210, 17)}         # (seed, row): the rows live scikit-learn decides otherwise, all on the thrice logs


def _sklearn_axes(t, p, degree, ms, thr, trials, seed):
    """make_pipeline(PolynomialFeatures, RANSACRegressor) per axis, live, on the legacy global generator: (per-axis masks or None, keep, generator state)"""
    from sklearn.linear_model import RANSACRegressor
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import PolynomialFeatures
    np.random.seed(seed)
    masks, keep = [], np.ones(len(t), bool)
    try:
        for ax in range(3):
            m = make_pipeline(PolynomialFeatures(degree=degree), RANSACRegressor(min_samples=ms, residual_threshold=thr, max_trials=trials))
            m.fit(t.reshape(-1, 1), p[:, ax])
            masks.append(m[-1].inlier_mask_.copy()); keep &= masks[-1]
    except ValueError:
        keep[:] = False
    _, key, pos, _, _ = np.random.get_state()
    return masks, keep, np.concatenate([key.astype(np.uint32), np.array([pos], dtype=np.uint32)])


def _minimum_norm_residuals(t, y, idx, degree):
    """|y - prediction| of LinearRegression on PolynomialFeatures of the RAW stamps for one sample: the minimum-norm solution in scikit-learn's basis"""
    X = np.vander(t, degree + 1, increasing=True)
    Xs, ys = X[idx], y[idx]
    xo, yo = Xs.mean(axis=0), ys.mean()
    coef = np.linalg.lstsq(Xs - xo, ys - yo, rcond=None)[0]
    return np.abs(y - (X @ coef + (yo - xo @ coef)))


def test_repeating_receiver_through_the_chain(B):
    """Logs of a receiver that repeats stamps three times running, one global window, degree 3 from 4 samples, through the chain: keep mask,
    window status and generator state are the exact replay's under the rank rule.  Two kinds of log.  FEW: 60 rows with four repeated
    stamps -- most walks draw no rank-open sample, and such a log must equal live scikit-learn (same track-relative stamps, same seed) row
    for row and in the generator state.  THRICE: every stamp three times (18 rows on 6 stamps): every walk draws samples with fewer than 4
    distinct stamps.  scikit-learn answers those with the minimum-norm solution in ITS basis (raw t, t^2, t^3): the same values at the
    sample's stamps, another polynomial away from them.  The rows it therefore decides otherwise are exactly MOVED_BY_MINIMUM_NORM; for each,
    the sample the walk accepted on the deciding axis is rank-open, the row lies off that sample's stamps, and the message names its
    residual under that sample's model by the rank rule and by the minimum norm."""
    few = R.usable_seeds(lambda s: R.dyadic_log(s, n=60, width=15.0, spikes=0.1, repeat=4), lambda log, s: R.replay_log(*log, s, 3, 4, 10.0, 50), 12, first_seed=400)
    thrice = R.usable_seeds(lambda s: R.dyadic_log(s, n=18, width=15.0, spikes=0.15, thrice=True), lambda log, s: R.replay_log(*log, s, 3, 4, 10.0, 50), 16, first_seed=200)
    picked = few + thrice
    keep, ws, state = _chain(B, [log for _, log, _ in picked], [s for s, _, _ in picked], 3, 4, 10.0, 50, None)
    n_plain, moved, lines = 0, set(), []
    for b, (seed, (t, p), r) in enumerate(picked):
        assert len(set(t.tolist())) < len(t)                                       # the receiver did repeat stamps
        np.testing.assert_array_equal(ws[b], r["win_status"], err_msg=f"seed {seed}")
        np.testing.assert_array_equal(keep[b], r["keep"], err_msg=f"seed {seed}")
        np.testing.assert_array_equal(state[b], r["state"], err_msg=f"seed {seed}")
        sk_masks, sk_keep, sk_state = _sklearn_axes(t, p, 3, 4, 10.0, 50, seed)
        diff = np.nonzero(sk_keep != keep[b].astype(bool))[0]
        if r["n_open"] == 0:                                                       # no rank-open sample drawn: nothing to decide differently
            n_plain += 1
            assert diff.size == 0, (f"seed {seed}: no rank-open sample was drawn, yet scikit-learn decides rows {diff.tolist()} otherwise",
                                    [(int(i), float(t[i]), p[i].tolist()) for i in diff])
            np.testing.assert_array_equal(state[b], sk_state, err_msg=f"seed {seed}: generator state against live scikit-learn")
            continue
        for i in diff:
            ax = next(a for a in range(3) if a >= len(sk_masks) or sk_masks[a][i] != r["fits"][a]["mask"][i])     # the axis that decides the row
            idx = r["fits"][ax]["best_idx"]
            stamps = sorted(set(t[idx].tolist()))
            res_rank = float(R.exact_residuals(t, p[:, ax], idx, 3, t[0])[0][i])
            res_min = float(_minimum_norm_residuals(t, p[:, ax], idx, 3)[i])
            line = (f"seed {seed} row {int(i)} (t = {t[i]:.6f} s), axis {ax}: kept {bool(keep[b][i])} here, {bool(sk_keep[i])} by scikit-learn; accepted sample rows "
                    f"{idx.tolist()} on stamps {[round(v, 6) for v in stamps]}; residual {res_rank:.3f} m by the rank rule, {res_min:.3f} m by the minimum norm (threshold 10 m)")
            lines.append(line)
            assert len(stamps) < 4 and float(t[i]) not in stamps, line               # a rank-open sample, and the row lies off its stamps
            assert (res_rank <= 10.0) != (res_min <= 10.0), line                     # ... where the two answers to that sample fall on either side of the threshold
            moved.add((seed, int(i)))
    print(f"repeating receiver: {n_plain} logs drew no rank-open sample and equal scikit-learn; rows the minimum-norm answer moves: {len(moved)}")
    for line in lines:
        print("  " + line)
    assert n_plain >= 5, n_plain
    assert moved == MOVED_BY_MINIMUM_NORM, (sorted(moved), lines)
