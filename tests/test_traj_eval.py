"""GPU tier of the trajectory evaluation (gsf_traj_eval_dev, batch.evaluate_trajectory_ragged, ekfgpsslam.evaluate_trajectory) against the
50-digit yardstick (tests/traj_eval_ref.py) on the batch of traj_eval_ref.build_cases: the smallest shapes at which the kernels can go wrong
(64-lane chunks of the compaction and of the d[] scan, 256-thread association blocks).  Flags, indices, states, pair counts and pairs are
exact, NaN patterns identical, values inside bounds derived from the operation counts; statistics are held to the device's own per-pose
values; a track's rows are the same bits alone and in the batch, with one scenario and with nine, traced or not, on clean and on dirty
workspaces.  Every test prints the largest ratio of error to bound before asserting it (the figures DESIGN 7r records)."""
import numpy as np
import pytest

import sim3_ref as S
import traj_eval_ref as ref
from hygiene import same_bytes_under_dirt
from test_sim3_yardstick import check_fits

pytestmark = pytest.mark.gpu

ASSOCS, ALIGNS = ("nearest", "interp"), ("none", "se3", "sim3")
PER_TRACK = ("R", "t", "s", "track_state", "ape_stats", "rpe_n", "rpe_sums")
PER_POSE = ("flags", "match_index", "ape_t", "ape_r")
TRACE = ("rpe_last", "rpe_t", "rpe_r")


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def _dev(c):
    import torch
    return {k: torch.as_tensor(c[k]).cuda() for k in ("ts", "pos", "quat", "offsets", "ref_ts", "ref_pos", "ref_quat", "ref_offsets", "run_status")}


def _scen(B, scenarios):
    import torch
    if not scenarios:
        return None
    return B.RpeScenarios(torch.tensor([s[0] for s in scenarios], dtype=torch.int32).cuda(), torch.tensor([s[1] for s in scenarios], dtype=torch.float64).cuda(),
                          torch.tensor([s[2] for s in scenarios], dtype=torch.int64).cuda())


def _call(B, d, assoc, align, scenarios=ref.SCENARIOS, trace=None):
    return B.evaluate_trajectory_ragged(d["ts"], d["pos"], d["quat"], d["offsets"], d["ref_ts"], d["ref_pos"], d["ref_quat"], d["ref_offsets"], align=align,
                                        assoc=assoc, max_diff=ref.MAX_DIFF[ref.ASSOC_OF[assoc]], rpe=_scen(B, scenarios), trace=trace,
                                        run_status=d["run_status"])


def _host(r):
    return {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in PER_TRACK + PER_POSE + TRACE}


@pytest.fixture(scope="module")
def runs(B):
    """every (assoc, align, trace) result the tests below read, computed once: {(assoc, align, trace): host arrays}"""
    d = _dev(ref.build_cases())
    return {(a, al, tr): _host(_call(B, d, a, al, trace=tr)) for a in ASSOCS for al in ALIGNS for tr in (None,) + ref.TRACED}


def _traced(c, want, k):
    """the yardstick's rpe_last / rpe_t / rpe_r of scenario k over the P poses, with their bounds"""
    P = c["P"]
    last, et, er, bt, br = np.full(P, -1, np.int32), np.full(P, np.nan), np.full(P, np.nan), np.ones(P), np.ones(P)
    for b, w in enumerate(want):
        lo = c["offsets"][b]
        for j, (f, l) in enumerate(w.pairs[k]):
            last[lo + f] = l
            if k in w.rpe_t:
                et[lo + f], er[lo + f], bt[lo + f], br[lo + f] = w.rpe_t[k][j], w.rpe_r[k][j], w.b_rpe_t[k][j], w.b_rpe_r[k][j]
    return last, et, er, bt, br


# ---------------------------------------------------------------------------------------------------------------- 1. the exact fields
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("assoc", ASSOCS)
def test_exact_fields(runs, assoc, align):
    """flags, match_index, track_state, rpe_n, rpe_last and the NaN patterns equal the yardstick"""
    c = ref.build_cases()
    want = ref.reference(ref.ASSOC_OF[assoc], ref.ALIGN_OF[align])
    got = runs[(assoc, align, None)]
    np.testing.assert_array_equal(got["track_state"], [w.state for w in want])
    np.testing.assert_array_equal(got["flags"], ref.flat(c, want, "flags", 0))
    np.testing.assert_array_equal(got["match_index"], ref.flat(c, want, "index", -1))
    np.testing.assert_array_equal(got["rpe_n"], [[len(p) for p in w.pairs] for w in want])
    for k in ("ape_t", "ape_r"):
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref.flat(c, want, k, np.nan)), err_msg=k)
    bad = np.array([w.state != 0 for w in want])
    assert np.isnan(got["R"][bad]).all() and np.isnan(got["t"][bad]).all() and np.isnan(got["s"][bad]).all()
    assert np.isfinite(got["R"][~bad]).all() and np.isfinite(got["t"][~bad]).all() and np.isfinite(got["s"][~bad]).all()
    assert (got["ape_stats"][bad][:, :, 0] == 0).all() and np.isnan(got["ape_stats"][bad][:, :, 1:]).all() and (got["rpe_n"][bad] == 0).all()
    for k in ref.TRACED:
        g = runs[(assoc, align, k)]
        last, et, er, _, _ = _traced(c, want, k)
        np.testing.assert_array_equal(g["rpe_last"], last, err_msg=f"scenario {k}")
        assert (np.isnan(g["rpe_t"]) == (last < 0)).all() and (np.isnan(g["rpe_r"]) == (last < 0)).all()
    assert (got["rpe_n"][:, 1] == 0).all() and got["rpe_n"][:, 0].max() == 270


# ---------------------------------------------------------------------------------------------------------------- 2. values, no alignment
@pytest.mark.parametrize("assoc", ASSOCS)
def test_values_without_alignment(runs, assoc):
    c = ref.build_cases()
    want = ref.reference(ref.ASSOC_OF[assoc], ref.ALIGN_NONE)
    got = runs[(assoc, "none", None)]
    worst = {}
    for k in ("ape_t", "ape_r"):
        worst[k], same = ref.worst_ratio(got[k], ref.flat(c, want, k, np.nan), ref.flat(c, want, "b_" + k, np.nan))
        assert same, k
    for k in ref.TRACED:
        g = runs[(assoc, "none", k)]
        _, et, er, bt, br = _traced(c, want, k)
        for name, v, w_, b_ in (("rpe_t", g["rpe_t"], et, bt), ("rpe_r", g["rpe_r"], er, br)):
            r, same = ref.worst_ratio(v, w_, b_)
            assert same, (name, k)
            worst[name] = max(worst.get(name, 0.0), r)
    print(f"traj_eval {assoc} none: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst
    tiny = slice(c["offsets"][c["notes"]["tiny"]], c["offsets"][c["notes"]["tiny"] + 1])
    assert (np.abs(got["ape_r"][tiny] - 1e-12) < 1e-14).all()              # the case acos fails: it returns 0 here


# ---------------------------------------------------------------------------------------------------------------- 3. aligned
@pytest.mark.parametrize("align", ["se3", "sim3"])
@pytest.mark.parametrize("assoc", ASSOCS)
def test_values_aligned(runs, assoc, align):
    """R, t, s under the gates of the Sim3 yardstick tests (NEAREST: the matched truth rows are stored float64 rows); the per-pose values and
    the pair errors against the yardstick evaluated with the device's own R, t, s"""
    c = ref.build_cases()
    a_, al = ref.ASSOC_OF[assoc], ref.ALIGN_OF[align]
    want = ref.reference(a_, al)
    got = runs[(assoc, align, None)]
    worst = {}
    if a_ == ref.NEAREST:
        ok = [b for b, w in enumerate(want) if w.state == 0]
        names = [c["names"][b] for b in ok]
        if al == ref.ALIGN_SIM3:
            misses = check_fits(f"traj_eval {assoc} sim3", names, [(want[b].src, want[b].dst, None) for b in ok], [want[b].y for b in ok],
                                got["R"][ok], got["t"][ok], got["s"][ok], np.array([want[b].y.status for b in ok]), shifted=False)
            assert not misses, misses
        else:
            from test_sim3_yardstick_host import Worst
            fits = Worst(f"traj_eval {assoc} se3")
            for b in ok:
                ref.gate_fit(fits, worst, c["names"][b], want[b], al, got["R"][b], got["t"][b], float(got["s"][b]))
            fits.report()
            assert not fits.misses, fits.misses
    else:                                                                # interpolated truth rows: sim3_ref's gates plus that rounding
        for b, w in enumerate(want):
            if w.state == 0:
                for k, v in ref.interp_fit_ratios(w, al, got["R"][b], got["t"][b], got["s"][b], w.src).items():
                    worst["interp_fit_" + k] = max(worst.get("interp_fit_" + k, 0.0), v)
        assert "interp_fit_R" in worst
    traced = (4, 5)
    evs = [ref.with_fit(c, b, a_, al, (got["R"][b], got["t"][b], got["s"][b]), errors_for=traced) if w.state == 0 else w for b, w in enumerate(want)]
    for k in ("ape_t", "ape_r"):
        worst[k], same = ref.worst_ratio(got[k], ref.flat(c, evs, k, np.nan), ref.flat(c, evs, "b_" + k, np.nan))
        assert same, k
    for k in traced:
        g = runs[(assoc, align, k)]
        last, et, er, bt, br = _traced(c, evs, k)
        np.testing.assert_array_equal(g["rpe_last"], last)
        for name, v, w_, b_ in (("rpe_t", g["rpe_t"], et, bt), ("rpe_r", g["rpe_r"], er, br)):
            r, same = ref.worst_ratio(v, w_, b_)
            assert same, (name, k)
            worst[name] = max(worst.get(name, 0.0), r)
    print(f"traj_eval {assoc} {align}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- 4. statistics
def _stats_check(x, st, worst):
    """x: the device's own per-pose values of one track (NaN where unmatched), st: its {n, mean, median, rmse, std, min, max, sse}.
    Order statistics and n bit for bit; sums within n u sum|x|; mean, rmse and std within that bound propagated (+ u per rounded
    operation on the way: one division and one square root)."""
    v = x[~np.isnan(x)]
    n = len(v)
    assert st[0] == n
    if n == 0:
        assert np.isnan(st[1:]).all()
        return
    assert st[2].tobytes() == np.median(v).tobytes() and st[5].tobytes() == v.min().tobytes() and st[6].tobytes() == v.max().tobytes()
    L = np.longdouble
    u, vl = ref.U, v.astype(L)
    s1, s2 = vl.sum(), (vl * vl).sum()                                      # (the kernel adds the squares by fma: they are not rounded)
    b1, b2 = n * u * float(np.abs(vl).sum()), n * u * float(s2)             # sums: n u sum|x|
    mean = float(s1 / n)
    b_mean = b1 / n + u * abs(mean)
    rmse = float(np.sqrt(s2 / n))
    dev2 = float(((vl - L(st[1])) ** 2).sum())                              # about the device's own mean: the second pass as it ran
    std = float(np.sqrt(L(dev2) / n))
    # the second pass sums e_i^2 with e_i = fl(v_i - mean): |e_i^2 - (v_i - mean)^2| <= (2u + u^2) (v_i - mean)^2 enters an n-term sum
    # held to n u sum|x| as above, x = e_i^2 <= (1 + 2u + u^2) (v_i - mean)^2
    b_dev2 = n * u * (1 + 3 * u) * dev2 + 3 * u * dev2
    for name, got, want, bound in (("sse", st[7], float(s2), b2), ("mean", st[1], mean, b_mean),
                                   ("rmse", st[3], rmse, (b2 / n) / (2 * rmse) + 2 * u * rmse if rmse > 0 else u),
                                   ("std", st[4], std, (b_dev2 / n) / (2 * std) + 2 * u * std if std > 0 else u)):
        if got != want:                                                     # (values that are all zero: a zero bound, met exactly)
            worst[name] = max(worst.get(name, 0.0), abs(got - want) / bound if bound > 0 else np.inf)


@pytest.mark.parametrize("assoc,align", [("nearest", "none"), ("interp", "se3"), ("nearest", "sim3")])
def test_statistics_of_the_devices_own_values(runs, assoc, align):
    c = ref.build_cases()
    got = runs[(assoc, align, None)]
    worst, seen = {}, 0
    for b in range(c["B"]):
        lo, hi = c["offsets"][b], c["offsets"][b + 1]
        for q, k in enumerate(("ape_t", "ape_r")):
            _stats_check(got[k][lo:hi], got["ape_stats"][b, q], worst)
            seen += int(got["ape_stats"][b, q, 0] > 0)
    print(f"traj_eval statistics {assoc} {align}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert seen >= 20 and max(worst.values()) <= 1.0, worst
    # the scenario sums against the device's own traced pair errors (squares by fma, quotients rounded: formed here the same way)
    worst_sum = 0.0
    for k in ref.TRACED:
        g = runs[(assoc, align, k)]
        for b in range(c["B"]):
            lo, hi = c["offsets"][b], c["offsets"][b + 1]
            et, er = g["rpe_t"][lo:hi], g["rpe_r"][lo:hi]
            et, er = et[~np.isnan(et)], er[~np.isnan(er)]
            n, sm = len(et), g["rpe_sums"][b, k]
            assert g["rpe_n"][b, k] == n
            metres = ref.SCENARIOS[k][0] == ref.METRES
            assert np.isnan(sm[6:]).all() != metres
            if n == 0:
                assert (sm[:6] == 0).all()
                continue
            assert sm[2] == et.max() and sm[5] == er.max()
            L = np.longdouble
            el, rl, val = et.astype(L), er.astype(L), ref.SCENARIOS[k][1]
            for j, x in ((0, el), (1, el * el), (3, rl), (4, rl * rl)) + (((6, (et / val).astype(L)), (7, (er / val).astype(L))) if metres else ()):
                diff, bound = abs(float(L(sm[j]) - x.sum())), n * ref.U * float(np.abs(x).sum())
                if diff:
                    worst_sum = max(worst_sum, diff / bound if bound > 0 else np.inf)
    print(f"traj_eval scenario sums {assoc} {align}: worst error / (n u sum|x|) {worst_sum:.3f}")
    assert worst_sum <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 5. the same bits
def _rows_equal(c, b, whole, alone, keys_track, keys_pose, what):
    lo, hi = c["offsets"][b], c["offsets"][b + 1]
    for k in keys_track:
        assert whole[k][b].tobytes() == alone[k][0].tobytes(), (what, c["names"][b], k)
    for k in keys_pose:
        assert whole[k][lo:hi].tobytes() == alone[k].tobytes(), (what, c["names"][b], k)


@pytest.mark.parametrize("assoc,align", [("nearest", "sim3"), ("interp", "se3")])
def test_same_bits_alone_and_in_the_batch(B, runs, assoc, align):
    c = ref.build_cases()
    whole = runs[(assoc, align, 4)]
    for name in ("m3", "m65", "m271", "midway", "quats", "tiny", "collinear", "skipped", "unsorted", "m2"):
        b = c["notes"][name]
        alone = _host(_call(B, _dev(ref.single(c, b)), assoc, align, trace=4))
        _rows_equal(c, b, whole, alone, PER_TRACK, PER_POSE + TRACE, "alone")


def test_same_bits_with_one_scenario_and_with_nine_traced_or_not(B, runs):
    c = ref.build_cases()
    d = _dev(c)
    nine, traced = runs[("nearest", "se3", None)], runs[("nearest", "se3", 4)]
    for k in PER_TRACK + PER_POSE:
        assert nine[k].tobytes() == traced[k].tobytes(), k                                    # the trace changes nothing else
    assert nine["rpe_last"] is None
    one = _host(_call(B, d, "nearest", "se3", scenarios=ref.SCENARIOS[4:5], trace=0))
    for k in ("R", "t", "s", "track_state", "ape_stats") + PER_POSE:
        assert one[k].tobytes() == nine[k].tobytes(), k
    assert np.ascontiguousarray(nine["rpe_n"][:, 4]).tobytes() == one["rpe_n"][:, 0].tobytes()
    assert np.ascontiguousarray(nine["rpe_sums"][:, 4]).tobytes() == one["rpe_sums"][:, 0].tobytes()
    for k in TRACE:
        assert one[k].tobytes() == traced[k].tobytes(), k
    none = _host(_call(B, d, "nearest", "se3", scenarios=()))                                  # K = 0: the scenario kernel is not launched
    for k in ("R", "t", "s", "track_state", "ape_stats") + PER_POSE:
        assert none[k].tobytes() == nine[k].tobytes(), k
    assert none["rpe_n"].shape == (c["B"], 0)


def test_same_bits_on_dirty_workspaces_and_prefilled_outputs(B, runs, monkeypatch):
    import torch
    c = ref.build_cases()
    d = _dev(c)
    big = {k: (torch.cat([v, v]) if k in ("ts", "pos", "quat", "ref_ts", "ref_pos", "ref_quat", "run_status") else
               torch.cat([v, v[1:] + v[-1]])) for k, v in d.items()}
    r = same_bytes_under_dirt(monkeypatch, B.context(), lambda: _call(B, d, "nearest", "sim3", trace=4), lambda: _call(B, big, "interp", "none", trace=0),
                              rows_of=c["offsets"])
    got, want = _host(r), runs[("nearest", "sim3", 4)]
    for k in PER_TRACK + PER_POSE + TRACE:
        assert got[k].tobytes() == want[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- 6. KITTI 04
def test_kitti04(B, golden):
    """the reference's ground truth and estimate of KITTI 04: the pair counts of the segments exactly, t_rel and r_rel within the summed
    bounds of the yardstick's pair errors; through the single-track wrapper"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    g = golden("traj_eval_kitti04.npz")
    assert abs(float(g["path_length"]) - 393.6) < 0.05 and g["n_pairs"].tolist() == [21, 15, 7, 0, 0, 0, 0, 0]
    # The file holds seven digits: its matrices are orthogonal to ~1e-7 only.  SciPy's quaternion (the fixture's) is that of the nearest
    # rotation, the reader's is the branch formula on the matrix as it stands; the two differ by no more than the matrix's own departure
    # from a rotation, max |R^T R - I|.
    q = B.kitti_rotations_to_quat(g["truth_rows"])
    Rm = g["truth_rows"].reshape(-1, 3, 4)[:, :, :3]
    off = float(np.abs(np.einsum("nji,njk->nik", Rm, Rm) - np.eye(3)).max())
    assert off < 1e-5 and np.abs(q - g["truth_quat"]).max() <= off and (q[:, 3] >= 0).all()
    est = {"timestamps": g["est_ts"], "positions": g["est_pos"], "quaternions": g["est_quat"]}
    truth = {"timestamps": g["truth_ts"], "positions": g["truth_pos"], "quaternions": g["truth_quat"]}
    lengths = tuple(float(v) for v in g["lengths"])
    r = E.evaluate_trajectory(est, truth, align="none", metres=lengths, stride=int(g["stride"]))
    assert r.rpe_n.cpu().numpy()[0].tolist() == g["n_pairs"].tolist()
    k = r.kitti()
    n = int(g["n_pairs"].sum())
    L = g["lengths"][g["pair_k"]]
    b_t = 100.0 * (float(np.sum(g["pair_bt"] / L)) + (n + 1) * ref.U * float(np.sum(g["pair_et"] / L))) / n
    b_r = (float(np.sum(g["pair_br"] / L)) + (n + 1) * ref.U * float(np.sum(g["pair_er"] / L))) / n
    print(f"KITTI 04: t_rel {k.t_rel:.6f} % (yardstick {float(g['t_rel']):.6f}, error / bound {abs(k.t_rel - float(g['t_rel'])) / b_t:.3f}), r_rel {k.r_rel:.6e} "
          f"rad/m = {k.r_rel_deg_per_100m:.5f} deg / 100 m (yardstick {float(g['r_rel']):.6e}, error / bound {abs(k.r_rel - float(g['r_rel'])) / b_r:.3f})")
    assert k.n == n and abs(k.t_rel - float(g["t_rel"])) <= b_t and abs(k.r_rel - float(g["r_rel"])) <= b_r
    assert float(k.t_rel_track[0]) == k.t_rel and int(k.n_track[0]) == n
    # the same track through one traced call per length: every pair and its errors
    for j in range(3):
        rj = E.evaluate_trajectory(est, truth, align="none", metres=lengths, stride=int(g["stride"]), trace=j)
        sel = g["pair_k"] == j
        last = np.full(271, -1, np.int32)
        last[g["pair_f"][sel]] = g["pair_l"][sel]
        np.testing.assert_array_equal(rj.rpe_last.cpu().numpy(), last)
        et, er = rj.rpe_t.cpu().numpy()[g["pair_f"][sel]], rj.rpe_r.cpu().numpy()[g["pair_f"][sel]]
        assert (np.abs(et - g["pair_et"][sel]) <= g["pair_bt"][sel]).all() and (np.abs(er - g["pair_er"][sel]) <= g["pair_br"][sel]).all()
    a = r.ape(0)
    assert a["translation"]["n"] == 271 and a["translation"]["rmse"] > 0 and "271" in r.table()


# ---------------------------------------------------------------------------------------------------------------- 7. the wrappers
def test_wrappers_refuse_bad_arguments_on_the_device(B):
    """on device tensors a good call is accepted, so every check has to raise by itself: each is matched by its own message"""
    import torch
    c = ref.single(ref.build_cases(), ref.build_cases()["notes"]["m3"])
    d = _dev(c)
    good = dict(ts=d["ts"], pos=d["pos"], quat=d["quat"], offsets=d["offsets"], ref_ts=d["ref_ts"], ref_pos=d["ref_pos"], ref_quat=d["ref_quat"],
                ref_offsets=d["ref_offsets"])
    B.evaluate_trajectory_ragged(**good)
    sc = _scen(B, ref.SCENARIOS[:3])
    short = B.RpeScenarios(sc.kind, sc.value[:2].contiguous(), sc.stride)
    n, g = c["P"], len(c["ref_ts"])
    off = lambda *v: torch.tensor(v, dtype=torch.int64).cuda()
    for bad, msg in ((dict(ts=d["ts"].float()), "^ts: expected"), (dict(pos=d["pos"][:, :2].contiguous()), "^pos: expected"),
                     (dict(quat=d["quat"][:-1]), "^quat: expected"), (dict(ref_ts=d["ref_ts"].reshape(-1, 1)), "^ref_ts: expected"),
                     (dict(ref_pos=d["ref_pos"].float()), "^ref_pos: expected"), (dict(ref_quat=d["ref_quat"][:-1]), "^ref_quat: expected"),
                     (dict(pos=d["pos"].t()), "^pos: expected"), (dict(ts=d["ts"].cpu()), "^ts: expected"),
                     (dict(offsets=d["offsets"].int()), "^offsets: expected"), (dict(ref_offsets=off(0, 2, g)), "same number of tracks"),
                     (dict(run_status=torch.zeros(1).cuda()), "^run_status: expected"), (dict(run_status=torch.zeros(2, dtype=torch.int32).cuda()), "^run_status: expected"),
                     (dict(trace=0), "names none of the 0 scenarios"), (dict(rpe=sc, trace=3), "names none of the 3 scenarios"),
                     (dict(rpe=short), r"^rpe\.value: expected"), (dict(rpe=B.RpeScenarios(sc.kind.long(), sc.value, sc.stride)), r"^rpe\.kind: expected"),
                     (dict(rpe=B.RpeScenarios(sc.kind, sc.value, sc.stride.int())), r"^rpe\.stride: expected"),
                     (dict(offsets=off(0, n + 1)), ": offsets must ascend"), (dict(offsets=off(-1, n)), ": offsets must ascend"),
                     (dict(ref_offsets=off(0, g + 1)), "ref_offsets must ascend"),
                     (dict(offsets=off(0, n, 1), ref_offsets=off(0, g, g)), ": offsets must ascend"),
                     (dict(offsets=off(0, 1, n), ref_offsets=off(0, g, 1)), "ref_offsets must ascend")):
        with pytest.raises(ValueError, match=msg):
            B.evaluate_trajectory_ragged(**dict(good, **bad))
    a = B.evaluate_trajectory_ragged(**good, rpe=sc, trace=2)
    b = B.evaluate_trajectory_ragged(**good, rpe=sc, trace=2, check_offsets=False)          # the switch only drops the check
    for k in PER_TRACK + PER_POSE + TRACE:
        assert getattr(a, k).cpu().numpy().tobytes() == getattr(b, k).cpu().numpy().tobytes(), k


def test_evaluate_fused_on_a_ragged_run(B, golden):
    """three tracks, one of them failed (the run of tests/test_pose_query.py): both evaluations are the direct calls on apply_sim3_batch and
    on r.fused bit for bit, keyword arguments reach both, the failed track comes back SKIPPED"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    from gps_optimize_slam_amd import _lib
    from test_sim3_rows import case_cfg, cases as row_cases
    g, _ = row_cases(golden)
    members = [("all_valid", 300), ("longer_than_180s", 2000), ("too_few_valid", 250)]
    cfg = case_cfg(E.CONFIG, g["all_valid_par"])
    cfg["gps_filtering_ransac"] = dict(cfg["gps_filtering_ransac"], enabled=False)
    tracks = [(g[f"{n}_ts"][:k], g[f"{n}_pos"][:k], g[f"{n}_quat"][:k]) for n, k in members]
    logs = [np.column_stack((g[f"{n}_gps_t"], g[f"{n}_gps_p"])) for n, _ in members]
    rb = B.RaggedGeodeticBatch.from_host(tracks, logs)
    r = B.run_fusion_ragged(rb, B.mt19937_seed([int(g[f"{n}_seed"]) for n, _ in members]), cfg, projected=True)
    assert r.run_status.cpu().numpy().tolist()[:2] == [0, 0] and int(r.run_status[2]) != 0
    ts, pos, quat, so = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), rb.slam_offsets
    # a truth of its own: every second fused position with the raw orientation turned by the run's rotation
    sp, sq, _ = B.apply_sim3_batch(pos, quat, so, r.R, r.t, r.s)
    keep = torch.arange(ts.numel(), device=ts.device) % 2 == 0
    counts = torch.stack([keep[a:b].sum() for a, b in zip(so[:-1].tolist(), so[1:].tolist())])
    ref_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=ts.device), torch.cumsum(counts, 0)])
    truth = (ts[keep].contiguous(), r.fused.pos.reshape(-1, 3)[keep].contiguous(), sq[keep].contiguous(), ref_off)
    sc = B.rpe_scenarios(frames=(1,), seconds=(2.0,), metres=(20.0,), stride=3)
    kw = dict(align="sim3", assoc="interp", max_diff=5.0, rpe=sc, trace=2)
    raw, fused = B.evaluate_fused(rb, r, truth, **kw)
    want_raw = B.evaluate_trajectory_ragged(ts, sp, sq, so, *truth, run_status=r.run_status, **kw)
    want_fused = B.evaluate_trajectory_ragged(ts, r.fused.pos.reshape(-1, 3), r.fused.quat.reshape(-1, 4), so, *truth, run_status=r.run_status, **kw)
    for got, want, what in ((raw, want_raw, "raw"), (fused, want_fused, "fused")):
        for k in PER_TRACK + PER_POSE + TRACE:
            assert getattr(got, k).cpu().numpy().tobytes() == getattr(want, k).cpu().numpy().tobytes(), (what, k)
        assert got.align == "sim3" and got.assoc == "interp" and got.scenarios is sc and got.rpe_n.shape == (3, 3)
        st = got.track_state.cpu().numpy()
        assert st.tolist() == [0, 0, _lib.TE_TRACK_SKIPPED]
        fl = got.flags.cpu().numpy()
        assert (fl[int(so[2]):] == _lib.TE_TRACK).all() and (fl[:int(so[2])] == _lib.TE_MATCHED).sum() > 2000
        assert int(got.rpe_n[:2].min()) > 0 and (got.rpe_last[:int(so[2])] >= 0).any() and (got.rpe_n[2] == 0).all()
        assert got.kitti().n == int(got.rpe_n[:, 1].sum())
    assert raw.ape_t.cpu().numpy().tobytes() != fused.ape_t.cpu().numpy().tobytes()          # two different tracks were graded
    plain = B.evaluate_fused(rb, r, truth, align="none", max_diff=0.5)[1]                   # defaults reach both calls too
    assert plain.align == "none" and plain.rpe_last is None and plain.rpe_n.shape == (3, 0)
