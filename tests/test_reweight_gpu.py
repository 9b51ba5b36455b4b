"""GPU tier of robust smoothing (gsf_ekf_smooth_reweighted_dev / batch.ekf_smooth_reweighted_ragged): the kernel against the per-pose
restatement of tests/reweight_ref.py at the chunk edges with outliers planted where a chunk can go wrong, against the 50-digit yardstick
on the CPU tier's tracks (never against itself), the two laws of include/gsf.h in bytes, the stop, and the rules that need no yardstick
-- a row without an update has no weight and changes nothing else, a track's bytes do not depend on its neighbours, on stale buffers
(the weight buffer's incoming bytes included), on the stream or on which optional outputs are asked for.

Gates, the project's own (head of tests/test_smooth_gpu.py): positions 1e-6 m; variances, nis and WEIGHTS 1e-10 relative; quaternions
1e-9.  tests/test_reweight_host.py measured what the restatement loses against the yardstick over four rounds (variances 2.7e-14, nis
4.5e-13, weights 3.9e-14): nothing that asks for a wider gate.  w_change is a difference of two weights <= 1, each inside 1e-10: 2e-10.
Flags, span starts, status words, rounds_used and everything called "the same" are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import hygiene
import reweight_ref as R
import weighted_ref as W
from test_cov_gpu import AXES_DIFFER, file_batch, planted_cov_tracks, small_dirt, words
from test_smooth_gpu import check_track, dev, flat, full_cfg, host, same, with_init
from test_smooth_host import GNSS_USED, SPAN_START
from test_weighted_gpu import empty_track, nis_err, runw

pytestmark = pytest.mark.gpu

POS_TOL, VAR_TOL = 1e-6, 1e-10
C2 = 7.81
LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129]
KINDS = (0, 3, 5, 9)        # test_cov_gpu's planted kinds: no outage; an outage to the end; one that recovers at lane 0 of a chunk; sharp and gentle outages
SHARED = ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags", "nis")
NAMES = SHARED + ("weight",)
PER_TRACK = ("status", "rounds_used", "w_change")
LOSS_OF = {"default": "huber", "axes-differ": "cauchy"}


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def runr(B, arrays, mv, cfg, loss="huber", c2=C2, rounds=2, **kw):
    """one launch of the reweighted entry on host arrays (flat()'s order) -> host dict"""
    import torch
    kw.setdefault("want_filtered", True); kw.setdefault("want_nis", True)
    d = [dev(x) for x in arrays]
    r = B.ekf_smooth_reweighted_ragged(*d, meas_var=None if mv is None else dev(mv), loss=loss, c2=c2, rounds=rounds, config=cfg, **kw)
    torch.cuda.synchronize()
    o = host(r)
    o.update(nis=None if r.nis is None else r.nis.cpu().numpy(), weight=r.weight.cpu().numpy(), rounds_used=r.rounds_used.cpu().numpy(),
             w_change=r.w_change.cpu().numpy())
    return o


def equal_calls(a, b, names=NAMES + PER_TRACK, what=""):
    for name in names:
        assert same(a[name], b[name]), (what, name)


@pytest.fixture(scope="module")
def planted(B):
    """Four planted tracks per length (one empty track for length 0), per-row variances of the five kinds, and outliers of 30 m on rows that
    take an update: row 1, lanes 0 and 63 of a chunk, both sides of a chunk boundary, every sharp-turn recovery, the last row.  One extra
    track holds a row whose effective variance reaches the cap.  Both configs (default: Huber, AXES_DIFFER: Cauchy): one launch of two
    rounds and one set of restatements each, made once."""
    tracks, mvs = [], []
    for N in LENGTHS:
        if N == 0:
            tracks.append(empty_track()); mvs.append(np.empty((0, 3)))
            continue
        made = planted_cov_tracks(N, 100 + N, with_pos=True)
        for kind in KINDS:
            rng = np.random.default_rng(9500 + 100 * N + kind)
            tracks.append(with_init(made[kind]))
            mvs.append(W.variances(W.VAR_KINDS[(kind + N) % len(W.VAR_KINDS)], N, full_cfg({})["ekf"]["meas_noise_diag"], rng))
    t = W.motivation_track(3, 65)
    capped_mv = t[7].copy(); capped_mv[40] = 1e7
    tracks.append(t[:7]); mvs.append(capped_mv)
    cfgs = {"default": full_cfg({}), "axes-differ": full_cfg(AXES_DIFFER)}
    # where the sharp-turn recoveries lie: the span starts of the weighted entry on the fixes as they are
    arrays, mv = flat(tracks), np.concatenate(mvs)
    offs = arrays[5]
    starts = runw(B, arrays, mv, cfgs["default"])["flags"] & SPAN_START
    rows_planted = np.zeros(int(offs[-1]), bool)
    recoveries = 0
    for k, t in enumerate(tracks):
        n = len(t[0])
        if n == 0:
            continue
        aligned = np.array(t[3], float)
        rec = [int(i) for i in np.flatnonzero(starts[offs[k]:offs[k + 1]]) if i > 0]
        recoveries += len(rec)
        for j, i in enumerate(sorted({1, 63, 64, 127, 128, n - 1, *rec})):
            if 0 < i < n:
                aligned[i, j % 3] += 30.0 if j % 2 else -30.0            # (a NaN fix stays one)
                rows_planted[offs[k] + i] = True
        if k == len(tracks) - 1:
            aligned[40] += 1e6                                          # r / w over 1e8
        tracks[k] = t[:3] + (aligned,) + t[4:]
    assert recoveries >= 4
    arrays = flat(tracks)
    out = {name: runr(B, arrays, mv, cfg, LOSS_OF[name]) for name, cfg in cfgs.items()}
    want = {name: [R.reweight_restate(*t[:5], m, *t[5:], cfg, R.LOSSES[LOSS_OF[name]], C2, 2) if len(t[0]) else None for t, m in zip(tracks, mvs)]
            for name, cfg in cfgs.items()}
    return tracks, mvs, arrays, mv, cfgs, out, want, rows_planted


def weight_err(got, want):
    used = ~np.isnan(want)
    assert (np.isnan(got) == ~used).all()
    return float(np.max(np.abs(got[used] - want[used]) / want[used], initial=0.0))


# ------------------------------------------------------------------------------------------------ 1. the chunk edges against the restatement
@pytest.mark.parametrize("config", ["default", "axes-differ"])
def test_planted_lengths_against_the_restatement(planted, config):
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    offs, o = arrays[5], out[config]
    worst = [0.0] * 5
    lanes = set()
    for k, (t, w) in enumerate(zip(tracks, want[config])):
        sl = slice(offs[k], offs[k + 1])
        if w is None:
            assert offs[k] == offs[k + 1] and o["status"][k] == 0 and o["rounds_used"][k] == 0 and o["w_change"][k] == 0.0      # an empty track
            continue
        what = (config, len(t[0]), k)
        en, ew = nis_err(o["nis"][sl], w["nis"]), weight_err(o["weight"][sl], w["weight"])
        assert en < VAR_TOL and ew < VAR_TOL, (what, en, ew)
        worst = [max(a, b) for a, b in zip(worst, check_track(o, sl, w, what) + (en, ew))]
        assert o["status"][k] == w["status"] and o["rounds_used"][k] == w["rounds_used"], (what, o["rounds_used"][k], w["rounds_used"])
        assert abs(o["w_change"][k] - w["w_change"]) <= 2e-10, (what, o["w_change"][k], w["w_change"])
        used = (o["flags"][sl] & GNSS_USED) != 0
        assert (np.isnan(o["weight"][sl]) == ~used).all(), what
        hit = rows_planted[sl] & used
        lanes |= {int(i) % 64 for i in np.flatnonzero(hit)}
        if len(t[0]) >= 63:                  # planted outliers: every round is used, and the weight fell where 30 m lies far outside the row's variance
            assert o["rounds_used"][k] == 2 and hit.sum() >= 1 and o["weight"][sl][hit].min() < 0.5, (what, o["weight"][sl][hit])
    assert {0, 1, 63} <= lanes
    cap = slice(offs[-2], offs[-1])                                      # the track whose row 40 reaches the cap
    assert o["weight"][cap][40] * 1e8 < 1e7
    print(f"{config} ({LOSS_OF[config]}, 2 rounds): largest deviation from the restatement: positions {worst[0]:.2e} m, variances {worst[1]:.2e} relative, "
          f"quaternions {worst[2]:.2e}, nis {worst[3]:.2e}, weights {worst[4]:.2e} relative")


# ------------------------------------------------------------------------------------------------ 2. the yardstick
@pytest.mark.parametrize("case", ["outliers-huber", "outliers-cauchy", "range-ends-cauchy"])
def test_against_the_50_digit_yardstick(B, case):
    cfg = full_cfg({})
    loss = "huber" if case.endswith("huber") else "cauchy"
    if case.startswith("outliers"):
        t = R.motivation(0, 129)
        tracks, mvs, rounds = [t[:7]], [t[7]], 4
    else:
        yt = W.yardstick_tracks()
        tracks, mvs, rounds = [t[1:8] for t in yt], [t[8] for t in yt], 2
    arrays = flat(tracks)
    o = runr(B, arrays, np.concatenate(mvs), cfg, loss, rounds=rounds)
    offs = arrays[5]
    worst = [0.0] * 4
    for k, (t, m) in enumerate(zip(tracks, mvs)):
        sl = slice(offs[k], offs[k + 1])
        r = R.reweight_restate(*t[:5], m, *t[5:], cfg, R.LOSSES[loss], C2, rounds)
        y = R.yardstick(r, t[3], t[5], cfg, R.LOSSES[loss], C2)
        e = R.yard_errors(dict(xf=o["pos_filt"][sl], xs=o["pos"][sl], Pf=o["cov_filt"][sl], Ps=o["cov"][sl], nis=o["nis"][sl], weight=o["weight"][sl]), y)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] < POS_TOL and e[1] < VAR_TOL and e[2] < VAR_TOL and e[3] < VAR_TOL, (case, k, e)
        assert o["rounds_used"][k] == r["rounds_used"] and same(o["flags"][sl], r["flags"]), (case, k)
    print(f"{case}: device against the 50-digit yardstick: positions {worst[0]:.2e} m, variances {worst[1]:.2e}, nis {worst[2]:.2e}, weights {worst[3]:.2e} relative")


# ------------------------------------------------------------------------------------------------ 3. the two laws
def test_law_a_rounds_zero_is_the_weighted_entry(B, planted):
    import torch
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    for name, cfg in cfgs.items():
        for loss in ("huber", "cauchy"):
            got = runr(B, arrays, mv, cfg, loss, rounds=0)
            ref = runw(B, arrays, mv, cfg)
            equal_calls(got, ref, SHARED + ("status",), (name, loss))
            assert (got["rounds_used"] == 0).all()
            used = (got["flags"] & GNSS_USED) != 0
            assert (np.isnan(got["weight"]) == ~used).all() and (got["weight"][used] < 1.0).any()
        # without variances: the weighted entry fed the config's R on every row, and the unweighted smoother
        const = np.tile(np.array(cfg["ekf"]["meas_noise_diag"], float), (len(mv), 1))
        got = runr(B, arrays, None, cfg, rounds=0)
        equal_calls(got, runw(B, arrays, const, cfg), SHARED + ("status",), (name, "no variances"))
        plain = B.ekf_smooth_ragged(*[dev(x) for x in arrays], config=cfg, want_filtered=True)
        torch.cuda.synchronize()
        equal_calls(got, host(plain), ("pos", "quat", "cov", "pos_filt", "cov_filt", "flags", "status"), (name, "the unweighted smoother"))


@pytest.mark.parametrize("rounds", [1, 3])
def test_law_b_a_round_is_the_weighted_entry_on_the_effective_variances(B, planted, rounds):
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    offs = arrays[5]
    for name, cfg in cfgs.items():
        loss = LOSS_OF[name]
        w = runr(B, arrays, mv, cfg, loss, rounds=rounds - 1)["weight"]
        with np.errstate(invalid="ignore", divide="ignore"):
            fed = np.where(np.isnan(w)[:, None], mv, np.minimum(mv / w[:, None], 1e8))
        got = runr(B, arrays, mv, cfg, loss, rounds=rounds)
        equal_calls(got, runw(B, arrays, fed, cfg), SHARED + ("status",), (name, rounds))
        if loss == "huber":
            assert (fed[offs[-2] + 40] == 1e8).all() and (mv[offs[-2] + 40] == 1e7).all()      # the row at the cap
    # the same through torch, as a caller composes it: ReweightedTrack.effective_var() of the call before
    import torch
    d = [dev(x) for x in arrays]
    before = B.ekf_smooth_reweighted_ragged(*d, meas_var=dev(mv), rounds=rounds - 1, c2=C2, config=cfgs["default"])
    by_hand = B.ekf_smooth_weighted_ragged(*d[:5], before.effective_var().contiguous(), *d[5:], config=cfgs["default"], want_filtered=True, want_nis=True)
    torch.cuda.synchronize()
    g = runr(B, arrays, mv, cfgs["default"], rounds=rounds)
    for key in ("pos", "cov", "nis", "flags"):
        assert same(getattr(by_hand, key).cpu().numpy(), g[key]), key


# ------------------------------------------------------------------------------------------------ 4. the stop
def test_a_clean_batch_stops_at_once(B):
    tracks = [W.motivation_track(seed, n) for seed, n in ((0, 2), (1, 63), (2, 64), (3, 65), (4, 129), (5, 271))]
    arrays, mv = flat([t[:7] for t in tracks] + [empty_track()]), np.concatenate([t[7] for t in tracks])
    cfg = full_cfg({})
    got = runr(B, arrays, mv, cfg, "huber", c2=1e6, rounds=5)
    used = (got["flags"] & GNSS_USED) != 0
    assert (got["rounds_used"] == 0).all() and (got["w_change"] == 0.0).all() and (got["weight"][used] == 1.0).all() and np.isnan(got["weight"][~used]).all()
    equal_calls(got, runw(B, arrays, mv, cfg), SHARED + ("status",))
    # Cauchy moves every weight a little: it runs until the weights repeat their own bits, or the rounds run out
    c = runr(B, arrays, mv, cfg, "cauchy", c2=1e6, rounds=5)
    want = [R.reweight_restate(*t[:5], t[7], t[5], t[6], cfg, R.CAUCHY, 1e6, 5)["rounds_used"] for t in tracks] + [0]
    assert (c["rounds_used"][:-1] >= 1).all() and (c["rounds_used"] <= 5).all() and c["rounds_used"][-1] == 0, (c["rounds_used"], want)
    assert (c["w_change"][c["rounds_used"] < 5] == 0.0).all(), (c["rounds_used"], c["w_change"])
    print(f"Cauchy, c2 = 1e6, up to 5 rounds on clean tracks: rounds used {c['rounds_used'].tolist()} (restatement: {want})")


# ------------------------------------------------------------------------------------------------ 5. rows without an update
def test_rows_without_an_update_have_no_weight_and_change_nothing_else(B, planted):
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    cfg, offs = cfgs["default"], arrays[5]
    base = out["default"]
    used = np.flatnonzero((base["flags"] & GNSS_USED) != 0)
    rng = np.random.default_rng(8)
    pick = rng.choice(used, 60, replace=False)
    how = np.arange(60) % 4
    dirty_arrays, dirty_mv = [x.copy() for x in arrays], mv.copy()
    dirty_mv[pick[how == 0], 1] = np.nan                                # a bad variance
    dirty_mv[pick[how == 1]] = np.inf                                   # "no information"
    dirty_arrays[3][pick[how == 2], 0] = np.nan                          # a NaN fix
    dirty_arrays[4][pick[how == 3]] = 0                                 # a cleared mask byte
    got = runr(B, dirty_arrays, dirty_mv, cfg)
    masked = [x.copy() for x in arrays]
    masked[4][pick] = 0                                                 # the same rows with their mask bytes cleared instead
    ref = runr(B, masked, mv, cfg)
    assert np.isnan(got["weight"][pick]).all() and not np.isnan(base["weight"][pick]).any()
    equal_calls(got, ref, ("pos", "quat", "cov", "pos_filt", "cov_filt", "nis", "weight") + PER_TRACK)
    np.testing.assert_array_equal(got["flags"] & np.uint8(255 - W.BAD_SIGMA), ref["flags"])
    np.testing.assert_array_equal(np.flatnonzero(got["flags"] & W.BAD_SIGMA), np.sort(pick[how == 0]))      # BAD_SIGMA is kept, on those rows alone
    # a skipped run: NaN rows, the weights included; nothing of it is read
    rs = np.zeros(len(tracks), np.int32)
    rs[[5, len(tracks) - 1]] = [8, 1]
    rows = np.zeros(int(offs[-1]), bool)
    for k in (5, len(tracks) - 1):
        rows[offs[k]:offs[k + 1]] = True
    poisoned = [x.copy() for x in arrays]
    for j in (0, 1, 2, 3):
        poisoned[j][rows] = np.nan
    r = runr(B, poisoned, np.where(rows[:, None], np.nan, mv), cfg, run_status=dev(rs))
    for name in NAMES:
        if name != "flags":
            assert np.isnan(r[name][rows]).all() and same(r[name][~rows], base[name][~rows]), name
    assert (r["flags"][rows] == 0).all() and same(r["flags"][~rows], base["flags"][~rows])
    for name in PER_TRACK:
        assert (r[name][rs != 0] == 0).all() and same(r[name][rs == 0], base[name][rs == 0]), name


# ------------------------------------------------------------------------------------------------ 6. batch independence and hygiene
def test_a_track_alone_in_the_batch_and_in_reversed_order(B, planted):
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    offs, o, cfg = arrays[5], out["default"], cfgs["default"]
    rev = list(range(len(tracks)))[::-1]
    r = runr(B, flat([tracks[k] for k in rev]), np.concatenate([mvs[k] for k in rev]), cfg)
    roffs = np.zeros(len(tracks) + 1, np.int64); roffs[1:] = np.cumsum([len(tracks[k][0]) for k in rev])
    for j, k in enumerate(rev):
        a, b = slice(offs[k], offs[k + 1]), slice(roffs[j], roffs[j + 1])
        for name in NAMES:
            assert same(o[name][a], r[name][b]), (name, k)
        for name in PER_TRACK:
            assert same(o[name][k], r[name][j]), (name, k)
    for k in (1, 5, 12, 16, 20, len(tracks) - 2):                        # lengths 1, 2, 63, 64, 65, 129
        alone = runr(B, flat([tracks[k]]), mvs[k], cfg)
        for name in NAMES:
            assert same(o[name][offs[k]:offs[k + 1]], alone[name]), (name, k)
        for name in PER_TRACK:
            assert same(o[name][k], alone[name][0]), (name, k)


def test_outputs_do_not_depend_on_stale_buffers(B, monkeypatch, planted):
    """outputs (weight, rounds_used and w_change among them) prefilled with two byte patterns behind guard bytes, workspaces poisoned and
    not: the same bytes.  Then the weight buffer handed in full of NaN and of 0xFF: its incoming bytes are not read."""
    import torch
    from gps_optimize_slam_amd import _lib
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    d, dmv, cfg, o = [dev(x) for x in arrays], dev(mv), cfgs["default"], out["default"]
    res = hygiene.same_bytes_under_dirt(monkeypatch, B.context(),
                                        lambda: B.ekf_smooth_reweighted_ragged(*d, meas_var=dmv, c2=C2, rounds=2, config=cfg, want_filtered=True, want_nis=True),
                                        small_dirt(B), rows_of=arrays[5])
    for name in NAMES + PER_TRACK:
        assert same(getattr(res, name).cpu().numpy(), o[name]), name
    assert np.isfinite(o["cov"]).all() and (o["cov"] >= 0).all() and not np.signbit(o["cov"]).any()      # no tag bit survives
    P, nb = int(arrays[5][-1]), len(tracks)
    c = _lib.EkfConfig.from_config(cfg)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f = dict(dtype=torch.float64, device="cuda")
    for fill in (float("nan"), None):
        weight = torch.full((P,), float("nan"), **f) if fill is not None else torch.full((P,), -1, dtype=torch.int64, device="cuda").view(torch.float64)
        pos, quat, cov = torch.empty((P, 3), **f), torch.empty((P, 4), **f), torch.empty((P, 7), **f)
        _lib.check(_lib.load().gsf_ekf_smooth_reweighted_dev(B.context().handle, *[p(x) for x in d[:5]], p(dmv), *[p(x) for x in d[5:]], None, C.byref(c), nb,
                                                             0, C2, 2, p(pos), p(quat), p(cov), None, None, None, None, None, p(weight), None, None))
        torch.cuda.synchronize()
        assert same(weight.cpu().numpy(), o["weight"]) and same(pos.cpu().numpy(), o["pos"]) and same(cov.cpu().numpy(), o["cov"]), fill


def test_optional_outputs_null_in_turn(B, planted):
    import torch
    from gps_optimize_slam_amd import _lib
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    o, cfg = out["default"], cfgs["default"]
    d, dmv = [dev(x) for x in arrays], dev(mv)
    P, nb = int(arrays[5][-1]), len(tracks)
    c = _lib.EkfConfig.from_config(cfg)
    f = dict(dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    opt = dict(pos_filt=(P, 3), cov_filt=(P, 7), flags=(P,), status=(nb,), nis=(P,), rounds_used=(nb,), w_change=(nb,))
    kinds = dict(flags=torch.uint8, status=torch.int32, rounds_used=torch.int32)
    for leave_out in list(opt) + ["all"]:
        pos, quat, cov, weight = (torch.full(s, float("nan"), **f) for s in ((P, 3), (P, 4), (P, 7), (P,)))
        t = {k: None if leave_out in (k, "all") else torch.zeros(s, dtype=kinds.get(k, torch.float64), device="cuda") for k, s in opt.items()}
        _lib.check(_lib.load().gsf_ekf_smooth_reweighted_dev(B.context().handle, *[p(x) for x in d[:5]], p(dmv), *[p(x) for x in d[5:]], None, C.byref(c), nb,
                                                             0, C2, 2, p(pos), p(quat), p(cov), p(t["pos_filt"]), p(t["cov_filt"]), p(t["flags"]), p(t["status"]),
                                                             p(t["nis"]), p(weight), p(t["rounds_used"]), p(t["w_change"])))
        torch.cuda.synchronize()
        for name, v in (("pos", pos), ("quat", quat), ("cov", cov), ("weight", weight)) + tuple(t.items()):
            if v is not None:
                assert same(v.cpu().numpy(), o[name]), (leave_out, name)


def test_side_stream_gives_the_same_bytes(B, planted):
    import torch
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    o = out["default"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
        busy = a @ a                                                    # keeps the stream busy while the inputs and the call are queued behind it
        up = lambda x: torch.as_tensor(np.ascontiguousarray(x)).pin_memory().to("cuda", non_blocking=True)
        got = B.ekf_smooth_reweighted_ragged(*[up(x) for x in arrays], meas_var=up(mv), c2=C2, rounds=2, config=cfgs["default"], want_filtered=True,
                                             want_nis=True)
        s.synchronize()
    for name in NAMES + PER_TRACK:
        assert same(getattr(got, name).cpu().numpy(), o[name]), name
    del busy


def test_invalid_arguments_are_refused(B, planted):
    import torch
    from gps_optimize_slam_amd import _lib
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    d, dmv = [dev(x) for x in arrays], dev(mv)
    P, nb = int(arrays[5][-1]), len(tracks)
    c = _lib.EkfConfig.from_config(cfgs["default"])
    f = dict(dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    pos, quat, cov, weight = (torch.full(s, 7.0, **f) for s in ((P, 3), (P, 4), (P, 7), (P,)))

    def call(loss, c2, rounds, w=weight):
        return _lib.load().gsf_ekf_smooth_reweighted_dev(B.context().handle, *[p(x) for x in d[:5]], p(dmv), *[p(x) for x in d[5:]], None, C.byref(c), nb,
                                                         loss, c2, rounds, p(pos), p(quat), p(cov), None, None, None, None, None, p(w), None, None)
    for loss, c2, rounds in ((2, C2, 2), (-1, C2, 2), (0, 0.0, 2), (0, -1.0, 2), (0, float("inf"), 2), (0, float("nan"), 2), (0, C2, -1), (0, C2, 33)):
        assert call(loss, c2, rounds) == 1, (loss, c2, rounds)          # GSF_ERR_INVALID_ARG
    assert call(0, C2, 2, None) == 1                                    # weight is required
    torch.cuda.synchronize()
    assert (pos == 7.0).all() and (weight == 7.0).all()                 # nothing was launched
    assert call(1, C2, 32) == 0 and call(0, 5e-324, 0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. composition
def test_smooth_reweighted_fused_is_its_steps_and_leaves_the_run_alone(B, golden, tmp_path):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    rb = file_batch(B, golden, tmp_path)
    seeds = [3, 4, 5, 6]
    r = B.run_fusion_ragged(rb, B.mt19937_seed(seeds), E.CONFIG)
    T = int(rb.gps_t.numel())
    rng = np.random.default_rng(5)
    codes = torch.as_tensor(rng.choice([1, 2, 4, 5, 9], T, p=[0.2, 0.1, 0.5, 0.15, 0.05])).cuda()
    fix_var = B.quality_to_var(codes, {4: (4e-4, 4e-4, 1.6e-3), 5: (0.25, 0.25, 1.0), 2: (1.0, 1.0, 4.0), 1: (9.0, 9.0, 36.0)})
    st = B.smooth_reweighted_fused(rb, r, fix_var, loss="cauchy", rounds=3)
    bare = B.smooth_reweighted_fused(rb, r, rounds=3)                   # no quality column: the config's R
    ts, offsets, v = rb.ts.reshape(-1), rb.slam_offsets, r.valid.reshape(-1).contiguous()
    pv = B.fix_var_at_poses_ragged(ts, offsets, rb.gps_t, rb.gps_offsets, fix_var, keep=r.gps_keep, valid=v)
    ip, iq = B._fused_init_pose(rb, r)
    args = (ts, rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), r.aligned.reshape(-1, 3), v, offsets, ip, iq)
    by_hand = B.ekf_smooth_reweighted_ragged(*args, meas_var=pv, loss="cauchy", rounds=3, run_status=r.run_status, want_filtered=True, want_nis=True)
    bare_by_hand = B.ekf_smooth_reweighted_ragged(*args, rounds=3, run_status=r.run_status, want_filtered=True, want_nis=True)
    smoothed = B.ekf_smooth_weighted_ragged(*args[:5], pv, *args[5:], run_status=r.run_status)      # step 6's third row: the weighted smoother itself
    rows = B._step6_rows(ts, offsets, (rb.pos.reshape(-1, 3), r.sim3_pos.reshape(-1, 3), smoothed.pos, by_hand.pos), r.aligned.reshape(-1, 3), v, 5.0)
    again = B.run_fusion_ragged(rb, B.mt19937_seed(seeds), E.CONFIG)    # the same context, after the reweighted calls
    torch.cuda.synchronize()
    assert isinstance(st, B.ReweightedTrack) and torch.equal(words(st.pose_var), words(pv)) and bare.pose_var is None
    assert torch.equal(words(st.smoothed_pos), words(smoothed.pos))
    for name in NAMES + PER_TRACK:
        assert torch.equal(words(getattr(st, name)), words(getattr(by_hand, name))), name
        assert torch.equal(words(getattr(bare, name)), words(getattr(bare_by_hand, name))), name
    assert torch.equal(words(st.err_stats4), words(torch.stack([x[0] for x in rows]))) and torch.equal(words(st.errors4), words(torch.stack([x[1] for x in rows])))
    assert tuple(st.err_stats4.shape) == (4, 4, 4) and tuple(st.errors4.shape) == (4, int(ts.numel()))
    for name in ("aligned", "valid", "sim3_pos", "gps_keep", "run_status", "err_stats", "R", "t", "s"):
        assert torch.equal(words(getattr(r, name)), words(getattr(again, name))), name
    assert torch.equal(words(r.fused.buf), words(again.fused.buf)) and torch.equal(r.fused.status, again.fused.status)
    rs, so = r.run_status.cpu().numpy(), offsets.cpu().numpy()
    weight, flags = st.weight.cpu().numpy(), st.flags.cpu().numpy()
    for b in range(4):
        sl = slice(so[b], so[b + 1])
        if rs[b] != 0:
            assert np.isnan(weight[sl]).all() and int(st.rounds_used[b]) == 0 and float(st.w_change[b]) == 0.0
        else:
            used = (flags[sl] & GNSS_USED) != 0
            assert used.any() and ((weight[sl][used] > 0) & (weight[sl][used] <= 1)).all() and int(st.rounds_used[b]) >= 1
    assert torch.equal(st.downweighted(), st.weight < 0.5) and tuple(st.effective_var().shape) == (int(ts.numel()), 3)


def test_single_track_entry(B, planted):
    from gps_optimize_slam_amd import ekfgpsslam as E
    tracks, mvs, arrays, mv, cfgs, out, want, rows_planted = planted
    k = len(tracks) - 2                                                  # 129 poses
    t = tracks[k]
    one = E.ekf_smooth_aligned_reweighted(*t[:7], meas_var=mvs[k], c2=C2, rounds=2, global_config=cfgs["default"])
    sl = slice(arrays[5][k], arrays[5][k + 1])
    for name in NAMES:
        assert same(one[name], out["default"][name][sl]), name
    for name in PER_TRACK:
        assert one[name] == out["default"][name][k], name


# ------------------------------------------------------------------------------------------------ 8. the objective and the motivation, on the device
def test_the_huber_objective_does_not_rise_on_the_device(B):
    cfg = R.one_span(full_cfg({}))
    ts, pos, quat, aligned, valid, ip, iq, mv, truth, rows = R.motivation(0, 271)
    first = W.weighted_restate(ts, pos, quat, aligned, valid, mv, ip, iq, cfg)      # the displacements, dt and the decisions: the same in every solve
    arrays = flat([(ts, pos, quat, aligned, valid, ip, iq)])
    J, err = [], []
    for rounds in range(6):
        o = runr(B, arrays, mv, cfg, "huber", rounds=rounds)
        assert o["rounds_used"][0] == rounds and same(o["flags"], first["flags"] )
        sol = dict(first, xr=o["pos"] - ip, e_rel=np.zeros_like(o["pos"]))      # the smoothed track, relative to init_pos
        J.append(R.objective(sol, aligned, ip, mv, cfg, C2))
        err.append(float(np.sqrt(np.mean(np.sum((o["pos"] - truth) ** 2, axis=1)))))
    print("Huber objective over rounds 0..5 on the device: " + " ".join(f"{v:.6g}" for v in J) + "; RMSE against the truth: " + " ".join(f"{v:.3f}" for v in err))
    for a, b in zip(J[:-1], J[1:]):
        assert b <= a * (1.0 + 1e-12), J
    assert err[-1] < err[0]
