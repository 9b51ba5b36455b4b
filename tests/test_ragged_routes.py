"""The ragged pose entries (gsf_ekf_fuse_ragged_dev / gsf_fuse_pipeline_ragged_dev, batch.ekf_fuse_ragged / fuse_pipeline_ragged) on
both builds a ragged call can take -- the one-wave build up to 2 048 tracks, the big-batch build (ekf_wave_big_kernel: rows fetched and
stored as 16-byte pieces of each chunk's slab) above --, and the whole-run chain at 2 049 tracks.

1. Against the oracle: the pool of tests/test_ragged_routes_host.py (about 250 distinct tracks: outages, NaN fixes, invalid quaternions,
   duplicate poses, yaw bursts, every row-rule corner) as a 253-track and a 2 049-track ragged batch, every copy of every track.  Gates:
   positions 1e-7 m, quaternions 1e-9, scale 1e-10, R 2e-9 (tests/test_gpu_parity.py), t through the transformed pose 0; status words,
   row flags and NaN patterns exact.
2. BITS: a track's bytes do not depend on whether it was launched dense or ragged, on its neighbours, on its place in the flat arrays or
   on how many tracks the call holds (gsf_wave_route.hpp: every family gives the same bits).  No tolerance.
3. Guard rows behind the last track stay untouched, every byte of every track is written, nothing is written for an empty one.
4. run_fusion_ragged on 2 049 tracks gives the bytes of two calls of 1 024 and 1 025 tracks."""
import copy
import ctypes as C

import numpy as np
import pytest

import test_ragged_routes_host as H
import test_tail_scans as TS
from test_tail_scans import POS_TOL, Q_TOL, S_TOL, as_bytes

pytestmark = pytest.mark.gpu

R_TOL = 2e-9                                                             # tests/test_gpu_parity.py, test_pipeline_batch_vs_oracle
ENTRIES = ("k4",) + H.RULES
FIT_INFO = 16 << 8                                                       # GSF_SIM3_FLAG_SVD_FALLBACK: informational, the oracle has no such bit
GUARD = 64


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


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def batches(B):
    """name -> (order, offsets, device tensors ts, pos, quat, gps, valid, offsets, init_pos, init_quat)"""
    out = {}
    for name, order in H.orders().items():
        host = H.ragged(order)
        out[name] = (order, host[5], [dev(a) for a in host])
    return out


def run_ragged(B, d, entry):
    """one ragged call -> name -> numpy array, as the caller gets them"""
    import torch
    if entry == "k4":
        res = dict(zip(("pos", "quat", "status"), B.ekf_fuse_ragged(*d)))
    else:
        res = dict(zip(("pos", "quat", "status", "R", "t", "s"), B.fuse_pipeline_ragged(*d[:6], config=H.rule_cfg(entry), fit_rows=H.rule_rows(entry))))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.fixture(scope="module")
def runs(B, batches):
    """(batch, entry) -> outputs; every test below reads these, none changes them"""
    return {(name, entry): run_ragged(B, d, entry) for name, (_, _, d) in batches.items() for entry in ENTRIES}


def test_the_batches_take_the_two_builds():
    """253 tracks: the one-wave build; 2 049: the smallest batch of the big-batch build, with both parities of the first row for every
    last-chunk row count (the CPU tier asserts the same on the same seeded shuffle)"""
    o = H.orders()
    assert len(o["small"]) <= 2048 < len(o["big"]) == H.B_BIG
    par = H.offset_parities(o["big"])
    assert sorted(par) == [1, 2, 3, 15, 16, 17, 31, 32, 33, 40, 63, 64]        # what the pool's lengths leave in a last chunk
    for rows, (even, odd) in par.items():
        assert even >= 1 and odd >= 1, (rows, even, odd)
    H.assert_coverage(H.coverage())


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["small", "big"])
def test_against_the_oracle(orc, batches, runs, name, entry):
    order, offs, _ = batches[name]
    got, tr, res = runs[(name, entry)], H.pool(), H.oracle_results()
    pipeline = entry != "k4"
    cfg = H.rule_cfg(entry) if pipeline else None
    worst = dict(dp=0.0, dq=0.0, ds=0.0, dR=0.0, dp_pose0=0.0, dq_pose0=0.0)
    failures, from_fit = [], {}
    fused = without_poses = 0
    flags_seen, bits_seen = set(), 0
    for k, i in enumerate(order):
        if i == H.EMPTY:
            assert offs[k] == offs[k + 1] and got["status"][k] == 0, k
            if pipeline:
                assert np.isnan(got["R"][k]).all() and np.isnan(got["t"][k]).all() and np.isnan(got["s"][k]), k
            continue
        want = res[entry][i] if pipeline else res["k4"][i]
        if want is None:                                                 # the duration settings are compared on the row-rule tracks
            continue
        t = tr[i]
        sl = slice(offs[k], offs[k + 1])
        p, q, st = got["pos"][sl], got["quat"][sl], int(got["status"][k])
        wp, wq, wst = want[0], want[1], int(want[2])
        if pipeline:
            st &= ~FIT_INFO
        if not (np.array_equal(np.isnan(p), np.isnan(wp)) and np.array_equal(np.isnan(q), np.isnan(wq))):
            failures.append((k, i, "NaN pattern")); continue
        if not np.isfinite(wp).all():                                    # the oracle has no poses: NaN rows here, and the same fit word
            assert pipeline and np.isnan(wp).all()
            without_poses += 1
            if st >> 8 != wst >> 8:
                failures.append((k, i, "fit word", hex(st), hex(wst)))
            flags_seen.add((st >> 8) & (H.FEW | H.ROWS_ALL | H.ROWS_SEG))
            continue
        fused += 1
        bits_seen |= st & 15
        if st != wst:
            failures.append((k, i, "status", hex(st), hex(wst)))
        ep, eq = np.abs(p - wp).max(), np.abs(q - wq).max()
        worst["dp"], worst["dq"] = max(worst["dp"], ep), max(worst["dq"], eq)
        if not (ep < POS_TOL and eq < Q_TOL):
            failures.append((k, i, "poses", ep, eq))
        if not pipeline:
            continue
        idx, flag, Ro, to, so = res["fit"][entry][i]
        flags_seen.add((st >> 8) & (H.FEW | H.ROWS_ALL | H.ROWS_SEG))
        if (st >> 8) & (H.FEW | H.ROWS_ALL | H.ROWS_SEG) != flag:
            failures.append((k, i, "row flags", hex(st), flag))
        R, tt, s = got["R"][k], got["t"][k], float(got["s"][k])
        eR, es = np.abs(R.reshape(3, 3) - Ro).max(), abs(s - so)
        worst["dR"], worst["ds"] = max(worst["dR"], eR), max(worst["ds"], es)
        if not (eR <= R_TOL and es < S_TOL):
            failures.append((k, i, "fit", eR, es))
        # t through the transformed pose 0: the oracle's EKF started from the DEVICE's fit (once per distinct fit of a track)
        key = (i, R.tobytes(), tt.tobytes(), got["s"][k].tobytes())
        if key not in from_fit:
            sp, sq = orc.transform_trajectory(t["pos"][:1], t["quat"][:1], R.reshape(3, 3), tt, s)
            from_fit[key] = orc.apply_ekf_correction_aligned(t["ts"], t["pos"], t["quat"], t["gps"], t["valid"], sp[0], sq[0], cfg, return_status=True)
        po, qo, sto = from_fit[key]
        ep, eq = np.abs(p - po).max(), np.abs(q - qo).max()
        worst["dp_pose0"], worst["dq_pose0"] = max(worst["dp_pose0"], ep), max(worst["dq_pose0"], eq)
        if not (ep < POS_TOL and eq < Q_TOL and (st & 0xff) == sto):
            failures.append((k, i, "poses from the device's fit", ep, eq, st & 0xff, sto))
    build = "one-wave build" if len(order) <= 2048 else "big-batch build"
    print(f"{build} ({len(order)} tracks), {'ekf_fuse_ragged' if not pipeline else 'fuse_pipeline_ragged/' + entry}: {fused} fused tracks compared, "
          f"{without_poses} without poses; max |dp| {worst['dp']:.2e} m, |dq| {worst['dq']:.2e}" +
          (f", |ds| {worst['ds']:.2e}, |dR| {worst['dR']:.2e}; from the device's fit |dp| {worst['dp_pose0']:.2e} m, |dq| {worst['dq_pose0']:.2e}, "
           f"{len(from_fit)} distinct fits" if pipeline else ""))
    assert not failures, (len(failures), [(k, i, tr[i]["family"], tr[i]["kind"], tr[i]["n"]) + tuple(rest) for k, i, *rest in failures[:6]])
    # the comparison is not empty
    assert fused > 0.8 * sum(1 for i in order if i != H.EMPTY and (res[entry][i] if pipeline else res["k4"][i]) is not None) and fused >= 70
    if pipeline:
        assert without_poses >= 1
    else:
        assert bits_seen == 15
    if entry in ("reference", "dur0"):
        assert H.FEW in flags_seen and H.ROWS_ALL in flags_seen and 0 in flags_seen, flags_seen


def test_row_flags_over_the_settings(runs):
    """FEW / ROWS_ALL / ROWS_SEG and the plain timed subset all occur on the device over the reference rule's settings"""
    seen = set()
    for (name, entry), got in runs.items():
        if entry not in ("k4", "all"):
            seen |= set(((got["status"] >> 8) & (H.FEW | H.ROWS_ALL | H.ROWS_SEG)).tolist())
    assert {0, H.FEW, H.ROWS_ALL, H.ROWS_SEG}.issubset(seen), seen


# ------------------------------------------------------------------------------------------------ 2. the same bits as the dense launch
def test_dense_launch_gives_the_bytes_of_the_ragged_one(B, batches, runs):
    """every length of the pool as a dense TrajectoryBatch (K4, pipeline under both row rules, default options): each track's bytes against
    its rows in the ragged 253-track call and against every copy in the ragged 2 049-track call"""
    slots = {name: {} for name in batches}
    for name, (order, _, _) in batches.items():
        for k, i in enumerate(order):
            if i != H.EMPTY:
                slots[name].setdefault(i, []).append(k)
    differing = {}
    compared = 0
    for N, ids in H.by_length().items():
        dense = TS.run_all(B, B.TrajectoryBatch.from_host(*H.stacked(ids), layout=0))
        for key, arr in dense.items():
            entry, field = key.split(".")
            for name, (order, offs, _) in batches.items():
                got = runs[(name, entry)][field]
                for j, i in enumerate(ids):
                    for k in slots[name][i]:
                        mine = got[offs[k]:offs[k + 1]] if field in ("pos", "quat") else got[k]
                        a, b = as_bytes(mine), as_bytes(arr[j])
                        assert a.shape == b.shape, (N, key, name, k)
                        n = int((a != b).sum())
                        compared += a.size
                        if n:
                            differing.setdefault((name, key), []).append((N, i, k, n))
    for what, rows in differing.items():
        print(what, len(rows), "track copies differ, first:", rows[:5])
    print(f"dense against ragged: {compared} bytes compared, {sum(r[3] for rows in differing.values() for r in rows)} differ")
    assert not differing, {w: (len(r), r[:3]) for w, r in differing.items()}
    assert compared > 5e7


def test_dense_big_batch_gives_the_bytes_of_the_ragged_big_batch(B):
    """the pool's 271-pose tracks tiled to 2 049: one dense call and one ragged call of the big-batch build, only `offsets` differs"""
    ids = H.by_length()[271]
    sel = np.arange(H.B_BIG) % len(ids)
    ts, pos, quat, gps, valid, ip, iq = (a[sel] for a in H.stacked(ids))
    dense = TS.run_all(B, B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=0))
    offs = np.arange(H.B_BIG + 1, dtype=np.int64) * 271
    d = [dev(a) for a in (ts.reshape(-1), pos.reshape(-1, 3), quat.reshape(-1, 4), gps.reshape(-1, 3), valid.reshape(-1).astype(np.uint8), offs, ip, iq)]
    total = 0
    for entry in ("k4", "reference", "all"):
        got = run_ragged(B, d, entry)
        for field, arr in got.items():
            a, b = as_bytes(arr), as_bytes(dense[f"{entry}.{field}"])
            assert a.shape == b.shape, (entry, field)
            n = int((a != b).sum())
            total += n
            print(f"dense against ragged at 2 049 x 271, {entry}.{field}: {n} differing bytes of {a.size}")
            assert n == 0, (entry, field, n)
    assert total == 0
    assert np.isfinite(dense["reference.pos"]).all(axis=(1, 2)).sum() > 1500 and not np.isfinite(dense["reference.pos"]).all()


# ------------------------------------------------------------------------------------------------ 3. guard rows
@pytest.mark.parametrize("entry", ["k4", "reference"])
def test_guard_rows_and_every_byte_written(B, batches, runs, entry):
    """the entry points themselves on caller-made outputs with 64 spare rows / entries behind the last track, under two prefill bytes"""
    import torch
    from gps_optimize_slam_amd import _lib
    order, offs, d = batches["big"]
    T, nb = int(offs[-1]), len(order)
    L, ctx = _lib.load(), B.context()
    cfg = _lib.EkfConfig.from_config(B.CONFIG)
    p = lambda t: C.c_void_p(t.data_ptr())
    sizes = {"pos": (T * 24, "pos"), "quat": (T * 32, "quat"), "status": (nb * 4, "status")}
    if entry != "k4":
        sizes.update({"R": (nb * 72, "R"), "t": (nb * 24, "t"), "s": (nb * 8, "s")})
    unit = {"pos": 24, "quat": 32, "status": 4, "R": 72, "t": 24, "s": 8}
    payloads = []
    for fill in (0x5A, 0xC3):
        o = {k: torch.full((n + GUARD * unit[k],), fill, dtype=torch.uint8, device="cuda") for k, (n, _) in sizes.items()}
        if entry == "k4":
            _lib.check(L.gsf_ekf_fuse_ragged_dev(ctx.handle, *(p(x) for x in d), C.byref(cfg), nb, p(o["pos"]), p(o["quat"]), p(o["status"])))
        else:
            ctx.set_sim3_rows("reference", B.CONFIG)
            _lib.check(L.gsf_fuse_pipeline_ragged_dev(ctx.handle, *(p(x) for x in d[:6]), C.byref(cfg), nb, p(o["R"]), p(o["t"]), p(o["s"]), p(o["pos"]),
                                                      p(o["quat"]), p(o["status"])))
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in o.items()}
        for k, (n, _) in sizes.items():
            assert host[k].size == n + GUARD * unit[k]
            touched = np.nonzero(host[k][n:] != fill)[0]
            assert touched.size == 0, (entry, k, hex(fill), "first guard byte written at +", int(touched[0]))
        payloads.append({k: host[k][:n] for k, (n, _) in sizes.items()})
    for k in sizes:
        # a byte nobody wrote holds 0x5a in one run and 0xc3 in the other; and the bytes are those of the plain call compared above
        assert np.array_equal(payloads[0][k], payloads[1][k]), (entry, k, int((payloads[0][k] != payloads[1][k]).sum()))
        assert np.array_equal(payloads[0][k], as_bytes(runs[("big", entry)][k])), (entry, k)
    status = payloads[0]["status"].view(np.int32)
    empty = [k for k, i in enumerate(order) if i == H.EMPTY]
    assert len(empty) == 4 and (status[empty] == 0).all() and all(offs[k] == offs[k + 1] for k in empty)


# ------------------------------------------------------------------------------------------------ 4. the whole-run chain at 2 049 tracks
RUN_LENGTHS = [0, 1, 5, 63, 64, 65, 66, 90, 130]


def run_tracks(orc, nb):
    """short file-less tracks as tests/test_run_ragged.py makes its 64: a log that runs on past the shortest tracks, fixes thrown 60 m off
    on every third, rows the loader removes on every fifth, an independent sparser ground-truth log on three of four"""
    from test_run_ragged import _log, _synthetic_case
    rng = np.random.default_rng(2049)
    lens = [RUN_LENGTHS[b] for b in range(len(RUN_LENGTHS))] + [int(v) for v in rng.choice(RUN_LENGTHS, nb - len(RUN_LENGTHS))]
    tracks, logs, gts = [], [], []
    for b, n in enumerate(lens):
        tt, pp, qq, uu = _synthetic_case(orc, max(n, 50), b)
        log = _log(orc, tt, uu, rng, 0.3, 0.03)
        m = len(log)
        if b % 3 == 0:
            for r_ in rng.choice(m, size=int(rng.integers(1, 6)), replace=False):
                log[r_, 1] += 60.0 / 111200.0 * rng.choice([-1, 1]); log[r_, 2] += 60.0 / 73000.0 * rng.choice([-1, 1])
        if b % 5 == 1:
            rr = rng.choice(m, size=4, replace=False)
            log[rr[0], 1] = 0.0; log[rr[1], 2] = 0.0; log[rr[2], 1] = 91.0; log[rr[3], 2] = -181.0
        gts.append(_log(orc, tt[::2], uu[::2], rng, 0.15, 0.05) if b % 4 != 3 else None)
        tracks.append((tt[:n], pp[:n], qq[:n])); logs.append(log)
    return tracks, logs, gts


PER_POSE = ("aligned", "valid", "sim3_pos", "inlier_mask", "gt_aligned", "gt_valid")
PER_FIX = ("gps_utm", "gps_keep")
PER_GT_FIX = ("gt_utm", "gt_keep")
PER_TRACK = ("R", "t", "s", "n_inliers", "zone", "south", "gt_zone", "gt_south", "plot_ref", "run_status", "trial_info")


@pytest.fixture(scope="module")
def whole_run(B, orc):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    tracks, logs, gts = run_tracks(orc, H.B_BIG)
    seeds = np.arange(H.B_BIG) + 7
    cfg = copy.deepcopy(E.CONFIG)

    def call(lo, hi, early_exit=False):
        rb = B.RaggedGeodeticBatch.from_host(tracks[lo:hi], logs[lo:hi], gts[lo:hi])
        st = B.mt19937_seed(seeds[lo:hi])
        r = B.run_fusion_ragged(rb, st, cfg, early_exit=early_exit)
        torch.cuda.synchronize()
        return rb, r, st
    return tracks, logs, gts, seeds, cfg, call(0, H.B_BIG), call


@pytest.mark.parametrize("early_exit", [False, True])
def test_whole_run_of_2049_tracks_equals_its_two_halves(whole_run, early_exit):
    """every output of run_fusion_ragged is per track, per pose or per fix: the 2 049-track call (its EKF on the big-batch build) gives the
    bytes of the calls on tracks 0..1 023 and 1 024..2 048 (one-wave build), and leaves the generators where they leave them -- with every
    trial drawn (the run the oracle is compared with below) and with the early exit a caller gets by default"""
    import torch
    from test_run_ragged import _same_words
    _, _, _, _, _, whole, call = whole_run
    rb, r, st = call(0, H.B_BIG, True) if early_exit else whole
    parts = [call(0, 1024, early_exit), call(1024, H.B_BIG, early_exit)]
    cat = lambda f, dim=0: torch.cat([f(x) for x in parts], dim=dim)
    _same_words(st, cat(lambda x: x[2]), "generator states")
    _same_words(r.fused.pos, cat(lambda x: x[1].fused.pos), "fused positions")
    _same_words(r.fused.quat, cat(lambda x: x[1].fused.quat), "fused quaternions")
    _same_words(r.fused.status, cat(lambda x: x[1].fused.status), "fused status")
    for names in (PER_POSE, PER_FIX, PER_GT_FIX, PER_TRACK):
        for k in names:
            assert getattr(r, k) is not None, k
            _same_words(getattr(r, k), cat(lambda x: getattr(x[1], k)), k)
    _same_words(r.err_stats, cat(lambda x: x[1].err_stats, dim=2), "err_stats")
    named = set(PER_POSE + PER_FIX + PER_GT_FIX + PER_TRACK) | {"fused", "err_stats", "slam_offsets", "gps_offsets", "gt_offsets"}   # (the offsets are the inputs')
    assert set(vars(r)) == named, set(vars(r)) ^ named                  # no batch-level output, and none left out
    assert int((r.run_status == 0).sum()) > 1200 and int((r.run_status != 0).sum()) > 200
    lens = np.diff(rb.slam_offsets.cpu().numpy())
    assert sorted(set(lens.tolist())) == RUN_LENGTHS and rb.B == H.B_BIG


def test_whole_run_of_2049_tracks_against_the_oracles_composition(B, orc, whole_run):
    """the first 64 tracks of the 2 049-track call against tests/test_run_ragged.py's composition of the oracle, at that file's gates"""
    from test_run_ragged import _oracle_run_gt, np_state
    tracks, logs, gts, seeds, cfg, (rb, r, st), _ = whole_run
    so = rb.slam_offsets.cpu().numpy()
    p, q = r.fused.pos.cpu().numpy(), r.fused.quat.cpu().numpy()
    stats, rs, pref = r.err_stats.cpu().numpy(), r.run_status.cpu().numpy(), r.plot_ref.cpu().numpy()
    va, gval, status = r.valid.cpu().numpy().astype(bool), r.gt_valid.cpu().numpy().astype(bool), r.fused.status.cpu().numpy()
    kinds, worst = set(), 0.0
    for b in range(64):
        ts, pos, quat = tracks[b]
        o = _oracle_run_gt(orc, ts, pos, quat, logs[b], gts[b], cfg, int(seeds[b]))
        key, ppos = np.random.get_state()[1:3]
        gk, gp = np_state(st[b])
        np.testing.assert_array_equal(gk, key, err_msg=str(b)); assert gp == int(ppos), b
        assert rs[b] == o["status"], (b, rs[b], o["status"])
        kinds.add(int(o["status"]))
        sl = slice(so[b], so[b + 1])
        if o["status"] != 0:
            assert np.isnan(p[sl]).all() and (stats[:, :, b, 0] == 0).all() and pref[b] == 0, b
            continue
        np.testing.assert_array_equal(va[sl], o["valid"], err_msg=str(b))
        assert int(r.n_inliers[b]) == o["n_inliers"] and (status[b] & 0xff) == o["st"], b
        k = max(1.0, o["amp"] / 100.0)                                   # the gates of test_ragged_chain_with_ground_truth_vs_the_oracles_composition
        short = 4e-9 / max(o["spread"], 1e-3)
        np.testing.assert_allclose(r.R[b].cpu().numpy().reshape(3, 3), o["R"], atol=max(2e-9 * k, short), rtol=0, err_msg=str(b))
        assert abs(float(r.s[b]) - o["s"]) < max(1e-11 * k, short), (b, abs(float(r.s[b]) - o["s"]))
        worst = max(worst, np.abs(p[sl] - o["pos"]).max())
        assert np.abs(p[sl] - o["pos"]).max() < 1e-6 * k and np.abs(q[sl] - o["quat"]).max() < 1e-8 * k, (b, np.abs(p[sl] - o["pos"]).max())
        for blk, errs in ((0, o["errs"]), (1, o["errs_gt"])):
            for row in range(3):
                if errs is None:
                    assert stats[blk, row, b, 0] == 0; continue
                e = errs[row]
                assert int(stats[blk, row, b, 0]) == e["count"], (b, blk, row)
                if e["count"]:
                    np.testing.assert_allclose(stats[blk, row, b, 1:], [e["mean"], e["median"], e["rmse"]], rtol=1e-12, atol=1e-6)
        if o["errs_gt"] is not None:
            np.testing.assert_array_equal(gval[sl], o["gt_valid"], err_msg=str(b))
        assert pref[b] == o["plot_ref"], b
    print(f"whole run at 2 049 tracks, first 64 against the oracle: max |dp| {worst:.2e} m, run_status kinds {sorted(kinds)}")
    assert {0, 256}.issubset(kinds) and len(kinds) >= 3, kinds
