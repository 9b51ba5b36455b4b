"""CPU tier of tests/test_ragged_routes.py: the track pool, the two ragged batches made of it, the oracle's results on the pool, and the
conditions on those inputs that need no device.

The pool holds about 250 distinct host-made tracks: the eight outage kinds of tests/test_tail_scans.py at 21 lengths around every chunk
boundary and scan-size threshold, the twenty row-rule kinds of tests/test_early_rows.py at four lengths, and one track without any
usable fix.  `small` is every pool track once in a seeded shuffled order (the one-wave build); `big` is the pool tiled and reshuffled to
exactly 2 049 tracks (the smallest batch the big-batch build takes), every track at least eight times at different row offsets.  Both
carry an empty track first, one last and two next to each other inside.  The oracle runs on the distinct tracks only."""
import copy
import functools

import numpy as np
import pytest

import test_early_rows as ER
import test_tail_scans as TS
from test_cov_host import restate

OUTAGE_LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 191, 193, 271, 1039]
ROWS_LENGTHS = [65, 129, 193, 271]
NO_FIX_LENGTH = 40
B_BIG = 2049                                                             # wave_route: B > 2 048 -> the big-batch build
COLS = ("ts", "pos", "quat", "gps", "valid", "ip", "iq")
RULES = ("reference", "all") + tuple(f"dur{k}" for k in range(len(ER.DURS)))   # the runs of the fused pipeline: both rules at the default CONFIG, the reference rule under ER.DURS
FEW, ROWS_ALL, ROWS_SEG = ER.FEW, ER.ROWS_ALL, ER.ROWS_SEG
EMPTY = -1                                                               # a slot of a batch that holds no pose


def rule_cfg(rule):
    """the CONFIG dict of a run: the default one, or test_early_rows' (min_samples, max_gap, max_initial_duration) setting k for "dur<k>\""""
    from gps_optimize_slam_amd import ekfgpsslam as E
    return ER.config(E, ER.DURS[int(rule[3:])]) if rule.startswith("dur") else copy.deepcopy(E.CONFIG)


def rule_rows(rule):
    return "all" if rule == "all" else "reference"


@functools.lru_cache(maxsize=None)
def pool():
    """the distinct tracks, made once and never changed (every array is read-only)"""
    tracks = []

    def add(family, kind, parts, b):
        t = {c: np.array(p[b]) for c, p in zip(COLS, parts)}
        t.update(family=family, kind=kind, n=len(t["ts"]))
        tracks.append(t)
    # (the seeds are chosen by the INPUTS they give: with these the random outages hold one that crosses exactly two chunk boundaries in
    # each family -- assert_coverage below --, and no track with a fit has an invalid quaternion at pose 0)
    for N in OUTAGE_LENGTHS:
        parts = TS.planted_batch(8, N, 5003 + N)
        for b in range(8):
            add("outage", b, parts, b)
    for N in ROWS_LENGTHS:
        parts = ER.planted_batch(ER.KINDS, N, 6003 + N)
        for b in range(ER.KINDS):
            add("rows", b, parts, b)
    add("no-fix", 0, TS.planted_batch(8, NO_FIX_LENGTH, 5000), 0)         # a clean track with every fix taken away
    tracks[-1]["valid"][:] = 0; tracks[-1]["gps"][:] = np.nan
    for t in tracks:
        for c in COLS:
            t[c].setflags(write=False)
    return tuple(tracks)


@functools.lru_cache(maxsize=None)
def by_length():
    """length -> pool indices of that length (one dense launch, one oracle call)"""
    d = {}
    for i, t in enumerate(pool()):
        d.setdefault(t["n"], []).append(i)
    return d


def stacked(ids):
    """the tracks `ids` (one length) as the (B, N, .) host arrays TrajectoryBatch.from_host and the oracle take"""
    return tuple(np.stack([pool()[i][c] for i in ids]) for c in COLS)


def _with_empties(order, rng):
    """an empty track first, one last, two next to each other somewhere inside"""
    k = int(rng.integers(len(order) // 4, 3 * len(order) // 4))
    return [EMPTY] + list(order[:k]) + [EMPTY, EMPTY] + list(order[k:]) + [EMPTY]


@functools.lru_cache(maxsize=None)
def orders():
    """name -> the pool index of every slot of the batch (EMPTY: no pose)"""
    P = len(pool())
    rng = np.random.default_rng(20490)
    small = _with_empties(rng.permutation(P).tolist(), rng)
    slots = B_BIG - 4
    tiled = np.concatenate([np.arange(P)] * (slots // P) + [rng.choice(P, slots % P, replace=False)])
    rng.shuffle(tiled)
    big = _with_empties(tiled.tolist(), rng)
    return {"small": tuple(small), "big": tuple(big)}


def ragged(order):
    """flat host arrays of the slots in `order` -> ts, pos, quat, gps, valid, offsets, init_pos, init_quat"""
    tr = pool()
    lens = [0 if i == EMPTY else tr[i]["n"] for i in order]
    offs = np.zeros(len(order) + 1, np.int64); offs[1:] = np.cumsum(lens)
    flat = [np.concatenate([tr[i][c] for i in order if i != EMPTY]) for c in COLS[:5]]
    ip = np.stack([np.zeros(3) if i == EMPTY else tr[i]["ip"] for i in order])
    iq = np.stack([np.array([0.0, 0.0, 0.0, 1.0]) if i == EMPTY else tr[i]["iq"] for i in order])
    return flat[0], flat[1], flat[2], flat[3], flat[4].astype(np.uint8), offs, ip, iq


def usable_rows(t):
    return (t["valid"] != 0) & np.isfinite(t["gps"]).all(axis=1)


@functools.lru_cache(maxsize=None)
def oracle_results():
    """What the oracle gives on every pool track.  "k4": [(pos, quat, status)]; rule -> [(pos, quat, status, R, t, s)] for every rule of
    RULES (the "dur<k>" rules on the row-rule tracks only, None elsewhere); "fit": rule -> [(rows or None, row flag, R, t, s)] from
    pick_sim3_rows and compute_sim3_transform on those rows."""
    from oracle import oracle as orc
    tr = pool()
    res = {"k4": [None] * len(tr), "fit": {r: [None] * len(tr) for r in RULES}}
    res.update({r: [None] * len(tr) for r in RULES})
    for N, ids in by_length().items():
        ts, pos, quat, gps, valid, ip, iq = stacked(ids)
        po, qo, st = orc.fuse_batch(ts, pos, quat, gps, valid, ip, iq)
        for j, i in enumerate(ids):
            res["k4"][i] = (po[j], qo[j], int(st[j]))
        for rule in RULES:
            sel = [j for j, i in enumerate(ids) if not rule.startswith("dur") or tr[i]["family"] == "rows"]
            if not sel:
                continue
            cfg = rule_cfg(rule)
            out = orc.fuse_pipeline_batch(ts[sel], pos[sel], quat[sel], gps[sel], valid[sel], cfg=cfg, fit_rows=rule_rows(rule))
            for k, j in enumerate(sel):
                i = ids[j]
                res[rule][i] = tuple(o[k] if o[k].ndim else o[k][()] for o in out)
                u = usable_rows(tr[i])
                if rule == "all":
                    idx, flag = (np.nonzero(u)[0] if u.sum() >= 3 else None), 0
                else:
                    idx, br = orc.pick_sim3_rows(tr[i]["ts"], u, cfg["sim3_ransac"]["min_samples"], cfg["time_alignment"]["max_gps_gap_threshold"],
                                                 cfg["sim3_ransac"]["max_initial_duration"], return_branch=True)
                    flag = FEW if idx is None else {0: 0, 1: ROWS_SEG, 2: ROWS_ALL}[br]
                fit = (None, None, None) if idx is None else orc.compute_sim3_transform(tr[i]["pos"][idx], tr[i]["gps"][idx])
                res["fit"][rule][i] = (idx, flag) + tuple(fit)
    return res


@functools.lru_cache(maxsize=None)
def decisions():
    """the outages of every pool track under the default CONFIG, from the restatement tests/test_cov_host.py pins to the reference:
    [(pool index, first row, end row, recovered)] (end = the recovery's row, or the track's length), and every (rate, threshold) compared"""
    cfg = rule_cfg("reference")
    outages, rates, status = [], [], []
    for i, t in enumerate(pool()):
        w = restate(t["ts"], t["quat"], t["gps"], t["valid"], cfg)
        rates += w["rates"]
        status.append(w["status"])
        for a, b in w["segments"] + w["sharp"]:
            outages.append((i, a, b, True))
        if w["status"] & 8:
            av = usable_rows(t)
            outages.append((i, int(np.nonzero(av)[0].max(initial=-1)) + 1, t["n"], False))
    return outages, rates, status


def coverage():
    """what the comparison must hold to be worth anything (sections 1 and 2 of the plan): counted, then asserted by both tiers"""
    res = oracle_results()
    outages, _, _ = decisions()
    bits = 0
    for _, _, st in res["k4"]:
        bits |= st
    flags = {f[1] for rule in RULES if rule != "all" for f in res["fit"][rule] if f is not None}
    crossings = {(b - 1) // 64 - a // 64 for _, a, b, rec in outages if rec}     # chunk boundaries between an outage's first and last row
    lanes = {b % 64 for _, _, b, rec in outages if rec}                          # lane of the recovering pose
    return dict(status_bits=bits & 15, row_flags=flags, crossings=crossings, recovery_lanes=lanes)


def assert_coverage(c):
    assert c["status_bits"] == 15, c                                             # HAD_OUTAGE, RTS_APPLIED, SHARP_TURN, ENDED_IN_OUTAGE
    assert {FEW, ROWS_ALL, ROWS_SEG}.issubset(c["row_flags"]), c
    assert {0, 1, 2}.issubset(c["crossings"]), c
    assert {0, 63}.issubset(c["recovery_lanes"]), c


def last_chunk_rows(n):
    return (n - 1) % 64 + 1


def offset_parities(order):
    """last-chunk row count -> [tracks starting at an even row, tracks starting at an odd row]"""
    tr = pool()
    count, row = {}, 0
    for i in order:
        if i == EMPTY:
            continue
        count.setdefault(last_chunk_rows(tr[i]["n"]), [0, 0])[row & 1] += 1
        row += tr[i]["n"]
    return count


# ------------------------------------------------------------------------------------------------ the tests of this tier
def test_pool_builds_and_its_tracks_are_distinct():
    tr = pool()
    assert len(tr) == 8 * len(OUTAGE_LENGTHS) + ER.KINDS * len(ROWS_LENGTHS) + 1
    assert sorted(by_length()) == sorted(set(OUTAGE_LENGTHS + ROWS_LENGTHS + [NO_FIX_LENGTH]))
    assert len({t["pos"].tobytes() + t["gps"].tobytes() + t["valid"].tobytes() for t in tr}) == len(tr)
    for t in tr:
        assert t["ts"].shape == (t["n"],) and t["pos"].shape == (t["n"], 3) and t["quat"].shape == (t["n"], 4) and t["gps"].shape == (t["n"], 3)
        assert t["valid"].shape == (t["n"],) and t["ip"].shape == (3,) and t["iq"].shape == (4,)
        assert np.isfinite(t["ip"]).all() and abs(np.linalg.norm(t["iq"]) - 1.0) < 1e-12
    assert not usable_rows(tr[-1]).any() and tr[-1]["family"] == "no-fix"


def test_batches_hold_what_the_plan_says():
    tr, o = pool(), orders()
    for name, order in o.items():
        assert order[0] == EMPTY and order[-1] == EMPTY
        inside = [k for k in range(1, len(order) - 2) if order[k] == EMPTY and order[k + 1] == EMPTY]
        assert len(inside) == 1 and order.count(EMPTY) == 4, name
        assert order[inside[0] - 1] != EMPTY and order[inside[0] + 2] != EMPTY, name
    assert len(o["small"]) == len(tr) + 4 <= 2048 and sorted(i for i in o["small"] if i != EMPTY) == list(range(len(tr)))
    assert len(o["big"]) == B_BIG
    copies = np.bincount([i for i in o["big"] if i != EMPTY], minlength=len(tr))
    assert copies.min() >= 4, copies.min()
    # every copy of a track at another row offset, and neighbouring lengths that differ (a tiling in pool order would be sorted by length)
    ts, pos, quat, gps, valid, offs, ip, iq = ragged(o["big"])
    assert ts.size == offs[-1] and pos.shape == (ts.size, 3) and ip.shape == (B_BIG, 3) and 2e5 < ts.size < 6e5
    for i in (0, len(tr) // 2, len(tr) - 1):
        assert len({int(offs[k]) for k, j in enumerate(o["big"]) if j == i}) == copies[i]
    lens = np.diff(offs)
    assert (lens[1:] != lens[:-1]).mean() > 0.9
    # both parities of the first row for every last-chunk row count the batch holds: an input condition, fixed by the seed
    par = offset_parities(o["big"])
    assert sorted(par) == sorted({last_chunk_rows(t["n"]) for t in tr})
    assert {1, 2, 3, 63, 64}.issubset(par) and any(r & 1 for r in par) and any(not r & 1 for r in par)
    for rows, (even, odd) in par.items():
        assert even >= 1 and odd >= 1, (rows, even, odd)


def test_oracle_is_finite_exactly_where_the_rule_has_its_rows():
    """K4 always has poses; the fused pipeline has none exactly where its row rule finds fewer rows than it needs (the reference raises,
    :975 / :997, or its fit is None below three rows, :430) -- and then every pose is NaN, never a part of the track"""
    tr, res = pool(), oracle_results()
    for i, t in enumerate(tr):
        p, q, st = res["k4"][i]
        assert np.isfinite(p).all() and np.isfinite(q).all(), i
        for rule in RULES:
            if res[rule][i] is None:
                assert rule.startswith("dur") and t["family"] != "rows"
                continue
            p, q, st, R, tt, s = res[rule][i]
            idx, flag, Ro, to, so = res["fit"][rule][i]
            few = idx is None
            assert few == (not np.isfinite(p).any()) == (not np.isfinite(q).any()), (i, rule)
            assert np.isfinite(p).all() == np.isfinite(q).all() == (not few), (i, rule)
            assert ((st >> 8) & 1 != 0) == few and (st >> 8) & (FEW | ROWS_ALL | ROWS_SEG) == flag, (i, rule, hex(st), flag)
            if not few:                                                  # the two routes through the oracle hold the same fit
                assert Ro is not None, (i, rule)
                np.testing.assert_array_equal(R.reshape(3, 3), Ro); np.testing.assert_array_equal(tt, to); assert s == so
                assert np.linalg.norm(t["quat"][0]) > 0.0, (i, rule)     # (pose 0 can be transformed: the comparison through it applies)
    ok = [res["reference"][i][2] >> 8 & 1 == 0 for i in range(len(tr))]
    assert 0.5 < np.mean(ok) < 1.0                                      # most tracks are fused, some are not
    assert res["reference"][len(tr) - 1][2] >> 8 == 1 | FEW and res["all"][len(tr) - 1][2] >> 8 == 1


def test_no_planted_decision_hangs_on_its_threshold():
    """every yaw rate the sharp-turn test compares lies more than 10 % from the threshold (the check of tests/test_cov_gpu.py on its planted
    tracks), and the restatement that lists those rates decides as the oracle does"""
    outages, rates, status = decisions()
    assert len(rates) >= 50                                              # (outages of two poses or more that are recovered: the others compare no rate)
    for rate, thr in rates:
        assert not (0.9 * thr <= rate <= 1.1 * thr), (rate, thr)
    assert any(rate > thr for rate, thr in rates) and any(rate < thr for rate, thr in rates)
    res = oracle_results()
    for i, st in enumerate(status):
        assert st == res["k4"][i][2] & 15, (i, st, res["k4"][i][2])


def test_the_comparison_is_not_empty():
    c = coverage()
    print(c)
    assert_coverage(c)
