"""CPU tier of the sharp-turn gate tests: the case grid, the references, and the product's gate compiled for the CPU.

At every GNSS recovery the EKF routes decide between RTS smoothing and a sharp-turn recovery (EKFGPSSLAM.py:808-826, :879-894):
max over the pairs of the outage of |wrap(yaw2 - yaw1)| / (t2 - t1) > threshold.  The reference forms two atan2 yaws; the kernels compare
the dot and cross products of the two heading vectors with sin / cos of thr dt (yaw_rate_exceeds_body, gsf_ekf_core.hpp).  This file
plants ONE pair per track at thr (1 +- delta), in 3-D attitudes, at every placement of the pair and of its outage inside the 64-pose
chunks of the wave kernels, over thr dt from 7.85e-8 to 6; tests/test_sharp_turn_gate.py runs every kernel on the same tracks.

References.  The float64 one is the oracle (oracle.is_sharp_turn_in_segment, fuse_batch).  The truth is `mp_segment`: the maximum rate of
an outage from the STORED float64 quaternions and stamps with mpmath at 50 digits.  A grid case is decidable when the oracle decides like
the 50-digit truth and the 50-digit |rate / thr - 1| is at least delta / 2; test_every_grid_case_is_decidable asserts that this is the
WHOLE grid, so nothing below is left out as too close to call.

Shape of the generator, and why.  A float64 heading vector (m00, -m01) of a unit quaternion carries an absolute error of ~2e-16, i.e. an
error of ~2e-16 / cos(pitch) in the yaw of ANY float64 evaluation, the reference's included.  On most tracks the pitch swings within
+-1.2 rad (error <= 6e-16 rad per pose), which the smallest margin of the grid, thr dt delta / 2 = 3.9e-15 rad, still clears.  The tracks
whose pitch reaches +-1.55 rad AT the planted pair (heading vector of length^2 4e-4, error 1e-14 rad) are therefore made only where
thr dt delta >= 1e-11 rad; elsewhere those track slots keep the +-1.2 rad swing.  Exact gimbal lock is left out.

The corner rows (a pose logged twice 1 ns / 10 ns / 1 ulp apart, thr = 0, thr < 0 with repeated stamps, a zero quaternion) carry their
expected decision with them; it is checked against the oracle and the 50-digit truth as well."""
import copy
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from test_cov_host import ENDED_IN_OUTAGE, HAD_OUTAGE, RTS_APPLIED, ST_SHARP
from test_host_math import _fuse, hh  # noqa: F401  (hh: the fixture that compiles tests/host_harness.cpp)

NB = 64
LENGTHS = [65, 200]                     # one chunk and a one-pose tail; three chunks and a ragged tail
LAYOUT_N = 200                          # a longer track (the early-variance shape, 256) keeps the outages of N = 200 and adds gentle valid poses
THR_DEG, DT = 45.0, 0.1                 # the default threshold and the nominal sampling step
GENTLE, BURST = 2.0 / 45.0, 140.0 / 45.0        # background turn rate and the rate on an UNCOUNTED pair, as shares of the threshold
C_GRID = [7.85e-6, 7.85e-4, 7.85e-3, 0.0785, 0.7849, 0.7851, 3.06]    # thr dt: around the 0.785 switch of the polynomial, and near pi
DELTAS = [1e-3, 1e-6, 1e-9]
C_TINY = 7.85e-8                        # delta = 1e-3 and 1e-6 only (at 1e-9 the reference itself is undecided)
C_NEVER = [3.2, 6.0]                    # thr dt >= pi: never sharp; planted steps of exactly pi and of 3.1 rad
STEEP_MARGIN = 1e-11                    # rad: the smallest thr dt delta at which a track's pitch reaches +-1.55 rad at the planted pair
BAD_QUAT = 16                           # GSF_ST_BAD_QUAT
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


# ------------------------------------------------------------------------------------------------ the batches
def _grid_batch(c, via, offset=3.0):
    """one thr dt value: 16 placements x 4 variants (delta, side s of the threshold; None: the side alternates with the placement)"""
    if c in C_NEVER:
        variants = [dict(delta=0.0, s=None, step=np.pi), dict(delta=0.0, s=None, step=3.1)] * 2
    elif c == C_TINY:
        variants = [dict(delta=1e-3, s=1), dict(delta=1e-3, s=-1), dict(delta=1e-6, s=1), dict(delta=1e-6, s=-1)]
    else:
        variants = [dict(delta=1e-3, s=None), dict(delta=1e-6, s=1), dict(delta=1e-6, s=-1), dict(delta=1e-9, s=None)]
    thr_deg = THR_DEG if via == "dt" else float(np.rad2deg(c / DT))
    return dict(kind="grid", c=c, via=via, offset=offset, variants=variants, thr_deg=thr_deg,
                pair_dt=(c / np.deg2rad(THR_DEG) if via == "dt" else DT))


BATCHES = {}
for _c in C_GRID + [C_TINY] + C_NEVER:                                   # thr dt reached through the pair's dt at 45 deg/s ...
    BATCHES[f"dt-{_c:g}"] = _grid_batch(_c, "dt")
for _c in C_GRID:                                                        # ... and through the threshold at dt = 0.1 s: 4.5e-3 .. 1 753 deg/s
    if _c != 0.0785:                                                     # (0.0785 at 0.1 s IS 45 deg/s: the batch dt-0.0785)
        BATCHES[f"thr-{_c:g}"] = _grid_batch(_c, "thr")
BATCHES["epoch-0.0785"] = _grid_batch(0.0785, "thr", offset=1.7e9)       # stamps of 1.7e9 s: one ulp is 2.4e-7 s
BATCHES["corner-dup-zero"] = dict(kind="corner", thr_deg=THR_DEG, offset=3.0, rows=["dup-1e-9", "dup-1e-8", "dup-ulp", "zero-skipped", "zero-rising"])
BATCHES["corner-thr0"] = dict(kind="corner", thr_deg=0.0, offset=3.0, rows=["identical", "differs-1e-12", "one-pose"])
BATCHES["corner-thr-neg"] = dict(kind="corner", thr_deg=-1.0, offset=3.0, rows=["neg-2-repeated", "neg-5-repeated", "neg-one-pose", "neg-rising"])
GRID_NAMES = [n for n, b in BATCHES.items() if b["kind"] == "grid"]
# what a corner row must give: the outage is judged a sharp turn (None: no decision, the outage has one pose)
CORNER_SHARP = {"dup-1e-9": False, "dup-1e-8": False, "dup-ulp": False, "zero-skipped": False, "zero-rising": True, "identical": False,
                "differs-1e-12": True, "one-pose": False, "neg-2-repeated": True, "neg-5-repeated": True, "neg-one-pose": False, "neg-rising": True}


def batch_config(base, name):
    cfg = copy.deepcopy(base)
    cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"] = BATCHES[name]["thr_deg"]
    return cfg


def thr_rad(name):
    """the threshold as every implementation forms it (np.deg2rad, :886)"""
    return float(np.deg2rad(BATCHES[name]["thr_deg"]))


def placements(N):
    """The 16 placements at length N: outs [(a, b)] (the planted outage first), k: the planted pair is (k-1, k), bursts: pairs that turn at
    BURST x thr but are NOT counted ((a-1, a) and (b-1, b)), other: a second outage in the same chunk, sharp exactly when the planted one is
    not.  Lengths 1, 2, 3, 70 and 130 (N = 65: what fits -- 54 .. 56 poses up to the chunk border, so that at least nine fixes are left for the
    pipeline's Sim3 fit); outages from pose 0 and to the end;
    the pair first (k = a + 1) and last (k = b - 1); k-1 on lane 63 and k on lane 0 (k = 64, 128); recoveries on lane 0."""
    big = N >= 200
    P = [
        dict(outs=[(20, 21)], k=21),                                                       # 0: one pose: no pair is counted, never sharp
        dict(outs=[(20, 22)], k=21),                                                       # 1: two poses: the single pair
        dict(outs=[(20, 23)], k=21),                                                       # 2: three poses, first pair
        dict(outs=[(20, 23)], k=22),                                                       # 3: three poses, last pair
        dict(outs=[(30, 100)], k=31) if big else dict(outs=[(8, 63)], k=9),                # 4: 70 poses across a chunk border, first pair
        dict(outs=[(30, 100)], k=99) if big else dict(outs=[(8, 63)], k=62),               # 5: ... last pair
        dict(outs=[(30, 100)], k=64) if big else dict(outs=[(8, 64)], k=40),               # 6: ... the pair across the border (N = 65: recovery on lane 0)
        dict(outs=[(20, 150)], k=21) if big else dict(outs=[(9, 64)], k=10),               # 7: 130 poses across two borders, first pair
        dict(outs=[(20, 150)], k=64) if big else dict(outs=[(9, 64)], k=33),               # 8: ... the pair across the first border
        dict(outs=[(20, 150)], k=128) if big else dict(outs=[(10, 64)], k=63),             # 9: ... across the second (N = 65: last pair, recovery on lane 0)
        dict(outs=[(20, 150)], k=149) if big else dict(outs=[(10, 64)], k=11),             # 10: ... last pair (N = 65: first pair)
        dict(outs=[(0, 12)], k=1),                                                         # 11: from pose 0, the pair (0, 1)
        dict(outs=[(N - 12, N)], k=N - 6) if big else dict(outs=[(N - 12, N)], k=64),      # 12: never recovered (N = 65: the pair across the border)
        dict(outs=[(20, 26)], k=23, bursts=[20, 26]),                                      # 13: the two uncounted pairs turn at 140 / 45 x thr
        dict(outs=[(30, 36), (10, 14)], k=33, other=12),                                   # 14: two outages in one chunk, one sharp and one not
        dict(outs=[(40, 64)], k=63),                                                       # 15: recovery on lane 0 of the next chunk, last pair
    ]
    assert len(P) == 16
    return P


_tracks = {}


def make_batch(name, N):
    """The 64 host-made tracks of a (batch, length), trajectory-major, made once and never changed: dict of ts (B,N), pos, quat, gps, valid,
    init_pos, init_quat and meta: per track dict(outs, k, delta, s, row, steep)."""
    key = (name, N)
    if key in _tracks:
        return _tracks[key]
    spec = BATCHES[name]
    rng = np.random.default_rng(9100 + 10 * list(BATCHES).index(name) + (N % 7))
    thr = thr_rad(name)
    g_thr = thr if thr > 0.0 else np.deg2rad(THR_DEG)                   # the corner batches with thr <= 0 turn as the default ones do
    LN = min(N, LAYOUT_N)
    ts, yaw, pitch, roll = (np.empty((NB, N)) for _ in range(4))
    valid = np.ones((NB, N), np.uint8)
    meta, fix = [], []
    for j in range(NB):
        m = dict(outs=[], k=None, delta=None, s=None, row=None, steep=False)
        dts = np.full(N, DT); dts[0] = 0.0
        turn = rng.choice([-1.0, 1.0])
        rate = np.full(N, GENTLE * g_thr * turn)                         # rad/s into pose i
        step = {}                                                        # pose -> the yaw step into it, set after the stamps are known
        if spec["kind"] == "grid":
            pl, var = placements(LN)[j // 4], spec["variants"][j % 4]
            s = var["s"] if var["s"] is not None else (1 if ((j // 4) + (N % 2)) % 2 == 0 else -1)
            m.update(outs=list(pl["outs"]), k=pl["k"], delta=var["delta"], s=s)
            dts[pl["k"]] = spec["pair_dt"]
            step[pl["k"]] = ("planted", var.get("step"))
            burst = [p for p in pl.get("bursts", [])]
            if "other" in pl and not (s > 0 and spec["c"] < np.pi):      # the second outage is the sharp one
                burst.append(pl["other"])
            for p in burst:
                if p < N:
                    step[p] = ("burst", None)
            m["steep"] = bool(j % 5 == 2 and (var["delta"] == 0.0 or spec["c"] * var["delta"] >= STEEP_MARGIN))
        else:
            row = spec["rows"][j % len(spec["rows"])]
            m["row"] = row
            a = 20
            b = {"one-pose": 21, "neg-one-pose": 21, "neg-2-repeated": 22, "neg-5-repeated": 25, "neg-rising": 23}.get(row, 26)
            m["outs"] = [(a, b)]
            if row == "neg-2-repeated":
                dts[21] = 0.0
            if row == "neg-5-repeated":
                dts[21:25] = 0.0
            if row == "zero-skipped":
                dts[b - 1] = 0.0
        for a, b in m["outs"]:
            valid[j, a:b] = 0
        t = spec["offset"] + np.cumsum(dts)
        if spec["kind"] == "corner" and m["row"].startswith("dup"):      # pose 23 is pose 22 logged again, a moment later
            t[23] = {"dup-1e-9": t[22] + 1e-9, "dup-1e-8": t[22] + 1e-8, "dup-ulp": np.nextafter(t[22], np.inf)}[m["row"]]
            t[24:] = t[22] + DT * np.arange(1, N - 23)
        ts[j] = t
        real = np.diff(t, prepend=t[0])                                  # the stamp differences as float64 holds them
        d = rate * real
        for p, (what, val) in step.items():
            if what == "burst":
                d[p] = turn * min(BURST * thr * real[p], 3.1)
            elif val is not None:
                d[p] = turn * val                                        # thr dt >= pi: a step of exactly pi / of 3.1 rad
            else:
                d[p] = turn * thr * (1.0 + m["s"] * m["delta"]) * real[p]
        d[0] = rng.uniform(-np.pi, np.pi)
        yaw[j] = np.cumsum(d)
        amp = 1.55 if m["steep"] else 1.2
        ph = (np.pi / 2 - 0.11 * m["k"] + rng.uniform(-0.05, 0.05)) if m["steep"] else rng.uniform(0, 2 * np.pi)
        pitch[j] = amp * np.sin(ph + 0.11 * np.arange(N))
        roll[j] = 1.0 * np.sin(rng.uniform(0, 2 * np.pi) + 0.07 * np.arange(N))
        if spec["kind"] == "corner":
            fix.append((j, m["row"]))
        meta.append(m)
    assert np.abs(np.cos(pitch)).min() > 1e-3                            # no gimbal lock
    quat = Rotation.from_euler("zyx", np.stack([yaw, pitch, roll], -1).reshape(-1, 3)).as_quat().reshape(NB, N, 4)
    quat = quat * rng.uniform(0.5, 2.0, size=(NB, N, 1)) * rng.choice([-1.0, 1.0], size=(NB, N, 1))
    real = np.diff(ts, axis=1, prepend=ts[:, :1])
    # the path curves in all three axes whatever the batch's turn rate is (a straight one leaves the pipeline's Sim3 fit without a rotation)
    course, i = rng.uniform(-np.pi, np.pi, size=(NB, 1)) + 0.02 * np.arange(N), np.arange(N)
    pos = rng.uniform(-200.0, 200.0, size=(NB, 1, 3)) + np.cumsum(20.0 * real[..., None] * np.stack([np.cos(course), np.sin(course), 0.3 * np.sin(0.1 * i + course)], -1), axis=1)
    for j, row in fix:                                                   # the corner rows: copies are bit for bit
        if row.startswith("dup"):
            quat[j, 23], pos[j, 23] = quat[j, 22], pos[j, 22]
        elif row == "identical":
            quat[j, 20:26], pos[j, 20:26] = quat[j, 20], pos[j, 20]
        elif row == "differs-1e-12":
            quat[j, 20:23], pos[j, 20:26] = quat[j, 20], pos[j, 20]
            e = np.array([yaw[j, 20] + 1e-12, pitch[j, 20], roll[j, 20]])
            quat[j, 23:26] = Rotation.from_euler("zyx", e).as_quat() * 1.25
        elif row.startswith("zero"):
            quat[j, 25] = 0.0
    gps = pos + rng.normal(0.0, 0.3, size=pos.shape)
    gps[valid == 0] = np.nan
    init_pos = np.where(np.isnan(gps[:, 0]), pos[:, 0], gps[:, 0])
    init_quat = quat[:, 0] / np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    out = dict(ts=ts, pos=pos, quat=quat, gps=gps, valid=valid, init_pos=init_pos, init_quat=init_quat)
    for v in out.values():
        v.setflags(write=False)
    out["meta"] = meta
    _tracks[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the 50-digit truth
def mp_yaw(q):
    """the reference's yaw atan2(-m01, m00) of a stored quaternion (scale-free), 50 digits; None: the quaternion is zero (:821)"""
    import mpmath as mp
    x, y, z, w = (mp.mpf(float(v)) for v in q)
    if x == 0 and y == 0 and z == 0 and w == 0:
        return None
    return mp.atan2(2 * (z * w - x * y), w * w + x * x - y * y - z * z)


def mp_segment(ts, quat, a, b, thr):
    """is_sharp_turn_in_segment (:808-826) over the poses a..b-1 at 50 digits -> (sharp, max rate as mpf or inf, [(k, exceeds)] of the
    evaluated pairs)"""
    import mpmath as mp
    pairs = []
    if b - a < 2:
        return False, mp.mpf(0), pairs                                   # :812
    yaws = [mp_yaw(quat[k]) for k in range(a, b)]
    rate, bad = mp.mpf(0), False
    for k in range(a + 1, b):
        if ts[k] <= ts[k - 1]:
            continue                                                     # :817
        y1, y2 = yaws[k - 1 - a], yaws[k - a]
        if y1 is None or y2 is None:
            bad = True                                                   # :821 returns True
            pairs.append((k, None))
            continue
        d = y2 - y1
        r = abs(mp.atan2(mp.sin(d), mp.cos(d))) / (mp.mpf(float(ts[k])) - mp.mpf(float(ts[k - 1])))
        pairs.append((k, bool(r > mp.mpf(thr))))
        rate = max(rate, r)
    return (True, mp.inf, pairs) if bad else (bool(rate > mp.mpf(thr)), rate, pairs)


_truth = {}


def truth(name, N):
    """Per track of a (batch, length): outages [(a, b, recovered, sharp, rate)] in track order (50 digits), the status word that follows,
    the evaluated pairs [(k, exceeds)] of all its outages; made once."""
    import mpmath as mp
    key = (name, N)
    if key not in _truth:
        t, thr = make_batch(name, N), thr_rad(name)
        rows = []
        with mp.workdps(50):
            for j, m in enumerate(t["meta"]):
                outs, pairs, status = [], [], 0
                for a, b in sorted(m["outs"]):
                    sharp, rate, pr = mp_segment(t["ts"][j], t["quat"][j], a, b, thr)
                    outs.append((a, b, b < N, sharp, rate))
                    pairs += pr
                    status |= HAD_OUTAGE | ((ST_SHARP if sharp else RTS_APPLIED) if b < N else ENDED_IN_OUTAGE)
                rows.append(dict(outs=outs, pairs=pairs, status=status))
        _truth[key] = rows
    return _truth[key]


def cell_of(name, m):
    """the (thr dt, delta) cell of a track, for the tables"""
    spec = BATCHES[name]
    return (f"{spec['c']:g}", f"{m['delta']:g}") if spec["kind"] == "grid" else (name, m["row"])


def flips_table(name, N, bad_tracks):
    """{cell: number of tracks} of the tracks listed"""
    t = make_batch(name, N)
    out = {}
    for j in bad_tracks:
        c = cell_of(name, t["meta"][j])
        out[c] = out.get(c, 0) + 1
    return out


_oracle = {}


def oracle_fused(orc, name, N):
    """oracle.fuse_batch of a (batch, length) under its config: (pos, quat, status), once"""
    key = (name, N)
    if key not in _oracle:
        t = make_batch(name, N)
        r = orc.fuse_batch(t["ts"], t["pos"], t["quat"], t["gps"], t["valid"], t["init_pos"], t["init_quat"], batch_config(orc.DEFAULT_CONFIG, name))
        for x in r:
            x.setflags(write=False)
        _oracle[key] = r
    return _oracle[key]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def gate(hh):  # noqa: F811
    hh.hh_yaw_gate.restype = None
    hh.hh_yaw_gate.argtypes = [f64p, f64p, f64p, f64p, C.c_int64, u8p]
    hh.hh_gate_sin_poly.restype = None
    hh.hh_gate_sin_poly.argtypes = [f64p, C.c_int64, f64p]
    return hh


def test_the_generator_plants_what_it_says():
    """the stored quaternions turn about the reference's yaw axis by the planned steps; the grid is the one of the issue"""
    from test_cov_host import yaw_of
    assert len(GRID_NAMES) == 17 and len(BATCHES) == 20
    cells = {(BATCHES[n]["c"], v["delta"]) for n in GRID_NAMES for v in BATCHES[n]["variants"]}
    assert cells == {(c, d) for c in C_GRID for d in DELTAS} | {(C_TINY, 1e-3), (C_TINY, 1e-6)} | {(c, 0.0) for c in C_NEVER}
    thr_degs = sorted(BATCHES[n]["thr_deg"] for n in GRID_NAMES if BATCHES[n]["via"] == "thr")
    assert 4.4e-3 < thr_degs[0] < 4.6e-3 and 1700 < thr_degs[-1] < 1800
    for N in LENGTHS:
        lens = {b - a for p in placements(N) for a, b in p["outs"][:1]}
        assert {1, 2, 3} <= lens and (lens >= {70, 130} if N == 200 else max(lens) == 56)
        t = make_batch("dt-0.0785", N)
        steep = 0
        for j, m in enumerate(t["meta"]):
            k, (a, b) = m["k"], m["outs"][0]
            y = np.array([yaw_of(q) for q in t["quat"][j]])
            d = np.diff(y); d = np.arctan2(np.sin(d), np.cos(d))
            want = np.deg2rad(THR_DEG) * (1 + m["s"] * m["delta"]) * (t["ts"][j, k] - t["ts"][j, k - 1])
            assert abs(abs(d[k - 1]) - want) < 1e-12, (N, j)
            gentle = np.delete(np.abs(d), [p - 1 for p in (k, a, b, 12) if 0 < p < N])
            assert gentle.max() < 0.06 * 0.0785, (N, j)                  # 2 deg/s elsewhere (only planted and burst pairs are taken out)
            steep += m["steep"]
        assert steep == 13                                               # every fifth slot: at 0.0785 even delta = 1e-9 keeps thr dt delta >= 1e-11


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_grid_case_is_decidable(orc, name):
    """The oracle decides every outage like the 50-digit truth, the planted pair lies on the planned side, and the 50-digit rate keeps
    delta / 2 from the threshold: the decidable set is the whole grid.  Corner rows: oracle == truth == the row's stated decision."""
    import mpmath as mp
    spec, thr = BATCHES[name], thr_rad(name)
    left_out = []
    for N in LENGTHS:
        t, tr = make_batch(name, N), truth(name, N)
        _, _, st = oracle_fused(orc, name, N)
        worst = None
        for j, (m, row) in enumerate(zip(t["meta"], tr)):
            for a, b, rec, sharp, rate in row["outs"]:
                o_sharp, o_rate = orc.is_sharp_turn_in_segment(t["quat"][j, a:b], t["ts"][j, a:b], thr, return_rate=True)
                if o_sharp != sharp:
                    left_out.append((N, j, cell_of(name, m), "oracle decides the other way"))
            if (int(st[j]) & 15) != row["status"]:
                left_out.append((N, j, cell_of(name, m), f"oracle status {int(st[j])}, truth {row['status']}"))
            a, b, rec, sharp, rate = sorted(row["outs"], key=lambda o: o[:2] != tuple(m["outs"][0]))[0]     # the planted outage
            if spec["kind"] == "corner":
                if sharp != CORNER_SHARP[m["row"]]:
                    left_out.append((N, j, m["row"], f"truth says sharp = {sharp}"))
                continue
            counted = (b - a >= 2) and a + 1 <= m["k"] <= b - 1
            planned = counted and m["s"] > 0 and spec["c"] < np.pi
            if sharp != planned:
                left_out.append((N, j, cell_of(name, m), f"planned sharp = {planned}, truth {sharp}"))
            if counted:
                with mp.workdps(50):
                    margin = float(abs(rate / mp.mpf(thr) - 1))
                    rel = float(abs(rate / mp.mpf(thr) - (1 + m["s"] * m["delta"])) / m["delta"]) if m["delta"] else 0.0
                worst = rel if worst is None else max(worst, rel)
                if not margin >= 0.5 * m["delta"]:
                    left_out.append((N, j, cell_of(name, m), f"|rate/thr - 1| = {margin:.3e}"))
        if worst is not None:
            print(f"{name} N={N}: the stored tracks realise the planted rate within {worst:.2e} of delta at worst")
    assert not left_out, (name, len(left_out), left_out[:8])


@pytest.mark.parametrize("name", list(BATCHES))
def test_gate_functions_equal_the_50_digit_decision(gate, name):
    """yaw_rate_exceeds and yaw_rate_exceeds_body (g++, libm) on every evaluated pair of every outage: the 50-digit decision"""
    thr = thr_rad(name)
    flips = {}
    n_pairs = 0
    for N in LENGTHS:
        t, tr = make_batch(name, N), truth(name, N)
        idx = [(j, k, ex) for j, row in enumerate(tr) for k, ex in row["pairs"]]
        if not idx:
            continue
        jj, kk = np.array([i[0] for i in idx]), np.array([i[1] for i in idx])
        q1, q2 = np.ascontiguousarray(t["quat"][jj, kk - 1]), np.ascontiguousarray(t["quat"][jj, kk])
        dt = np.ascontiguousarray(t["ts"][jj, kk] - t["ts"][jj, kk - 1])
        out = np.zeros(len(idx), np.uint8)
        gate.hh_yaw_gate(q1, q2, dt, np.full(len(idx), thr), len(idx), out)
        n_pairs += len(idx)
        for (j, k, ex), o in zip(idx, out):
            if ex is None:
                assert o & 4, (name, N, j, k)                            # the zero quaternion is reported, the callers count the pair as sharp
                continue
            for bit, fn in ((1, "yaw_rate_exceeds"), (2, "yaw_rate_exceeds_body")):
                if bool(o & bit) != ex:
                    c = (fn,) + cell_of(name, t["meta"][j]) + (("planted" if k == t["meta"][j]["k"] else "other"),)
                    flips[c] = flips.get(c, 0) + 1
    print(f"{name}: {n_pairs} pairs, flipped decisions by (function, thr dt, delta, pair): {flips or 'none'}")
    assert not flips, (name, flips)


@pytest.mark.parametrize("name", list(BATCHES))
def test_core_fuses_like_the_oracle(hh, orc, name):  # noqa: F811
    """EkfTraj (hh_ekf_fuse) on every track: the oracle's status word, its poses within the gates of tests/test_host_math.py"""
    cfg = batch_config(orc.DEFAULT_CONFIG, name)
    problems = []
    for N in LENGTHS:
        t = make_batch(name, N)
        po, qo, sto = oracle_fused(orc, name, N)
        bad, ep, eq = [], 0.0, 0.0
        for j in range(NB):
            p, q, st = _fuse(hh, t["ts"][j], t["pos"][j], t["quat"][j], t["gps"][j], t["valid"][j], t["init_pos"][j], t["init_quat"][j], cfg)
            if st != sto[j]:
                bad.append(j)
            else:
                ep, eq = max(ep, float(np.abs(p - po[j]).max())), max(eq, float(np.abs(q - qo[j]).max()))
        print(f"{name} N={N}: {len(bad)} status words differ {flips_table(name, N, bad) or ''}; tracks with equal status: max |dp| {ep:.2e} m, max |dq| {eq:.2e}")
        if bad:
            problems.append((N, "status words differ", flips_table(name, N, bad)))
        if not (ep < 2e-8 and eq < 1e-12):
            problems.append((N, f"max |dp| {ep:.3e}, max |dq| {eq:.3e}"))
    assert not problems, (name, problems)


def test_polynomial_sine_of_the_gate(gate):
    """gate_sin_poly against a 50-digit sine on 10 001 points of [0, 0.785] and at 0.785 +- 1 ulp.  Bound: 2 ulp of 1.0 absolute (what a
    correctly rounded minimax polynomial of this degree achieves on the interval with margin: its approximation error is below 2^-58, the
    rest is the rounding of the evaluation) -- and, since a sine is compared through its RELATIVE accuracy at small angles, 2 ulp of the
    value itself as well.  Measured: 0.69 ulp of the value at most, 7.7e-17 absolute (0.35 ulp of 1.0)."""
    import mpmath as mp
    c = np.concatenate([np.linspace(0.0, 0.785, 10001), [np.nextafter(0.785, 0.0), 0.785, np.nextafter(0.785, 1.0)]])
    s = np.empty_like(c)
    gate.hh_gate_sin_poly(c, len(c), s)
    with mp.workdps(50):
        err = np.array([float(abs(mp.mpf(float(v)) - mp.sin(mp.mpf(float(x))))) for x, v in zip(c, s)])
        ref = np.array([float(mp.sin(mp.mpf(float(x)))) for x in c])
    ulps = err / np.spacing(np.maximum(ref, np.finfo(float).tiny))
    print(f"gate_sin_poly: largest error {err.max():.3e} absolute = {err.max() / np.finfo(float).eps:.2f} ulp of 1.0; {ulps[1:].max():.2f} ulp of the value")
    assert s[0] == 0.0
    assert err.max() <= 2 * np.finfo(float).eps
    assert ulps[1:].max() <= 2.0
