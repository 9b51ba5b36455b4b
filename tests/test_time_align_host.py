"""CPU tier of the time-alignment tests: the yardstick of tests/time_align_ref.py held to the definition (the dense textbook system, cubic
data reproduced, knots interpolated), the grid held to what it claims and to decidability, and the oracle's dynamic_time_alignment held to
both -- its decisions exactly, its values within 4 ulp of the largest value of the case.  oracle_error() is the per-case figure the GPU
tier (tests/test_time_align.py) builds its tolerance from."""
import mpmath as mp
import numpy as np
import pytest

import time_align_ref as ref

NAMES = list(ref.cases())


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


_e_orc = {}


def oracle_error(orc, name):
    """e_orc(case) = max |oracle - yardstick| over the valid rows; the oracle's decisions are asserted on the way.  Once per case."""
    name = ref.SHUFFLED.get(name, name)
    if name not in _e_orc:
        c, t = ref.cases()[name], ref.truth(name)
        al, va = orc.dynamic_time_alignment(c["st"], c["gt"], c["gp"], 500, c["max_gap"])
        np.testing.assert_array_equal(va, t["valid"], err_msg=name)
        np.testing.assert_array_equal(np.isnan(al), np.isnan(t["aligned"]), err_msg=name)
        _e_orc[name] = np.max(np.abs(al[va] - t["aligned"][va]), axis=0, initial=0.0)      # per component
        _e_orc[name].setflags(write=False)
    return float(_e_orc[name].max())


def tolerance(orc, name):
    """tol(case) = 4 max(ulp(S), e_orc(case)), S the largest |yardstick value| of the case"""
    return 4.0 * max(ref.truth(name)["ulp"], oracle_error(orc, name))


def usable_segments(name):
    c, d = ref.cases()[name], ref.truth(name)["dec"]
    return [(d["knots"][s:e + 1], c["gp"][d["src"][s:e + 1]]) for s, e, usable in d["segs"] if usable]


# ---------------------------------------------------------------------------- the yardstick
def test_banded_solve_equals_dense_lu():
    """solve_banded == the dense LU solve (mp.lu_solve's steps) of the textbook matrix to 1e-40 relative, on every cubic segment of the
    grid with m <= 67 (the ns family and the shuffled copies repeat the knots of others and are left out)"""
    n = 0
    with mp.workdps(ref.DPS):
        for name in NAMES:
            if ref.cases()[name]["family"] == "ns" or name in ref.SHUFFLED or name == "nan_stamp":
                continue
            for x, y in usable_segments(name):
                if not 4 <= len(x) <= 67:
                    continue
                xm = [mp.mpf(float(v)) for v in x]
                systems = [ref.textbook_rows(xm, [mp.mpf(float(v)) for v in y[:, c]]) for c in range(3)]
                dense = ref.solve_dense(systems[0][0], [rhs for _, rhs in systems])
                for c, (rows, rhs) in enumerate(systems):
                    Mb, Md = ref.solve_banded(rows, rhs), dense[c]
                    scale = max(abs(v) for v in Md)                      # (0 for the straight northing on exact stamps: then both are 0)
                    assert max(abs(a - b) for a, b in zip(Mb, Md)) <= mp.mpf("1e-40") * scale, (name, len(x), c)
                n += 1
    assert n >= 12                                                       # m = 4, 5, 6, 65, 66, 67, the segments of multi_seg, the planted logs


@pytest.mark.parametrize("name", ["knots_m4", "knots_m5", "knots_m67", "sp_logu6", "sp_ends_4_1e-3", "sp_tail_1e-4_4", "epoch_jitter"])
def test_cubic_data_is_reproduced(name):
    """Independent of any row algebra: the not-a-knot spline through samples of a cubic IS that cubic.  Knots of a grid case, values of
    three cubics with integer coefficients taken exactly (mpf) at the knots: every query inside the segment gives the cubic to 1e-40."""
    c = ref.cases()[name]
    x = usable_segments(name)[0][0]
    tq = c["st"][(c["st"] >= x[0]) & (c["st"] <= x[-1])]
    assert len(tq) >= 300
    with mp.workdps(ref.DPS):
        x0 = mp.mpf(float(x[0]))
        polys = [lambda u: 3 * u ** 3 - 7 * u ** 2 + 11 * u + 5400000, lambda u: -u ** 3 + 450000, lambda u: 2 * u ** 3 + u ** 2 - 13 * u + 100]
        y = [[p(mp.mpf(float(v)) - x0) for p in polys] for v in x]
        got = ref.segment_values_mp(x, y, tq)
        for t, row in zip(tq, got):
            for p, v in zip(polys, row):
                want = p(mp.mpf(float(t)) - x0)
                assert abs(v - want) <= mp.mpf("1e-40") * max(1, abs(want)), (name, t)


def test_a_query_on_a_knot_returns_the_knot():
    n = 0
    for name in NAMES:
        if name in ref.SHUFFLED:                                         # (the values of its original)
            continue
        c, t = ref.cases()[name], ref.truth(name)
        d = t["dec"]
        rows = np.where(t["on_knot"])[0]
        for i in rows:
            k = int(np.where(d["knots"] == c["st"][i])[0][0])
            np.testing.assert_array_equal(t["aligned"][i], c["gp"][d["src"][k]], err_msg=f"{name} query {i}")
        n += len(rows)
    assert n >= 400


# ---------------------------------------------------------------------------- the grid
def test_every_case_is_decidable():
    """apart from the planted rows no query lies within 1e-6 (stamp units) of a segment end, no gap within 1e-6 of max_gap, and no
    increment within 1e-12 of the 1e-9 a usable segment needs"""
    for name in NAMES:
        c = ref.cases()[name]
        d = ref.decisions(np.zeros(1), c["gt"], c["max_gap"])           # (the knots and segments do not depend on the queries)
        knots = d["knots"][np.isfinite(d["knots"])]
        ends = np.array([knots[min(k, len(knots) - 1)] for s, e, _ in d["segs"] for k in (s, e)])
        plain = c["st"][c["qkind"] == ref.Q_PLAIN]
        if len(plain) and len(ends):
            assert np.min(np.abs(plain[:, None] - ends[None, :])) > 1e-6 * c["unit"], name
        assert np.isin(c["st"][c["qkind"] == ref.Q_KNOT], knots).all(), name
        if not c["planted"]:
            assert np.min(np.abs(np.diff(knots) - c["max_gap"])) > 1e-6 * c["unit"], name
            assert np.min(np.abs(np.diff(knots) - ref.EPS)) > 1e-12, name


def test_the_grid_contains_what_it_claims():
    g = ref.cases()
    assert all(len(c["gt"]) <= ref.MAX_KNOTS + 10 and len(c["st"]) <= ref.MAX_QUERIES for c in g.values())
    segs = {name: ref.truth(name)["dec"]["segs"] for name in NAMES}
    # knot counts: one usable segment of m knots each; kk = m - 2 at the edges of the scan chunks
    for m in ref.KNOT_COUNTS:
        assert segs[f"knots_m{m}"] == [(0, m - 1, True)]
    kk = {e - s - 1 for v in segs.values() for s, e, usable in v if usable and e - s + 1 >= 4}
    assert {2, 3, 4, 63, 64, 65, 128, 129, 198} <= kk
    # several segments: the knot counts, the skipped one, none but the first at a multiple of 64
    ms = segs["multi_seg"]
    assert tuple(e - s + 1 for s, e, _ in ms) == ref.MULTI_SEGMENTS and [u for _, _, u in ms] == [n >= 2 for n in ref.MULTI_SEGMENTS]
    assert all(s % 64 != 0 for s, _, _ in ms[1:]) and (ms[0][1] - ms[0][0] + 1, ms[1][1] - ms[1][0] + 1) == (67, 4)
    # spacing: one segment of 200 knots each, with the intervals of the name
    h = {name: np.diff(g[name]["gt"]) for name in NAMES if g[name]["family"] in ("spacing", "epoch", "units")}
    assert len(h) == 13 and all(segs[name] == [(0, 199, True)] for name in h)
    for name in ("sp_logu3", "sp_logu6"):
        lo = 1e-3 if name == "sp_logu3" else 1e-6
        assert h[name].min() >= lo * (1 - 1e-6) and h[name].max() <= 4.9 * (1 + 1e-6) and h[name].max() / h[name].min() >= 1e3
    r = h["sp_logu6"][1:] / h["sp_logu6"][:-1]
    assert h["sp_logu6"].max() / h["sp_logu6"].min() >= 1e6 and r.max() >= 1e6 and r.min() <= 1e-6
    assert np.allclose(h["sp_alternating"][:4], [1e-3, 1.0, 1e-3, 1.0], rtol=1e-9)
    assert np.allclose(h["sp_ends_4_1e-3"][:3], [4.0, 1e-3, 1.0], rtol=1e-9) and np.allclose(h["sp_ends_1e-3_4"][:3], [1e-3, 4.0, 1.0], rtol=1e-9)
    assert np.allclose(h["sp_tail_1e-4_4"][-3:], [1.0, 1e-4, 4.0], rtol=1e-6)
    assert g["epoch_uniform"]["gt"].min() >= 1.7e9 and g["epoch_jitter"]["st"].min() >= 1.7e9 - 3
    assert g["units_ms"]["max_gap"] == 5e3 and g["units_us"]["max_gap"] == 5e6 and np.median(h["units_us"]) > 5e4
    assert all(h[name].min() >= 0.04 * g[name]["unit"] * (1 - 1e-6) for name in ("sp_jitter", "epoch_jitter", "units_ms", "units_us"))
    # queries
    assert {len(g[f"ns{n}"]["st"]) for n in (0, 1, 63, 64, 65)} == {0, 1, 63, 64, 65}
    for name in NAMES:
        if g[name]["family"] == "ns":
            continue
        c, t = g[name], ref.truth(name)
        d, k = t["dec"], c["qkind"]
        inside = (d["owner"] >= 0) & d["inside"]
        assert (k == ref.Q_PLAIN).sum() >= 295 and (inside & (k == ref.Q_PLAIN)).sum() >= 50 and (k == ref.Q_KNOT).sum() == -(-np.isfinite(d["knots"]).sum() // 7), name
        assert ((d["owner"] < 0) & (k == ref.Q_PLAIN)).sum() >= 2, name      # outside the log (and in its gaps)
        assert (k == ref.Q_END).sum() == 2 * len(d["segs"]), name
        if c["unit"] == 1.0 and c["gt"][0] < 1e6:                        # (5e-10 is below the spacing of epoch- and microsecond-sized stamps)
            usable = sum(u for _, _, u in d["segs"])
            assert ((d["owner"] >= 0) & ~d["inside"] & (k == ref.Q_IN_EPS)).sum() >= 2 * usable - 1, name       # written as NaN
            assert ((d["owner"] < 0) & (k == ref.Q_BEYOND_EPS)).sum() >= 2, name                                   # untouched
    # planted decisions
    d = ref.truth("planted_gap")["dec"]
    kn = d["knots"]
    assert [(s, e) for s, e, _ in d["segs"]] == [(0, 8), (9, 13)] and kn[5] - kn[4] == 5.0 and kn[9] - kn[8] == np.nextafter(5.0, np.inf)
    d = ref.truth("planted_inc_1e-9")["dec"]
    assert d["segs"] == [(0, 7, False), (8, 14, True)] and d["knots"][3] == 0.0 and d["knots"][4] == 1e-9
    assert not ref.truth("planted_inc_1e-9")["valid"][g["planted_inc_1e-9"]["st"] < 10].any()
    d = ref.truth("planted_inc_2e-9")["dec"]
    assert d["segs"] == [(0, 7, True)] and d["knots"][4] - d["knots"][3] == 2e-9
    # order: both routes (a log in order skips the rank sort, a shuffled one takes it), ten fixes logged twice
    for name, of in ref.SHUFFLED.items():
        a, b = g[name], g[of]
        assert np.all(np.diff(b["gt"]) > 0) and not np.all(np.diff(a["gt"]) > 0) and len(a["gt"]) == len(b["gt"]) + 10
        assert a["st"] is b["st"] and len(np.unique(a["gt"])) == len(b["gt"])
        da, db = ref.decisions(a["st"], a["gt"], a["max_gap"]), ref.truth(of)["dec"]
        np.testing.assert_array_equal(a["gp"][da["src"]], b["gp"][db["src"]])
        assert da["segs"] == db["segs"] and (da["owner"] == db["owner"]).all()
    d = ref.truth("nan_stamp")["dec"]
    assert np.isnan(g["nan_stamp"]["gt"][-1]) and [u for _, _, u in d["segs"]] == [n >= 2 for n in ref.MULTI_SEGMENTS[:-1]] + [False]
    assert ref.truth("nan_stamp")["valid"].sum() > 150
    c, d = g["dup_split"], ref.truth("dup_split")["dec"]
    first, second = np.where(c["gt"] == 16.0)[0]
    assert d["segs"] == [(0, 9, True), (10, 23, True)] and d["knots"][10] == 16.0 and d["src"][10] == first
    assert not np.array_equal(c["gp"][first], c["gp"][second]) and not np.all(np.diff(c["gt"]) > 0)


# ---------------------------------------------------------------------------- the oracle
def test_oracle_decides_like_the_reference_and_stays_within_4_ulp(orc):
    """valid and the NaN pattern identical on every case (oracle_error asserts them); e_orc <= 4 ulp(S).  Measured: at most 2 ulp
    (1.9e-9 m) on every family."""
    problems = []
    for name in NAMES:
        e, ulp = oracle_error(orc, name), ref.truth(name)["ulp"]
        with np.errstate(invalid="ignore", divide="ignore"):
            per = np.nan_to_num(_e_orc[ref.SHUFFLED.get(name, name)] / ref.truth(name)["ulp3"])
        print(f"{name}: e_orc {e:.2e} m = {e / ulp if ulp else 0.0:.1f} ulp(S); per component {per[0]:.1f}, {per[1]:.1f}, {per[2]:.1f} ulp(S_c)")
        if not e <= 4 * ulp:
            problems.append((name, e, ulp))
    assert not problems, problems
