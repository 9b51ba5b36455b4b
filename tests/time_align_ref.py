"""The yardstick of the time-alignment entries (gsf_time_align_batch[_dev], gsf_time_align_loaded_rows_batch_dev,
ekfgpsslam.dynamic_time_alignment) and the grid of logs both tiers run.  Never imports the product.

Values.  yardstick(): dynamic_time_alignment's values (EKFGPSSLAM.py:325-387) restated in 50-digit arithmetic (mpmath) and rounded once to
float64.  A segment of >= 4 knots is the not-a-knot cubic spline of scipy's interp1d(kind='cubic'), from its textbook system for the knot
second derivatives: interior rows h[i-1] M[i-1] + 2 (h[i-1] + h[i]) M[i] + h[i] M[i+1] = 6 (d[i] - d[i-1]), rows 0 and m-1 the
continuity of the third derivative at x[1] and x[m-2] -- the form tests/test_oracle_golden.py::test_alignment_exact_spline writes down, not
the folded rows of the kernel and the oracle.  solve_banded() eliminates that matrix in O(m); tests/test_time_align_host.py holds it to
mp.lu_solve of the dense matrix.  A segment of 2 or 3 knots follows scipy's _call_linear.

Decisions.  decisions(): lines :339-379 in float64 numpy -- the reference takes them in float64 as well, so float64 is their yardstick:
stable sort, first of equal stamps, split where diff > max_gap, a segment is usable iff it has >= 2 knots and every diff > 1e-9, a query
belongs to a segment iff t0 - 1e-9 <= t <= t1 + 1e-9, its value is NaN outside [t0, t1], later segments overwrite earlier ones.

Grid.  cases(): named logs {st, gt, gp, max_gap, qkind, ...} from a fixed seed on a smooth UTM-sized track, at most 200 knots and 450
queries each (the whole grid is one ragged launch per max_gap); see the family list at cases()."""
import numpy as np

DPS = 50
EPS = 1e-9                      # :364 and :372
SEED = 20250611
MAX_KNOTS, MAX_QUERIES = 200, 450

# kinds of query (case["qkind"])
Q_PLAIN, Q_KNOT, Q_END, Q_IN_EPS, Q_BEYOND_EPS = 0, 1, 2, 3, 4


def _mp():
    import mpmath
    return mpmath


# ---------------------------------------------------------------------------- decisions (:339-379), float64
def decisions(st, gt, max_gap):
    """-> dict: src (input index of every kept knot, in stamp order), knots (their stamps), segs [(first, last, usable)],
    owner (ns,) = index of the LAST usable segment that claims the query (-1: no segment writes the row),
    inside (ns,) = the owner evaluates it (False: it writes NaN)"""
    st, gt = np.asarray(st, dtype=np.float64).ravel(), np.asarray(gt, dtype=np.float64).ravel()
    ns, ng = len(st), len(gt)
    out = dict(src=np.zeros(0, np.int64), knots=np.zeros(0), segs=[], owner=np.full(ns, -1, np.int64), inside=np.zeros(ns, bool))
    if ns == 0 or ng < 2:                                                # :333
        return out
    with np.errstate(invalid="ignore"):
        order = np.argsort(gt, kind="stable")                            # :340 (NaN stamps last)
        ut, first = np.unique(gt[order], return_index=True)              # :342 (the first of equal stamps)
        if len(ut) < 2:                                                  # :344
            return out
        out["src"], out["knots"] = order[first], ut
        gaps = np.where(np.diff(ut) > max_gap)[0]                        # :351-352
        starts, ends = [0] + (gaps + 1).tolist(), gaps.tolist() + [len(ut) - 1]
        for k, (s, e) in enumerate(zip(starts, ends)):
            usable = e - s + 1 >= 2 and bool(np.all(np.diff(ut[s:e + 1]) > EPS))          # :361, :364
            out["segs"].append((s, e, usable))
            if not usable:
                continue
            t0, t1 = ut[s], ut[e]
            claim = (st >= t0 - EPS) & (st <= t1 + EPS)                  # :373
            out["owner"][claim] = k                                      # :376 (a later segment overwrites)
            out["inside"][claim] = (st[claim] >= t0) & (st[claim] <= t1)  # interp1d(bounds_error=False, fill_value=nan)
    return out


# ---------------------------------------------------------------------------- values, 50 digits
def textbook_rows(x, y):
    """the not-a-knot system of one component in its textbook form: rows [{column: coefficient}], right-hand side; x, y lists of mpf"""
    m = len(x)
    h = [x[i + 1] - x[i] for i in range(m - 1)]
    rows, rhs = [None] * m, [0] * m
    for i in range(1, m - 1):
        rows[i] = {i - 1: h[i - 1], i: 2 * (h[i - 1] + h[i]), i + 1: h[i]}
        rhs[i] = 6 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
    rows[0] = {0: 1 / h[0], 1: -(1 / h[0] + 1 / h[1]), 2: 1 / h[1]}
    last = {m - 3: 1 / h[m - 3], m - 2: -(1 / h[m - 3] + 1 / h[m - 2]), m - 1: 1 / h[m - 2]}
    rows[m - 1] = last
    return rows, rhs


def solve_banded(rows, rhs):
    """Gaussian elimination of a matrix whose rows reach at most two columns below the diagonal (the textbook rows do), without pivoting:
    O(m).  The pivots are those of the diagonally dominant folded system, none is zero for increasing knots."""
    m = len(rows)
    rows, rhs = [dict(r) for r in rows], list(rhs)
    for k in range(m):
        piv = rows[k][k]
        for i in range(k + 1, min(k + 3, m)):
            f = rows[i].pop(k, None)
            if f is None:
                continue
            f = f / piv
            for j, v in rows[k].items():
                if j > k:
                    rows[i][j] = rows[i].get(j, 0) - f * v
            rhs[i] = rhs[i] - f * rhs[k]
    M = [0] * m
    for i in range(m - 1, -1, -1):
        acc = rhs[i]
        for j, v in rows[i].items():
            if j > i:
                acc = acc - v * M[j]
        M[i] = acc / rows[i][i]
    return M


def solve_dense(rows, rhs_list):
    """the same system as a dense matrix through the steps of mp.lu_solve (LU_decomp with partial pivoting, L_solve, U_solve), the
    factorisation shared by the right-hand sides (the check of solve_banded; O(m^3))"""
    mp = _mp()
    m = len(rows)
    A = mp.zeros(m, m)
    for i, row in enumerate(rows):
        for j, v in row.items():
            A[i, j] = v
    LU, p = mp.mp.LU_decomp(A)
    out = []
    for rhs in rhs_list:
        M = mp.mp.U_solve(LU, mp.mp.L_solve(LU, mp.matrix(rhs), p))
        out.append([M[i] for i in range(m)])
    return out


def segment_values_mp(x, y, tq, solve=solve_banded):
    """one usable segment at the stamps tq inside [x[0], x[-1]]: [[mpf] * ncomp] per query, not rounded.  x: floats (or mpf) increasing,
    y: (m, ncomp) floats or mpf.  Must run under mp.workdps(DPS)."""
    mp = _mp()
    m, nc = len(x), len(y[0])
    xm = [mp.mpf(v) for v in x]
    ym = [[mp.mpf(y[i][c]) for i in range(m)] for c in range(nc)]
    xf = np.array([float(v) for v in x])
    out = []
    if m >= 4:                                                           # :362 cubic
        Ms = []
        for c in range(nc):
            rows, rhs = textbook_rows(xm, ym[c])
            Ms.append(solve(rows, rhs))
        for t in tq:
            lo = int(np.clip(np.searchsorted(xf, float(t), "right") - 1, 0, m - 2))
            tm = mp.mpf(t)
            h = xm[lo + 1] - xm[lo]
            a, b = (xm[lo + 1] - tm) / h, (tm - xm[lo]) / h
            ca, cb = (a ** 3 - a) * h * h / 6, (b ** 3 - b) * h * h / 6
            out.append([a * ym[c][lo] + b * ym[c][lo + 1] + ca * Ms[c][lo] + cb * Ms[c][lo + 1] for c in range(nc)])
    else:                                                                # scipy _call_linear
        for t in tq:
            hi = int(np.clip(np.searchsorted(xf, float(t), "left"), 1, m - 1))
            lo = hi - 1
            tm = mp.mpf(t)
            out.append([(ym[c][hi] - ym[c][lo]) / (xm[hi] - xm[lo]) * (tm - xm[lo]) + ym[c][lo] for c in range(nc)])
    return out


def yardstick(st, gt, gp, max_gap, dec=None, solve=solve_banded):
    """-> aligned (ns, 3) float64 (NaN where no value is defined), valid (ns,) bool"""
    mp = _mp()
    st, gt = np.asarray(st, dtype=np.float64).ravel(), np.asarray(gt, dtype=np.float64).ravel()
    gp = np.asarray(gp, dtype=np.float64).reshape(-1, 3)
    dec = dec or decisions(st, gt, max_gap)
    al = np.full((len(st), 3), np.nan)
    with mp.workdps(DPS):
        for k, (s, e, usable) in enumerate(dec["segs"]):
            rows = np.where((dec["owner"] == k) & dec["inside"])[0]
            if not usable or len(rows) == 0:
                continue
            vals = segment_values_mp(dec["knots"][s:e + 1], gp[dec["src"][s:e + 1]], st[rows], solve)
            al[rows] = [[float(v) for v in row] for row in vals]
    return al, np.isfinite(al).all(axis=1)                               # :377-379


# ---------------------------------------------------------------------------- the grid
def track(t):
    """the smooth UTM-sized track, t in seconds"""
    t = np.asarray(t, dtype=np.float64)
    return np.column_stack((4.5e5 + 50.0 * np.sin(t), 5.4e6 + 13.0 * t, 100.0 + np.cos(t / 3.0)))


def _stamps(h, t0=0.0):
    return np.concatenate(([t0], t0 + np.cumsum(h)))


def _queries(rng, gt, max_gap, unit, n_uniform=300):
    """the queries of one log: n_uniform uniform inside the span, every 7th knot, and per segment t0, t1, t0 - 5e-10, t1 + 5e-10, the
    neighbours of t0 - 1e-9 and t1 + 1e-9 on the far side, the middle of every gap, two stamps outside the log.  Plain queries closer
    than 1e-5 (stamp units) to a segment end are left out."""
    dec = decisions(np.zeros(1), gt, max_gap)
    ut = dec["knots"][np.isfinite(dec["knots"])]
    ends = np.array([ut[min(k, len(ut) - 1)] for s, e, _ in dec["segs"] for k in (s, e)])
    plain = [rng.uniform(ut[0], ut[-1], n_uniform), [ut[0] - 2.5 * unit, ut[-1] + 2.5 * unit]]
    plain.append([0.5 * (ut[e] + ut[e + 1]) for s, e, _ in dec["segs"] if e + 1 < len(ut)])
    plain = np.concatenate([np.asarray(p, dtype=np.float64) for p in plain])
    plain = plain[np.min(np.abs(plain[:, None] - ends[None, :]), axis=1) > 1e-5 * unit]
    q, kind = [plain], [np.full(len(plain), Q_PLAIN)]
    q.append(ut[::7]); kind.append(np.full(len(ut[::7]), Q_KNOT))
    for s, e, _ in dec["segs"]:
        t0, t1 = ut[min(s, len(ut) - 1)], ut[min(e, len(ut) - 1)]
        q.append([t0, t1, t0 - 5e-10, t1 + 5e-10, np.nextafter(t0 - EPS, -np.inf), np.nextafter(t1 + EPS, np.inf)])
        kind.append([Q_END, Q_END, Q_IN_EPS, Q_IN_EPS, Q_BEYOND_EPS, Q_BEYOND_EPS])
    q, kind = np.concatenate([np.asarray(v, dtype=np.float64) for v in q]), np.concatenate([np.asarray(v) for v in kind])
    o = np.argsort(q, kind="stable")
    return np.ascontiguousarray(q[o]), kind[o].astype(np.int64)


def _case(rng, tb, max_gap=5.0, scale=1.0, shift=0.0, noise=False, n_uniform=300, family=""):
    """base stamps tb (seconds) -> a log with stamps tb * scale + shift, the track's positions at tb"""
    tb = np.asarray(tb, dtype=np.float64)
    gp = track(tb)
    if noise:
        assert np.all(np.diff(tb) >= 0.04 - 1e-12), family               # noise and the spike only where every h >= 0.04 s
        gp = gp + rng.normal(0.0, 0.3, gp.shape)
        gp[int(rng.integers(1, len(tb) - 1)) if len(tb) > 2 else 0, 0] += 50.0
    gt = tb * scale + shift
    st, kind = _queries(rng, gt, max_gap * scale, scale, n_uniform)
    return dict(st=st, gt=np.ascontiguousarray(gt), gp=np.ascontiguousarray(gp), max_gap=float(max_gap * scale), qkind=kind, family=family,
                planted=False, unit=float(scale))


def _shuffled(rng, c, ndup=10):
    """the same log with ndup fixes logged twice (identical positions), in random order"""
    pick = rng.choice(len(c["gt"]), ndup, replace=False)
    gt, gp = np.r_[c["gt"], c["gt"][pick]], np.r_[c["gp"], c["gp"][pick]]
    perm = rng.permutation(len(gt))
    return dict(c, gt=np.ascontiguousarray(gt[perm]), gp=np.ascontiguousarray(gp[perm]), family="order")


KNOT_COUNTS = (2, 3, 4, 5, 6, 65, 66, 67, 130, 131, 200)
MULTI_SEGMENTS = (67, 4, 1, 30, 3, 2, 50)                                # knots per segment of "multi_seg"
SHUFFLED = {"shuffled_multi_seg": "multi_seg", "shuffled_logu3": "sp_logu3", "shuffled_m67": "knots_m67"}
HOST_ENTRY = ("sp_logu6", "sp_ends_4_1e-3", "sp_tail_1e-4_4", "epoch_jitter", "multi_seg")

_cases = None


def cases():
    """name -> case, built once.  Families:
    knots   knots_m<m>, m in KNOT_COUNTS, sorted-uniform stamps: 2 / 3 knots (linear), kk = m - 2 in {2, 3, 4} (both folded rows touch),
            {63, 64, 65, 128, 129, 198} (the edges of one and two 64-row scan chunks);
    multi   multi_seg: segments of MULTI_SEGMENTS knots 8 s apart (the 1-knot one is skipped, the 4-knot one follows the 67-knot one; no
            segment but the first starts at a multiple of 64);
    spacing m = 200: uniform 1 Hz, sorted-uniform, 10 Hz +- 0.03 s, log-uniform h in 1e-3..4.9 and 1e-6..4.9 (1e-6 next to 4.9 planted),
            alternating 1e-3 / 1 s, first intervals (4, 1e-3) and (1e-3, 4), last intervals (1e-4, 4);
    epoch   uniform and jitter with 1.7e9 s added;     units: jitter in milli- and microseconds (stamps and max_gap x 1e3, x 1e6);
    ns      0, 1, 63, 64, 65 queries;
    planted a gap of exactly max_gap and one of nextafter(max_gap); increments of exactly 1e-9 (stamps 0 and 1e-9) and of 2e-9;
    order   three logs shuffled with ten fixes logged twice; a NaN stamp appended; a fix logged twice (different positions) whose stamp
            starts a segment."""
    global _cases
    if _cases is not None:
        return _cases
    rng = np.random.default_rng(SEED)
    g = {}
    for m in KNOT_COUNTS:
        g[f"knots_m{m}"] = _case(rng, np.sort(rng.uniform(0.0, 0.5 * m, m)), family="knots")
    # several segments in one log: 1 Hz +- 0.2 s inside a segment, 8 s between segments
    tb, t = [], 0.0
    for n in MULTI_SEGMENTS:
        seg = t + np.arange(n) + rng.uniform(-0.2, 0.2, n)
        tb.append(seg); t = seg[-1] + 8.0
    g["multi_seg"] = _case(rng, np.concatenate(tb), noise=True, family="multi")
    # spacing, m = 200
    m = MAX_KNOTS
    jitter = lambda: np.arange(m) * 0.1 + rng.uniform(-0.03, 0.03, m)
    g["sp_uniform"] = _case(rng, np.arange(m) * 1.0, noise=True, family="spacing")
    g["sp_sorted_uniform"] = _case(rng, np.sort(rng.uniform(0.0, 100.0, m)), family="spacing")
    g["sp_jitter"] = _case(rng, jitter(), noise=True, family="spacing")
    g["sp_logu3"] = _case(rng, _stamps(np.exp(rng.uniform(np.log(1e-3), np.log(4.9), m - 1))), family="spacing")
    h = np.exp(rng.uniform(np.log(1e-6), np.log(4.9), m - 1)); h[50], h[51], h[120], h[121] = 1e-6, 4.9, 4.9, 1e-6
    g["sp_logu6"] = _case(rng, _stamps(h), family="spacing")
    g["sp_alternating"] = _case(rng, _stamps(np.where(np.arange(m - 1) % 2 == 0, 1e-3, 1.0)), family="spacing")
    h = np.ones(m - 1); h[0], h[1] = 4.0, 1e-3
    g["sp_ends_4_1e-3"] = _case(rng, _stamps(h), family="spacing")
    h = np.ones(m - 1); h[0], h[1] = 1e-3, 4.0
    g["sp_ends_1e-3_4"] = _case(rng, _stamps(h), family="spacing")
    h = np.ones(m - 1); h[-2], h[-1] = 1e-4, 4.0
    g["sp_tail_1e-4_4"] = _case(rng, _stamps(h), family="spacing")
    g["epoch_uniform"] = _case(rng, np.arange(m) * 1.0, shift=1.7e9, noise=True, family="epoch")
    g["epoch_jitter"] = _case(rng, jitter(), shift=1.7e9, noise=True, family="epoch")
    g["units_ms"] = _case(rng, jitter(), scale=1e3, noise=True, family="units")
    g["units_us"] = _case(rng, jitter(), scale=1e6, noise=True, family="units")
    for ns in (0, 1, 63, 64, 65):
        c = _case(rng, np.arange(67) * 1.0, noise=True, family="ns")
        keep = np.where(c["qkind"] == Q_PLAIN)[0][1:-1][:ns]             # (not the two stamps outside the log)
        c["st"], c["qkind"] = np.ascontiguousarray(c["st"][keep]), c["qkind"][keep]
        g[f"ns{ns}"] = c
    # planted decisions: dyadic and small-integer stamps, every difference exact
    up = float(np.nextafter(5.0, np.inf))
    tb = np.r_[np.arange(-12.0, -7.0), np.arange(-3.0, 1.0), up + 0.5 * np.arange(5)]     # -8 -> -3: exactly 5; 0 -> up: the next double
    g["planted_gap"] = dict(_case(rng, tb, family="planted"), planted=True)
    assert tb[5] - tb[4] == 5.0 and tb[9] - tb[8] == up and np.all(np.diff(tb[9:]) == 0.5)
    tb = np.r_[np.arange(-3.0, 1.0), 1e-9, np.arange(1.0, 4.0), np.arange(20.0, 27.0)]    # the first segment is not usable, the second is
    g["planted_inc_1e-9"] = dict(_case(rng, tb, family="planted"), planted=True)
    tb = np.r_[np.arange(-3.0, 1.0), 2e-9, np.arange(1.0, 4.0)]
    g["planted_inc_2e-9"] = dict(_case(rng, tb, family="planted"), planted=True)
    # order
    for name, of in SHUFFLED.items():
        g[name] = _shuffled(rng, g[of])
    c = g["multi_seg"]
    g["nan_stamp"] = dict(c, gt=np.r_[c["gt"], np.nan], gp=np.r_[c["gp"], track([1.0])], family="order")
    # a fix logged twice, with two positions, whose stamp starts the segment after a gap: the first one in input order is the knot
    tb = np.r_[np.arange(0.0, 10.0), 16.0, 16.0, np.arange(17.0, 30.0)]
    c = _case(rng, tb, family="order")
    c["gp"][11] += [3.0, -2.0, 1.0]
    perm = rng.permutation(len(tb))
    g["dup_split"] = dict(c, gt=np.ascontiguousarray(c["gt"][perm]), gp=np.ascontiguousarray(c["gp"][perm]))
    for name, c in g.items():
        assert len(c["gt"]) <= MAX_KNOTS + 10 and len(c["st"]) <= MAX_QUERIES, name
        for k in ("st", "gt", "gp", "qkind"):
            c[k].setflags(write=False)
    _cases = g
    return g


_truth = {}


def truth(name):
    """decisions and yardstick of a grid case: once, read-only.  A shuffled copy shares its original's."""
    name = SHUFFLED.get(name, name)
    if name not in _truth:
        c = cases()[name]
        dec = decisions(c["st"], c["gt"], c["max_gap"])
        al, va = yardstick(c["st"], c["gt"], c["gp"], c["max_gap"], dec)
        al.setflags(write=False); va.setflags(write=False)
        on_knot = np.isin(c["st"], dec["knots"]) & va
        S = float(np.max(np.abs(al[va]))) if va.any() else 0.0
        S3 = np.max(np.abs(al[va]), axis=0) if va.any() else np.zeros(3)                    # per component: easting, northing, altitude
        _truth[name] = dict(dec=dec, aligned=al, valid=va, on_knot=on_knot, S=S, ulp=float(np.spacing(S)) if S > 0 else 0.0,
                            S3=S3, ulp3=np.where(S3 > 0, np.spacing(S3), 0.0))
    return _truth[name]


def ragged(names, key_gt="gt", key_gp="gp"):
    """the cases as one ragged batch: st, slam offsets, gt, gp, gps offsets"""
    g = cases()
    so = np.zeros(len(names) + 1, np.int64); go = np.zeros(len(names) + 1, np.int64)
    so[1:] = np.cumsum([len(g[n]["st"]) for n in names]); go[1:] = np.cumsum([len(g[n][key_gt]) for n in names])
    cat = lambda k, shape: np.ascontiguousarray(np.concatenate([np.asarray(g[n][k], dtype=np.float64).reshape(shape) for n in names]))
    return cat("st", (-1,)), so, cat(key_gt, (-1,)), cat(key_gp, (-1, 3)), go
