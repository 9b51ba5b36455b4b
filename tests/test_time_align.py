"""GPU tier of the time-alignment tests: time_align_kernel (gsf_align.hip) against the 50-digit not-a-knot yardstick and the float64
decisions of tests/time_align_ref.py, on its grid -- knot counts at the edges of the 64-row scan chunks, several segments per log, interval
ratios up to 4.9e6, uneven ends, epoch-sized and milli-/microsecond stamps, decisions planted on their thresholds, shuffled logs.

Gates.  status 0; valid and the NaN pattern exact; a query on a knot returns the knot's position bit for bit; every other valid value within
tol(case) = 4 max(ulp(S), e_orc(case)) of the yardstick, S = the largest |value| of the case, e_orc = what the oracle's float64 Thomas
sweep deviates from the yardstick on the same case (tests/test_time_align_host.py; never anything the kernel returns).  The kernel differs
from the sweep in the order of association (tree scans), in 1/x being good to 1 ulp instead of correctly rounded, and in fused
multiply-adds: all of them rounding, none of them conditioning -- hence a small multiple of the sweep's own error, and 4 ulp at the least.

The grid is one ragged launch per max_gap (the threshold is an argument of the launch: seconds, milliseconds, microseconds)."""
import ctypes as C

import numpy as np
import pytest

import time_align_ref as ref
from test_time_align_host import oracle_error, tolerance

pytestmark = pytest.mark.gpu

NAMES = list(ref.cases())
FAMILIES = ("knots", "multi", "spacing", "epoch", "units", "ns", "planted", "order")


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def E():
    from gps_optimize_slam_amd import ekfgpsslam
    return ekfgpsslam


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def masked_log(name):
    """the log with fixes added whose easting and northing are NaN (the loader's mark): 5 % at random places, one as the first fix, one
    as the last, and three at rows 63, 64, 65.  Their stamps would change every segment if they reached the spline."""
    c = ref.cases()[name]
    rng = np.random.default_rng([ref.SEED, NAMES.index(name)])
    gt, gp = np.array(c["gt"]), np.array(c["gp"])
    lo, hi = np.nanmin(gt), np.nanmax(gt)

    def insert(gt, gp, at, stamps):
        rows = np.column_stack((np.full(len(stamps), np.nan), np.full(len(stamps), np.nan), np.full(len(stamps), 123.0)))
        return np.insert(gt, at, stamps), np.insert(gp, at, rows, axis=0)
    k = max(1, len(gt) // 20)
    gt, gp = insert(gt, gp, np.sort(rng.integers(0, len(gt) + 1, k)), rng.uniform(lo, hi, k))
    gt, gp = insert(gt, gp, [0], [lo - 100.0 * c["unit"]])
    gt, gp = insert(gt, gp, [len(gt)], [hi + 1e-3 * c["unit"]])
    if len(gt) > 66:
        gt, gp = insert(gt, gp, [63, 63, 63], rng.uniform(lo, hi, 3))
        assert np.isnan(gp[63:66, :2]).all()
    assert np.isnan(gp[0, 0]) and np.isnan(gp[-1, 1]) and np.isnan(gp[:, 0]).sum() >= k + 2
    return np.ascontiguousarray(gt), np.ascontiguousarray(gp)


_runs = {}


def run_grid(B, route):
    """the whole grid through one entry: name -> (aligned (ns, 3), valid (ns,) uint8, status).  route: "lds" (max_gps_per_trajectory =
    512), "slab" (2561: the global-scratch instantiation), "masked" (gsf_time_align_loaded_rows_batch_dev on masked_log()).  Once."""
    if route in _runs:
        return _runs[route]
    import torch
    from gps_optimize_slam_amd import _lib
    g = ref.cases()
    L, h = _lib.load(), B.context().handle
    entry = L.gsf_time_align_loaded_rows_batch_dev if route == "masked" else L.gsf_time_align_batch_dev
    max_g = 2561 if route == "slab" else 512
    logs = {name: masked_log(name) if route == "masked" else (g[name]["gt"], g[name]["gp"]) for name in NAMES}
    out = {}
    for gap in sorted({g[name]["max_gap"] for name in NAMES}):
        names = [name for name in NAMES if g[name]["max_gap"] == gap]
        so = np.zeros(len(names) + 1, np.int64); so[1:] = np.cumsum([len(g[n]["st"]) for n in names])
        go = np.zeros(len(names) + 1, np.int64); go[1:] = np.cumsum([len(logs[n][0]) for n in names])
        assert max(np.diff(go)) <= 512
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        dst, dgt = d(np.concatenate([g[n]["st"] for n in names])), d(np.concatenate([logs[n][0] for n in names]))
        dgp, dso, dgo = d(np.concatenate([logs[n][1] for n in names])), d(so), d(go)
        al = torch.full((int(so[-1]), 3), 7.0, dtype=torch.float64, device="cuda")     # (every row must be written: 7.0 is no value of the grid)
        va = torch.full((int(so[-1]),), 7, dtype=torch.uint8, device="cuda")
        stt = torch.full((len(names),), 7, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(entry(h, p(dst), p(dso), p(dgt), p(dgp), p(dgo), len(names), max_g, float(gap), p(al), p(va), p(stt)))
        torch.cuda.synchronize()
        al, va, stt = al.cpu().numpy(), va.cpu().numpy(), stt.cpu().numpy()
        for i, n in enumerate(names):
            out[n] = (al[so[i]:so[i + 1]].copy(), va[so[i]:so[i + 1]].copy(), int(stt[i]))
    for v in out.values():
        v[0].setflags(write=False); v[1].setflags(write=False)
    _runs[route] = out
    return out


def check_against_yardstick(orc, what, got, names=NAMES):
    """the gates of the module docstring on the outputs `got` of a route; prints the worst value error per family next to e_orc"""
    problems, worst, comp = [], {}, {}
    for name in names:
        al, va, status = got[name]
        c, t = ref.cases()[name], ref.truth(name)
        tol, e_orc = tolerance(orc, name), oracle_error(orc, name)
        if status != 0:
            problems.append((name, f"status {status}"))
        if not np.array_equal(va, t["valid"].astype(np.uint8)):
            rows = np.where(va != t["valid"])[0]
            problems.append((name, f"valid differs at {len(rows)} rows", rows[:5].tolist(), c["st"][rows[:5]].tolist(), c["qkind"][rows[:5]].tolist()))
        if not np.array_equal(np.isnan(al), np.isnan(t["aligned"])):
            rows = np.where((np.isnan(al) != np.isnan(t["aligned"])).any(axis=1))[0]
            problems.append((name, f"NaN pattern differs at {len(rows)} rows", rows[:5].tolist(), c["st"][rows[:5]].tolist(), c["qkind"][rows[:5]].tolist()))
            continue
        k = t["on_knot"]
        off = np.where(k & (al.view(np.int64) != t["aligned"].view(np.int64)).any(axis=1))[0]
        if len(off):
            problems.append((name, f"{len(off)} of {int(k.sum())} queries on a knot do not return the knot", c["st"][off[:5]].tolist(),
                             (al[off[:5]] - t["aligned"][off[:5]]).tolist()))
        rows = t["valid"] & ~k
        err3 = np.max(np.abs(al[rows] - t["aligned"][rows]), axis=0, initial=0.0)
        err = float(err3.max())
        with np.errstate(invalid="ignore", divide="ignore"):                 # (printed, not gated: easting, northing, altitude in ulp of their own largest value)
            comp.setdefault(c["family"], []).append(np.nan_to_num(err3 / t["ulp3"]))
        fam = worst.setdefault(c["family"], dict(err=0.0, ulp=0.0, e_orc=0.0, tol=np.inf, name=""))
        if t["ulp"] and err / t["ulp"] >= fam["ulp"]:
            fam.update(err=err, ulp=err / t["ulp"], name=name)
        if t["ulp"]:
            fam["e_orc"], fam["tol"] = max(fam["e_orc"], e_orc), min(fam["tol"], tol)
        if not err <= tol:
            i = int(np.argmax(np.max(np.abs(np.where(rows[:, None], al - t["aligned"], 0.0)), axis=1)))
            problems.append((name, f"max |device - yardstick| {err:.3e} m = {err / t['ulp']:.1f} ulp(S) > tol {tol:.3e} (e_orc {e_orc:.2e})", f"query {i} at {c['st'][i]!r}"))
    for f in FAMILIES:
        if f in worst:
            w = worst[f]
            print(f"{what} {f:8s}: worst device error {w['err']:.2e} m = {w['ulp']:.1f} ulp(S) ({w['name']}); e_orc <= {w['e_orc']:.2e} m, smallest tol {w['tol']:.2e} m; "
                  f"per component {', '.join(f'{v:.1f}' for v in np.max(comp[f], axis=0))} ulp(S_c)")
    return problems


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_lds_route_against_the_yardstick(B, orc):
    """(a) gsf_time_align_batch_dev, max_gps_per_trajectory = 512: the LDS-staged instantiation.

    Measured on an MI355X, worst |device - yardstick| over the valid rows off the knots, per family (the global-slab route of (b) gives the
    same figures to the digit); S is about 5.4e6 m (the northing), ulp(S) = 9.31e-10 m, the smallest tol 3.73e-9 m:

        family    device error              e_orc (oracle)    case of the worst error
        knots     1.86e-09 m = 2 ulp(S)     <= 1.86e-09 m     knots_m131 (kk = 129)
        multi     1.86e-09 m = 2 ulp(S)     <= 1.86e-09 m     multi_seg
        spacing   1.86e-09 m = 2 ulp(S)     <= 1.86e-09 m     sp_alternating
        epoch     1.86e-09 m = 2 ulp(S)     <= 9.31e-10 m     epoch_uniform
        units     1.86e-09 m = 2 ulp(S)     <= 1.86e-09 m     units_ms
        ns        9.31e-10 m = 1 ulp(S)     <= 9.31e-10 m     ns65
        planted   1.86e-09 m = 2 ulp(S)     <= 9.31e-10 m     planted_inc_2e-9
        order     1.86e-09 m = 2 ulp(S)     <= 1.86e-09 m     dup_split

    (Both sides are float64 numbers next to a correctly rounded one, so the figures are whole ulps.)  Per component, in ulp of the
    component's own largest value (printed, not gated): at most 2 for easting, northing and altitude on every case but one --
    sp_tail_1e-4_4, where the last interval is 4e4 times its neighbour: easting 4.07e-10 m = 7 ulp (the oracle: 7 as well), altitude
    1.85e-13 m = 13 ulp (the oracle: 1).  M[m-1] = M[m-2] + r1 (M[m-2] - M[m-3]) multiplies the rounding of the two inner values by
    r1 = 4e4 in the kernel and in the oracle alike; it stays 4 orders of magnitude below the northing's ulp."""
    problems = check_against_yardstick(orc, "lds", run_grid(B, "lds"))
    assert not problems, problems


def test_global_slab_route_against_the_yardstick(B, orc):
    """(b) the same batch with max_gps_per_trajectory = 2561: the double* instantiation (staging in global scratch) on small logs."""
    problems = check_against_yardstick(orc, "slab", run_grid(B, "slab"))
    assert not problems, problems


def test_loader_masked_rows_never_reach_the_spline(B):
    """(c) gsf_time_align_loaded_rows_batch_dev on every log with NaN-marked fixes added (masked_log): the bytes of (a) on the log without
    them -- the same instantiation and arithmetic, only the indices move."""
    plain, masked = run_grid(B, "lds"), run_grid(B, "masked")
    differ = [name for name in NAMES if not same_bytes(plain[name], masked[name])]
    assert not differ, differ


def test_order_of_the_log_does_not_matter(B, orc):
    """(d) a shuffled log with ten fixes logged twice gives the bytes of its sorted original; the log with a NaN stamp loses its last
    segment only; of a fix logged twice with two positions the first in input order is the knot."""
    got = run_grid(B, "lds")
    differ = [name for name, of in ref.SHUFFLED.items() if not same_bytes(got[name], got[of])]
    assert not differ, differ
    t, plain = ref.truth("nan_stamp"), ref.truth("multi_seg")
    lost = plain["valid"] & ~t["valid"]
    assert lost.sum() > 30 and t["valid"].sum() > 150 and not (t["valid"] & ~plain["valid"]).any()
    keep = t["valid"]
    assert got["nan_stamp"][0][keep].tobytes() == got["multi_seg"][0][keep].tobytes() and np.isnan(got["nan_stamp"][0][lost]).all()
    problems = check_against_yardstick(orc, "order", got, ["nan_stamp", "dup_split"])
    assert not problems, problems


def test_host_entry_gives_the_bytes_of_the_batch(B, E):
    """(e) ekfgpsslam.dynamic_time_alignment (gsf_time_align_batch: one log, staging sized by it) on the two spacing extremes, an uneven
    tail, the epoch case and the multi-segment case"""
    got, g = run_grid(B, "lds"), ref.cases()
    differ = []
    for name in ref.HOST_ENTRY:
        c = g[name]
        al, va = E.dynamic_time_alignment({"timestamps": c["st"]}, {"timestamps": c["gt"], "positions": c["gp"]},
                                          {"max_samples_for_corr": 500, "max_gps_gap_threshold": c["max_gap"]})
        assert va.dtype == bool and al.shape == (len(c["st"]), 3)
        if not (al.tobytes() == got[name][0].tobytes() and np.array_equal(va, got[name][1].astype(bool))):
            differ.append(name)
    assert not differ, differ
