"""Outputs must not depend on stale buffers, on what a workspace held, or on the stream (tests/hygiene.py has the machinery).

1. Every device entry of batch.py, at shapes that reach the launcher branches of DESIGN section 4, run three times on fixed inputs: on
   fresh workspaces, and twice after a larger foreign call with every workspace overwritten by gsf_set_option "poison_workspaces" (word 0,
   word 3) and every output pre-filled with the same word, between guard bytes.  All output bytes and generator states must be the same in
   the three runs, and no guard byte may change.  The inputs hold failing, empty and too-short tracks: that is where writes get skipped.
2. One host-pointer entry per family, numpy outputs pre-filled the same way (staging arena + pinned mirror).
3. The same calls on a side stream with their inputs still in flight, and two contexts on two streams interleaved.

Byte equality of the product with itself; no tolerance."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest

import hygiene
from test_run_ragged import _make_batch
from test_tail_scans import planted_batch

pytestmark = pytest.mark.gpu

# What a check may leave out: only what include/gsf.h says is not written.  (entry point, field, the header's words.)  The masked bytes are
# computed from the call's own inputs and their count is asserted (hygiene.same_bytes_under_dirt), so an entry cannot quietly grow.
# Empty today: every byte of every output of every entry below is compared.  (The dense whole-run entry no longer hands out zone / south
# under projected=True; the sets of a stream with n_population[b] < k turned out to be zero-filled by both samplers, and the header says so now.)
EXCEPTIONS = []

DEFAULTS = {"tail_scan_stages": 1, "duo_kernel": -1, "block_kernel": -1, "lane_min_traj": 32768, "k2b_screen": 1, "tape_draws": -1,
            "ransac_probe_trials": 64, "prefilter_speculate": 1, "ransac_early_exit": 0}


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


@contextlib.contextmanager
def options(ctx, **opts):
    before = {k: ctx.options.get(k, DEFAULTS[k]) for k in opts}
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield ctx
    finally:
        for k, v in before.items():
            ctx.set_option(k, v)


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


# ------------------------------------------------------------------------------------------------ the foreign call that dirties a context
class Dirt:
    """A larger call of every family on the context of the current stream: afterwards each workspace holds another batch's data (a plain
    and a robust chain, the transposed time-major route, the workgroup kernel's row marks, a whole run, a host-pointer call)."""

    def __init__(self, B):
        self.B = B
        self.big = B.TrajectoryBatch.synthetic(96, 1100, layout=0, seed=5)
        self.tm = B.TrajectoryBatch.synthetic(300, 1100, layout=1, seed=6)
        self.mid = B.TrajectoryBatch.synthetic(300, 700, layout=0, seed=7)
        self.gb = B.GeodeticBatch.synthetic(96, 1100, seed=8).with_outliers(0.02)
        self.st = B.mt19937_seed(np.arange(96) + 900)
        rng = np.random.default_rng(3)
        self.e, self.n = rng.uniform(3e5, 7e5, 300000), rng.uniform(1e6, 8e6, 300000)

    def __call__(self):
        from gps_optimize_slam_amd import _lib
        B, ctx = self.B, self.B.context()
        with options(ctx, block_kernel=1):
            B.fuse_pipeline_batch(self.mid)
        B.ekf_fuse_batch(self.tm)
        B.fuse_pipeline_robust_batch(self.big, self.st.clone(), fit_rows="all", early_exit=False)
        B.fuse_pipeline_robust_batch(self.big, self.st.clone(), fit_rows="all", early_exit=True)
        B.run_fusion_batch(self.gb, self.st.clone())
        lat, lon = np.empty_like(self.e), np.empty_like(self.e)
        _lib.check(_lib.load().gsf_utm_inverse(ctx.handle, _lib.hptr(self.e), _lib.hptr(self.n), self.e.size, 32, 0, _lib.hptr(lat), _lib.hptr(lon)))
        ctx.set_option("ransac_early_exit", 0)


@pytest.fixture(scope="module")
def dirt(B):
    return Dirt(B)


# ------------------------------------------------------------------------------------------------ the helper itself
def test_guard_check_names_the_allocation_and_the_offset(B, monkeypatch):
    """a byte written past the end of one guarded allocation, and one before another: assert_guards_intact names allocation and offset"""
    import torch
    alloc = hygiene.GuardedAllocator(3)
    with alloc.installed(monkeypatch):
        a = torch.empty((5, 3), dtype=torch.float64, device="cuda")
        b = torch.empty_like(a, dtype=torch.uint8)
        c = torch.empty(7, dtype=torch.int32, device="cuda")
        host = torch.empty((4,), dtype=torch.float64)                       # a CPU request passes through
    assert torch.empty is alloc._empty and len(alloc.records) == 3 and not host.is_cuda
    assert a.shape == (5, 3) and a.data_ptr() % 256 == 0 and b.dtype == torch.uint8 and b.shape == (5, 3) and c.shape == (7,)
    assert (a.view(torch.int64) == 3).all() and c.tolist() == [3, 0, 3, 0, 3, 0, 3]        # the word 3 through float64 bits and through int32
    torch.cuda.synchronize()
    alloc.assert_guards_intact()
    assert [p.size for p in alloc.payloads()] == [120, 15, 28]
    assert (alloc.payloads()[1] == np.array([3, 0, 0, 0, 0, 0, 0, 0] * 2, np.uint8)[:15]).all()
    assert alloc.find(b) is alloc.records[1] and alloc.find(a[2:]) is alloc.records[0]
    rec = alloc.records[1]
    rec.block[rec.off + rec.nbytes + 2] = 0x11                               # the third byte after b's last
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"guard bytes after allocation #1 \(5, 3\) uint8 .*first at offset \+2 from the payload's end \(value 0x11\)"):
        alloc.assert_guards_intact()
    rec.block[rec.off + rec.nbytes + 2] = hygiene.GUARD_BYTE
    rec = alloc.records[2]
    rec.block[rec.off - 8:rec.off - 4] = 0
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"guard bytes before allocation #2 \(7,\) int32 .*4 byte\(s\), first at offset -8 from the payload's start"):
        alloc.assert_guards_intact()
    h = hygiene.HostAllocator(3)
    x = h.new((3, 2), np.int32)
    assert x.tolist() == [[3, 0], [3, 0], [3, 0]] and x.ctypes.data % 256 == 0
    h.assert_guards_intact()
    h.records[0].block[h.records[0].off - 1] = 0
    with pytest.raises(AssertionError, match=r"guard bytes before allocation #0 \(3, 2\) int32 .*first at offset -1 "):
        h.assert_guards_intact()


def test_an_unwritten_byte_is_named(B, monkeypatch, dirt):
    """the central check on a stand-in for a product call that leaves one row of its output unwritten"""
    import torch
    ctx = B.context()

    def leaky():
        out = torch.empty((8, 3), dtype=torch.float64, device="cuda")
        out[:5] = 1.5; out[6:] = 2.5                                        # row 5 is never written
        return out
    with pytest.raises(AssertionError, match=r"dirty A .* vs dirty B .*: allocation #0 \(8, 3\) float64 .*3 element\(s\) differ \(3 bytes\), first at element \(5, 0\) = track 5"):
        hygiene.same_bytes_under_dirt(monkeypatch, ctx, leaky, dirt)


def test_poison_option_range(B):
    """-1 and 0..255 are taken, anything else fails like the other keys' bad values"""
    from gps_optimize_slam_amd import _lib
    ctx = B.context()
    for bad in (-2, 256, 1 << 40):
        with pytest.raises(_lib.GsfError, match="poison_workspaces"):
            ctx.set_option("poison_workspaces", bad)
    with pytest.raises(_lib.GsfError, match="unknown key"):
        ctx.set_option("poison_workspace", 0)
    ctx.set_option("poison_workspaces", -1)


# ------------------------------------------------------------------------------------------------ 1a. K4 and the fused pipeline, dense
def tm_batch(B, nb, N, seed, layout=0):
    """planted_batch's eight kinds of tracks plus, from 16 tracks on: one without any fix (its fit fails), one with three valid rows (fewer
    than min_samples), one whose fixes are all NaN under a set mask"""
    ts, pos, quat, gps, valid, ip, iq = planted_batch(nb, N, seed)
    if nb >= 16:
        valid[8] = 0; gps[8] = np.nan
        valid[9, 3:] = 0; gps[9, 3:] = np.nan
        gps[10] = np.nan
    return B.TrajectoryBatch.from_host(ts, pos, quat, gps, valid, ip, iq, layout=layout)


EKF_CASES = [
    (0, 256, 1, {}), (0, 256, 15, {"tail_scan_stages": 0}), (0, 256, 15, {"tail_scan_stages": 1}), (0, 256, 64, {}),
    (0, 256, 65, {"duo_kernel": 0}), (0, 256, 65, {"duo_kernel": 1}), (0, 256, 271, {"duo_kernel": 0, "tail_scan_stages": 1}),
    (0, 256, 271, {"duo_kernel": 1, "tail_scan_stages": 0}), (0, 256, 271, {"block_kernel": 1}), (0, 256, 1039, {"tail_scan_stages": 1}),
    (0, 256, 1039, {"tail_scan_stages": 0}), (0, 2304, 65, {}), (0, 2304, 271, {}),
    (1, 256, 65, {}), (1, 256, 271, {}), (1, 256, 271, {"lane_min_traj": 0}),
]


def _case_id(c):
    return f"{'time' if c[0] else 'traj'}-major-B{c[1]}-N{c[2]}" + "".join(f"-{k}={v}" for k, v in c[3].items())


@pytest.mark.parametrize("case", EKF_CASES, ids=_case_id)
def test_ekf_and_pipeline_dense(B, monkeypatch, dirt, case):
    layout, nb, N, opts = case
    bt = tm_batch(B, nb, N, 100 + N, layout)
    ctx = B.context()

    def fn():
        with options(ctx, **opts):
            return B.ekf_fuse_batch(bt), B.fuse_pipeline_batch(bt, fit_rows="reference"), B.fuse_pipeline_batch(bt, fit_rows="all")
    hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt)


# ------------------------------------------------------------------------------------------------ 1b. ragged K4 / pipeline
RAGGED_LENGTHS = [0, 1, 63, 64, 65, 513, 1700, 3, 40, 0, 271, 2, 130]


def ragged_inputs(lengths, seed):
    """flat rows of tracks of the given lengths, kinds of planted_batch in turn; track 8 (40 poses) has no fix at all"""
    cols = [[] for _ in range(7)]
    for b, n in enumerate(lengths):
        parts = planted_batch(8, max(n, 1), seed + b)
        k = b % 8
        for c, p in zip(cols[:5], parts[:5]):
            c.append(p[k][:n])
        cols[5].append(parts[5][k]); cols[6].append(parts[6][k])
    ts, pos, quat, gps, valid = (np.concatenate(c) for c in cols[:5])
    ip, iq = np.stack(cols[5]), np.stack(cols[6])
    offs = np.zeros(len(lengths) + 1, np.int64); offs[1:] = np.cumsum(lengths)
    valid[offs[8]:offs[9]] = 0; gps[offs[8]:offs[9]] = np.nan
    return ts, pos, quat, gps, valid, offs, ip, iq


RAGGED_BIG = 2049                                                        # the smallest ragged batch that takes the big-batch build (gsf_wave_route.hpp)


@pytest.mark.parametrize("order", ["as-listed", "reversed", "tiled-to-2049"])
def test_ekf_and_pipeline_ragged(B, monkeypatch, dirt, order):
    lengths = {"as-listed": RAGGED_LENGTHS, "reversed": RAGGED_LENGTHS[::-1],
               "tiled-to-2049": (RAGGED_LENGTHS * (RAGGED_BIG // len(RAGGED_LENGTHS) + 1))[:RAGGED_BIG]}[order]
    ts, pos, quat, gps, valid, offs, ip, iq = ragged_inputs(lengths, 40)
    assert ts.size == sum(lengths) and pos.shape == (ts.size, 3) and ip.shape == (len(lengths), 3)
    d = [dev(a) for a in (ts, pos, quat, gps)] + [dev(valid.astype(np.uint8)), dev(offs)]
    dip, diq = dev(ip), dev(iq)
    ctx = B.context()

    def fn():
        return (B.ekf_fuse_ragged(*d, dip, diq), B.fuse_pipeline_ragged(*d, fit_rows="reference"), B.fuse_pipeline_ragged(*d, fit_rows="all"))
    hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt, rows_of=offs)


# ------------------------------------------------------------------------------------------------ 1c. the robust chain
def robust_batch(B, nb, N, seed):
    """synthetic tracks; every 3rd with one fix 30 m off among the rows of its fit (never saturates), every 5th one 3.9 m off (late or
    never); track 1 without any fix, track 2 with three valid rows (fewer than min_samples): their fit fails before it draws"""
    import torch
    bt = B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=seed)
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    rowmask = B.sim3_fit_rows_batch(bt.ts, bt.gps, bt.valid)[0].cpu()
    for b in range(nb):
        rows = torch.nonzero(rowmask[b] != 0).ravel()
        if rows.numel() > 8 and b % 3 == 0:
            bt.gps[b, int(rows[int(torch.randint(0, rows.numel(), (1,), generator=g))])] += 30.0
        elif rows.numel() > 8 and b % 5 == 0:
            bt.gps[b, int(rows[int(torch.randint(0, rows.numel(), (1,), generator=g))]), 0] += 3.9
    bt.valid[1] = 0; bt.gps[1] = float("nan")
    bt.valid[2, 3:] = 0; bt.gps[2, 3:] = float("nan")
    torch.cuda.synchronize()
    return bt


# nb, N, fit_rows, early_exit, options, want_mask, return_info
ROBUST_CASES = [
    (40, 271, "reference", True, {}, True, True),                               # > 32 sets, probe decides the clean tracks
    (40, 271, "reference", False, {}, True, True),                              # every trial drawn: keys cleared by the launcher
    (40, 271, "reference", True, {"ransac_probe_trials": 2}, True, True),       # hand-over to the wide kernels after two trials
    (9, 271, "reference", True, {"ransac_probe_trials": 2}, True, True),        # <= 32 sets: split K2b; <= 16 streams: chip-wide draws
    (9, 271, "reference", False, {"tape_draws": 0}, True, True),
    (9, 271, "reference", False, {"tape_draws": -1}, True, True),
    (40, 700, "all", True, {}, True, True),                                     # > 512 chosen rows: the final fit is left to K2b
    (40, 700, "all", False, {"k2b_screen": 0}, True, False),
    (40, 271, "reference", True, {"k2b_screen": 0}, False, False),
]


@pytest.mark.parametrize("case", ROBUST_CASES, ids=lambda c: f"B{c[0]}-N{c[1]}-rows={c[2]}-early_exit={int(c[3])}" + "".join(f"-{k}={v}" for k, v in c[4].items())
                         + f"-mask={int(c[5])}-info={int(c[6])}")
def test_robust_chain(B, monkeypatch, dirt, case):
    import torch
    nb, N, rows, ee, opts, want_mask, info = case
    bt = robust_batch(B, nb, N, 20 + nb + N)
    st0 = B.mt19937_seed(np.arange(nb) + 300)
    ctx = B.context()

    def fn(st):
        with options(ctx, **opts):
            return B.fuse_pipeline_robust_batch(bt, st, fit_rows=rows, early_exit=ee, want_mask=want_mask, return_info=info)
    res = hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt, states=(st0,))
    ctx.set_option("ransac_early_exit", 0)
    status = res[0].status
    sat = ((status >> 8) & 256) != 0
    failed = ((status >> 8) & (1 | 32)) != 0                                    # GSF_SIM3_NONE / GSF_SIM3_FLAG_FEW_ROWS
    assert failed[1] and failed[2] and not failed.all()                         # the cases hold failing tracks ...
    assert not sat[[0, 3, 6]].any()                                             # ... tracks that never saturate (a fix 30 m off) ...
    if not ee:
        assert not sat.any()
    elif "ransac_probe_trials" not in opts:
        assert sat.any()                                                        # ... and tracks that do


# ------------------------------------------------------------------------------------------------ 1d. whole runs
@pytest.fixture(scope="module")
def run_inputs(B, orc):
    tracks, logs, gts = _make_batch(orc)
    return tracks, logs, gts


def _run_cfg(gt_filter=False):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = copy.deepcopy(E.CONFIG)
    cfg["ground_truth_gps_filtering"]["enabled"] = bool(gt_filter)
    return cfg


# ground truth, projected, ground-truth filter, options, max_windows, early_exit, want_mask
RAGGED_RUN_CASES = [
    (True, False, True, {}, 0, True, True), (True, False, False, {"prefilter_speculate": 0}, 0, False, True), (False, False, False, {}, 0, True, False),
    (True, True, True, {}, 0, True, True), (False, True, False, {"prefilter_speculate": 0}, 0, False, True), (True, False, True, {}, 1, True, True),
]


@pytest.mark.parametrize("case", RAGGED_RUN_CASES, ids=lambda c: f"gt={int(c[0])}-projected={int(c[1])}-gt_filter={int(c[2])}" + "".join(f"-{k}={v}" for k, v in c[3].items())
                         + f"-max_windows={c[4]}-early_exit={int(c[5])}-mask={int(c[6])}")
def test_run_fusion_ragged(B, monkeypatch, dirt, run_inputs, case):
    import torch
    from gps_optimize_slam_amd import _lib
    gt, projected, gtf, opts, max_windows, ee, want_mask = case
    tracks, logs, gts = run_inputs
    rb = B.RaggedGeodeticBatch.from_host(tracks, logs, gts if gt else None)
    cfg = _run_cfg(gtf)
    st0 = B.mt19937_seed(np.arange(rb.B) + 100)
    ctx = B.context()
    if projected:                                                               # the logs as load_gps_data's projection leaves them
        r0 = B.run_fusion_ragged(rb, st0.clone(), cfg)
        rb = B.RaggedGeodeticBatch(rb.ts, rb.pos, rb.quat, rb.slam_offsets, rb.gps_t, r0.gps_utm.clone(), rb.gps_offsets, rb.gt_t,
                                   r0.gt_utm.clone() if gt else None, rb.gt_offsets)
        torch.cuda.synchronize()

    def fn(st):
        with options(ctx, **opts):
            return B.run_fusion_ragged(rb, st, cfg, early_exit=ee, max_windows=max_windows, want_mask=want_mask, projected=projected)
    r = hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt, states=(st0,), rows_of=rb.slam_offsets.cpu().numpy())
    assert (r.zone is None) == projected and (r.gt_utm is None) == (not gt)
    rs = r.run_status.cpu().numpy()
    assert (rs != 0).sum() >= 3 and (max_windows or (rs == 0).sum() >= 20), rs
    if max_windows:
        assert (rs & _lib.RUN_PREFILTER_UNHANDLED).any(), rs
    elif gt and not projected:
        assert (rs & _lib.RUN_GT_EMPTY).any() and (rs & _lib.RUN_SLAM_EMPTY).any() and (rs & _lib.RUN_GPS_FEW).any(), rs


def dense_run_batch(B, nb, N, seed, rate=None, orc=None):
    """test_run_chain's 64 logs: fixes 60 m off, rows the loader removes, logs of three fixes / one fix / none in range"""
    src = B.GeodeticBatch.synthetic(nb, N, seed=seed)
    offs = src.gps_offsets.cpu().numpy()
    gt, llh = src.gps_t.cpu().numpy(), src.gps_llh.cpu().numpy()
    ts, pos, quat = src.ts.cpu().numpy(), src.pos.cpu().numpy(), src.quat.cpu().numpy()
    rng = np.random.default_rng(5)
    logs = []
    for b in range(nb):
        log = np.column_stack((gt[offs[b]:offs[b + 1]], llh[offs[b]:offs[b + 1]]))
        n = len(log)
        if rate is not None:                                                    # the same path sampled at `rate` Hz (linear between the fixes)
            tg = np.arange(log[0, 0], log[-1, 0], 1.0 / rate)
            log = np.column_stack([tg] + [np.interp(tg, log[:, 0], log[:, c]) for c in (1, 2, 3)])
            n = len(log)
        if b % 3 == 0 and n > 40:
            for r_ in rng.choice(n, size=int(rng.integers(1, 6)), replace=False):
                log[r_, 1] += 60.0 / 111200.0 * rng.choice([-1, 1]); log[r_, 2] += 60.0 / 73000.0 * rng.choice([-1, 1])
        if b % 5 == 1 and n > 40:
            rr = rng.choice(n, size=4, replace=False)
            log[rr[0], 1] = 0.0; log[rr[1], 2] = 0.0; log[rr[2], 1] = 91.0; log[rr[3], 2] = -181.0
        if b == 10: log = log[[0, n // 2, n - 1]]
        if b == 11: log = log[[n // 2]]
        if b == 12: log[:, 1] = 0.0
        if b == 13: log = log[:0]
        logs.append(log)
    return B.GeodeticBatch.from_host(ts, pos, quat, logs)


# tracks, poses, rate of the log (None: one fix per pose), projected, options, max_windows, early_exit, want_mask
DENSE_RUN_CASES = [
    (64, 271, None, False, {}, 0, True, True), (64, 271, None, False, {"prefilter_speculate": 0}, 0, False, False), (64, 271, None, True, {}, 0, True, True),
    (16, 271, 50.0, False, {}, 0, True, True), (64, 271, None, False, {}, 1, True, True), (24, 1700, None, False, {}, 0, True, True),
]


@pytest.mark.parametrize("case", DENSE_RUN_CASES, ids=lambda c: f"B{c[0]}-N{c[1]}-rate={c[2]}-projected={int(c[3])}" + "".join(f"-{k}={v}" for k, v in c[4].items())
                         + f"-max_windows={c[5]}-early_exit={int(c[6])}-mask={int(c[7])}")
def test_run_fusion_batch(B, monkeypatch, dirt, case):
    import torch
    from gps_optimize_slam_amd import _lib
    nb, N, rate, projected, opts, max_windows, ee, want_mask = case
    gb = dense_run_batch(B, nb, N, 77, rate)
    cfg = _run_cfg()
    st0 = B.mt19937_seed(np.arange(nb) + 500)
    ctx = B.context()
    if projected:
        r0 = B.run_fusion_batch(gb, st0.clone(), cfg)
        gb = B.GeodeticBatch(gb.B, gb.N, gb.ts, gb.pos, gb.quat, gb.gps_offsets, gb.gps_t, r0.gps_utm.clone(), gb.max_fixes)
        torch.cuda.synchronize()

    def fn(st):
        with options(ctx, **opts):
            return B.run_fusion_batch(gb, st, cfg, early_exit=ee, max_windows=max_windows, want_mask=want_mask, projected=projected)
    r = hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt, states=(st0,))
    ctx.set_option("ransac_early_exit", 0)
    assert (r.zone is None) == projected and (r.south is None) == projected      # no field handed out unwritten
    rs = r.run_status.cpu().numpy()
    assert (rs[[11, 12, 13]] != 0).all() and (max_windows or (rs == 0).sum() >= nb // 2), rs
    if max_windows:
        assert (rs & _lib.RUN_PREFILTER_UNHANDLED).any(), rs
    else:
        assert not (rs & _lib.RUN_PREFILTER_UNHANDLED).any(), rs


# ------------------------------------------------------------------------------------------------ 1e. step 7
@pytest.mark.parametrize("fmt", ["utm", "wgs84"])
def test_step7_rows_and_text(B, monkeypatch, dirt, fmt):
    rng = np.random.default_rng(12)
    lens = [0, 1, 271, 5, 0, 1000, 64, 65, 1, 130, 3, 777]
    P = sum(lens)
    offs = np.zeros(len(lens) + 1, np.int64); offs[1:] = np.cumsum(lens)
    ts = dev(rng.uniform(1.2e9, 1.8e9, P))
    pos = dev(np.column_stack([rng.uniform(2e5, 8e5, P), rng.uniform(1e5, 9.3e6, P), rng.uniform(-100, 4000, P)]))
    quat = dev(rng.normal(size=(P, 4)))
    zone, south = dev(rng.integers(1, 61, len(lens)).astype(np.int32)), dev(rng.integers(0, 2, len(lens)).astype(np.int32))
    status = np.zeros(len(lens), np.int32); status[[3, 6]] = 8, 1                # two failed tracks: NaN rows, no text
    o, rs = dev(offs), dev(status)
    ctx = B.context()

    def fn():
        xyz = B.utm_to_wgs84_ragged(pos, o, zone, south, rs) if fmt == "wgs84" else pos
        texts, st = B.tum_text_ragged(ts, xyz, quat, o, fmt=fmt, run_status=rs)
        assert texts[3] is None and texts[6] is None and texts[0] is not None
        return xyz, texts, st
    a = hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt, rows_of=offs)
    assert list(a[2]) == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 1f. the single-stage entries
def ragged_sets(rng, lens, scale=1.0):
    offs = np.zeros(len(lens) + 1, np.int64); offs[1:] = np.cumsum(lens)
    T = int(offs[-1])
    src = rng.normal(size=(T, 3)) * 30.0
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    dst = scale * src @ R.T + np.array([4.5e5, 5.4e6, 110.0]) + rng.normal(size=(T, 3)) * 0.3
    return src, dst, offs


SET_LENGTHS = [0, 1, 2, 3, 4, 5, 64, 65, 300, 0, 700, 9]


def test_from_geodetic_chain(B, monkeypatch, dirt):
    gb = B.GeodeticBatch.synthetic(96, 271, seed=31).with_outliers(0.02)
    hygiene.same_bytes_under_dirt(monkeypatch, B.context(), lambda: B.fuse_from_geodetic(gb), dirt)
    gb2 = dense_run_batch(B, 32, 271, 9)                                        # logs of three fixes, one fix, none
    hygiene.same_bytes_under_dirt(monkeypatch, B.context(), lambda: B.fuse_from_geodetic(gb2), dirt)


def test_time_alignment_global_staging_length(B, monkeypatch, dirt):
    """a log longer than the alignment's LDS staging (the 'global staging' route) next to short and empty ones"""
    import torch
    rng = np.random.default_rng(8)
    N = 400
    ts = np.tile(1000.0 + 0.1 * np.arange(N), (8, 1))
    pos = rng.normal(size=(8, N, 3)); quat = np.tile([0.0, 0, 0, 1], (8, N, 1))
    logs = []
    for b, m in enumerate([9000, 0, 1, 2, 40, 300, 5000, 12]):
        t = np.sort(rng.uniform(995.0, 1045.0, m))
        logs.append(np.column_stack((t, 49.0 + rng.uniform(0, 1e-3, m), 8.4 + rng.uniform(0, 1e-3, m), rng.uniform(100, 120, m))))
    gb = B.GeodeticBatch.from_host(ts, pos, quat, logs)
    hygiene.same_bytes_under_dirt(monkeypatch, B.context(), lambda: B.fuse_from_geodetic(gb), dirt)


def test_sim3_entries(B, monkeypatch, dirt):
    import torch
    rng = np.random.default_rng(4)
    ctx = B.context()
    src, dst, offs = ragged_sets(rng, SET_LENGTHS, 1.03)
    dst[offs[8] + 5] += 40.0                                                    # an outlier for the RANSAC entry
    mask = (rng.random(len(src)) < 0.8).astype(np.uint8)
    mask[offs[4]:offs[5]] = 0                                                   # a set with no row left
    d_src, d_dst, d_off, d_mask = dev(src), dev(dst), dev(offs), dev(mask)
    win_s, win_d = dev(rng.normal(size=(70, 50, 3))), dev(rng.normal(size=(70, 50, 3)))
    win_m = (rng.random((70, 50)) < 0.7).astype(np.uint8); win_m[3] = 0; win_m[4, 2:] = 0
    d_wm = dev(win_m)
    nsets = len(SET_LENGTHS)
    idx = np.stack([np.stack([rng.choice(max(n, 4), 4, replace=False) for _ in range(24)]) for n in SET_LENGTHS]).astype(np.int32)
    d_idx = dev(idx)
    idx_many = np.stack([np.stack([rng.choice(max(n, 4), 4, replace=False) for _ in range(256)]) for n in SET_LENGTHS]).astype(np.int32)
    d_idx_many = dev(idx_many)                                                  # <= 32 sets and >= 256 trials: hypotheses spread over the chip, keys in small_scratch
    R = dev(np.tile(np.eye(3).reshape(9), (nsets, 1))); t = dev(rng.normal(size=(nsets, 3))); s = dev(rng.uniform(0.5, 2.0, nsets))
    quat = rng.normal(size=(len(src), 4)); quat[offs[6] + 3] = 0.0               # a bad quaternion
    d_quat = dev(quat)
    # rows for the row rule: dense and ragged
    tsd, _, _, gpsd, vald, _, _ = planted_batch(24, 271, 3)
    vald[5] = 0; vald[6, 3:] = 0
    d_ts, d_gps, d_val = dev(tsd), dev(gpsd), dev(vald.astype(np.uint8))
    rts, _, _, rgps, rval, roffs, _, _ = ragged_inputs(RAGGED_LENGTHS, 70)
    d_rts, d_rgps, d_rval, d_roffs = dev(rts), dev(rgps), dev(rval.astype(np.uint8)), dev(roffs)

    def fn():
        with options(ctx, **opts):
            return (B.sim3_umeyama_batch(d_src, d_dst, d_off), B.sim3_umeyama_batch(d_src, d_dst, d_off, d_mask), B.sim3_umeyama_batch(win_s, win_d),
                    B.sim3_umeyama_batch(win_s, win_d, mask=d_wm), B.sim3_ransac_batch(d_src, d_dst, d_off, d_idx, 2.0, 4),
                    B.sim3_ransac_batch(d_src[:offs[9]], d_dst[:offs[9]], d_off[:10], d_idx[:9], 2.0, 4), B.sim3_ransac_batch(d_src, d_dst, d_off, d_idx_many, 2.0, 4),
                    B.apply_sim3_batch(d_src, d_quat, d_off, R, t, s), B.sim3_fit_rows_batch(d_ts, d_gps, d_val), B.sim3_fit_rows_batch(d_ts, None, d_val),
                    B.sim3_fit_rows_batch(d_rts, d_rgps, d_rval, offsets=d_roffs))
    for opts in ({"k2b_screen": 1}, {"k2b_screen": 0}):
        hygiene.same_bytes_under_dirt(monkeypatch, ctx, fn, dirt, rows_of=offs)


def test_geodesy_entries(B, monkeypatch, dirt):
    rng = np.random.default_rng(6)
    lens = [0, 1, 8, 300, 0, 65, 1000]
    offs = np.zeros(len(lens) + 1, np.int64); offs[1:] = np.cumsum(lens)
    T = int(offs[-1])
    lat, lon, alt = rng.uniform(-80, 84, T), rng.uniform(-180, 180, T), rng.uniform(0, 3000, T)
    lat[offs[3] + 2] = np.nan
    d_lat, d_lon, d_alt, d_off = dev(lat), dev(lon), dev(alt), dev(offs)
    zone, south = dev(rng.integers(1, 61, len(lens)).astype(np.int32)), dev(rng.integers(0, 2, len(lens)).astype(np.int32))
    ref = dev(np.column_stack((rng.uniform(-80, 84, len(lens)), rng.uniform(-180, 180, len(lens)), rng.uniform(0, 100, len(lens)))))

    def fn():
        e, n, z, so = B.utm_forward_batch(d_lat, d_lon, d_off)
        e2, n2, _, _ = B.utm_forward_batch(d_lat, d_lon, d_off, zone, south)
        return e, n, z, so, e2, n2, B.utm_inverse_batch(e2, n2, d_off, zone, south), B.geodetic_to_enu_batch(d_lat, d_lon, d_alt, d_off, ref)
    hygiene.same_bytes_under_dirt(monkeypatch, B.context(), fn, dirt, rows_of=offs)


def test_ransac_poly_and_error_metric(B, monkeypatch, dirt):
    rng = np.random.default_rng(2)
    lens = [0, 3, 6, 7, 150, 40, 0, 750]
    offs = np.zeros(len(lens) + 1, np.int64); offs[1:] = np.cumsum(lens)
    T = int(offs[-1])
    t = np.concatenate([np.sort(rng.uniform(0, 15, n)) for n in lens]); y = 3.0 + 0.5 * t - 0.02 * t * t + rng.normal(size=T) * 0.5
    y[offs[4] + 7] += 80.0
    idx = np.stack([np.stack([rng.choice(max(n, 6), 6, replace=False) for _ in range(50)]) for n in lens]).astype(np.int32)
    d_t, d_y, d_off, d_idx = dev(t), dev(y), dev(offs), dev(idx)
    metric = []
    for N in (8, 271, 400, 401, 1536, 1537):                                    # both LDS forms and the all-pairs kernel
        ts_, pos_, _, gps_, val_, _, _ = planted_batch(16, N, 60 + N)
        val_[3] = 0; gps_[3] = np.nan                                           # a track with nothing to evaluate
        metric.append((dev(ts_), dev(pos_), dev(gps_), dev(val_.astype(np.uint8))))

    def fn():
        return [B.ransac_poly_batch(d_t, d_y, d_off, d_idx, 2, 10.0)] + [B.eval_errors_batch(*m, skip_seconds=sk) for m in metric for sk in (0.0, 5.0)]
    hygiene.same_bytes_under_dirt(monkeypatch, B.context(), fn, dirt)


def test_device_draws(B, monkeypatch, dirt):
    """np.random.choice and scikit-learn's sampler on all three routes, with streams whose population is below k"""
    import torch
    ctx = B.context()
    k, trials = 6, 20
    pops = {"one-wave": [271, 5, 6, 1000, 3, 64, 7, 28000] * 3, "chip-wide": [271, 5, 6, 1000, 3, 64, 7, 2040, 9]}
    for name, n in pops.items():
        st0 = B.mt19937_seed(np.arange(len(n)) + 11)
        idx = hygiene.same_bytes_under_dirt(monkeypatch, ctx, lambda st: B.mt19937_choice_batch(st, n, trials, k), dirt, states=(st0,))
        sets = idx.cpu().numpy()
        assert (sets[np.array(n) < k] == 0).all() and sets[0].any(), name          # a stream below k: untouched, its sets zero
    # permutation (0.01 < k/n < 0.99), tracking selection (k/n <= 0.01), n == k, and n < k (sets zero-filled: nothing excluded)
    n = [271, 750, 6, 5, 600, 601, 100000, 0, 64, 2_000_000_000, 7, 3]
    st0 = B.mt19937_seed(np.arange(len(n)) + 17)
    res = hygiene.same_bytes_under_dirt(monkeypatch, ctx, lambda st: B.sample_without_replacement_batch(st, n, trials, k), dirt, states=(st0,))
    assert (res[[3, 7, 11]] == 0).all()
    hygiene.same_bytes_under_dirt(monkeypatch, ctx, lambda: B.mt19937_seed(np.arange(40) + 5), dirt)


# ------------------------------------------------------------------------------------------------ 2. host-pointer entries
def test_host_pointer_entries(B, monkeypatch, dirt, run_inputs):
    """one per family: gsf_ekf_fuse_batch, gsf_run_fusion_ragged, gsf_utm_inverse -- staging arena and pinned mirror dirtied as well"""
    from gps_optimize_slam_amd import _lib
    from gps_optimize_slam_amd import ekfgpsslam as E
    L, hp, ctx = _lib.load(), _lib.hptr, B.context()
    nb, N = 64, 271
    ts, pos, quat, gps, valid, ip, iq = (np.ascontiguousarray(a) for a in planted_batch(nb, N, 91))
    valid = valid.astype(np.uint8)
    cfg = _lib.EkfConfig.from_config(E.CONFIG)

    def k4(alloc):
        po, qo, st = alloc.new((nb, N, 3), np.float64), alloc.new((nb, N, 4), np.float64), alloc.new((nb,), np.int32)
        _lib.check(L.gsf_ekf_fuse_batch(ctx.handle, 0, hp(ts), hp(pos), hp(quat), hp(gps), hp(valid), hp(ip), hp(iq), C.byref(cfg), nb, N, hp(po), hp(qo), hp(st)))
    hygiene.same_bytes_under_dirt(monkeypatch, ctx, k4, dirt, host=True)

    rng = np.random.default_rng(1)
    e, n = rng.uniform(2e5, 8e5, 5001), rng.uniform(1e5, 9.3e6, 5001)

    def inv(alloc):
        lat, lon = alloc.new(e.size, np.float64), alloc.new(e.size, np.float64)
        _lib.check(L.gsf_utm_inverse(ctx.handle, hp(e), hp(n), e.size, 33, 1, hp(lat), hp(lon)))
    hygiene.same_bytes_under_dirt(monkeypatch, ctx, inv, dirt, host=True)

    tracks, logs, gts = run_inputs
    rb = B.RaggedGeodeticBatch.from_host(tracks, logs, gts, device="cpu")
    h = {k: getattr(rb, k).numpy() for k in ("ts", "pos", "quat", "slam_offsets", "gps_t", "gps_llh", "gps_offsets", "gt_t", "gt_llh", "gt_offsets")}
    nb2, P, T, Tg = rb.B, h["ts"].size, h["gps_t"].size, h["gt_t"].size
    rc = _lib.RunConfig.from_config(_run_cfg(True))
    gf = _lib.PrefilterConfig.from_config(_run_cfg(True)["ground_truth_gps_filtering"])
    st0 = B.mt19937_seed(np.arange(nb2) + 100).cpu()

    def run(alloc, st):
        mt = st.numpy()
        f8, i4, u1 = np.float64, np.int32, np.uint8
        outs = [alloc.new(s, d) for s, d in (((nb2, 9), f8), ((nb2, 3), f8), (nb2, f8), ((P, 3), f8), ((P, 4), f8), (nb2, i4), (nb2, i4), (nb2, i4), (nb2, i4),
                                             ((T, 3), f8), (T, u1), ((P, 3), f8), (P, u1), ((P, 3), f8), (nb2, i4), (nb2, i4), ((Tg, 3), f8), (Tg, u1),
                                             ((P, 3), f8), (P, u1), ((2, 3, nb2, 4), f8), (nb2, i4), (nb2, i4), (P, u1), ((nb2, 2), i4))]
        with options(ctx, ransac_early_exit=1):
            _lib.check(L.gsf_run_fusion_ragged(ctx.handle, hp(h["ts"]), hp(h["pos"]), hp(h["quat"]), hp(h["slam_offsets"]), nb2, hp(h["gps_t"]), hp(h["gps_llh"]),
                                               hp(h["gps_offsets"]), hp(h["gt_t"]), hp(h["gt_llh"]), hp(h["gt_offsets"]), C.byref(rc), C.byref(gf), hp(mt),
                                               *[hp(o) for o in outs]))
        return outs
    outs = hygiene.same_bytes_under_dirt(monkeypatch, ctx, run, dirt, states=(st0,), host=True, rows_of=h["slam_offsets"])
    assert (outs[22] == 0).sum() >= 20 and (outs[22] != 0).sum() >= 3


# ------------------------------------------------------------------------------------------------ 3. side streams and two contexts
def flatten(res):
    """every tensor / array / bytes object inside a result, as host byte arrays, in a fixed order"""
    import torch
    if res is None:
        return [np.zeros(0, np.uint8)]
    if torch.is_tensor(res):
        return [res.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8).copy()]
    if isinstance(res, np.ndarray):
        return [np.ascontiguousarray(res).reshape(-1).view(np.uint8).copy()]
    if isinstance(res, (bytes, bytearray)):
        return [np.frombuffer(bytes(res), np.uint8).copy()]
    if isinstance(res, (list, tuple)):
        return [x for r in res for x in flatten(r)]
    if hasattr(res, "buf") and hasattr(res, "status"):                          # FusedPoses
        return flatten(res.buf) + flatten(res.status)
    if hasattr(res, "__dict__"):                                                # RunResult
        return [x for k in sorted(res.__dict__) for x in flatten(res.__dict__[k])]
    raise TypeError(type(res))


def same_flat(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.size == y.size and (x == y).all(), f"{what}: output {k} differs ({int((x != y).sum()) if x.size == y.size else 'size'} bytes)"


def stream_entries(B, orc_inputs):
    """name -> (host inputs -> device inputs, device inputs -> result), two input sets of different shapes per entry"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    tracks, logs, gts = orc_inputs

    def up(a):
        """H2D from pinned memory, asynchronous on the current stream"""
        t = torch.as_tensor(np.ascontiguousarray(a)).pin_memory()
        return t.to("cuda", non_blocking=True), t                               # (the pinned source is kept alive by the caller)

    def build_tm(host):
        keep, bt = [], B.TrajectoryBatch(0, host[0].shape[0], host[0].shape[1])
        for name, a in zip(("ts", "pos", "quat", "gps", "valid", "init_pos", "init_quat"), host):
            d, p = up(a.astype(np.uint8) if name == "valid" else a)
            keep.append(p)
            setattr(bt, name, d.clone())
        bt._keep = keep
        return bt

    def build_rb(host):
        tr, lg, gt = host
        cpu = B.RaggedGeodeticBatch.from_host(tr, lg, gt, device="cpu")
        keep, dv = [], {}
        for k in ("ts", "pos", "quat", "slam_offsets", "gps_t", "gps_llh", "gps_offsets", "gt_t", "gt_llh", "gt_offsets"):
            d, p = up(getattr(cpu, k).numpy())
            keep.append(p); dv[k] = d.clone()
        rb = B.RaggedGeodeticBatch(dv["ts"], dv["pos"], dv["quat"], dv["slam_offsets"], dv["gps_t"], dv["gps_llh"], dv["gps_offsets"], dv["gt_t"], dv["gt_llh"],
                                   dv["gt_offsets"], cpu.max_poses, cpu.max_fixes, cpu.gt_max_fixes)
        rb._keep = keep
        return rb

    def seeds(n):
        return B.mt19937_seed(np.arange(n) + 100)

    def robust(bt):
        bt.gps[::3, 40] += 30.0                                                 # tracks that never saturate
        return B.fuse_pipeline_robust_batch(bt, seeds(bt.B), return_info=True)

    def step7(rb):
        r = B.run_fusion_ragged(rb, seeds(rb.B), E.CONFIG)
        lla = B.utm_to_wgs84_ragged(r.fused.pos, rb.slam_offsets, r.zone, r.south, r.run_status)
        return (lla, B.tum_text_ragged(rb.ts, r.fused.pos, r.fused.quat, rb.slam_offsets, "utm", r.run_status),
                B.tum_text_ragged(rb.ts, lla, r.fused.quat, rb.slam_offsets, "wgs84", r.run_status))
    tm1, tm2 = planted_batch(256, 271, 5), planted_batch(100, 400, 6)
    rb1, rb2 = (tracks, logs, gts), (tracks[20:50], logs[20:50], gts[20:50])
    cfg = _run_cfg(True)
    return {"fuse_pipeline_batch": (build_tm, lambda bt: B.fuse_pipeline_batch(bt), tm1, tm2),
            "fuse_pipeline_robust_batch": (build_tm, robust, tm1, tm2),
            "run_fusion_ragged": (build_rb, lambda rb: B.run_fusion_ragged(rb, seeds(rb.B), cfg), rb1, rb2),
            "save_fusion_ragged-device-part": (build_rb, step7, rb1, rb2)}


STREAM_ENTRIES = ["fuse_pipeline_batch", "fuse_pipeline_robust_batch", "run_fusion_ragged", "save_fusion_ragged-device-part"]


def long_op():
    """something that keeps the current stream busy for longer than a launch takes to arrive: 2 x 8192^3 multiply-adds"""
    import torch
    a = torch.ones((8192, 8192), dtype=torch.float32, device="cuda")
    return a @ a


@pytest.mark.parametrize("entry", STREAM_ENTRIES)
def test_side_stream_equals_default_stream(B, run_inputs, entry):
    """inputs built on a side stream behind a long operation, so that they are still in flight when the call is issued; read back after
    synchronising that stream only"""
    import torch
    build, call, host, _ = stream_entries(B, run_inputs)[entry]
    ctx0 = B.context()
    want = flatten(call(build(host)))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        busy = long_op()
        inputs = build(host)
        assert B.context() is not ctx0
        res = call(inputs)
        s.synchronize()
        got = flatten(res)
    same_flat(want, got, f"{entry} on a side stream")
    ctx0.set_option("ransac_early_exit", 0)
    del busy


@pytest.mark.parametrize("entry", STREAM_ENTRIES)
def test_two_contexts_interleaved(B, run_inputs, entry):
    """call 1 on s1, call 2 on s2, call 1 on s1, call 2 on s2 -- different batches of different shapes, nothing synchronised in between:
    each result is what the same call gives alone"""
    import torch
    build, call, host1, host2 = stream_entries(B, run_inputs)[entry]
    in1, in2 = build(host1), build(host2)
    torch.cuda.synchronize()
    alone = []
    for inp in (in1, in2):
        fresh = build(host1 if inp is in1 else host2)                            # (the robust entry edits its input: a copy per call)
        alone.append(flatten(call(fresh)))
        torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    copies = [build(host1), build(host2), build(host1), build(host2)]
    torch.cuda.synchronize()
    res = []
    for k, st in enumerate((s1, s2, s1, s2)):
        with torch.cuda.stream(st):
            res.append(call(copies[k]))
    with torch.cuda.stream(s1):
        c1 = B.context()
    with torch.cuda.stream(s2):
        c2 = B.context()
    assert c1 is not c2 and c1 is not B.context()
    s1.synchronize(); s2.synchronize()
    for k in range(4):
        same_flat(alone[k % 2], flatten(res[k]), f"{entry}: call {k % 2 + 1}{chr(39) * (k // 2)} of the interleaved sequence")
    B.context().set_option("ransac_early_exit", 0)
