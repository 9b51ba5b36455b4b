"""The ragged whole-run entry's host side (no GPU): gsf_run_fusion_ragged[_dev] in header, library and ctypes table, its argument checks
before any device work, and RaggedGeodeticBatch.from_files against the drop-in's own loaders (load_slam_trajectory, load_gps_data)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsf_run_fusion_ragged_dev", "gsf_run_fusion_ragged")


@pytest.fixture(scope="module")
def lib():
    from gps_optimize_slam_amd import _lib
    if not os.path.exists(_lib.library_path()):
        pytest.skip("libgsf.so not built")
    return _lib


def test_ragged_symbols_in_header_library_and_table(lib):
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    L = C.CDLL(lib.library_path())
    for n in NEW:
        assert f"GSF_API int {n}(" in hdr and hasattr(L, n) and n in lib.SIGNATURES, n
    for name, v in (("GT_EMPTY", 32), ("GT_FEW", 64), ("GT_UNHANDLED", 128), ("SLAM_EMPTY", 256)):
        assert f"#define GSF_RUN_{name} {v}" in hdr and getattr(lib, f"RUN_{name}") == v
    # the dense entry's config struct is unchanged (test_capi_symbols pins every offset)
    assert C.sizeof(lib.RunConfig) == C.sizeof(lib.EkfConfig) + C.sizeof(lib.PrefilterConfig) + 4 * 8 + 4 * 4
    assert len(lib.SIGNATURES["gsf_run_fusion_ragged_dev"][1]) == 46 and len(lib.SIGNATURES["gsf_run_fusion_ragged"][1]) == 40


def _host_call(lib, slam_offsets, gps_offsets, gt_offsets=None, drop=None, gt_filter=None):
    """gsf_run_fusion_ragged with a NULL context handle replaced by a dummy one: every argument check runs before the context is touched"""
    from gps_optimize_slam_amd.ekfgpsslam import CONFIG
    L = lib.load()
    B = len(slam_offsets) - 1
    P, T = int(slam_offsets[-1]), int(gps_offsets[-1])
    Tg = int(gt_offsets[-1]) if gt_offsets is not None else 0
    z = lambda n, dt=np.float64: np.zeros(max(n, 1), dt)
    so, go = np.asarray(slam_offsets, np.int64), np.asarray(gps_offsets, np.int64)
    to = None if gt_offsets is None else np.asarray(gt_offsets, np.int64)
    rc = lib.RunConfig.from_config(CONFIG)
    gf = lib.PrefilterConfig.from_config(gt_filter or CONFIG["ground_truth_gps_filtering"])
    arrs = dict(ts=z(P), pos=z(P * 3), quat=z(P * 4), gps_t=z(T), gps_llh=z(T * 3), gt_t=z(Tg), gt_llh=z(Tg * 3), mt=z(B * 625, np.uint32),
                R=z(B * 9), t=z(B * 3), s=z(B), po=z(P * 3), qo=z(P * 4), st=z(B, np.int32), ni=z(B, np.int32), zone=z(B, np.int32),
                south=z(B, np.int32), utm=z(T * 3), keep=z(T, np.uint8), al=z(P * 3), va=z(P, np.uint8), sp=z(P * 3), gz=z(B, np.int32),
                gs=z(B, np.int32), gu=z(Tg * 3), gk=z(Tg, np.uint8), ga=z(P * 3), gv=z(P, np.uint8), err=z(B * 24), pr=z(B, np.int32),
                rs=z(B, np.int32), mask=z(P, np.uint8), info=z(B * 2, np.int32))
    if drop:
        arrs[drop] = None
    p = lambda k: lib.hptr(arrs[k])
    dummy = C.c_void_p(1)                                                     # never dereferenced when a check fails first
    return L.gsf_run_fusion_ragged(dummy, p("ts"), p("pos"), p("quat"), lib.hptr(so), B, p("gps_t"), p("gps_llh"), lib.hptr(go),
                                   p("gt_t") if to is not None else None, p("gt_llh") if to is not None else None, lib.hptr(to), C.byref(rc),
                                   C.byref(gf), p("mt"), p("R"), p("t"), p("s"), p("po"), p("qo"), p("st"), p("ni"), p("zone"), p("south"),
                                   p("utm"), p("keep"), p("al"), p("va"), p("sp"), p("gz"), p("gs"), p("gu"), p("gk"), p("ga"), p("gv"),
                                   p("err"), p("pr"), p("rs"), p("mask"), p("info"))


def test_ragged_host_entry_rejects_bad_offsets_before_the_device(lib):
    GSF_ERR_INVALID_ARG = 1
    assert _host_call(lib, [0, 5, 3], [0, 4, 8]) == GSF_ERR_INVALID_ARG                      # decreasing slam_offsets
    assert "slam_offsets" in lib.last_error()
    assert _host_call(lib, [0, 5, 9], [0, 6, 4]) == GSF_ERR_INVALID_ARG                      # decreasing gps_offsets
    assert "gps_offsets" in lib.last_error()
    assert _host_call(lib, [0, 5, 9], [0, 4, 8], [0, 3, 1]) == GSF_ERR_INVALID_ARG           # decreasing gt_offsets
    assert "gt_offsets" in lib.last_error()
    assert _host_call(lib, [0, 28001, 28005], [0, 4, 8]) == GSF_ERR_INVALID_ARG              # a track over 28 000 poses
    assert "28000" in lib.last_error()
    assert _host_call(lib, [0, 5, 9], [0, 14001, 14002]) == GSF_ERR_INVALID_ARG              # a log over 14 000 fixes
    assert "14000" in lib.last_error()
    for k in ("ts", "pos", "quat", "mt", "R", "err", "rs", "gps_llh"):                         # a NULL required array
        assert _host_call(lib, [0, 5, 9], [0, 4, 8], drop=k) == GSF_ERR_INVALID_ARG, k
        assert "NULL" in lib.last_error(), k
    assert _host_call(lib, [0, 5, 9], [0, 4, 8], [0, 3, 3], drop="gt_llh") == GSF_ERR_INVALID_ARG
    assert "ground-truth" in lib.last_error()
    assert _host_call(lib, [0, 5, 9], [0, 4, 8], [0, 14001, 14003]) == GSF_ERR_INVALID_ARG   # a ground-truth log over 14 000 fixes
    assert "14000" in lib.last_error()
    # an unusable ground-truth filter fails the call before the primary pre-filter could draw
    from gps_optimize_slam_amd.ekfgpsslam import CONFIG
    for bad in (dict(max_trials=0), dict(min_samples=40), dict(polynomial_degree=5)):
        assert _host_call(lib, [0, 5, 9], [0, 4, 8], [0, 3, 6], gt_filter=dict(CONFIG["ground_truth_gps_filtering"], **bad)) == GSF_ERR_INVALID_ARG, bad
        assert "pre-filter" in lib.last_error(), bad


def test_run_fusion_ragged_fails_loudly_without_gpu(lib):
    """a well-formed batch handed to run_fusion_ragged without a GPU: an error, never a host fall-back"""
    import torch
    from gps_optimize_slam_amd import batch
    if lib.load().gsf_device_count() > 0 or torch.cuda.is_available():
        pytest.skip("a GPU is present")
    slam, gps, gt = _write_files_like()
    rb = batch.RaggedGeodeticBatch.from_host(slam, gps, gt, device="cpu")
    st = torch.zeros((rb.B, 625), dtype=torch.int32)
    with pytest.raises(lib.GsfError, match="GPU"):
        batch.run_fusion_ragged(rb, st)


def _write_files_like():
    rng = np.random.default_rng(4)
    tracks, logs, gts = [], [], []
    for n, m in ((30, 9), (12, 4)):
        q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        tracks.append((np.arange(n) * 0.1, rng.normal(size=(n, 3)), q))
        logs.append(np.column_stack((np.arange(m) * 0.3, 49 + rng.uniform(0, 1e-3, m), 8.4 + rng.uniform(0, 1e-3, m), rng.uniform(100, 120, m))))
        gts.append(logs[-1][::2])
    return tracks, logs, gts


def test_ragged_batch_sizes_come_from_the_offsets(lib):
    """RaggedGeodeticBatch reads max_poses / max_fixes / gt_max_fixes from the offsets when they are left out, refuses sizes below the longest
    track or log, and run_fusion_ragged refuses a batch whose sizes were lowered afterwards -- before any device work"""
    import torch
    from gps_optimize_slam_amd import batch
    tracks, logs, gts = _write_files_like()
    rb = batch.RaggedGeodeticBatch.from_host(tracks, logs, gts, device="cpu")
    kw = dict(gt_t=rb.gt_t, gt_llh=rb.gt_llh, gt_offsets=rb.gt_offsets)
    args = (rb.ts, rb.pos, rb.quat, rb.slam_offsets, rb.gps_t, rb.gps_llh, rb.gps_offsets)
    r2 = batch.RaggedGeodeticBatch(*args, **kw)
    assert (r2.max_poses, r2.max_fixes, r2.gt_max_fixes) == (30, 9, 5) == (rb.max_poses, rb.max_fixes, rb.gt_max_fixes)
    assert batch.RaggedGeodeticBatch(*args, max_poses=40, **kw).max_poses == 40
    for bad in (dict(max_poses=29), dict(max_fixes=0), dict(gt_max_fixes=4)):
        with pytest.raises(ValueError, match="below the longest"):
            batch.RaggedGeodeticBatch(*args, **kw, **bad)
    with pytest.raises(ValueError, match="slam_offsets"):
        batch.RaggedGeodeticBatch(rb.ts, rb.pos, rb.quat, torch.tensor([0, 43, 42]), rb.gps_t, rb.gps_llh, rb.gps_offsets)
    with pytest.raises(ValueError, match="gps_offsets"):
        batch.RaggedGeodeticBatch(rb.ts, rb.pos, rb.quat, rb.slam_offsets, rb.gps_t, rb.gps_llh, torch.tensor([0, 14, 13]))
    r2.max_poses = 1
    with pytest.raises(ValueError, match="max_poses"):
        batch.run_fusion_ragged(r2, torch.zeros((2, 625), dtype=torch.int32))


def _write_files(tmp_path):
    rng = np.random.default_rng(3)
    slam, gps, gt = [], [], []
    for k, (n, m, delim) in enumerate(((40, 12, " "), (1, 1, ","), (17, 5, ","), (63, 20, " "))):
        ts = np.sort(rng.uniform(0, 100, n))
        q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        rows = np.column_stack((ts, rng.normal(size=(n, 3)), q))
        ps = tmp_path / f"slam{k}.txt"; np.savetxt(ps, rows, fmt="%.9f")
        log = np.column_stack((np.sort(rng.uniform(0, 100, m)), 49 + rng.uniform(0, 1e-3, m), 8.4 + rng.uniform(0, 1e-3, m), rng.uniform(100, 120, m)))
        pg = tmp_path / f"gps{k}.txt"; np.savetxt(pg, log, fmt="%.10f", delimiter=delim)
        pt = tmp_path / f"gt{k}.txt"; np.savetxt(pt, log[::-1][:max(1, m // 2)][::-1], fmt="%.10f", delimiter=delim)
        slam.append(str(ps)); gps.append(str(pg)); gt.append(str(pt) if k != 2 else None)
    return slam, gps, gt


def test_from_files_reads_what_the_drop_in_loaders_read(tmp_path):
    from gps_optimize_slam_amd import batch
    from gps_optimize_slam_amd import ekfgpsslam as E
    slam, gps, gt = _write_files(tmp_path)
    rb = batch.RaggedGeodeticBatch.from_files(slam, gps, gt, device="cpu")
    so, go, to = rb.slam_offsets.numpy(), rb.gps_offsets.numpy(), rb.gt_offsets.numpy()
    assert rb.B == 4 and rb.max_poses == 63 and rb.max_fixes == 20 and rb.gt_max_fixes == 10
    for b in range(4):
        d = E.load_slam_trajectory(slam[b])
        np.testing.assert_array_equal(rb.ts.numpy()[so[b]:so[b + 1]], d["timestamps"])
        np.testing.assert_array_equal(rb.pos.numpy()[so[b]:so[b + 1]], d["positions"])
        np.testing.assert_array_equal(rb.quat.numpy()[so[b]:so[b + 1]], d["quaternions"])
        for path, t_, llh, o in ((gps[b], rb.gps_t, rb.gps_llh, go), (gt[b], rb.gt_t, rb.gt_llh, to)):
            if path is None:
                assert o[b + 1] == o[b]; continue
            try:
                raw = np.loadtxt(path, delimiter=" ")                                       # load_gps_data's own reading (ref :252-254)
            except ValueError:
                raw = np.loadtxt(path, delimiter=",")
            raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
            np.testing.assert_array_equal(t_.numpy()[o[b]:o[b + 1]], raw[:, 0])
            np.testing.assert_array_equal(llh.numpy()[o[b]:o[b + 1]], raw[:, 1:4])
    assert int(rb.ts.numel()) == 40 + 1 + 17 + 63


def test_from_files_names_the_bad_file(tmp_path):
    from gps_optimize_slam_amd import batch
    slam, gps, gt = _write_files(tmp_path)
    bad = tmp_path / "bad_slam.txt"; bad.write_text("1 2 3\n4 5 6\n")
    with pytest.raises(ValueError, match="bad_slam.txt"):
        batch.RaggedGeodeticBatch.from_files([slam[0], str(bad)], gps[:2], device="cpu")
    badg = tmp_path / "bad_gnss.txt"; badg.write_text("1;2;3;4\n")
    with pytest.raises(ValueError, match="bad_gnss.txt"):
        batch.RaggedGeodeticBatch.from_files(slam[:2], [gps[0], str(badg)], device="cpu")
    with pytest.raises(ValueError, match="missing_gt.txt"):
        batch.RaggedGeodeticBatch.from_files(slam[:2], gps[:2], [None, str(tmp_path / "missing_gt.txt")], device="cpu")
