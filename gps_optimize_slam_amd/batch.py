"""Batched device entry points: B independent trajectories resident in HBM as torch tensors.

torch is plumbing here (device memory, the current HIP stream, torch.distributed for the N>1
collect); every numerical stage is a libgsf.so kernel launched on torch's current stream.
Additions to the reference's surface (which is single-trajectory): `*_batch` functions taking
(B, N, .) trajectory-major or (N, ., B) time-major tensors -- SURVEY 8(b).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import LAYOUT_TIME_MAJOR, LAYOUT_TRAJ_MAJOR, EkfConfig, GsfError, check  # noqa: F401
from .ekfgpsslam import CONFIG

_ctxs = {}


def context(device=None):
    """gsf context bound to torch's CURRENT stream on `device` (cached per device/stream)."""
    if not torch.cuda.is_available():
        raise GsfError("torch sees no GPU: the batched fusion path needs an MI355X (no CPU fallback)")
    dev = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (dev, stream)
    if key not in _ctxs:
        _ctxs[key] = _lib.Context(dev, stream)
    return _ctxs[key]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype, shape, name):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{name}: expected contiguous cuda {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def shapes(layout, B, N):
    """tensor shapes of (ts, pos, quat, gps, valid) for a layout"""
    if layout == LAYOUT_TIME_MAJOR:
        return (N, B), (N, 3, B), (N, 4, B), (N, 3, B), (N, B)
    return (B, N), (B, N, 3), (B, N, 4), (B, N, 3), (B, N)


class TrajectoryBatch:
    """B trajectories x N poses on one GPU: original SLAM track + time-aligned GNSS (+ Sim3-aligned first pose)."""

    def __init__(self, layout, B, N, device="cuda"):
        self.layout, self.B, self.N = int(layout), int(B), int(N)
        s_ts, s_pos, s_quat, s_gps, s_val = shapes(layout, B, N)
        f = dict(dtype=torch.float64, device=device)
        self.ts, self.pos, self.quat, self.gps = torch.empty(s_ts, **f), torch.empty(s_pos, **f), torch.empty(s_quat, **f), torch.empty(s_gps, **f)
        self.valid = torch.empty(s_val, dtype=torch.uint8, device=device)
        self.init_pos, self.init_quat = torch.empty((B, 3), **f), torch.empty((B, 4), **f)

    @classmethod
    def synthetic(cls, B, N, layout=LAYOUT_TIME_MAJOR, seed=20250523, traj0=0, device="cuda", variant=0):
        """Deterministic KITTI-04-shaped batch generated on the device (gsf_synth_batch_dev).  variant 0: white 2 cm noise on
        the SLAM positions (the default workload); variant 1: SURVEY 8d to the letter -- a random-walk drift of 2 cm per pose and the
        sharp-turn burst on 5 % of the tracks."""
        b = cls(layout, B, N, device)
        ctx = context()
        previous = ctx.options.get("synth_variant", 0)
        ctx.set_option("synth_variant", int(variant))
        try:
            check(_lib.load().gsf_synth_batch_dev(ctx.handle, b.layout, C.c_uint64(seed), int(traj0), b.B, b.N, _p(b.ts), _p(b.pos),
                                                  _p(b.quat), _p(b.gps), _p(b.valid), _p(b.init_pos), _p(b.init_quat)))
        finally:
            ctx.set_option("synth_variant", previous)
        return b

    @classmethod
    def replicated(cls, ts, pos, quat, gps, valid, B, gnss_sigma=0.45, seed=0, layout=LAYOUT_TRAJ_MAJOR, device="cuda"):
        """B copies of ONE real track (ts (N,), pos (N,3), quat (N,4), time-aligned gps (N,3) with NaN where invalid, valid (N,)) with
        independent white GNSS noise of gnss_sigma metres per copy (copy 0 keeps the fixes as they are) -- e.g. the bundled KITTI-04
        track of config C1 as a batch.  init_pos / init_quat are pose 0 of the track (placeholders: the fused pipeline fits its own)."""
        import numpy as np
        ts, pos, quat, gps = (np.asarray(a, dtype=np.float64) for a in (ts, pos, quat, gps))
        N = ts.shape[0]
        rng = np.random.default_rng(seed)
        g = np.repeat(gps[None], B, axis=0)
        noise = rng.normal(scale=gnss_sigma, size=(B, N, 3)); noise[0] = 0.0
        g = g + noise
        rep = lambda a: np.repeat(np.asarray(a)[None], B, axis=0)
        return cls.from_host(rep(ts), rep(pos), rep(quat), g, rep(np.asarray(valid).astype(np.uint8)), rep(pos[0]), rep(quat[0]), layout=layout, device=device)

    @classmethod
    def from_host(cls, ts, pos, quat, gps, valid, init_pos, init_quat, layout=LAYOUT_TRAJ_MAJOR, device="cuda"):
        """(B,N,.) trajectory-major host arrays -> device batch in `layout`."""
        B, N = ts.shape
        tm = cls(LAYOUT_TRAJ_MAJOR, B, N, device)
        for name, arr in (("ts", ts), ("pos", pos), ("quat", quat), ("gps", gps)):
            getattr(tm, name).copy_(torch.as_tensor(arr, dtype=torch.float64).reshape(getattr(tm, name).shape))
        tm.valid.copy_(torch.as_tensor(valid).to(torch.uint8).reshape(B, N))
        tm.init_pos.copy_(torch.as_tensor(init_pos, dtype=torch.float64).reshape(B, 3))
        tm.init_quat.copy_(torch.as_tensor(init_quat, dtype=torch.float64).reshape(B, 4))
        return tm if layout == LAYOUT_TRAJ_MAJOR else tm.to_layout(layout)

    def to_layout(self, layout):
        if layout == self.layout:
            return self
        o = TrajectoryBatch(layout, self.B, self.N, self.ts.device)
        L, h = _lib.load(), context().handle
        fn = L.gsf_transpose_to_time_major_dev if layout == LAYOUT_TIME_MAJOR else L.gsf_transpose_to_traj_major_dev
        for name, Cc, eb in (("ts", 1, 8), ("pos", 3, 8), ("quat", 4, 8), ("gps", 3, 8), ("valid", 1, 1)):
            check(fn(h, _p(getattr(self, name)), _p(getattr(o, name)), self.B, self.N, Cc, eb))
        o.init_pos.copy_(self.init_pos); o.init_quat.copy_(self.init_quat)
        return o

    def host_traj_major(self):
        """-> dict of (B,N,.) numpy arrays (for the oracle / file output)"""
        t = self.to_layout(LAYOUT_TRAJ_MAJOR)
        torch.cuda.synchronize()
        return {k: getattr(t, k).cpu().numpy() for k in ("ts", "pos", "quat", "gps", "valid", "init_pos", "init_quat")}


def _shift_stamps(t, offsets, tau, name):
    """t + tau[b] on every fix of log b (one double addition per fix, as dynamic_time_alignment's adjusted_gps_times, EKFGPSSLAM.py:338)"""
    B = int(offsets.numel()) - 1
    tau = torch.as_tensor(tau, dtype=torch.float64).to(t.device).reshape(-1)
    if tau.numel() == 1:
        tau = tau.expand(B)
    if tau.numel() != B:
        raise ValueError(f"{name}: expected one offset per track ({B}), got {tau.numel()}")
    counts = (offsets[1:] - offsets[:-1]).to(t.device)
    return t + torch.repeat_interleave(tau.contiguous(), counts)


class GeodeticBatch:
    """B trajectories x N poses whose GNSS side is still what the reference's loader reads (load_gps_data, EKFGPSSLAM.py:258):
    a ragged log of fixes with their own stamps, rows (lat deg, lon deg, alt m).  Input of fuse_from_geodetic()."""

    def __init__(self, B, N, ts, pos, quat, gps_offsets, gps_t, gps_llh, max_fixes):
        self.B, self.N, self.ts, self.pos, self.quat = int(B), int(N), ts, pos, quat
        self.gps_offsets, self.gps_t, self.gps_llh, self.max_fixes = gps_offsets, gps_t, gps_llh, int(max_fixes)
        self.slam_offsets = torch.arange(0, (self.B + 1) * self.N, self.N, dtype=torch.int64, device=ts.device)

    @classmethod
    def from_host(cls, ts, pos, quat, logs, device="cuda"):
        """B equal-length SLAM tracks (ts (B,N), pos (B,N,3), quat (B,N,4)) and their GNSS logs as the reference's loader reads them:
        logs = list of B arrays (n_b, >= 4) with columns stamp, col 1, col 2, col 3 of the text file (read as lat, lon, alt; ref :258)."""
        import numpy as np
        ts = np.asarray(ts, dtype=np.float64)
        Bn, N = ts.shape
        counts = np.array([len(l) for l in logs], dtype=np.int64)
        offs = np.zeros(Bn + 1, dtype=np.int64); offs[1:] = np.cumsum(counts)
        allr = np.concatenate([np.asarray(l, dtype=np.float64)[:, :4] for l in logs]) if counts.sum() else np.zeros((0, 4))
        f = dict(dtype=torch.float64, device=device)
        return cls(Bn, N, torch.as_tensor(ts, **f).contiguous(), torch.as_tensor(np.asarray(pos, dtype=np.float64), **f).contiguous(),
                   torch.as_tensor(np.asarray(quat, dtype=np.float64), **f).contiguous(), torch.as_tensor(offs, device=device),
                   torch.as_tensor(np.ascontiguousarray(allr[:, 0]), **f), torch.as_tensor(np.ascontiguousarray(allr[:, 1:4]), **f), int(counts.max(initial=0)))

    @classmethod
    def synthetic(cls, B, N, seed=20250523, traj0=0, device="cuda"):
        """Deterministic KITTI-04-shaped trajectories with a geodetic GNSS log around (49.0336 N, 8.3950 E)."""
        L, h = _lib.load(), context().handle
        f = dict(dtype=torch.float64, device=device)
        ts, pos, quat = torch.empty((B, N), **f), torch.empty((B, N, 3), **f), torch.empty((B, N, 4), **f)
        counts = torch.empty((B,), dtype=torch.int64, device=device)
        check(L.gsf_synth_geodetic_batch_dev(h, C.c_uint64(seed), int(traj0), B, N, None, None, None, _p(counts), None, None, None))
        offs = torch.zeros((B + 1,), dtype=torch.int64, device=device)
        offs[1:] = torch.cumsum(counts, 0)
        total, mx = int(offs[-1].item()), int(counts.max().item())      # sizing of the ragged log (host values, once per batch)
        gps_t, gps_llh = torch.empty((total,), **f), torch.empty((total, 3), **f)
        check(L.gsf_synth_geodetic_batch_dev(h, C.c_uint64(seed), int(traj0), B, N, _p(ts), _p(pos), _p(quat), None, _p(offs), _p(gps_t), _p(gps_llh)))
        return cls(B, N, ts, pos, quat, offs, gps_t, gps_llh, mx)


    def with_outliers(self, share, metres=40.0, seed=7):
        """A copy of the batch whose GNSS log has `share` of its fixes pushed `metres` north (multipath-like jumps the pre-filter is there
        for, ref :136-247); deterministic in `seed`.  SLAM side shared, log copied."""
        g = torch.Generator(device="cpu"); g.manual_seed(int(seed))
        hit = (torch.rand(self.gps_t.numel(), generator=g) < float(share)).to(self.gps_llh.device)
        llh = self.gps_llh.clone()
        llh[:, 0] += hit.double() * (float(metres) / 111320.0)
        return GeodeticBatch(self.B, self.N, self.ts, self.pos, self.quat, self.gps_offsets, self.gps_t, llh, self.max_fixes)


    def with_clock_offset(self, tau):
        """A copy of the batch whose GNSS stamps carry + tau[b] on every fix of log b (tau: (B,) or a scalar) -- the reference's way of
        applying a clock offset: GPSmerge.py:73-80 writes it into the stamps of the GNSS file.  SLAM side and fixes shared, stamps new."""
        return GeodeticBatch(self.B, self.N, self.ts, self.pos, self.quat, self.gps_offsets, _shift_stamps(self.gps_t, self.gps_offsets, tau, "tau"),
                             self.gps_llh, self.max_fixes)


FIT_ROWS_DEFAULT = "reference"


def fuse_from_geodetic(gb, config=None, out=None, fit_rows=FIT_ROWS_DEFAULT):
    """The whole path from the geodetic GNSS log on the device, no host round trip: geodesy slice (mask, zone pick, UTM forward,
    [E, N, alt] rows; ref :258-271) -> dynamic_time_alignment to the SLAM stamps (ref :325-387, :971) -> Umeyama on the rows
    main_process_gui picks (ref :973-998; fit_rows="all": on every valid row) -> Sim3 of pose 0 -> EKF+RTS (ref :1002-1010, plain
    fit).  Returns (FusedPoses, R, t, s, aux) with aux = dict(zone, south, utm_rows, aligned, valid)."""
    g = config or CONFIG
    context().set_sim3_rows(fit_rows, g)
    cfg = EkfConfig.from_config(g)
    L, h, dev = _lib.load(), context().handle, gb.ts.device
    f = dict(dtype=torch.float64, device=dev)
    utm = torch.empty_like(gb.gps_llh)
    zone, south = torch.empty((gb.B,), dtype=torch.int32, device=dev), torch.empty((gb.B,), dtype=torch.int32, device=dev)
    check(L.gsf_gps_rows_to_utm_batch_dev(h, _p(gb.gps_llh), _p(gb.gps_offsets), gb.B, _p(utm), _p(zone), _p(south)))
    aligned = torch.empty((gb.B, gb.N, 3), **f)
    valid = torch.empty((gb.B, gb.N), dtype=torch.uint8, device=dev)
    # (rows the loader removes -- lat/lon zero or out of range, ref :259-264 -- come out of the geodesy slice as NaN rows and are dropped
    # when the log is staged: the alignment sees the fixes load_gps_data would have returned)
    check(L.gsf_time_align_loaded_rows_batch_dev(h, _p(gb.ts), _p(gb.slam_offsets), _p(gb.gps_t), _p(utm), _p(gb.gps_offsets), gb.B, max(2, gb.max_fixes),
                                                 float(g["time_alignment"]["max_gps_gap_threshold"]), _p(aligned), _p(valid), None))
    out = out or FusedPoses(LAYOUT_TRAJ_MAJOR, gb.B, gb.N, dev)
    R, t, s = torch.empty((gb.B, 9), **f), torch.empty((gb.B, 3), **f), torch.empty((gb.B,), **f)
    check(L.gsf_fuse_pipeline_batch_dev(h, LAYOUT_TRAJ_MAJOR, _p(gb.ts), _p(gb.pos), _p(gb.quat), _p(aligned), _p(valid), C.byref(cfg), gb.B, gb.N,
                                        _p(R), _p(t), _p(s), _p(out.pos), _p(out.quat), _p(out.status)))
    return out, R, t, s, {"zone": zone, "south": south, "utm_rows": utm, "aligned": aligned, "valid": valid}


class RunResult:
    """What steps 1-6 of main_process_gui leave behind for B trajectories (run_fusion_batch): fused = FusedPoses, R / t / s, n_inliers,
    inlier_mask, trial_info (deciding trial, trials drawn), zone / south, gps_utm (NaN rows where the loader drops the fix), gps_keep (fixes
    that survive loader and pre-filter), aligned / valid (step 2), sim3_pos (step 4), err_stats (3, B, 4) = count / mean / median / RMSE of
    raw SLAM, Sim3, EKF against the primary GPS (step 6), run_status (B,) = RUN_* bits (0 = the reference's run completes)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def run_fusion_batch(gb, mt_state, config=None, early_exit=True, skip_seconds=5.0, max_windows=0, want_mask=True, projected=False, want_cov=False):
    """Steps 1-6 of main_process_gui (EKFGPSSLAM.py:959-1033) for the B trajectories of a GeodeticBatch as ONE device chain on torch's
    current stream: load-side geodesy (:258-271) -> GPS RANSAC pre-filter with its windows walked on the device (:275, :136-247) ->
    time alignment (:971) -> row choice (:973-998) -> robust Sim3 (:1002) -> apply (:1006) -> EKF + RTS (:1010) -> error metric (:1013-1033).
    mt_state (B, 625): every trajectory's NumPy legacy generator (mt19937_seed / mt19937_from_numpy), advanced by the pre-filter's and
    the fit's draws in the reference's order; early_exit as in fuse_pipeline_robust_batch (the pre-filter's draws are unaffected).
    projected=True: gb.gps_llh already holds (E, N, alt) rows -- what load_gps_data's projection returns -- and the chain starts at the
    pre-filter; zone / south are then None (there is no projector, as in run_fusion_ragged).  The pre-filter covers logs of any rate (scikit-learn's sampler on its permutation and tracking-selection routes); a log is
    flagged RUN_PREFILTER_UNHANDLED only for unsorted stamps in the sliding mode or more than max_windows windows.  Returns a RunResult."""
    g = config or CONFIG
    ctx = context()
    ctx.set_option("ransac_early_exit", 1 if early_exit else 0)
    rc = _lib.RunConfig.from_config(g, skip_seconds, max_windows)
    B, N, dev = gb.B, gb.N, gb.ts.device
    f = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    total = int(gb.gps_t.numel())
    out = FusedPoses(LAYOUT_TRAJ_MAJOR, B, N, dev)
    r = RunResult(fused=out, R=torch.empty((B, 9), **f), t=torch.empty((B, 3), **f), s=torch.empty((B,), **f), n_inliers=torch.empty((B,), **i32),
                  zone=None if projected else torch.empty((B,), **i32), south=None if projected else torch.empty((B,), **i32),
                  gps_utm=gb.gps_llh.clone() if projected else torch.empty((total, 3), **f),
                  gps_keep=torch.empty((total,), dtype=torch.uint8, device=dev), aligned=torch.empty((B, N, 3), **f),
                  valid=torch.empty((B, N), dtype=torch.uint8, device=dev), sim3_pos=torch.empty((B, N, 3), **f), err_stats=torch.empty((3, B, 4), **f),
                  run_status=torch.empty((B,), **i32), inlier_mask=torch.empty((B, N), dtype=torch.uint8, device=dev) if want_mask else None,
                  trial_info=torch.empty((B, 2), **i32))
    check(_lib.load().gsf_run_fusion_batch_dev(ctx.handle, _p(gb.ts), _p(gb.pos), _p(gb.quat), B, N, _p(gb.gps_t), None if projected else _p(gb.gps_llh), _p(gb.gps_offsets), total,
                                               int(gb.max_fixes), C.byref(rc), _p(mt_state), _p(r.R), _p(r.t), _p(r.s), _p(out.pos), _p(out.quat), _p(out.status),
                                               _p(r.n_inliers), _p(r.zone), _p(r.south), _p(r.gps_utm), _p(r.gps_keep), _p(r.aligned), _p(r.valid), _p(r.sim3_pos),
                                               _p(r.err_stats), _p(r.run_status), _p(r.inlier_mask), _p(r.trial_info)))
    if want_cov:                                                         # one more launch after the chain; r.cov = FusedCovariance over the B * N rows
        r.cov = ekf_covariance_ragged(gb.ts.view(B * N), gb.quat.view(B * N, 4), r.aligned.view(B * N, 3), r.valid.view(B * N), gb.slam_offsets,
                                      config=g, run_status=r.run_status)
    return r


def _read_slam_file(path):
    """rows of a TUM file exactly as load_slam_trajectory parses them (EKFGPSSLAM.py:110-125): (ts (n,), pos (n,3), quat (n,4))"""
    import numpy as np
    try:
        data = np.loadtxt(path)
        if data.ndim == 1:
            data = data.reshape(1, -1)
        if data.shape[1] != 8:
            raise ValueError(f"expected 8 columns (ts x y z qx qy qz qw), got {data.shape[1]}")
    except Exception as e:
        raise ValueError(f"SLAM file {path}: {e}") from e
    return data[:, 0].astype(float), data[:, 1:4].astype(float), data[:, 4:8].astype(float)


def _read_gnss_file(path):
    """rows of a GNSS text file exactly as load_gps_data reads them (EKFGPSSLAM.py:252-256): split on space, then on comma; (n, 4)"""
    import numpy as np
    try:
        try:
            raw = np.loadtxt(path, delimiter=" ")
        except ValueError:
            raw = np.loadtxt(path, delimiter=",")
        if raw.ndim == 1:
            raw = raw.reshape(1, -1)
        if raw.shape[1] < 4:
            raise ValueError(f"needs at least 4 columns (ts lat lon alt), got {raw.shape[1]}")
    except Exception as e:
        raise ValueError(f"GNSS file {path}: {e}") from e
    return np.ascontiguousarray(raw[:, :4], dtype=np.float64)


class RaggedGeodeticBatch:
    """B SLAM tracks of ANY lengths with their primary GNSS logs and optional ground-truth logs, as the reference's loaders read them:
    flat ts (P,), pos (P,3), quat (P,4) with slam_offsets (B+1,); fixes gps_t (T,), gps_llh (T,3) with gps_offsets (B+1,); ground truth
    gt_t / gt_llh / gt_offsets (None: no track has one; an empty range: that track has none).  max_poses / max_fixes / gt_max_fixes are
    host values that size the device workspace: the longest track / log, read here from the offsets (one small copy to the host per batch);
    a value given that is below it raises ValueError.  Input of run_fusion_ragged()."""

    def __init__(self, ts, pos, quat, slam_offsets, gps_t, gps_llh, gps_offsets, gt_t=None, gt_llh=None, gt_offsets=None, max_poses=None,
                 max_fixes=None, gt_max_fixes=None):
        self.ts, self.pos, self.quat, self.slam_offsets = ts, pos, quat, slam_offsets
        self.gps_t, self.gps_llh, self.gps_offsets = gps_t, gps_llh, gps_offsets
        self.gt_t, self.gt_llh, self.gt_offsets = gt_t, gt_llh, gt_offsets
        self.B = int(slam_offsets.numel()) - 1
        sizes = [self._longest(slam_offsets, max_poses, "slam_offsets", "max_poses", int(ts.numel())),
                 self._longest(gps_offsets, max_fixes, "gps_offsets", "max_fixes", int(gps_t.numel())),
                 (0, 0) if gt_offsets is None else self._longest(gt_offsets, gt_max_fixes, "gt_offsets", "gt_max_fixes", int(gt_t.numel()))]
        self._ranges = tuple(lo for lo, _ in sizes)                      # the longest ranges themselves (run_fusion_ragged checks against them)
        self.max_poses, self.max_fixes, self.gt_max_fixes = (v for _, v in sizes)

    def _longest(self, offsets, given, name, size_name, rows):
        """(longest range of `offsets`, the size to use): offsets must hold B+1 non-decreasing values from 0 to `rows`; `given` may not be below it"""
        o = offsets.detach().to("cpu", torch.int64)
        if o.numel() != self.B + 1:
            raise ValueError(f"{name}: expected {self.B + 1} values, got {o.numel()}")
        d = o[1:] - o[:-1]
        if int(o[0]) != 0 or int(o[-1]) != rows or (d < 0).any():
            raise ValueError(f"{name} must rise from 0 to {rows} (the rows given) without decreasing")
        longest = int(d.max()) if d.numel() else 0
        if given is None:
            return longest, longest
        if int(given) < longest:
            raise ValueError(f"{size_name} = {int(given)} is below the longest range of {name} ({longest}): it sizes the device workspace")
        return longest, int(given)

    @staticmethod
    def _flat(arrs, cols):
        import numpy as np
        counts = np.array([len(a) for a in arrs], dtype=np.int64)
        offs = np.zeros(len(arrs) + 1, dtype=np.int64); offs[1:] = np.cumsum(counts)
        rows = [np.asarray(a, dtype=np.float64).reshape(len(a), -1)[:, :cols] if len(a) else np.zeros((0, cols)) for a in arrs]
        flat = np.concatenate(rows) if counts.sum() else np.zeros((0, cols))
        return np.ascontiguousarray(flat), offs, int(counts.max(initial=0))

    @classmethod
    def from_host(cls, tracks, logs, gt_logs=None, device="cuda"):
        """tracks: list of B (ts (n_b,), pos (n_b,3), quat (n_b,4)); logs: B arrays (m_b, >= 4) = stamp, lat, lon, alt columns of the text file
        (ref :258); gt_logs: None, or B entries each None (no ground truth for that track) or such an array."""
        import numpy as np
        if len(logs) != len(tracks) or (gt_logs is not None and len(gt_logs) != len(tracks)):
            raise ValueError("tracks, logs and gt_logs must have one entry per track")
        rows = [np.column_stack((np.asarray(t_, np.float64).reshape(-1), np.asarray(p_, np.float64).reshape(-1, 3), np.asarray(q_, np.float64).reshape(-1, 4)))
                for t_, p_, q_ in tracks]
        slam, so, mp = cls._flat(rows, 8)
        g, go, mf = cls._flat(logs, 4)
        f = dict(dtype=torch.float64, device=device)
        tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), **f)
        gt_t = gt_llh = gt_o = None
        gmf = 0
        if gt_logs is not None:
            gl, gto, gmf = cls._flat([np.zeros((0, 4)) if l is None else l for l in gt_logs], 4)
            gt_t, gt_llh, gt_o = tt(gl[:, 0]), tt(gl[:, 1:4]), torch.as_tensor(gto, device=device)
        return cls(tt(slam[:, 0]), tt(slam[:, 1:4]), tt(slam[:, 4:8]), torch.as_tensor(so, device=device), tt(g[:, 0]), tt(g[:, 1:4]),
                   torch.as_tensor(go, device=device), gt_t, gt_llh, gt_o, mp, mf, gmf)

    @classmethod
    def from_files(cls, slam_paths, gps_paths, gt_paths=None, device="cuda"):
        """B SLAM (TUM) / GNSS / optional ground-truth GNSS files (an entry of gt_paths may be None), parsed exactly as load_slam_trajectory
        and load_gps_data parse them; ValueError naming the file on any unreadable one, before any device work."""
        if len(gps_paths) != len(slam_paths) or (gt_paths is not None and len(gt_paths) != len(slam_paths)):
            raise ValueError("slam_paths, gps_paths and gt_paths must have one entry per track")
        tracks = [_read_slam_file(p) for p in slam_paths]
        logs = [_read_gnss_file(p) for p in gps_paths]
        gts = None if gt_paths is None else [None if p is None else _read_gnss_file(p) for p in gt_paths]
        return cls.from_host(tracks, logs, gts, device=device)


    def with_clock_offset(self, tau, gt_tau=None):
        """A copy of the batch whose primary GNSS stamps carry + tau[b] on every fix of log b (tau: (B,) or a scalar) and, with gt_tau, whose
        ground-truth stamps carry + gt_tau[b] (None: the ground-truth log keeps its stamps -- it is another receiver's file) -- the reference's
        way of applying a clock offset: GPSmerge.py:73-80 writes it into the stamps of the GNSS file.  estimate_clock_offset ->
        with_clock_offset -> run_fusion_ragged is the whole workflow.  Everything but the stamps is shared with this batch."""
        gt_t = self.gt_t
        if gt_tau is not None:
            if self.gt_offsets is None:
                raise ValueError("with_clock_offset: gt_tau given, but the batch has no ground-truth log")
            gt_t = _shift_stamps(self.gt_t, self.gt_offsets, gt_tau, "gt_tau")
        return RaggedGeodeticBatch(self.ts, self.pos, self.quat, self.slam_offsets, _shift_stamps(self.gps_t, self.gps_offsets, tau, "tau"), self.gps_llh,
                                   self.gps_offsets, gt_t, self.gt_llh, self.gt_offsets, self.max_poses, self.max_fixes, self.gt_max_fixes)


def run_fusion_ragged(rb, mt_state, config=None, early_exit=True, skip_seconds=5.0, max_windows=0, want_mask=True, projected=False, want_cov=False):
    """Steps 1-6 of main_process_gui (EKFGPSSLAM.py:959-1075) for the tracks of a RaggedGeodeticBatch as ONE device chain
    (gsf_run_fusion_ragged_dev): the chain of run_fusion_batch on tracks of different lengths, plus the optional ground-truth log --
    loaded with config['ground_truth_gps_filtering'] (:964) between the primary pre-filter and the fit, so its draws come between theirs --
    and step 6 against it (:1035-1062).  mt_state (B, 625) as in run_fusion_batch.  projected=True: gps_llh / gt_llh hold (E, N, alt) rows
    already; zone / south / gt_zone / gt_south are then None.  The context's ransac_early_exit is restored afterwards.
    Returns a RunResult: per-pose fields flat over the P rows (fused.pos (P,3), fused.quat (P,4), aligned, valid, sim3_pos, inlier_mask,
    gt_aligned, gt_valid), slam_offsets / gps_offsets / gt_offsets, gt_utm / gt_keep, err_stats (2, 3, B, 4) = {primary, ground truth} x
    {raw SLAM, Sim3, EKF} x {count, mean, median, RMSE}, plot_ref (B,) = 0 none / 1 primary / 2 ground truth (:1064-1075), run_status.
    Both pre-filters cover logs of any rate; RUN_PREFILTER_UNHANDLED / RUN_GT_UNHANDLED flag only unsorted stamps in the sliding mode or
    more than max_windows windows."""
    # the host-known sizes first, before any device work: below the longest track / log they would undersize the workspace
    for v, lo, name in zip((rb.max_poses, rb.max_fixes, rb.gt_max_fixes), rb._ranges, ("max_poses", "max_fixes", "gt_max_fixes")):
        if int(v) < lo:
            raise ValueError(f"run_fusion_ragged: {name} = {int(v)} is below the longest range of the batch ({lo})")
    if rb.max_poses > 28000 or rb.max_fixes > 14000 or rb.gt_max_fixes > 14000:
        raise ValueError("run_fusion_ragged: at most 28 000 poses per track and 14 000 fixes per log")
    g = config or CONFIG
    ctx = context()
    rc = _lib.RunConfig.from_config(g, skip_seconds, max_windows)
    gtf = _lib.PrefilterConfig.from_config(g["ground_truth_gps_filtering"], max_windows)
    B, dev = rb.B, rb.ts.device
    P, T = int(rb.ts.numel()), int(rb.gps_t.numel())
    has_gt = rb.gt_offsets is not None
    Tg = int(rb.gt_t.numel()) if has_gt else 0
    f = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    out = FusedPoses(LAYOUT_TRAJ_MAJOR, 1, P, dev, status=torch.empty((B,), **i32))
    out.pos, out.quat = out.pos.view(P, 3), out.quat.view(P, 4)
    r = RunResult(fused=out, R=torch.empty((B, 9), **f), t=torch.empty((B, 3), **f), s=torch.empty((B,), **f), n_inliers=torch.empty((B,), **i32),
                  zone=None if projected else torch.empty((B,), **i32), south=None if projected else torch.empty((B,), **i32),
                  gps_utm=rb.gps_llh.clone() if projected else torch.empty((T, 3), **f), gps_keep=torch.empty((T,), **u8),
                  aligned=torch.empty((P, 3), **f), valid=torch.empty((P,), **u8), sim3_pos=torch.empty((P, 3), **f),
                  gt_zone=torch.empty((B,), **i32) if has_gt and not projected else None, gt_south=torch.empty((B,), **i32) if has_gt and not projected else None,
                  gt_utm=(rb.gt_llh.clone() if projected else torch.empty((Tg, 3), **f)) if has_gt else None,
                  gt_keep=torch.empty((Tg,), **u8) if has_gt else None, gt_aligned=torch.empty((P, 3), **f) if has_gt else None,
                  gt_valid=torch.empty((P,), **u8) if has_gt else None, err_stats=torch.empty((2, 3, B, 4), **f), plot_ref=torch.empty((B,), **i32),
                  run_status=torch.empty((B,), **i32), inlier_mask=torch.empty((P,), **u8) if want_mask else None, trial_info=torch.empty((B, 2), **i32),
                  slam_offsets=rb.slam_offsets, gps_offsets=rb.gps_offsets, gt_offsets=rb.gt_offsets)
    saved = ctx.options.get("ransac_early_exit", 0)
    ctx.set_option("ransac_early_exit", 1 if early_exit else 0)
    try:
        check(_lib.load().gsf_run_fusion_ragged_dev(
            ctx.handle, _p(rb.ts), _p(rb.pos), _p(rb.quat), _p(rb.slam_offsets), B, P, rb.max_poses, _p(rb.gps_t), None if projected else _p(rb.gps_llh),
            _p(rb.gps_offsets), T, rb.max_fixes, _p(rb.gt_t) if has_gt else None, None if (projected or not has_gt) else _p(rb.gt_llh), _p(rb.gt_offsets),
            Tg, rb.gt_max_fixes, C.byref(rc), C.byref(gtf), _p(mt_state), _p(r.R), _p(r.t), _p(r.s), _p(out.pos), _p(out.quat), _p(out.status),
            _p(r.n_inliers), _p(r.zone), _p(r.south), _p(r.gps_utm), _p(r.gps_keep), _p(r.aligned), _p(r.valid), _p(r.sim3_pos), _p(r.gt_zone),
            _p(r.gt_south), _p(r.gt_utm), _p(r.gt_keep), _p(r.gt_aligned), _p(r.gt_valid), _p(r.err_stats), _p(r.plot_ref), _p(r.run_status),
            _p(r.inlier_mask), _p(r.trial_info)))
    finally:
        ctx.set_option("ransac_early_exit", saved)
    if want_cov:                                                         # one more launch after the chain; r.cov = FusedCovariance over the P rows
        r.cov = ekf_covariance_ragged(rb.ts, rb.quat, r.aligned, r.valid, rb.slam_offsets, config=g, run_status=r.run_status)
    return r


class ClockOffset:
    """Result of estimate_clock_offset for B tracks x K candidates: J (B, K) = RMSE in metres of the Sim3 fit with the GNSS clock shifted by
    tau (B, K) (NaN: no fit), n_rows (B, K) int32 = rows of that fit, best_k (B,) int32 = first arg-min of J (-1: none), tau_best (B,) =
    tau[b, best_k], tau_refined (B,) = vertex of the parabola through J^2 at best_k and its neighbours (tau_best where that does not apply),
    R (B, 9) / t (B, 3) / s (B,) = the fit of best_k, status (B,) int32 = _lib.CLK_NONE | CLK_AT_EDGE (widen the grid) | CLK_FLAT (the offset
    is not observable on this track)."""

    def __init__(self, J, n_rows, best_k, tau_best, tau_refined, R, t, s, status, tau):
        self.J, self.n_rows, self.best_k, self.tau_best, self.tau_refined = J, n_rows, best_k, tau_best, tau_refined
        self.R, self.t, self.s, self.status, self.tau = R, t, s, status, tau


def estimate_clock_offset(rb_or_arrays, tau0=None, dtau=0.05, K=41, config=None, run=None, min_rows=0, flat_threshold=0.0, fit_rows=FIT_ROWS_DEFAULT):
    """The offset between the SLAM clock and the GNSS clock of B tracks, searched on the device (gsf_clock_offset_search_dev): for every
    candidate tau[b, k] = tau0[b] + k * dtau the fixes are re-stamped t + tau (dynamic_time_alignment's adjusted_gps_times,
    EKFGPSSLAM.py:337-338), aligned to the SLAM stamps (:325-387), the rows of main_process_gui's fit are picked (:973-998; fit_rows="all":
    every valid row) and compute_sim3_transform (:428-459) is scored by its RMSE.  The reference itself has no such step: its
    estimate_time_offset is identically 0 and the number is typed in (GPSmerge.py:73-80).
    rb_or_arrays: a RaggedGeodeticBatch / GeodeticBatch, or device tensors (ts (P,), pos (P,3), slam_offsets (B+1,), gps_t (T,),
    gps_utm (T,3) = (E, N, alt) rows with NaN easting and northing on dropped fixes, gps_offsets (B+1,)[, gps_keep (T,) uint8]).
    run: the RunResult of a whole run of that batch at offset 0 -- its gps_utm / gps_keep are used, i.e. the fixes its pre-filter kept;
    without it a batch is projected here (gsf_gps_rows_to_utm_batch_dev) and every fix the loader keeps is used.
    tau0 (B,) / scalar / None = 0; min_rows <= 0: the row rule's min_samples; flat_threshold in metres (<= 0: CLK_FLAT is never set).
    Asynchronous on torch's current stream.  Returns a ClockOffset."""
    g = config or CONFIG
    ctx = context()
    L = _lib.load()
    keep = None
    if isinstance(rb_or_arrays, (tuple, list)):
        ts, pos, so, gps_t, utm, go = rb_or_arrays[:6]
        keep = rb_or_arrays[6] if len(rb_or_arrays) > 6 else None
        max_fixes = None
    else:
        b = rb_or_arrays
        ts, pos, so, gps_t, go, max_fixes = b.ts.reshape(-1), b.pos.reshape(-1, 3), b.slam_offsets, b.gps_t, b.gps_offsets, int(b.max_fixes)
        utm = None if run is not None else b.gps_llh
    B = _offsets_chk(so)
    if _offsets_chk(go) != B:
        raise ValueError("estimate_clock_offset: slam_offsets and gps_offsets must describe the same number of tracks")
    dev = ts.device
    if run is not None:
        utm, keep = run.gps_utm, run.gps_keep
    elif not isinstance(rb_or_arrays, (tuple, list)):
        llh, utm = utm, torch.empty_like(utm)
        zone, south = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        check(L.gsf_gps_rows_to_utm_batch_dev(ctx.handle, _p(llh), _p(go), B, _p(utm), _p(zone), _p(south)))
    P, T = int(ts.numel()), int(gps_t.numel())
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos")
    _chk(gps_t, torch.float64, (T,), "gps_t"); _chk(utm, torch.float64, (T, 3), "gps_utm")
    if keep is not None:
        _chk(keep, torch.uint8, (T,), "gps_keep")
    if max_fixes is None:
        max_fixes = int((go[1:] - go[:-1]).max().item()) if B else 0          # sizing of the staging (a host value, once per call)
    K = int(K)
    if not 1 <= K <= 4096:
        raise ValueError(f"estimate_clock_offset: K must be in 1..4096, got {K}")
    f = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    if tau0 is not None:
        tau0 = torch.as_tensor(tau0, dtype=torch.float64).to(dev).reshape(-1)
        tau0 = (tau0.expand(B) if tau0.numel() == 1 else tau0).contiguous()
        _chk(tau0, torch.float64, (B,), "tau0")
    ctx.set_sim3_rows(fit_rows, g)
    r = ClockOffset(J=torch.empty((B, K), **f), n_rows=torch.empty((B, K), **i32), best_k=torch.empty((B,), **i32), tau_best=torch.empty((B,), **f),
                    tau_refined=torch.empty((B,), **f), R=torch.empty((B, 9), **f), t=torch.empty((B, 3), **f), s=torch.empty((B,), **f),
                    status=torch.empty((B,), **i32),
                    tau=(torch.zeros((B, 1), **f) if tau0 is None else tau0[:, None]) + torch.arange(K, **f)[None, :] * float(dtau))
    check(L.gsf_clock_offset_search_dev(ctx.handle, _p(ts), _p(pos), _p(so), _p(gps_t), _p(utm), _p(keep), _p(go), B, max_fixes, _p(tau0), float(dtau), K,
                                        float(g["time_alignment"]["max_gps_gap_threshold"]), int(min_rows), float(flat_threshold), _p(r.J), _p(r.n_rows),
                                        _p(r.best_k), _p(r.tau_best), _p(r.tau_refined), _p(r.R), _p(r.t), _p(r.s), _p(r.status)))
    return r


# ---------------------------------------------------------------------------- step 7 (EKFGPSSLAM.py:1085-1104) for ragged runs
TEXT_GROUP_BYTES = 256 << 20        # save_fusion_ragged: text of one group of tracks = one device buffer and one copy into pinned memory
_TUM_FORMATS = {"utm": _lib.TUM_UTM, "wgs84": _lib.TUM_WGS84}


def corrected_utm_name(slam_path):
    """The default name main_process_gui offers for the corrected track (ref :1087-1088): the SLAM file's base name with '.txt' ->
    '_corrected_utm.txt', or '_corrected_utm.txt' appended."""
    base = str(slam_path).split("/")[-1].split("\\")[-1]
    return base.replace(".txt", "_corrected_utm.txt") if ".txt" in base else base + "_corrected_utm.txt"


def _offsets_chk(offsets):
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or not offsets.is_cuda or offsets.numel() < 1:
        raise ValueError("offsets: expected a contiguous cuda int64 tensor of B+1 values")
    return int(offsets.numel()) - 1


def utm_to_wgs84_ragged(pos, offsets, zone, south, run_status=None):
    """utm_to_wgs84(corrected_pos, projector) (ref :1097, :291-296) for ragged tracks: pos (P, 3) rows [E, N, alt], offsets (B+1,) int64, zone /
    south (B,) int32 = the primary log's projector (RunResult.zone / .south).  Returns (P, 3) rows [lon, lat, alt]; lon / lat are bit for bit
    what the drop-in's UtmProjector(zone, south)(E, N, inverse=True) returns.  run_status (B,) int32 or None: tracks with run_status != 0 get
    NaN rows (their zone / south are not read)."""
    B = _offsets_chk(offsets)
    P = int(pos.shape[0]) if pos.dim() == 2 else -1
    _chk(pos, torch.float64, (P, 3), "pos")
    if zone is None or south is None:
        raise ValueError("utm_to_wgs84_ragged: zone / south are None (projected input has no projector, ref :1096)")
    _chk(zone, torch.int32, (B,), "zone"); _chk(south, torch.int32, (B,), "south")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    out = torch.empty((P, 3), dtype=torch.float64, device=pos.device)
    check(_lib.load().gsf_utm_to_wgs84_rows_dev(context().handle, _p(pos), _p(offsets), _p(zone), _p(south), _p(run_status), B, _p(out)))
    return out


def _text_args(ts, xyz, quat, offsets, run_status):
    B = _offsets_chk(offsets)
    P = int(ts.numel())
    _chk(ts, torch.float64, (P,), "ts"); _chk(xyz, torch.float64, (P, 3), "xyz"); _chk(quat, torch.float64, (P, 4), "quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    return B, P


def _text_sizes(form, ts, xyz, quat, offsets, run_status, B, P):
    """the size call of gsf_tum_text_dev: (text_offsets (B+1,) int64, track_state (B,) int32) on the device"""
    text_offsets = torch.empty((B + 1,), dtype=torch.int64, device=ts.device)
    state = torch.empty((max(B, 1),), dtype=torch.int32, device=ts.device)
    check(_lib.load().gsf_tum_text_dev(context().handle, form, _p(ts), _p(xyz), _p(quat), _p(offsets), _p(run_status), B, P, _p(text_offsets),
                                       _p(state), None))
    return text_offsets, state[:B]


def _savetxt_track(form, path, ts, xyz, quat, lo, hi):
    """the drop-in's writer on one track's rows (tracks whose values the device does not cover, track_state 2)"""
    from . import ekfgpsslam as E
    writer = E.save_tum_utm if form == _lib.TUM_UTM else E.save_tum_wgs84
    writer(path, ts[lo:hi].cpu().numpy(), xyz[lo:hi].cpu().numpy(), quat[lo:hi].cpu().numpy())


def tum_text_ragged(ts, xyz, quat, offsets, fmt="utm", run_status=None):
    """The bytes np.savetxt writes for each track (ref :1091-1092 for fmt="utm", :1098-1101 for fmt="wgs84", xyz = utm_to_wgs84_ragged rows),
    formatted on the device (gsf_tum_text_dev).  ts (P,), xyz (P, 3), quat (P, 4), offsets (B+1,) int64, run_status (B,) int32 or None.
    Returns (texts, track_state): texts = B bytes objects (None for a track with run_status != 0); track_state (B,) numpy int32 = 0 formatted on
    the device, 1 skipped, 2 holds a finite |x| >= 2^63 and was written here through np.savetxt."""
    import io
    import numpy as np
    if fmt not in _TUM_FORMATS:
        raise ValueError(f"fmt must be 'utm' or 'wgs84', got {fmt!r}")
    form = _TUM_FORMATS[fmt]
    B, P = _text_args(ts, xyz, quat, offsets, run_status)
    text_offsets, state = _text_sizes(form, ts, xyz, quat, offsets, run_status, B, P)
    toff = text_offsets.cpu().numpy()
    total = int(toff[-1])
    text = torch.empty((max(total, 1),), dtype=torch.uint8, device=ts.device)
    check(_lib.load().gsf_tum_text_dev(context().handle, form, _p(ts), _p(xyz), _p(quat), _p(offsets), _p(run_status), B, P, _p(text_offsets),
                                       _p(state), _p(text)))
    host = text[:total].cpu().numpy().tobytes()
    st = state.cpu().numpy()
    offs = offsets.cpu().numpy()
    texts = []
    for b in range(B):
        if st[b] == _lib.TEXT_SKIPPED:
            texts.append(None)
        elif st[b] == _lib.TEXT_HOST:
            f = io.BytesIO()
            _savetxt_track(form, f, ts, xyz, quat, int(offs[b]), int(offs[b + 1]))
            texts.append(f.getvalue())
        else:
            texts.append(host[toff[b]:toff[b + 1]])
    return texts, st


def save_fusion_ragged(rb, r, utm_paths):
    """Step 7 of main_process_gui (ref :1085-1104) for a run_fusion_ragged result: per track b, utm_paths[b] (None: not saved, the dialog of
    :1086-1090) gets the corrected track as *_corrected_utm.txt (:1091-1092) and, when the run has a projector (r.zone is not None, :1096), its
    WGS84 file named by the drop-in's rule (ekfgpsslam.wgs84_path, :1099-1100) -- byte for byte what np.savetxt writes for the same rows.
    Tracks with run_status != 0 get no file (the reference raised before step 7).  The text is formatted on the device (gsf_tum_text_dev)
    in groups of tracks of at most TEXT_GROUP_BYTES bytes (a longer track is a group of its own): one copy per group into pinned memory,
    one write per file.  Returns, per track, the tuple of the paths written."""
    import numpy as np
    from . import ekfgpsslam as E
    B = rb.B
    if len(utm_paths) != B:
        raise ValueError(f"save_fusion_ragged: {len(utm_paths)} paths for {B} tracks")
    status = r.run_status.cpu().numpy()
    want = np.array([p is not None and int(status[b]) == 0 for b, p in enumerate(utm_paths)], dtype=bool)
    written = [[] for _ in range(B)]
    if not want.any():
        return [tuple(w) for w in written]
    dev = rb.ts.device
    skip = torch.as_tensor((~want).astype(np.int32), device=dev)      # run_status of the text calls: every track not to be saved
    ts, pos, quat, so = rb.ts, r.fused.pos, r.fused.quat, rb.slam_offsets
    _, P = _text_args(ts, pos, quat, so, skip)
    jobs = [(_lib.TUM_UTM, pos, [str(p) if w else None for p, w in zip(utm_paths, want)])]
    if r.zone is not None:
        lla = utm_to_wgs84_ragged(pos, so, r.zone, r.south, skip)
        jobs.append((_lib.TUM_WGS84, lla, [E.wgs84_path(str(p)) if w else None for p, w in zip(utm_paths, want)]))
    offs = so.cpu().numpy()
    L, h = _lib.load(), context().handle
    dbuf = hbuf = None
    for form, xyz, paths in jobs:
        text_offsets, state = _text_sizes(form, ts, xyz, quat, so, skip, B, P)
        toff, st = text_offsets.cpu().numpy(), state.cpu().numpy()
        groups, b = [], 0
        while b < B:                                                    # consecutive tracks whose text fits the budget
            e = b + 1
            while e < B and toff[e + 1] - toff[b] <= TEXT_GROUP_BYTES:
                e += 1
            groups.append((b, e))
            b = e
        need = max(int(toff[e] - toff[b]) for b, e in groups)
        if need and (dbuf is None or dbuf.numel() < need):
            dbuf = torch.empty((need,), dtype=torch.uint8, device=dev)
            hbuf = torch.empty((need,), dtype=torch.uint8, pin_memory=True)
        for b, e in groups:
            n = int(toff[e] - toff[b])
            if n:
                rel = text_offsets[b:e + 1] - text_offsets[b]
                check(L.gsf_tum_text_dev(h, form, _p(ts), _p(xyz), _p(quat), _p(so[b:]), _p(skip[b:]), e - b, P, _p(rel), _p(state[b:]), _p(dbuf)))
                hbuf[:n].copy_(dbuf[:n])
                mv = memoryview(hbuf.numpy())
                for k in range(b, e):
                    if st[k] == _lib.TEXT_DEVICE:
                        with open(paths[k], "wb") as fh:
                            fh.write(mv[toff[k] - toff[b]:toff[k + 1] - toff[b]])
                        written[k].append(paths[k])
            for k in range(b, e):
                if st[k] == _lib.TEXT_HOST:
                    _savetxt_track(form, paths[k], ts, xyz, quat, int(offs[k]), int(offs[k + 1]))
                    written[k].append(paths[k])
    return [tuple(w) for w in written]


class FusedPoses:
    """Fused poses of a batch.  pos and quat are views of ONE allocation `buf` = [pos | quat] (7 doubles per pose), so the
    multi-GPU collect is a single all-gather of `buf`.  `buf` may be a caller-provided slice of a larger arena; `status` a
    caller-provided int32 tensor (the ragged whole run has one word per track, not per row of its flat pose array)."""

    def __init__(self, layout, B, N, device="cuda", buf=None, status=None):
        _, s_pos, s_quat, _, _ = shapes(layout, B, N)
        self.layout, self.B, self.N = layout, B, N
        P = B * N
        if buf is None:
            buf = torch.empty((P * 7,), dtype=torch.float64, device=device)
        elif buf.dtype != torch.float64 or buf.numel() != P * 7 or not buf.is_contiguous():
            raise ValueError(f"FusedPoses: buf must be a contiguous float64 tensor of {P * 7} elements")
        self.buf = buf.view(-1)
        self.pos = self.buf[: P * 3].view(s_pos)
        self.quat = self.buf[P * 3:].view(s_quat)
        self.status = torch.empty((B,), dtype=torch.int32, device=self.buf.device) if status is None else status

    def host_traj_major(self):
        """-> (pos (B,N,3), quat (B,N,4), status (B,)) numpy"""
        if self.layout == LAYOUT_TRAJ_MAJOR:
            pos, quat = self.pos, self.quat
        else:
            pos = torch.empty((self.B, self.N, 3), dtype=torch.float64, device=self.pos.device)
            quat = torch.empty((self.B, self.N, 4), dtype=torch.float64, device=self.pos.device)
            L, h = _lib.load(), context().handle
            check(L.gsf_transpose_to_traj_major_dev(h, _p(self.pos), _p(pos), self.B, self.N, 3, 8))
            check(L.gsf_transpose_to_traj_major_dev(h, _p(self.quat), _p(quat), self.B, self.N, 4, 8))
        torch.cuda.synchronize()
        return pos.cpu().numpy(), quat.cpu().numpy(), self.status.cpu().numpy()


def ekf_fuse_batch(batch, config=None, out=None):
    """K4 over a device batch: apply_ekf_correction (EKFGPSSLAM.py:831-935, after its :847 alignment) per trajectory.
    Asynchronous on torch's current stream; returns FusedPoses in the batch's layout."""
    cfg = EkfConfig.from_config(config or CONFIG)
    out = out or FusedPoses(batch.layout, batch.B, batch.N, batch.ts.device)
    check(_lib.load().gsf_ekf_fuse_batch_dev(context().handle, batch.layout, _p(batch.ts), _p(batch.pos), _p(batch.quat), _p(batch.gps),
                                             _p(batch.valid), _p(batch.init_pos), _p(batch.init_quat), C.byref(cfg), batch.B, batch.N,
                                             _p(out.pos), _p(out.quat), _p(out.status)))
    return out


def fuse_pipeline_batch(batch, config=None, out=None, fit_rows=FIT_ROWS_DEFAULT):
    """Umeyama -> Sim3 of pose 0 -> EKF+RTS in one launch (steps 3-5 of EKFGPSSLAM.py:1002-1010, plain fit).  fit_rows="reference":
    the fit sees the rows main_process_gui hands to its fit (first gap-free segment of the valid rows, <= max_initial_duration, two
    fall-backs; ref :973-998); "all": every row with valid finite GNSS.  status >> 8 carries the GSF_SIM3_* bits (FEW_ROWS = the
    reference's ValueError).  Returns (FusedPoses, R (B,9), t (B,3), s (B,))."""
    cfg = EkfConfig.from_config(config or CONFIG)
    context().set_sim3_rows(fit_rows, config or CONFIG)
    out = out or FusedPoses(batch.layout, batch.B, batch.N, batch.ts.device)
    f = dict(dtype=torch.float64, device=batch.ts.device)
    R, t, s = torch.empty((batch.B, 9), **f), torch.empty((batch.B, 3), **f), torch.empty((batch.B,), **f)
    check(_lib.load().gsf_fuse_pipeline_batch_dev(context().handle, batch.layout, _p(batch.ts), _p(batch.pos), _p(batch.quat), _p(batch.gps),
                                                  _p(batch.valid), C.byref(cfg), batch.B, batch.N, _p(R), _p(t), _p(s), _p(out.pos),
                                                  _p(out.quat), _p(out.status)))
    return out, R, t, s


def mt19937_seed(seeds, device="cuda"):
    """np.random.seed(seeds[b]) for B independent legacy-MT19937 streams -> state (B, 625) uint32 on the device (key[624] + pos)."""
    seeds = torch.as_tensor(seeds, dtype=torch.int64).to(device)
    st = torch.empty((seeds.numel(), 625), dtype=torch.int32, device=device)
    check(_lib.load().gsf_mt19937_seed_batch_dev(context().handle, _p(seeds.to(torch.int32)), seeds.numel(), _p(st)))
    return st


def mt19937_from_numpy(device="cuda"):
    """NumPy's GLOBAL legacy generator as a one-stream device state (1, 625): what a seeded reference run would draw from next."""
    import numpy as np
    _, key, pos = np.random.get_state()[:3]
    st = np.concatenate([key.astype(np.uint32), np.array([pos], dtype=np.uint32)]).view(np.int32)
    return torch.from_numpy(st.copy()).reshape(1, 625).to(device)


def mt19937_choice_batch(state, n_population, trials, k):
    """sample_idx (B, trials, k) int32 = np.random.choice(n_population[b], k, replace=False) drawn `trials` times from stream b;
    `state` (B, 625) is advanced in place exactly as NumPy's generator would be."""
    B = state.shape[0]
    # populations given on the host: their maximum lets the library take the chip-wide route for a few streams (gsf.h); a device
    # tensor is passed as it is (no synchronising read-back)
    n_max = 0 if (torch.is_tensor(n_population) and n_population.is_cuda) else int(max((int(v) for v in torch.as_tensor(n_population).reshape(-1)), default=0))
    n = torch.as_tensor(n_population, dtype=torch.int32).to(state.device).contiguous()
    idx = torch.empty((B, trials, k), dtype=torch.int32, device=state.device)
    check(_lib.load().gsf_mt19937_choice_bounded_batch_dev(context().handle, _p(state), _p(n), n_max, B, int(trials), int(k), _p(idx)))
    return idx


def sample_without_replacement_batch(state, n_population, trials, k):
    """sample_idx (B, trials, k) int32 = sklearn.utils.random.sample_without_replacement(n_population[b], k) called `trials` times on
    stream b (method "auto": permutation for 0.01 < k/n < 0.99, tracking selection for k/n <= 0.01, rows 0..k-1 for n == k); `state`
    (B, 625) is advanced in place exactly as NumPy's generator would be.  Streams with n_population[b] < k are left untouched and their
    sets are zero."""
    B = state.shape[0]
    n = torch.as_tensor(n_population, dtype=torch.int32).to(state.device).contiguous()
    idx = torch.empty((B, trials, k), dtype=torch.int32, device=state.device)
    check(_lib.load().gsf_mt19937_sample_without_replacement_batch_dev(context().handle, _p(state), _p(n), B, int(trials), int(k), _p(idx)))
    return idx


def fuse_pipeline_robust_batch(batch, mt_state, config=None, out=None, want_mask=True, fit_rows=FIT_ROWS_DEFAULT, early_exit=True, return_info=False):
    """Steps 3-5 of main_process_gui with the reference's robust fit (EKFGPSSLAM.py:1002-1010): the rows main_process_gui picks
    (ref :973-998; fit_rows="all": every valid row) -> RANSAC hypotheses drawn on the device from each trajectory's legacy MT19937
    stream -> inlier refit -> Sim3 of pose 0 -> EKF+RTS, one chain on torch's current stream.  Trajectory-major batches.
    early_exit (default on): a trajectory stops drawing at the first trial that counts every row of its fit -- the reference keeps a trial
    only on a strictly larger count (ref :413), so R, t, s, mask, n_inliers and the fused poses are those of all max_trials, bit for bit;
    only where `mt_state` is left differs (after fewer trials).  early_exit=False: every generator ends where np.random ends in the
    reference.  Returns (FusedPoses, R, t, s, n_inliers (B,), inlier_mask (B, N) uint8 or None[, trial_info (B, 2) int32 = deciding trial,
    trials drawn])."""
    if batch.layout != LAYOUT_TRAJ_MAJOR:
        raise ValueError("fuse_pipeline_robust_batch: trajectory-major batches only")
    g = config or CONFIG
    ctx = context()
    ctx.set_sim3_rows(fit_rows, g)
    ctx.set_option("ransac_early_exit", 1 if early_exit else 0)
    cfg, r = EkfConfig.from_config(g), g["sim3_ransac"]
    out = out or FusedPoses(batch.layout, batch.B, batch.N, batch.ts.device)
    f = dict(dtype=torch.float64, device=batch.ts.device)
    R, t, s = torch.empty((batch.B, 9), **f), torch.empty((batch.B, 3), **f), torch.empty((batch.B,), **f)
    nin = torch.empty((batch.B,), dtype=torch.int32, device=batch.ts.device)
    mask = torch.empty((batch.B, batch.N), dtype=torch.uint8, device=batch.ts.device) if want_mask else None
    info = torch.empty((batch.B, 2), dtype=torch.int32, device=batch.ts.device) if return_info else None
    check(_lib.load().gsf_fuse_pipeline_robust_info_batch_dev(ctx.handle, _p(batch.ts), _p(batch.pos), _p(batch.quat), _p(batch.gps), _p(batch.valid),
                                                              C.byref(cfg), batch.B, batch.N, int(r["min_samples"]), float(r["residual_threshold"]),
                                                              int(r["max_trials"]), int(r["min_inliers_needed"]), _p(mt_state), _p(R), _p(t), _p(s),
                                                              _p(out.pos), _p(out.quat), _p(out.status), _p(nin), _p(mask), _p(info)))
    return (out, R, t, s, nin, mask, info) if return_info else (out, R, t, s, nin, mask)


def sim3_fit_rows_batch(ts, gps, valid, config=None, offsets=None):
    """main_process_gui's choice of the rows that feed the global Sim3 (EKFGPSSLAM.py:973-998) for B trajectories on the device: ts (B,N),
    gps (B,N,3) or None, valid (B,N) uint8 -- or flat tensors with int64 offsets (B+1,).  Returns row_mask (uint8, shape of valid),
    n_rows (B,) int32 (-1 where the reference raises ValueError), status (B,) int32 (GSF_SIM3_FLAG_FEW_ROWS / _ROWS_ALL / _ROWS_SEGMENT)."""
    g = config or CONFIG
    Bn = (offsets.numel() - 1) if offsets is not None else ts.shape[0]
    N = 0 if offsets is not None else ts.shape[1]
    mask = torch.empty(valid.shape, dtype=torch.uint8, device=ts.device)
    n_rows, st = torch.empty((Bn,), dtype=torch.int32, device=ts.device), torch.empty((Bn,), dtype=torch.int32, device=ts.device)
    check(_lib.load().gsf_sim3_fit_rows_batch_dev(context().handle, _p(ts), _p(gps), _p(valid), _p(offsets), Bn, N, int(g["sim3_ransac"]["min_samples"]),
                                                  float(g["time_alignment"]["max_gps_gap_threshold"]), float(g["sim3_ransac"]["max_initial_duration"]),
                                                  _p(mask), _p(n_rows), _p(st)))
    return mask, n_rows, st


def sim3_umeyama_batch(src, dst, offsets=None, mask=None):
    """K2 over device tensors.  src/dst: (total,3) with int64 offsets (B+1,), or (B,W,3) equal-size windows (config C4; mask (B,W)).
    Returns R (B,9), t (B,3), s (B,), status (B,) int32."""
    f = dict(dtype=torch.float64, device=src.device)
    if src.dim() == 3:
        B, W, _ = src.shape
        _chk(src, torch.float64, (B, W, 3), "src"); _chk(dst, torch.float64, (B, W, 3), "dst")
        R, t, s = torch.empty((B, 9), **f), torch.empty((B, 3), **f), torch.empty((B,), **f)
        st = torch.empty((B,), dtype=torch.int32, device=src.device)
        check(_lib.load().gsf_sim3_umeyama_windows_dev(context().handle, _p(src), _p(dst), _p(mask), B, W, _p(R), _p(t), _p(s), _p(st)))
        return R, t, s, st
    B = offsets.numel() - 1
    _chk(src, torch.float64, src.shape, "src"); _chk(dst, torch.float64, src.shape, "dst")
    R, t, s = torch.empty((B, 9), **f), torch.empty((B, 3), **f), torch.empty((B,), **f)
    st = torch.empty((B,), dtype=torch.int32, device=src.device)
    check(_lib.load().gsf_sim3_umeyama_batch_dev(context().handle, _p(src), _p(dst), _p(mask), _p(offsets), B, _p(R), _p(t), _p(s), _p(st)))
    return R, t, s, st


def sim3_ransac_batch(src, dst, offsets, sample_idx, residual_threshold, min_inliers_needed):
    """K2b over device tensors; sample_idx (B,trials,ms) int32 drawn by the caller with the reference's RNG call."""
    B, trials, ms = sample_idx.shape
    f = dict(dtype=torch.float64, device=src.device)
    R, t, s = torch.empty((B, 9), **f), torch.empty((B, 3), **f), torch.empty((B,), **f)
    st, nin = torch.empty((B,), dtype=torch.int32, device=src.device), torch.empty((B,), dtype=torch.int32, device=src.device)
    mask = torch.empty((src.shape[0],), dtype=torch.uint8, device=src.device)
    check(_lib.load().gsf_sim3_ransac_batch_rows_dev(context().handle, _p(src), _p(dst), _p(offsets), int(src.shape[0]), B, _p(sample_idx), trials, ms,
                                                     float(residual_threshold), int(min_inliers_needed), _p(R), _p(t), _p(s), _p(st), _p(mask), _p(nin)))
    return R, t, s, st, mask, nin


def apply_sim3_batch(pos, quat, offsets, R, t, s):
    """K3 over device tensors: pos (total,3), quat (total,4) -> transformed copies (+ bad_quat flags (B,))."""
    B = offsets.numel() - 1
    po, qo = torch.empty_like(pos), torch.empty_like(quat)
    bad = torch.empty((B,), dtype=torch.int32, device=pos.device)
    check(_lib.load().gsf_apply_sim3_batch_dev(context().handle, _p(pos), _p(quat), _p(offsets), B, _p(R), _p(t), _p(s), _p(po), _p(qo), _p(bad)))
    return po, qo, bad


def utm_forward_batch(lat, lon, offsets, zone=None, south=None):
    """K1 over device tensors (ragged trajectories).  zone/south None -> picked per trajectory like auto_utm_projection."""
    B = offsets.numel() - 1
    L, h = _lib.load(), context().handle
    if zone is None:
        zone = torch.empty((B,), dtype=torch.int32, device=lat.device)
        south = torch.empty((B,), dtype=torch.int32, device=lat.device)
        check(L.gsf_utm_zone_batch_dev(h, _p(lat), _p(lon), _p(offsets), B, _p(zone), _p(south)))
    e, n = torch.empty_like(lat), torch.empty_like(lat)
    check(L.gsf_utm_forward_batch_dev(h, _p(lat), _p(lon), _p(offsets), _p(zone), _p(south), B, _p(e), _p(n)))
    return e, n, zone, south


def utm_inverse_batch(e, n, offsets, zone, south):
    B = offsets.numel() - 1
    lat, lon = torch.empty_like(e), torch.empty_like(e)
    check(_lib.load().gsf_utm_inverse_batch_dev(context().handle, _p(e), _p(n), _p(offsets), _p(zone), _p(south), B, _p(lat), _p(lon)))
    return lat, lon


def fuse_pipeline_ragged(ts, pos, quat, gps, valid, offsets, config=None, fit_rows=FIT_ROWS_DEFAULT):
    """Fused Umeyama -> Sim3(pose 0) -> EKF+RTS for trajectories of DIFFERENT lengths: flat device tensors ts (T,), pos (T,3),
    quat (T,4), gps (T,3), valid (T,) uint8 and int64 offsets (B+1,); fit_rows as in fuse_pipeline_batch.  Returns pos_out, quat_out,
    status, R, t, s."""
    cfg = EkfConfig.from_config(config or CONFIG)
    context().set_sim3_rows(fit_rows, config or CONFIG)
    B = offsets.numel() - 1
    f = dict(dtype=torch.float64, device=ts.device)
    po, qo = torch.empty_like(pos), torch.empty_like(quat)
    R, t, s = torch.empty((B, 9), **f), torch.empty((B, 3), **f), torch.empty((B,), **f)
    st = torch.empty((B,), dtype=torch.int32, device=ts.device)
    check(_lib.load().gsf_fuse_pipeline_ragged_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), C.byref(cfg), B,
                                                   _p(R), _p(t), _p(s), _p(po), _p(qo), _p(st)))
    return po, qo, st, R, t, s


def ekf_fuse_ragged(ts, pos, quat, gps, valid, offsets, init_pos, init_quat, config=None):
    """K4 for trajectories of different lengths (flat tensors + offsets, see fuse_pipeline_ragged)."""
    cfg = EkfConfig.from_config(config or CONFIG)
    B = offsets.numel() - 1
    po, qo = torch.empty_like(pos), torch.empty_like(quat)
    st = torch.empty((B,), dtype=torch.int32, device=ts.device)
    check(_lib.load().gsf_ekf_fuse_ragged_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), _p(init_pos),
                                              _p(init_quat), C.byref(cfg), B, _p(po), _p(qo), _p(st)))
    return po, qo, st


def geodetic_to_enu_batch(lat, lon, alt, offsets, ref_llh):
    """WGS84 geodetic -> local ENU about ref_llh (B,3) per trajectory (device tensors).  Offered in addition to UTM."""
    B = offsets.numel() - 1
    e, n, u = torch.empty_like(lat), torch.empty_like(lat), torch.empty_like(lat)
    check(_lib.load().gsf_geodetic_to_enu_batch_dev(context().handle, _p(lat), _p(lon), _p(alt), _p(offsets), _p(ref_llh), B, _p(e), _p(n), _p(u)))
    return e, n, u


def ransac_poly_batch(t, y, offsets, sample_idx, degree, residual_threshold, stop_probability=0.99):
    """next-3 kernel over device tensors: P polynomial-RANSAC problems (rows offsets[p]..offsets[p+1] of t, y), sample sets
    sample_idx (P, max_trials, min_samples) int32 drawn by the caller.  Returns inlier_mask (rows,) uint8, n_trials, n_inliers,
    status (P,) int32 -- see gsf_ransac_poly_batch_dev."""
    P, trials, ms = sample_idx.shape
    mask = torch.empty((t.shape[0],), dtype=torch.uint8, device=t.device)
    ntr, nin, st = (torch.empty((P,), dtype=torch.int32, device=t.device) for _ in range(3))
    check(_lib.load().gsf_ransac_poly_batch_dev(context().handle, _p(t), _p(y), _p(offsets), P, _p(sample_idx), trials, ms, int(degree),
                                                float(residual_threshold), float(stop_probability), _p(mask), _p(ntr), _p(nin), _p(st)))
    return mask, ntr, nin, st


def eval_errors_batch(ts, traj_pos, gps, valid, skip_seconds=0.0):
    """next-4 over device tensors (trajectory-major (B,N) / (B,N,3)): nearest-fix error of every fused pose (ref :1013-1033).
    Returns stats (B,4) = count, mean, median, RMSE and errors (B,N) (NaN where not evaluated)."""
    Bn, N = ts.shape
    stats = torch.empty((Bn, 4), dtype=torch.float64, device=ts.device)
    err = torch.empty((Bn, N), dtype=torch.float64, device=ts.device)
    check(_lib.load().gsf_eval_errors_batch_dev(context().handle, _p(ts), _p(traj_pos), _p(gps), _p(valid), Bn, N, float(skip_seconds), _p(stats), _p(err)))
    return stats, err


class FusedCovariance:
    """Per-pose covariance of fused tracks (ekf_covariance_ragged), flat over the P rows of the batch: filtered (P,7) or None = the diagonal
    of the reference's ekf_covs_filt_hist; cov (P,7) = the covariance of the pose the fuse entries return (smoothed on POSE_SMOOTHED rows,
    filtered elsewhere); flags (P,) uint8 of _lib.POSE_* bits; status (B,) int32 = ST_HAD_OUTAGE | ST_RTS_APPLIED | ST_SHARP_TURN |
    ST_ENDED_IN_OUTAGE; offsets (B+1,).  Rows are [x y z qx qy qz qw]; the reference's matrices are exactly diagonal."""

    def __init__(self, filtered, cov, flags, status, offsets):
        self.filtered, self.cov, self.flags, self.status, self.offsets = filtered, cov, flags, status, offsets

    def dense(self, which="cov"):
        """(P,7,7) matrices, the shape the reference's lists hold (which="filtered": ekf_covs_filt_hist)"""
        d = self.filtered if which == "filtered" else self.cov
        return torch.diag_embed(d)


def ekf_covariance_ragged(ts, quat, gps, valid, offsets, config=None, run_status=None, want_filtered=True):
    """The covariances apply_ekf_correction computes and drops (EKFGPSSLAM.py:852-853, :902-903, :917), for ragged tracks: ts (P,), quat (P,4)
    = the original SLAM quaternions, gps (P,3) / valid (P,) uint8 = the time-aligned fixes, offsets (B+1,) int64.  run_status (B,) int32 or
    None: tracks with run_status != 0 get NaN rows, zero flags and status 0.  One launch on torch's current stream; returns a FusedCovariance."""
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(quat, torch.float64, (P, 4), "quat"); _chk(gps, torch.float64, (P, 3), "gps")
    _chk(valid, torch.uint8, (P,), "valid")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    cfg = EkfConfig.from_config(config or CONFIG)
    f = dict(dtype=torch.float64, device=ts.device)
    filt = torch.empty((P, 7), **f) if want_filtered else None
    cov = torch.empty((P, 7), **f)
    flags = torch.empty((P,), dtype=torch.uint8, device=ts.device)
    st = torch.empty((B,), dtype=torch.int32, device=ts.device)
    check(_lib.load().gsf_ekf_cov_ragged_dev(context().handle, _p(ts), _p(quat), _p(gps), _p(valid), _p(offsets), _p(run_status), C.byref(cfg), B,
                                             _p(filt), _p(cov), _p(flags), _p(st)))
    return FusedCovariance(filt, cov, flags, st, offsets)


def ekf_covariance_batch(batch, config=None, want_filtered=True):
    """ekf_covariance_ragged for a trajectory-major TrajectoryBatch: the same memory with offsets = arange(B+1) * N (rows b*N .. b*N+N-1
    belong to track b).  A time-major batch raises ValueError (convert it with to_layout first)."""
    if batch.layout != LAYOUT_TRAJ_MAJOR:
        raise ValueError("ekf_covariance_batch: trajectory-major batches only")
    P = batch.B * batch.N
    offsets = torch.arange(batch.B + 1, dtype=torch.int64, device=batch.ts.device) * batch.N
    return ekf_covariance_ragged(batch.ts.view(P), batch.quat.view(P, 4), batch.gps.view(P, 3), batch.valid.view(P), offsets, config=config,
                                 want_filtered=want_filtered)


# ---------------------------------------------------------------------------- whole-track RTS smoothing (gsf_ekf_smooth_ragged_dev)
class SmoothedTrack:
    """The fixed-interval RTS smoother over fused tracks (ekf_smooth_ragged), flat over the P rows of the batch: pos (P,3) / quat (P,4) = the
    smoothed track (the quaternion is the filter's: GNSS never touches it); cov (P,7) = the smoothed diagonal [x y z qx qy qz qw];
    pos_filt (P,3) / cov_filt (P,7) or None = the causal filter's own track and diagonal; flags (P,) uint8 of _lib.POSE_* bits, where
    POSE_SMOOTHED means "a later fix of the same span was applied" (every other row holds the filter's bytes) and POSE_SPAN_START marks row 0
    and every sharp-turn recovery; status (B,) int32 of _lib.ST_* bits (ST_RTS_APPLIED: some row is POSE_SMOOTHED); offsets (B+1,)."""

    def __init__(self, pos, quat, cov, pos_filt, cov_filt, flags, status, offsets):
        self.pos, self.quat, self.cov, self.pos_filt, self.cov_filt = pos, quat, cov, pos_filt, cov_filt
        self.flags, self.status, self.offsets = flags, status, offsets

    def dense(self, which="cov"):
        """(P,7,7) matrices, the shape the reference's lists hold (which="filtered": the filter's, needs want_filtered=True)"""
        d = self.cov_filt if which == "filtered" else self.cov
        if d is None:
            raise ValueError("SmoothedTrack.dense: the filtered covariance was not asked for (want_filtered=True)")
        return torch.diag_embed(d)

    def correction(self):
        """pos - pos_filt (P,3): what the later fixes moved every pose by (needs want_filtered=True)"""
        if self.pos_filt is None:
            raise ValueError("SmoothedTrack.correction: the filtered track was not asked for (want_filtered=True)")
        return self.pos - self.pos_filt


def ekf_smooth_ragged(ts, pos, quat, gps, valid, offsets, init_pos, init_quat, config=None, run_status=None, want_filtered=False):
    """The fixed-interval RTS smoother over whole tracks (gsf_ekf_smooth_ragged_dev; definition: include/gsf.h), one launch on torch's
    current stream.  Inputs as ekf_fuse_ragged -- ts (P,), pos (P,3) / quat (P,4) = the original SLAM poses, gps (P,3) / valid (P,) uint8 =
    the time-aligned fixes, offsets (B+1,) int64, init_pos (B,3) / init_quat (B,4) -- plus run_status (B,) int32 or None: tracks with
    run_status != 0 get NaN rows, zero flags and status 0.  The forward pass is the filter of ekf_fuse_ragged; every sharp-turn recovery
    starts a new span, and each span is smoothed backwards from its last pose.  want_filtered: also the filter's own track and diagonal.
    Returns a SmoothedTrack."""
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
    _chk(init_pos, torch.float64, (B, 3), "init_pos"); _chk(init_quat, torch.float64, (B, 4), "init_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    cfg = EkfConfig.from_config(config or CONFIG)
    f = dict(dtype=torch.float64, device=ts.device)
    st = SmoothedTrack(torch.empty((P, 3), **f), torch.empty((P, 4), **f), torch.empty((P, 7), **f),
                       torch.empty((P, 3), **f) if want_filtered else None, torch.empty((P, 7), **f) if want_filtered else None,
                       torch.empty((P,), dtype=torch.uint8, device=ts.device), torch.empty((B,), dtype=torch.int32, device=ts.device), offsets)
    check(_lib.load().gsf_ekf_smooth_ragged_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), _p(init_pos),
                                                _p(init_quat), _p(run_status), C.byref(cfg), B, _p(st.pos), _p(st.quat), _p(st.cov), _p(st.pos_filt),
                                                _p(st.cov_filt), _p(st.flags), _p(st.status)))
    return st


# ---------------------------------------------------------------------------- EKF noise sweep (gsf_ekf_noise_sweep_dev)
NOISE_P0_MAX, NOISE_R_MIN, NOISE_R_MAX, NOISE_QDT_MAX = 1e8, 1e-8, 1e8, 1e14      # the stated range of the noise values (include/gsf.h, gsf_ekf_config)
_LN_2PI = 1.8378770664093453


def _noise_domain_chk(cand, max_dt):
    import numpy as np
    c = np.asarray(cand, dtype=np.float64)
    p0, q, r = c[:, 0:3], c[:, 3:6], c[:, 6:9]
    step = max(float(max_dt), 1e-6)
    ok = np.isfinite(c).all(axis=1) & ((p0 >= 0.0) & (p0 <= NOISE_P0_MAX)).all(axis=1) & ((r >= NOISE_R_MIN) & (r <= NOISE_R_MAX)).all(axis=1) \
        & ((q >= 0.0) & (q * step <= NOISE_QDT_MAX)).all(axis=1)
    if not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"noise candidate {k} = {c[k].tolist()} is outside the stated range 0 <= P0 <= 1e8, 1e-8 <= R <= 1e8, "
                         f"0 <= Q dt <= 1e14 (dt up to {step} in the stamps' unit)")


def noise_candidates(config, q_scales, r_scales, p0_scales=(1.0,), max_dt=1.0):
    """Candidates for ekf_noise_sweep_ragged on a grid around config['ekf']: the position entries of initial_cov_diag / process_noise_diag /
    meas_noise_diag times every combination of p0_scales x q_scales x r_scales.  Returns (cand (K,9) float64 numpy rows
    [P0x P0y P0z Qx Qy Qz Rx Ry Rz], shape = (len(p0_scales), len(q_scales), len(r_scales))); candidate k is the grid point
    np.unravel_index(k, shape) (C order).  ValueError for a candidate outside the stated range of the noise values (include/gsf.h);
    max_dt = the longest step between two stamps the candidates will meet, in the stamps' unit (the range bounds Q dt)."""
    import numpy as np
    e = (config or CONFIG)["ekf"]
    p0, q, r = (np.asarray([float(x) for x in e[n]][:3]) for n in ("initial_cov_diag", "process_noise_diag", "meas_noise_diag"))
    ps, qs, rs = (np.asarray(list(v), dtype=np.float64).reshape(-1) for v in (p0_scales, q_scales, r_scales))
    shape = (ps.size, qs.size, rs.size)
    K = ps.size * qs.size * rs.size
    if not 1 <= K <= 4096:
        raise ValueError(f"noise_candidates: {K} candidates, 1..4096 per call")
    cand = np.empty(shape + (9,))
    cand[..., 0:3] = ps[:, None, None, None] * p0
    cand[..., 3:6] = qs[None, :, None, None] * q
    cand[..., 6:9] = rs[None, None, :, None] * r
    cand = np.ascontiguousarray(cand.reshape(K, 9))
    _noise_domain_chk(cand, max_dt)
    return cand, shape


class NoiseSweep:
    """Result of ekf_noise_sweep_ragged for B tracks x K candidates (definitions: include/gsf.h, gsf_ekf_noise_sweep_dev).  Device tensors:
    stats (B,K,12); nll / mean_nis / rho1 (B,K) derived from it (nll = (3 n ln 2pi + sum log S + sum NIS) / 2, mean_nis = sum NIS / n,
    rho1 = lag-one term / (3 pairs); NaN where n is 0); best_k (B,2) int32 = the picks by nll and by |mean_nis - 3| (-1: none);
    pooled (K,12), pooled_nll / pooled_mean_nis (K,), pooled_best (2,) int32: the same over all usable tracks together -- the pick to use,
    noise being a property of the receiver; status (B,) int32 = _lib.NS_NONE | NS_TIE; innov / innov_var (P,3) = y and S of the traced
    candidate (None without trace); candidates (K,9)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def config(self, k, base=None):
        """A CONFIG dict (deep copy of base, default the module's CONFIG) with candidate k written into the position entries of ['ekf']:
        ready for run_fusion_ragged."""
        import copy
        k = int(k)
        if not 0 <= k < int(self.candidates.shape[0]):
            raise ValueError(f"NoiseSweep.config: no candidate {k} (a pick of -1 means that nothing was picked)")
        g = copy.deepcopy(base or CONFIG)
        row = [float(x) for x in self.candidates[k].cpu().tolist()]
        for name, lo in (("initial_cov_diag", 0), ("process_noise_diag", 3), ("meas_noise_diag", 6)):
            v = [float(x) for x in g["ekf"][name]]
            v[0:3] = row[lo:lo + 3]
            g["ekf"][name] = v
        return g

    def at_edge(self, shape, criterion=0):
        """For a grid made by noise_candidates(shape): does a pick lie on the grid's edge along an axis with more than one value -- the
        minimum may then lie outside the grid, widen it (the counterpart of CLK_AT_EDGE).  Returns (per track (B,) bool numpy, pooled bool);
        a pick of -1 is not on an edge."""
        import numpy as np
        shape = tuple(int(n) for n in shape)
        if int(np.prod(shape)) != int(self.candidates.shape[0]):
            raise ValueError("NoiseSweep.at_edge: the shape does not describe the swept candidates")

        def edge(k):
            if k < 0:
                return False
            return any(n > 1 and (i == 0 or i == n - 1) for i, n in zip(np.unravel_index(int(k), shape), shape))
        per = np.array([edge(int(k)) for k in self.best_k[:, criterion].cpu().tolist()], dtype=bool)
        return per, edge(int(self.pooled_best[criterion].item()))


def _noise_derived(rows):
    n = rows[..., 0]
    nis = (rows[..., 1] + rows[..., 2]) + rows[..., 3]
    ls = (rows[..., 4] + rows[..., 5]) + rows[..., 6]
    nll = 0.5 * (((3.0 * n) * _LN_2PI + ls) + nis)
    return nll, nis / n, rows[..., 10] / (3.0 * rows[..., 11])


def ekf_noise_sweep_ragged(ts, pos, quat, gps, valid, offsets, init_pos, init_quat, candidates, config=None, run_status=None, skip_seconds=0.0,
                           min_updates=1, trace=None):
    """Innovation statistics of the EKF for K noise candidates per track, one launch chain on torch's current stream
    (gsf_ekf_noise_sweep_dev).  Inputs as ekf_fuse_ragged: flat device tensors ts (P,), pos (P,3), quat (P,4) = the original SLAM track,
    gps (P,3) / valid (P,) uint8 = the time-aligned fixes, offsets (B+1,) int64, init_pos (B,3) / init_quat (B,4) = row 0 of the
    Sim3-aligned track.  candidates (K,9) rows [P0 Q R] x 3 axes (numpy or tensor; noise_candidates builds a grid), inside the stated
    range of the noise values.  The sharp-turn settings come from config.  skip_seconds: updates up to ts[0] + skip_seconds are not
    counted (<= 0: all are); min_updates: fewer counted updates give no pick; trace = k: y and S of candidate k per pose.  Returns a NoiseSweep."""
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
    _chk(init_pos, torch.float64, (B, 3), "init_pos"); _chk(init_quat, torch.float64, (B, 4), "init_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    dev = ts.device
    cand = torch.as_tensor(candidates, dtype=torch.float64).to(dev).contiguous()
    if cand.dim() != 2 or cand.shape[1] != 9 or not 1 <= int(cand.shape[0]) <= 4096:
        raise ValueError(f"ekf_noise_sweep_ragged: candidates must be (K, 9) with 1 <= K <= 4096, got {tuple(cand.shape)}")
    K = int(cand.shape[0])
    trace_k = -1 if trace is None else int(trace)
    if trace is not None and not 0 <= trace_k < K:
        raise ValueError(f"ekf_noise_sweep_ragged: trace = {trace_k} names no candidate (K = {K})")
    cfg = EkfConfig.from_config(config or CONFIG)
    f = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    r = NoiseSweep(stats=torch.empty((B, K, 12), **f), best_k=torch.empty((B, 2), **i32), pooled=torch.empty((K, 12), **f),
                   pooled_best=torch.empty((2,), **i32), status=torch.empty((B,), **i32),
                   innov=torch.empty((P, 3), **f) if trace is not None else None, innov_var=torch.empty((P, 3), **f) if trace is not None else None,
                   candidates=cand)
    check(_lib.load().gsf_ekf_noise_sweep_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), _p(run_status), _p(init_pos),
                                              _p(init_quat), C.byref(cfg), B, _p(cand), K, float(skip_seconds), int(min_updates), trace_k, _p(r.stats),
                                              _p(r.best_k), _p(r.pooled), _p(r.pooled_best), _p(r.status), _p(r.innov), _p(r.innov_var)))
    r.nll, r.mean_nis, r.rho1 = _noise_derived(r.stats)
    r.pooled_nll, r.pooled_mean_nis, _ = _noise_derived(r.pooled)
    return r


def sweep_noise_fused(rb, r, candidates, config=None, skip_seconds=0.0, min_updates=1, trace=None):
    """ekf_noise_sweep_ragged on the result r of run_fusion_ragged / run_fusion_batch for the batch rb: the aligned fixes, their mask and
    run_status are r's; the initial pose of every track is row 0 of transform_trajectory's output (EKFGPSSLAM.py:1006) -- r.sim3_pos and
    the Sim3 rotation applied to the first SLAM quaternion -- and NOT row 0 of r.fused, which RTS may have rewritten (an outage from pose 0)."""
    ts, pos, quat = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4)
    offsets = rb.slam_offsets
    B, P = _offsets_chk(offsets), int(ts.numel())
    dev = ts.device
    if P == 0:
        first = torch.zeros((B,), dtype=torch.int64, device=dev)
        ip, iq = torch.zeros((B, 3), dtype=torch.float64, device=dev), torch.zeros((B, 4), dtype=torch.float64, device=dev)
    else:
        first = torch.clamp(offsets[:-1], max=P - 1)                      # (an empty track's row is never read)
        one = torch.arange(B + 1, dtype=torch.int64, device=dev)
        ip = r.sim3_pos.reshape(-1, 3)[first].contiguous()
        _, iq, _ = apply_sim3_batch(pos[first].contiguous(), quat[first].contiguous(), one, r.R, r.t, r.s)
    return ekf_noise_sweep_ragged(ts, pos, quat, r.aligned.reshape(-1, 3), r.valid.reshape(-1), offsets, ip, iq, candidates, config=config,
                                  run_status=r.run_status, skip_seconds=skip_seconds, min_updates=min_updates, trace=trace)


# ---------------------------------------------------------------------------- GNSS outage study (gsf_outage_study_dev)
def outage_scenarios(starts, lengths):
    """Scenarios for outage_study_ragged: every combination of starts x lengths (both in the stamps' unit, starts relative to a track's first
    stamp) as a (K, 2) float64 numpy array of rows [start, length], length-major: scenario k = il * len(starts) + is_."""
    import numpy as np
    st, ln = (np.asarray(list(v) if not np.isscalar(v) else [v], dtype=np.float64).reshape(-1) for v in (starts, lengths))
    K = st.size * ln.size
    if not 1 <= K <= 4096:
        raise ValueError(f"outage_scenarios: {K} scenarios, 1..4096 per call")
    out = np.empty((ln.size, st.size, 2))
    out[..., 0] = st[None, :]
    out[..., 1] = ln[:, None]
    return np.ascontiguousarray(out.reshape(K, 2))


_OS_UNUSABLE = _lib.OS_EMPTY | _lib.OS_UNSORTED | _lib.OS_SKIPPED


class OutageStudy:
    """Result of outage_study_ragged for B tracks x K scenarios (definitions: include/gsf.h, gsf_outage_study_dev).  Device tensors: stats
    (B,K,13); seg (B,K,2) int32 = the outage [a, b) of every scenario, relative to its track; flags (B,K) int32 of _lib.OS_* bits; rms_dr /
    rms_fused (B,K) = sqrt(sum e^2 / |E|) dead-reckoned and fused (NaN where E is empty); drift_pct (B,K) = 100 |y| at the recovery / distance
    travelled; err_dr / err_fused (P,) and trace_pos (P,3) of the traced scenario (None without trace); scenarios (K,2)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def usable(self):
        """(B,K) bool: rows with none of EMPTY | UNSORTED | SKIPPED and at least one evaluated pose"""
        return ((self.flags & _OS_UNUSABLE) == 0) & (self.stats[..., 0] > 0)

    def curve(self):
        """Per distinct scenario length, pooled over the usable rows of all tracks and starts (torch reductions on the device): a dict of
        (n_lengths,) float64 tensors 'length', 'rows', 'rms_dr', 'rms_fused', 'max_dr', 'max_fused', 'mean_gap', 'mean_dist',
        'mean_recovery_nis' (over the rows with a recovery), 'share_smoothed', 'share_sharp'.  NaN where a length has no usable row."""
        st, fl = self.stats, self.flags
        lengths = torch.unique(self.scenarios[:, 1][~torch.isnan(self.scenarios[:, 1])])
        ok = self.usable()
        out = {k: [] for k in ("rows", "rms_dr", "rms_fused", "max_dr", "max_fused", "mean_gap", "mean_dist", "mean_recovery_nis",
                               "share_smoothed", "share_sharp")}
        nan = torch.full((), float("nan"), dtype=torch.float64, device=st.device)
        for L in lengths:
            m = ok & (self.scenarios[:, 1] == L)[None, :]
            w = m.to(torch.float64)
            n, nE = w.sum(), torch.where(m, st[..., 0], torch.zeros_like(w)).sum()       # (where, not a product: skipped rows hold NaN)
            mean = lambda v, ww=w: torch.where(ww.sum() > 0, (torch.where(ww > 0, v, torch.zeros_like(v))).sum() / ww.sum(), nan)
            rec = w * ((fl & _lib.OS_NO_RECOVERY) == 0).to(torch.float64)
            out["rows"].append(n)
            out["rms_dr"].append(torch.where(nE > 0, torch.sqrt((torch.where(m, st[..., 5], torch.zeros_like(w))).sum() / nE), nan))
            out["rms_fused"].append(torch.where(nE > 0, torch.sqrt((torch.where(m, st[..., 7], torch.zeros_like(w))).sum() / nE), nan))
            out["max_dr"].append(torch.where(n > 0, torch.where(m, st[..., 6], torch.zeros_like(w)).max(), nan))
            out["max_fused"].append(torch.where(n > 0, torch.where(m, st[..., 8], torch.zeros_like(w)).max(), nan))
            out["mean_gap"].append(mean(st[..., 3])); out["mean_dist"].append(mean(st[..., 4]))
            out["mean_recovery_nis"].append(mean(st[..., 12], rec))
            out["share_smoothed"].append(mean(((fl & _lib.OS_SMOOTHED) != 0).to(torch.float64)))
            out["share_sharp"].append(mean(((fl & _lib.OS_SHARP_TURN) != 0).to(torch.float64)))
        res = {k: (torch.stack(v) if v else torch.empty((0,), dtype=torch.float64, device=st.device)) for k, v in out.items()}
        res["length"] = lengths
        return res


def outage_study_ragged(ts, pos, quat, gps, valid, offsets, init_pos, init_quat, scenarios, config=None, run_status=None, truth=None,
                        truth_valid=None, trace=None):
    """Drift and RTS gain of the fused track for K withheld GNSS windows per track, one launch chain on torch's current stream
    (gsf_outage_study_dev).  Inputs as ekf_noise_sweep_ragged; the filter runs under config's own noise.  scenarios (K,2) rows
    [start, length] in the stamps' unit, start relative to a track's first stamp (numpy or tensor; outage_scenarios builds a grid), shared by
    all tracks.  truth (P,3) / truth_valid (P,) uint8: what the errors are measured against; both None: the fixes themselves.  trace = k:
    per-pose errors and fused positions of scenario k.  Returns an OutageStudy."""
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
    _chk(init_pos, torch.float64, (B, 3), "init_pos"); _chk(init_quat, torch.float64, (B, 4), "init_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    if (truth is None) != (truth_valid is None):
        raise ValueError("outage_study_ragged: truth and truth_valid go together (both None: the fixes themselves)")
    if truth is not None:
        _chk(truth, torch.float64, (P, 3), "truth"); _chk(truth_valid, torch.uint8, (P,), "truth_valid")
    dev = ts.device
    scen = torch.as_tensor(scenarios, dtype=torch.float64).to(dev).contiguous()
    if scen.dim() != 2 or scen.shape[1] != 2 or not 1 <= int(scen.shape[0]) <= 4096:
        raise ValueError(f"outage_study_ragged: scenarios must be (K, 2) with 1 <= K <= 4096, got {tuple(scen.shape)}")
    K = int(scen.shape[0])
    trace_k = -1 if trace is None else int(trace)
    if trace is not None and not 0 <= trace_k < K:
        raise ValueError(f"outage_study_ragged: trace = {trace_k} names no scenario (K = {K})")
    cfg = EkfConfig.from_config(config or CONFIG)
    f = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    tr = trace is not None
    r = OutageStudy(stats=torch.empty((B, K, 13), **f), seg=torch.empty((B, K, 2), **i32), flags=torch.empty((B, K), **i32),
                    err_dr=torch.empty((P,), **f) if tr else None, err_fused=torch.empty((P,), **f) if tr else None,
                    trace_pos=torch.empty((P, 3), **f) if tr else None, scenarios=scen)
    check(_lib.load().gsf_outage_study_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), _p(run_status), _p(init_pos),
                                           _p(init_quat), C.byref(cfg), B, _p(truth), _p(truth_valid), _p(scen), K, trace_k, _p(r.stats), _p(r.seg),
                                           _p(r.flags), _p(r.err_dr), _p(r.err_fused), _p(r.trace_pos)))
    r.rms_dr, r.rms_fused = torch.sqrt(r.stats[..., 5] / r.stats[..., 0]), torch.sqrt(r.stats[..., 7] / r.stats[..., 0])
    r.drift_pct = 100.0 * r.stats[..., 11] / r.stats[..., 4]
    return r


def outage_study_fused(rb, r, scenarios, truth="primary", config=None, trace=None):
    """outage_study_ragged on the result r of run_fusion_ragged / run_fusion_batch for the batch rb: the aligned fixes, their mask and
    run_status are r's, the initial pose of every track is built as sweep_noise_fused builds it.  truth = "primary": errors against the
    withheld fixes themselves; "gt": against the time-aligned ground-truth leg (r.gt_aligned / r.gt_valid; ValueError without one)."""
    if truth not in ("primary", "gt"):
        raise ValueError(f"outage_study_fused: truth must be 'primary' or 'gt', got {truth!r}")
    tr = tv = None
    if truth == "gt":
        if getattr(r, "gt_aligned", None) is None or getattr(r, "gt_valid", None) is None:
            raise ValueError("outage_study_fused: truth = 'gt' needs a run with a ground-truth leg (r.gt_aligned / r.gt_valid)")
        tr, tv = r.gt_aligned.reshape(-1, 3), r.gt_valid.reshape(-1)
    ts, pos, quat = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4)
    offsets = rb.slam_offsets
    B, P = _offsets_chk(offsets), int(ts.numel())
    dev = ts.device
    if P == 0:
        ip, iq = torch.zeros((B, 3), dtype=torch.float64, device=dev), torch.zeros((B, 4), dtype=torch.float64, device=dev)
    else:
        first = torch.clamp(offsets[:-1], max=P - 1)                      # (an empty track's row is never read)
        one = torch.arange(B + 1, dtype=torch.int64, device=dev)
        ip = r.sim3_pos.reshape(-1, 3)[first].contiguous()
        _, iq, _ = apply_sim3_batch(pos[first].contiguous(), quat[first].contiguous(), one, r.R, r.t, r.s)
    return outage_study_ragged(ts, pos, quat, r.aligned.reshape(-1, 3), r.valid.reshape(-1), offsets, ip, iq, scenarios, config=config,
                               run_status=r.run_status, truth=tr, truth_valid=tv, trace=trace)


# ---------------------------------------------------------------------------- innovation gate (gsf_innovation_gate_dev)
GATE_MAX_K = 64


def _chi2_cdf(x, dof):
    import math
    if dof == 1:
        return math.erf(math.sqrt(x / 2.0))
    if dof == 2:
        return 1.0 - math.exp(-x / 2.0)
    return math.erf(math.sqrt(x / 2.0)) - math.sqrt(2.0 * x / math.pi) * math.exp(-x / 2.0)


def chi2_gate(p, dof=3):
    """The p-quantile of the chi-square distribution with dof degrees of freedom: the gate below which a consistent filter's NIS falls
    with probability p (3 dof: 0.95 -> 7.8147, 0.99 -> 11.3449, 0.999 -> 16.2662).  dof 2 has a closed form; dof 1 and 3 invert the CDF
    (3 dof: erf(sqrt(x/2)) - sqrt(2x/pi) exp(-x/2)) by bisection with math.erf.  Other dof raise ValueError."""
    import math
    p = float(p)
    if dof not in (1, 2, 3):
        raise ValueError(f"chi2_gate: dof must be 1, 2 or 3, got {dof!r}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"chi2_gate: p must be in [0, 1), got {p!r}")
    if dof == 2:
        return -2.0 * math.log1p(-p)
    lo, hi = 0.0, 1.0
    while _chi2_cdf(hi, dof) < p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if _chi2_cdf(mid, dof) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _gates_arg(gates):
    """gates of innovation_gate_ragged -> a float64 (K,) tensor, 1 <= K <= 64.  A sequence or a numpy array is a host array that the
    binding uploads; a tensor is taken as the device array itself, so a host tensor is an error."""
    if isinstance(gates, torch.Tensor):
        if not gates.is_cuda:
            raise ValueError("gates: a tensor must live on the device (pass a sequence or a numpy array to have it uploaded)")
        if gates.dtype != torch.float64:
            raise ValueError(f"gates: expected float64, got {gates.dtype}")
        gt = gates
    else:
        import numpy as np
        a = np.asarray(gates)
        if a.dtype.kind not in "fiu":
            raise ValueError(f"gates: expected numbers, got dtype {a.dtype}")
        gt = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if gt.dim() != 1 or not 1 <= int(gt.shape[0]) <= GATE_MAX_K:
        raise ValueError(f"gates: expected (K,) with 1 <= K <= {GATE_MAX_K}, got {tuple(gt.shape)}")
    return gt


class InnovationGate:
    """Result of innovation_gate_ragged for B tracks x K gates (definitions: include/gsf.h, gsf_innovation_gate_dev).  Device tensors:
    valid_out (K,P) uint8; stats (B,K,8) = n_avail, n_tested, n_rejected, n_forced, longest rejected run, first rejected pose (-1: none),
    largest and summed NIS of the tested fixes that were applied; status (B,) int32 of _lib.GATE_* bits; nis_out (K,P) or None; gates
    (K,); valid_in (P,) = the mask the gate started from; offsets (B+1,); init_pos / init_quat as passed in."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def _k(self, k):
        k = int(k)
        if not 0 <= k < int(self.gates.shape[0]):
            raise ValueError(f"InnovationGate: no gate {k} (K = {int(self.gates.shape[0])})")
        return k

    def valid(self, k=0):
        """(P,) uint8: the mask with gate k's rejected bytes cleared -- feed it to ekf_fuse_ragged / ekf_covariance_ragged"""
        return self.valid_out[self._k(k)]

    def rejected(self, k=0):
        """(P,) bool: the poses whose fix gate k rejected (none on a track the gate skipped, whose bytes are all zero)"""
        rej = (self.valid_in != 0) & (self.valid_out[self._k(k)] == 0)
        if getattr(self, "status", None) is None or getattr(self, "offsets", None) is None:
            return rej
        skipped = (self.status & _lib.GATE_SKIPPED) != 0
        n = self.offsets[1:] - self.offsets[:-1]
        return rej & ~torch.repeat_interleave(skipped, n, output_size=int(rej.shape[0]))

    def nis(self, k=0):
        if self.nis_out is None:
            raise ValueError("InnovationGate.nis: the call was made without want_nis")
        return self.nis_out[self._k(k)]

    @property
    def reject_rate(self):
        """(B,K): rejected / tested per track and gate (NaN where nothing was tested)"""
        return self.stats[..., 2] / self.stats[..., 1]

    def table(self):
        """Per gate, pooled over the tracks that ran (no SKIPPED / EMPTY / UNSORTED bit): a dict of (K,) float64 tensors 'gate', 'tested',
        'rejected', 'forced', 'reject_rate', 'longest_run' -- what a threshold is chosen from."""
        bad = _lib.GATE_SKIPPED | _lib.GATE_EMPTY | _lib.GATE_UNSORTED
        ok = ((self.status & bad) == 0)[:, None, None].expand_as(self.stats)
        st = torch.where(ok, self.stats, torch.zeros_like(self.stats))    # (where, not a product: skipped rows hold NaN)
        tested, rej = st[..., 1].sum(dim=0), st[..., 2].sum(dim=0)
        longest = st[..., 4].max(dim=0).values if st.shape[0] else torch.zeros_like(tested)
        return dict(gate=self.gates, tested=tested, rejected=rej, forced=st[..., 3].sum(dim=0), reject_rate=rej / tested, longest_run=longest)


def innovation_gate_ragged(ts, pos, quat, gps, valid, offsets, init_pos, init_quat, gates, config=None, run_status=None, arm_seconds=0.0,
                           max_run=0, want_nis=False):
    """Chi-square gate on the filter's own innovations for K thresholds per track, one launch on torch's current stream
    (gsf_innovation_gate_dev).  Inputs as ekf_noise_sweep_ragged; the filter runs under config's own noise.  gates: K thresholds on the
    NIS, 1 <= K <= 64 (a sequence, a numpy array or a tensor on ts's device; chi2_gate gives quantiles; inf rejects nothing).  A fix is
    tested once its stamp exceeds ts[0] + arm_seconds and rejected when its NIS is above the gate, unless the max_run fixes before it were
    all rejected (max_run <= 0: no limit).  A rejected fix is a pose without a fix in every respect, so the returned masks go straight
    into ekf_fuse_ragged / ekf_covariance_ragged.  want_nis: also the NIS of every usable fix, (K,P).  Returns an InnovationGate."""
    gt = _gates_arg(gates)                                                # (first: these errors need no device)
    arm_seconds = float(arm_seconds)
    if arm_seconds != arm_seconds:
        raise ValueError("innovation_gate_ragged: arm_seconds is NaN")
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
    _chk(init_pos, torch.float64, (B, 3), "init_pos"); _chk(init_quat, torch.float64, (B, 4), "init_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    dev = ts.device
    gt = gt.to(dev).contiguous()
    K = int(gt.shape[0])
    cfg = EkfConfig.from_config(config or CONFIG)
    g = InnovationGate(valid_out=torch.empty((K, P), dtype=torch.uint8, device=dev), stats=torch.empty((B, K, 8), dtype=torch.float64, device=dev),
                       status=torch.empty((B,), dtype=torch.int32, device=dev),
                       nis_out=torch.empty((K, P), dtype=torch.float64, device=dev) if want_nis else None, gates=gt, valid_in=valid, offsets=offsets,
                       init_pos=init_pos, init_quat=init_quat, arm_seconds=arm_seconds, max_run=int(max_run))
    check(_lib.load().gsf_innovation_gate_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), _p(run_status), _p(init_pos),
                                              _p(init_quat), C.byref(cfg), B, _p(gt), K, arm_seconds, int(max_run), _p(g.valid_out), _p(g.nis_out),
                                              _p(g.stats), _p(g.status)))
    return g


def _fused_init_pose(rb, r):
    """init_pos (B,3) / init_quat (B,4) of every track of a run_fusion_ragged result, as sweep_noise_fused builds them"""
    ts, pos, quat = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4)
    offsets = rb.slam_offsets
    B, P = _offsets_chk(offsets), int(ts.numel())
    dev = ts.device
    if P == 0:
        return torch.zeros((B, 3), dtype=torch.float64, device=dev), torch.zeros((B, 4), dtype=torch.float64, device=dev)
    first = torch.clamp(offsets[:-1], max=P - 1)                          # (an empty track's row is never read)
    one = torch.arange(B + 1, dtype=torch.int64, device=dev)
    ip = r.sim3_pos.reshape(-1, 3)[first].contiguous()
    _, iq, _ = apply_sim3_batch(pos[first].contiguous(), quat[first].contiguous(), one, r.R, r.t, r.s)
    return ip, iq


def gate_fused(rb, r, gates, config=None, arm_seconds=0.0, max_run=0, want_nis=False):
    """innovation_gate_ragged on the result r of run_fusion_ragged / run_fusion_batch for the batch rb: the aligned fixes, their mask and
    run_status are r's, the initial pose of every track is built as sweep_noise_fused builds it."""
    ip, iq = _fused_init_pose(rb, r)
    return innovation_gate_ragged(rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), r.aligned.reshape(-1, 3), r.valid.reshape(-1),
                                  rb.slam_offsets, ip, iq, gates, config=config, run_status=r.run_status, arm_seconds=arm_seconds,
                                  max_run=max_run, want_nis=want_nis)


def _step6_rows(ts, offsets, trajs, aligned, valid, skip_seconds):
    """step 6's nearest-fix error of several trajectories of the same ragged batch (eval_errors_batch on the tracks padded to one length;
    padded rows are not evaluated) -> [(stats (B,4), errors (P,))] in the order of trajs"""
    B, P = _offsets_chk(offsets), int(ts.numel())
    dev = ts.device
    if P == 0:
        return [(torch.zeros((B, 4), dtype=torch.float64, device=dev), torch.empty((0,), dtype=torch.float64, device=dev)) for _ in trajs]
    off = offsets.cpu().tolist()
    N = max([off[b + 1] - off[b] for b in range(B)] + [1])
    row = torch.arange(N, dtype=torch.int64, device=dev)[None, :]
    n = (offsets[1:] - offsets[:-1])[:, None]
    inside = row < n
    idx = torch.clamp(offsets[:-1, None] + torch.minimum(row, torch.clamp(n - 1, min=0)), max=max(P - 1, 0))
    dv = torch.where(inside, valid[idx], torch.zeros_like(valid[idx])).contiguous()
    out = []
    for p in trajs:
        stats, err = eval_errors_batch(ts[idx].contiguous(), p[idx].contiguous(), aligned[idx].contiguous(), dv, skip_seconds=skip_seconds)
        errors = torch.full((P,), float("nan"), dtype=torch.float64, device=dev)
        errors[idx[inside]] = err[inside]
        out.append((stats, errors))
    return out


def smooth_fused(rb, r, valid=None, config=None, skip_seconds=5.0):
    """ekf_smooth_ragged on the result r of run_fusion_ragged for the batch rb: the aligned fixes, their mask and run_status are r's (valid=:
    another mask over the same rows, e.g. g.valid(k) of gate_fused), the initial pose of every track is built as sweep_noise_fused builds
    it.  Returns the SmoothedTrack (with the filter's own track) carrying step 6's nearest-fix error of the fused track r returned and of
    the smoothed one against the fixes of the mask: err_stats2 (2,B,4) = {fused, smoothed} x {count, mean, median, RMSE}, errors2 (2,P)
    (NaN where not evaluated)."""
    ts, aligned, offsets = rb.ts.reshape(-1), r.aligned.reshape(-1, 3), rb.slam_offsets
    v = (r.valid.reshape(-1) if valid is None else valid).contiguous()
    ip, iq = _fused_init_pose(rb, r)
    st = ekf_smooth_ragged(ts, rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), aligned, v, offsets, ip, iq, config=config, run_status=r.run_status,
                           want_filtered=True)
    rows = _step6_rows(ts, offsets, (r.fused.pos.reshape(-1, 3), st.pos), aligned, v, skip_seconds)
    st.err_stats2, st.errors2 = torch.stack([x[0] for x in rows]), torch.stack([x[1] for x in rows])
    st.valid, st.init_pos, st.init_quat = v, ip, iq
    return st


def refuse_gated(rb, r, g, k=0, want_cov=False, skip_seconds=5.0, config=None):
    """Fuse again with gate k's mask: the existing ekf_fuse_ragged on g.valid(k) (g from gate_fused), optionally ekf_covariance_ragged on
    the same mask, and step 6's nearest-fix error of the gated track against the fixes the gate kept (eval_errors_batch on the tracks
    padded to one length; padded rows are not evaluated).  Tracks the run skipped (r.run_status != 0) are fused from whatever their rows
    hold and should be ignored, as g.status says.  Returns a RunResult with pos (P,3), quat (P,4), status (B,), valid (P,), err_stats
    (B,4) = count, mean, median, RMSE, errors (P,) (NaN where not evaluated) and cov (FusedCovariance or None)."""
    ts, pos, quat = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4)
    aligned, offsets = r.aligned.reshape(-1, 3), rb.slam_offsets
    vk = g.valid(k).contiguous()
    po, qo, st = ekf_fuse_ragged(ts, pos, quat, aligned, vk, offsets, g.init_pos, g.init_quat, config=config)
    cov = ekf_covariance_ragged(ts, quat, aligned, vk, offsets, config=config, run_status=r.run_status) if want_cov else None
    (stats, errors), = _step6_rows(ts, offsets, (po,), aligned, vk, skip_seconds)
    return RunResult(pos=po, quat=qo, status=st, valid=vk, err_stats=stats, errors=errors, cov=cov)


# ---------------------------------------------------------------------------- per-fix GNSS noise (gsf_ekf_smooth_weighted_dev, gsf_fix_var_at_poses_dev)
class WeightedTrack(SmoothedTrack):
    """ekf_smooth_weighted_ragged's result: a SmoothedTrack of the filter and smoother run with a measurement variance per pose, plus
    nis (P,) or None = the normalised innovation squared of every used row (NaN elsewhere; mean 3 for a consistent filter) and
    bad_sigma (P,) bool = the rows flagged _lib.POSE_BAD_SIGMA: a fix whose variance was not usable and that was treated as missing."""

    def __init__(self, pos, quat, cov, pos_filt, cov_filt, flags, status, offsets, nis=None):
        super().__init__(pos, quat, cov, pos_filt, cov_filt, flags, status, offsets)
        self.nis = nis

    @property
    def bad_sigma(self):
        return (self.flags & _lib.POSE_BAD_SIGMA) != 0

    def mean_nis(self):
        """(B,) mean of nis over the used rows of every track (NaN for a track without one; needs want_nis=True)"""
        if self.nis is None:
            raise ValueError("WeightedTrack.mean_nis: nis was not asked for (want_nis=True)")
        B, P = int(self.offsets.numel()) - 1, int(self.nis.numel())
        used = ~torch.isnan(self.nis)
        n = (self.offsets[1:] - self.offsets[:-1]).to(self.nis.device)
        track = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=self.nis.device), n, output_size=P)
        zero = torch.zeros((B,), dtype=torch.float64, device=self.nis.device)
        total = zero.index_add(0, track, torch.where(used, self.nis, torch.zeros_like(self.nis)))
        count = zero.index_add(0, track, used.to(torch.float64))
        return total / count


def ekf_smooth_weighted_ragged(ts, pos, quat, gps, valid, meas_var, offsets, init_pos, init_quat, config=None, run_status=None, want_filtered=False,
                               want_nis=False):
    """ekf_smooth_ragged with a measurement variance per pose (gsf_ekf_smooth_weighted_dev; definition: include/gsf.h), one launch on torch's
    current stream.  meas_var (P,3) float64 = the variance of fix i per axis in the unit of config['ekf']['meas_noise_diag'], which is not
    read.  A variance is usable when 1e-8 <= v <= 1e8; a row with a fix but an unusable variance is a pose without a fix in every respect
    and is flagged POSE_BAD_SIGMA -- unless all three are +inf ("no information": no fix, no flag).  The other arguments as
    ekf_smooth_ragged; want_nis: also the normalised innovation squared of every used row.  Returns a WeightedTrack."""
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid"); _chk(meas_var, torch.float64, (P, 3), "meas_var")
    _chk(init_pos, torch.float64, (B, 3), "init_pos"); _chk(init_quat, torch.float64, (B, 4), "init_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    cfg = EkfConfig.from_config(config or CONFIG)
    f = dict(dtype=torch.float64, device=ts.device)
    st = WeightedTrack(torch.empty((P, 3), **f), torch.empty((P, 4), **f), torch.empty((P, 7), **f),
                       torch.empty((P, 3), **f) if want_filtered else None, torch.empty((P, 7), **f) if want_filtered else None,
                       torch.empty((P,), dtype=torch.uint8, device=ts.device), torch.empty((B,), dtype=torch.int32, device=ts.device), offsets,
                       torch.empty((P,), **f) if want_nis else None)
    check(_lib.load().gsf_ekf_smooth_weighted_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(meas_var), _p(offsets),
                                                  _p(init_pos), _p(init_quat), _p(run_status), C.byref(cfg), B, _p(st.pos), _p(st.quat), _p(st.cov),
                                                  _p(st.pos_filt), _p(st.cov_filt), _p(st.flags), _p(st.status), _p(st.nis)))
    return st


def fix_var_at_poses_ragged(ts, slam_offsets, gps_t, gps_offsets, fix_var, keep=None, valid=None):
    """Per-fix variances carried onto SLAM stamps (gsf_fix_var_at_poses_dev; definition: include/gsf.h): ts (P,) with slam_offsets (B+1,),
    gps_t (T,) ascending per log with gps_offsets (B+1,), fix_var (T,3), keep (T,) uint8 = the pre-filter's mask (None: all kept), valid
    (P,) uint8 or None.  A pose takes, per axis, the larger variance of the kept fixes that bracket its stamp; +inf x3 where valid is 0 or
    a side of the bracket is missing.  ValueError where the offsets do not end at the rows given (the kernel would hand the poses behind
    the last offset to the last track).  Returns pose_var (P,3), the meas_var of ekf_smooth_weighted_ragged."""
    B = _offsets_chk(slam_offsets)
    if _offsets_chk(gps_offsets) != B:
        raise ValueError("fix_var_at_poses_ragged: slam_offsets and gps_offsets must describe the same tracks")
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    T = int(gps_t.shape[0]) if gps_t.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(gps_t, torch.float64, (T,), "gps_t"); _chk(fix_var, torch.float64, (T, 3), "fix_var")
    if keep is not None:
        _chk(keep, torch.uint8, (T,), "keep")
    if valid is not None:
        _chk(valid, torch.uint8, (P,), "valid")
    ends = torch.stack((slam_offsets[0], slam_offsets[-1], gps_offsets[0], gps_offsets[-1])).cpu().tolist()      # one small copy to the host
    if ends != [0, P, 0, T]:
        raise ValueError(f"fix_var_at_poses_ragged: slam_offsets must run from 0 to the {P} poses given and gps_offsets from 0 to the {T} fixes given "
                         f"(they run {ends[0]}..{ends[1]} and {ends[2]}..{ends[3]})")
    out = torch.empty((P, 3), dtype=torch.float64, device=ts.device)
    check(_lib.load().gsf_fix_var_at_poses_dev(context().handle, _p(ts), _p(slam_offsets), _p(gps_t), _p(gps_offsets), _p(keep), _p(fix_var),
                                               _p(valid), B, P, _p(out)))
    return out


def read_gnss_quality(paths):
    """The columns behind the fourth of each GNSS text file (GPSmerge.py:41-60 writes numsats and velmode there; load_gps_data and
    RaggedGeodeticBatch.from_files drop them), parsed as _read_gnss_file parses the file, in from_files order: a flat (T, C) float64 numpy
    array on the host whose rows line up with the batch's gps_t.  ValueError naming the file if it has no such column, or another count
    of them than the files before it."""
    import numpy as np
    parts, C_ = [], None
    for path in paths:
        try:
            try:
                raw = np.loadtxt(path, delimiter=" ")
            except ValueError:
                raw = np.loadtxt(path, delimiter=",")
        except Exception as e:
            raise ValueError(f"GNSS file {path}: {e}") from e
        if raw.ndim == 1:
            raw = raw.reshape(1, -1)
        if raw.shape[1] < 4:                                             # an empty file included: _read_gnss_file raises on it as well
            raise ValueError(f"GNSS file {path}: needs at least 4 columns (ts lat lon alt), got {raw.shape[1]}")
        if raw.shape[1] < 5:
            raise ValueError(f"GNSS file {path}: no quality column behind ts lat lon alt ({raw.shape[1]} columns)")
        if C_ is not None and raw.shape[1] - 4 != C_:
            raise ValueError(f"GNSS file {path}: {raw.shape[1] - 4} quality columns, the files before it have {C_}")
        C_ = raw.shape[1] - 4
        parts.append(np.asarray(raw[:, 4:], dtype=np.float64))
    if not parts:
        return np.zeros((0, 0))
    return np.ascontiguousarray(np.concatenate(parts))


def quality_to_var(codes, table, default=float("inf")):
    """A lookup from an integer quality column (velmode, an NMEA fix type, ...) to a variance triple: codes (T,) of any integer or float
    dtype, table = {code: (var_x, var_y, var_z)} (e.g. {4: (s_h**2, s_h**2, s_v**2)} for RTK-fixed) -> (T,3) float64 on codes' device;
    a code the table does not hold gets `default` on all three axes (+inf: "no information", the fix is not used and not flagged)."""
    codes = torch.as_tensor(codes)
    out = torch.full((int(codes.numel()), 3), float(default), dtype=torch.float64, device=codes.device)
    flat = codes.reshape(-1)
    for code, var in table.items():
        v = torch.as_tensor([float(x) for x in var], dtype=torch.float64, device=codes.device)
        if v.numel() != 3:
            raise ValueError(f"quality_to_var: code {code} needs three variances")
        out[flat == code] = v
    return out


def smooth_weighted_fused(rb, r, fix_var, valid=None, config=None, skip_seconds=5.0):
    """ekf_smooth_weighted_ragged on the result r of run_fusion_ragged for the batch rb.  fix_var (T,3) = a variance per fix of rb's logs
    (quality_to_var of read_gnss_quality's columns, or a receiver's own figures); fix_var_at_poses_ragged carries it onto the SLAM stamps
    through the fixes the pre-filter kept (r.gps_keep) and the mask (r.valid, or valid=: another mask over the same rows, e.g. g.valid(k)
    of gate_fused); the initial pose of every track is built as sweep_noise_fused builds it.  Returns the WeightedTrack (with the filter's
    own track and nis) carrying pose_var (P,3) and step 6's nearest-fix error of four tracks against the fixes of the mask: err_stats4
    (4,B,4) = {raw SLAM, Sim3, weighted filter, weighted smoother} x {count, mean, median, RMSE}, errors4 (4,P) (NaN where not evaluated)."""
    ts, aligned, offsets = rb.ts.reshape(-1), r.aligned.reshape(-1, 3), rb.slam_offsets
    v = (r.valid.reshape(-1) if valid is None else valid).contiguous()
    pose_var = fix_var_at_poses_ragged(ts, offsets, rb.gps_t, rb.gps_offsets, fix_var, keep=r.gps_keep, valid=v)
    ip, iq = _fused_init_pose(rb, r)
    st = ekf_smooth_weighted_ragged(ts, rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), aligned, v, pose_var, offsets, ip, iq, config=config,
                                    run_status=r.run_status, want_filtered=True, want_nis=True)
    rows = _step6_rows(ts, offsets, (rb.pos.reshape(-1, 3), r.sim3_pos.reshape(-1, 3), st.pos_filt, st.pos), aligned, v, skip_seconds)
    st.err_stats4, st.errors4 = torch.stack([x[0] for x in rows]), torch.stack([x[1] for x in rows])
    st.valid, st.init_pos, st.init_quat, st.pose_var = v, ip, iq, pose_var
    return st


# ---------------------------------------------------------------------------- robust smoothing (gsf_ekf_smooth_reweighted_dev)
_LOSSES = {"huber": _lib.REWEIGHT_HUBER, "cauchy": _lib.REWEIGHT_CAUCHY}


class ReweightedTrack(WeightedTrack):
    """ekf_smooth_reweighted_ragged's result: the WeightedTrack of the LAST solve (nis under its effective variances), plus weight (P,) =
    the weights computed from that solve's track (NaN on rows without an update), rounds_used (B,) int32 = the reweighted solves done,
    w_change (B,) = the largest step of a weight in the last solve (0 at a fixed point), and meas_var (P,3) = the variances given."""

    def __init__(self, pos, quat, cov, pos_filt, cov_filt, flags, status, offsets, nis, weight, rounds_used, w_change, meas_var):
        super().__init__(pos, quat, cov, pos_filt, cov_filt, flags, status, offsets, nis)
        self.weight, self.rounds_used, self.w_change, self.meas_var = weight, rounds_used, w_change, meas_var

    def downweighted(self, below=0.5):
        """(P,) bool: the used rows whose weight fell below `below` -- the fixes the loss disbelieves"""
        return self.weight < below                                      # (NaN compares false)

    def effective_var(self):
        """(P,3): min(meas_var / weight, 1e8) on the used rows -- what one more solve would run with -- and meas_var elsewhere"""
        cap = torch.full_like(self.meas_var, 1e8)
        return torch.where(torch.isnan(self.weight)[:, None], self.meas_var, torch.minimum(self.meas_var / self.weight[:, None], cap))


def ekf_smooth_reweighted_ragged(ts, pos, quat, gps, valid, offsets, init_pos, init_quat, meas_var=None, loss="huber", c2=None, rounds=5, config=None,
                                 run_status=None, want_filtered=False, want_nis=False):
    """The weighted smoother made robust by iteratively reweighted least squares, every round inside ONE launch
    (gsf_ekf_smooth_reweighted_dev; definition: include/gsf.h).  Solve 0 is ekf_smooth_weighted_ragged on meas_var (P,3) -- None:
    config['ekf']['meas_noise_diag'] on every row; after each solve every used fix's residual against the smoothed track gives u2 (with the
    GIVEN variance) and a weight -- loss 'huber': 1 for u2 <= c2, else sqrt(c2 / u2); 'cauchy': 1 / (1 + u2 / c2) -- and the next solve runs
    with min(meas_var / w, 1e8).  c2: a chi-square threshold of 3 degrees of freedom (None: chi2_gate(0.95) = 7.81).  It stops after
    `rounds` reweighted solves (0..32) or, per track, at a fixed point of the weights.  The other arguments as ekf_smooth_weighted_ragged.
    Returns a ReweightedTrack."""
    if loss not in _LOSSES:
        raise ValueError(f"ekf_smooth_reweighted_ragged: loss must be 'huber' or 'cauchy', got {loss!r}")
    c2 = chi2_gate(0.95) if c2 is None else float(c2)
    if not (0.0 < c2 < float("inf")):
        raise ValueError(f"ekf_smooth_reweighted_ragged: c2 must be finite and > 0, got {c2!r}")
    if not (isinstance(rounds, int) and 0 <= rounds <= _lib.REWEIGHT_MAX_ROUNDS):
        raise ValueError(f"ekf_smooth_reweighted_ragged: rounds must be an int in [0, {_lib.REWEIGHT_MAX_ROUNDS}], got {rounds!r}")
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
    if meas_var is not None:
        _chk(meas_var, torch.float64, (P, 3), "meas_var")
    _chk(init_pos, torch.float64, (B, 3), "init_pos"); _chk(init_quat, torch.float64, (B, 4), "init_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    cfg = EkfConfig.from_config(config or CONFIG)
    f = dict(dtype=torch.float64, device=ts.device)
    given = meas_var if meas_var is not None else torch.tensor(list(cfg.meas_noise_diag)[:3], **f).expand(P, 3)
    st = ReweightedTrack(torch.empty((P, 3), **f), torch.empty((P, 4), **f), torch.empty((P, 7), **f),
                         torch.empty((P, 3), **f) if want_filtered else None, torch.empty((P, 7), **f) if want_filtered else None,
                         torch.empty((P,), dtype=torch.uint8, device=ts.device), torch.empty((B,), dtype=torch.int32, device=ts.device), offsets,
                         torch.empty((P,), **f) if want_nis else None, torch.empty((P,), **f),
                         torch.empty((B,), dtype=torch.int32, device=ts.device), torch.empty((B,), **f), given)
    check(_lib.load().gsf_ekf_smooth_reweighted_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(meas_var), _p(offsets),
                                                    _p(init_pos), _p(init_quat), _p(run_status), C.byref(cfg), B, _LOSSES[loss], c2, rounds,
                                                    _p(st.pos), _p(st.quat), _p(st.cov), _p(st.pos_filt), _p(st.cov_filt), _p(st.flags),
                                                    _p(st.status), _p(st.nis), _p(st.weight), _p(st.rounds_used), _p(st.w_change)))
    return st


def smooth_reweighted_fused(rb, r, fix_var=None, valid=None, loss="huber", c2=None, rounds=5, config=None, skip_seconds=5.0):
    """ekf_smooth_reweighted_ragged on the result r of run_fusion_ragged for the batch rb, built like smooth_weighted_fused: fix_var (T,3)
    (None: the config's meas_noise_diag for every fix) is carried onto the SLAM stamps by fix_var_at_poses_ragged through the fixes the
    pre-filter kept and the mask (r.valid, or valid=: another mask over the same rows, e.g. g.valid(k) of gate_fused).  Returns the
    ReweightedTrack (with the filter's own track and nis) carrying pose_var (P,3) or None, smoothed_pos (P,3) = the weighted smoother's
    track before any round (one more launch, rounds = 0), and step 6's nearest-fix error of four tracks against the fixes of the mask:
    err_stats4 (4,B,4) = {raw SLAM, Sim3, the weighted smoother, the reweighted smoother} x {count, mean, median, RMSE}, errors4 (4,P)
    (NaN where not evaluated).  The fixes of the mask include the outliers: the figures say how far each track follows them."""
    ts, aligned, offsets = rb.ts.reshape(-1), r.aligned.reshape(-1, 3), rb.slam_offsets
    v = (r.valid.reshape(-1) if valid is None else valid).contiguous()
    pose_var = None if fix_var is None else fix_var_at_poses_ragged(ts, offsets, rb.gps_t, rb.gps_offsets, fix_var, keep=r.gps_keep, valid=v)
    ip, iq = _fused_init_pose(rb, r)
    st = ekf_smooth_reweighted_ragged(ts, rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), aligned, v, offsets, ip, iq, meas_var=pose_var, loss=loss, c2=c2,
                                      rounds=rounds, config=config, run_status=r.run_status, want_filtered=True, want_nis=True)
    base = ekf_smooth_reweighted_ragged(ts, rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), aligned, v, offsets, ip, iq, meas_var=pose_var, loss=loss, c2=c2,
                                        rounds=0, config=config, run_status=r.run_status)
    rows = _step6_rows(ts, offsets, (rb.pos.reshape(-1, 3), r.sim3_pos.reshape(-1, 3), base.pos, st.pos), aligned, v, skip_seconds)
    st.err_stats4, st.errors4 = torch.stack([x[0] for x in rows]), torch.stack([x[1] for x in rows])
    st.valid, st.init_pos, st.init_quat, st.pose_var, st.smoothed_pos = v, ip, iq, pose_var, base.pos
    return st


# ---------------------------------------------------------------------------- local Sim3 alignment (gsf_sim3_local_fit_dev / _apply_dev)
_LOCAL_MODES = {"scale": _lib.LOC_SCALE, "sim3": _lib.LOC_SIM3}


def _local_config(mode, min_rows, spacing, half_window, rot_open, ratio_max):
    """the arguments of the local alignment as a gsf_local_config, checked as the entry checks them (these errors need no device)"""
    if mode not in _LOCAL_MODES:
        raise ValueError(f"local alignment: mode must be 'scale' or 'sim3', got {mode!r}")
    c = _lib.LocalConfig()
    c.mode, c.min_rows = _LOCAL_MODES[mode], int(min_rows)
    c.spacing, c.half_window, c.rot_open, c.ratio_max = float(spacing), float(half_window), float(rot_open), float(ratio_max)
    if c.min_rows < (3 if c.mode == _lib.LOC_SIM3 else 2):
        raise ValueError("local alignment: min_rows must be >= 2 (mode 'scale') / >= 3 (mode 'sim3')")
    if not (0.0 < c.spacing < float("inf")):
        raise ValueError("local alignment: spacing must be positive and finite")
    if not c.half_window >= 0.0:
        raise ValueError("local alignment: half_window must be >= 0")
    if not (c.rot_open >= 0.0 and c.ratio_max >= 1.0):
        raise ValueError("local alignment: rot_open must be >= 0 and ratio_max >= 1")
    return c


class LocalAlignment:
    """Result of local_align_ragged / local_apply_ragged for B tracks with a knot stride of Kmax (definitions: include/gsf.h,
    gsf_sim3_local_fit_dev).  Device tensors: knot_R (B,Kmax,9), knot_t (B,Kmax,3), knot_s, knot_rms (B,Kmax), knot_n, knot_flags (B,Kmax)
    int32 (_lib.KNOT_* bits), n_knots, track_status (B,) int32 (_lib.LOC_* bits), and per pose pos (P,3), quat (P,4), scale_at (P,),
    pose_flags (P,) int32 (_lib.LP_* bits).  pos / quat are a track like any other: they go straight into ekf_fuse_ragged,
    outage_study_ragged, ekf_noise_sweep_ragged and innovation_gate_ragged as the motion source."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def scale_curve(self, b):
        """(stamps, s_k, valid) of track b's knots, on the host: tau_k = t0 + k spacing, s_k (NaN where invalid), valid as bool"""
        K = int(self.n_knots[b].item())
        o = int(self.offsets[b].item())
        t0 = float(self.ts[o].item()) if K else 0.0
        s = self.knot_s[b, :K].cpu().numpy()
        ok = (self.knot_flags[b, :K].cpu().numpy() & (_lib.KNOT_FEW | _lib.KNOT_VAR0 | _lib.KNOT_SCALE)) == 0
        return (t0 + self.spacing * torch.arange(K, dtype=torch.float64)).numpy(), s, ok

    def drift(self, b):
        """(largest, smallest) valid s_k / s_global of track b; (nan, nan) where no knot is valid"""
        _, s, ok = self.scale_curve(b)
        if not ok.any():
            return float("nan"), float("nan")
        r = s[ok] / float(self.s[b].item())
        return float(r.max()), float(r.min())


def _local_args(ts, pos, quat, offsets, R, t, s):
    B = _offsets_chk(offsets)
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(R, torch.float64, (B, 9), "R"); _chk(t, torch.float64, (B, 3), "t"); _chk(s, torch.float64, (B,), "s")
    return B, P


def _knot_stride(ts, offsets, spacing, B, P):
    """the largest K_b of the batch (one small reduction and one number read back), at least 1 and at most _lib.LOC_KMAX"""
    if B == 0 or P == 0:
        return 1
    n = offsets[1:] - offsets[:-1]
    first, last = torch.clamp(offsets[:-1], max=P - 1), torch.clamp(offsets[1:] - 1, min=0, max=P - 1)
    K = torch.floor((ts[last] - ts[first]) / spacing) + 2.0
    K = torch.where((n > 0) & torch.isfinite(K), K, torch.ones_like(K))
    return int(min(max(float(K.max().item()), 1.0), float(_lib.LOC_KMAX)))


def local_apply_ragged(ts, pos, quat, offsets, R, t, s, spacing, knot_R, knot_t, knot_s, knot_flags, n_knots, track_status):
    """The blend of gsf_sim3_local_apply_dev under FED knots (the caller's own, or a LocalAlignment's after editing): knot_R (B,Kmax,9),
    knot_t (B,Kmax,3), knot_s (B,Kmax), knot_flags (B,Kmax) int32, n_knots, track_status (B,) int32.  One launch pair on torch's current
    stream.  Returns pos (P,3), quat (P,4), scale_at (P,), pose_flags (P,) int32."""
    B, P = _local_args(ts, pos, quat, offsets, R, t, s)
    Kmax = int(knot_s.shape[1]) if knot_s.dim() == 2 else -1
    if not 1 <= Kmax <= _lib.LOC_KMAX:
        raise ValueError(f"local_apply_ragged: the knot stride must be in [1, {_lib.LOC_KMAX}]")
    _chk(knot_R, torch.float64, (B, Kmax, 9), "knot_R"); _chk(knot_t, torch.float64, (B, Kmax, 3), "knot_t"); _chk(knot_s, torch.float64, (B, Kmax), "knot_s")
    _chk(knot_flags, torch.int32, (B, Kmax), "knot_flags"); _chk(n_knots, torch.int32, (B,), "n_knots"); _chk(track_status, torch.int32, (B,), "track_status")
    dev = ts.device
    po, qo = torch.empty_like(pos), torch.empty_like(quat)
    sc, fl = torch.empty((P,), dtype=torch.float64, device=dev), torch.empty((P,), dtype=torch.int32, device=dev)
    check(_lib.load().gsf_sim3_local_apply_dev(context().handle, _p(ts), _p(pos), _p(quat), _p(offsets), B, _p(R), _p(t), _p(s), float(spacing), Kmax,
                                               _p(knot_R), _p(knot_t), _p(knot_s), _p(knot_flags), _p(n_knots), _p(track_status), _p(po), _p(qo),
                                               _p(sc), _p(fl)))
    return po, qo, sc, fl


def local_align_ragged(ts, pos, quat, gps, valid, offsets, R, t, s, spacing=30.0, half_window=30.0, min_rows=8, mode="scale", rot_open=1e-3,
                       ratio_max=2.0, run_status=None, max_knots=None):
    """Local Sim3 alignment of B ragged tracks on torch's current stream: Sim3 knots every `spacing` seconds, each fitted on the usable
    rows within `half_window` of it, and every pose mapped by the blend of its neighbouring valid knots (gsf_sim3_local_fit_dev then
    gsf_sim3_local_apply_dev; definitions in include/gsf.h).  ts (P,), pos (P,3), quat (P,4): the original SLAM tracks; gps (P,3) / valid
    (P,) uint8 as the time alignment returns them; R (B,9), t (B,3), s (B,): each track's global Sim3.  mode "scale" fits scale and
    translation per knot under the global rotation (well posed on a straight road), "sim3" the full closed form with "scale" as the
    fall-back of a rotation-open window.  run_status (B,) int32: tracks with a non-zero word pass through as NaN rows
    (_lib.LOC_SKIPPED).  max_knots: the knot stride, by default the largest K_b of the batch (one number read back).  Returns a
    LocalAlignment."""
    cfg = _local_config(mode, min_rows, spacing, half_window, rot_open, ratio_max)
    if max_knots is not None and not 1 <= int(max_knots) <= _lib.LOC_KMAX:
        raise ValueError(f"local_align_ragged: max_knots must be in [1, {_lib.LOC_KMAX}]")
    B, P = _local_args(ts, pos, quat, offsets, R, t, s)
    _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    Kmax = int(max_knots) if max_knots is not None else _knot_stride(ts, offsets, cfg.spacing, B, P)
    dev = ts.device
    f = dict(dtype=torch.float64, device=dev)
    i = dict(dtype=torch.int32, device=dev)
    la = LocalAlignment(knot_R=torch.empty((B, Kmax, 9), **f), knot_t=torch.empty((B, Kmax, 3), **f), knot_s=torch.empty((B, Kmax), **f),
                        knot_n=torch.empty((B, Kmax), **i), knot_rms=torch.empty((B, Kmax), **f), knot_flags=torch.empty((B, Kmax), **i),
                        n_knots=torch.empty((B,), **i), track_status=torch.empty((B,), **i), ts=ts, offsets=offsets, R=R, t=t, s=s,
                        spacing=cfg.spacing, half_window=cfg.half_window, mode=mode)
    check(_lib.load().gsf_sim3_local_fit_dev(context().handle, _p(ts), _p(pos), _p(gps), _p(valid), _p(offsets), B, _p(R), _p(t), _p(s), C.byref(cfg),
                                             Kmax, _p(la.knot_R), _p(la.knot_t), _p(la.knot_s), _p(la.knot_n), _p(la.knot_rms), _p(la.knot_flags),
                                             _p(la.n_knots), _p(la.track_status)))
    if run_status is not None:                                            # failed runs: no knots, NaN rows (the blend sees the status word)
        skip = run_status != 0
        la.track_status = torch.where(skip, la.track_status | _lib.LOC_SKIPPED, la.track_status)
        la.n_knots = torch.where(skip, torch.zeros_like(la.n_knots), la.n_knots)
        nan = float("nan")
        la.knot_R, la.knot_t = la.knot_R.masked_fill(skip[:, None, None], nan), la.knot_t.masked_fill(skip[:, None, None], nan)
        la.knot_s, la.knot_rms = la.knot_s.masked_fill(skip[:, None], nan), la.knot_rms.masked_fill(skip[:, None], nan)
        la.knot_n, la.knot_flags = la.knot_n.masked_fill(skip[:, None], 0), la.knot_flags.masked_fill(skip[:, None], 0)
    la.pos, la.quat, la.scale_at, la.pose_flags = local_apply_ragged(ts, pos, quat, offsets, R, t, s, cfg.spacing, la.knot_R, la.knot_t, la.knot_s,
                                                                     la.knot_flags, la.n_knots, la.track_status)
    return la


def local_align_fused(rb, r, **kw):
    """local_align_ragged on the result r of run_fusion_ragged / run_fusion_batch for the batch rb: the run's global Sim3, the aligned
    fixes, their mask and run_status are r's, as at gate_fused.  Failed runs pass through as NaN rows."""
    return local_align_ragged(rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), r.aligned.reshape(-1, 3), r.valid.reshape(-1),
                              rb.slam_offsets, r.R, r.t, r.s, run_status=r.run_status, **kw)


def refuse_local(rb, r, la, want_cov=False, skip_seconds=5.0, config=None):
    """Fuse again with the locally aligned track la (local_align_fused) as the motion source: the existing ekf_fuse_ragged on la.pos /
    la.quat with their row 0 as every track's initial pose -- calculate_relative_pose is linear in the positions and invariant under a
    common rotation, so the filter's increments then carry the local scale; no fuse kernel knows of it -- optionally
    ekf_covariance_ragged, and step 6's nearest-fix error rows for the raw SLAM track, the locally aligned one and the fused one.  Tracks
    the run skipped are fused from NaN rows and should be ignored, as la.track_status says.  Returns a RunResult in the shape of
    refuse_gated's: pos (P,3), quat (P,4), status (B,), valid (P,), err_stats (B,4) / errors (P,) of the fused track, cov, and
    err_stats3 (3,B,4) / errors3 (3,P) for raw / local-aligned / fused."""
    ts, pos = rb.ts.reshape(-1), rb.pos.reshape(-1, 3)
    aligned, valid, offsets = r.aligned.reshape(-1, 3), r.valid.reshape(-1).contiguous(), rb.slam_offsets
    B, P = _offsets_chk(offsets), int(ts.numel())
    dev = ts.device
    if P:
        first = torch.clamp(offsets[:-1], max=P - 1)                      # (an empty track's row is never read)
        ip, iq = la.pos[first].contiguous(), la.quat[first].contiguous()
    else:
        ip, iq = torch.zeros((B, 3), dtype=torch.float64, device=dev), torch.zeros((B, 4), dtype=torch.float64, device=dev)
    po, qo, st = ekf_fuse_ragged(ts, la.pos, la.quat, aligned, valid, offsets, ip, iq, config=config)
    cov = ekf_covariance_ragged(ts, la.quat, aligned, valid, offsets, config=config, run_status=r.run_status) if want_cov else None
    rows = _step6_rows(ts, offsets, (pos, la.pos, po), aligned, valid, skip_seconds)
    return RunResult(pos=po, quat=qo, status=st, valid=valid, err_stats=rows[2][0], errors=rows[2][1], cov=cov, init_pos=ip, init_quat=iq,
                     err_stats3=torch.stack([x[0] for x in rows]), errors3=torch.stack([x[1] for x in rows]))


# ---------------------------------------------------------------------------- antenna lever arm (gsf_lever_fit_dev / gsf_lever_apply_dev)
def _lever_config(sigma_fix, sigma_prior, sigma_rot, fit_scale, fit_rotation, iters, min_rows, ratio_max, pivot_min, weak_ratio, conv_tol):
    """the arguments of the lever-arm fit as a gsf_lever_config, checked as the entry checks them (these errors need no device)"""
    c = _lib.LeverConfig()
    sp = tuple(float(v) for v in ((sigma_prior,) * 3 if isinstance(sigma_prior, (int, float)) else sigma_prior))
    if len(sp) != 3:
        raise ValueError("lever arm: sigma_prior must be one number or three")
    c.sigma_fix, c.sigma_rot, c.ratio_max, c.pivot_min = float(sigma_fix), float(sigma_rot), float(ratio_max), float(pivot_min)
    c.sigma_prior[0], c.sigma_prior[1], c.sigma_prior[2] = sp
    c.weak_ratio, c.conv_tol, c.min_rows, c.iters = float(weak_ratio), float(conv_tol), int(min_rows), int(iters)
    c.fit_scale, c.fit_rotation = int(bool(fit_scale)), int(bool(fit_rotation))
    if not (0.0 < c.sigma_fix < float("inf")):
        raise ValueError("lever arm: sigma_fix must be positive and finite")
    if not (all(v > 0.0 for v in sp) and c.sigma_rot > 0.0):
        raise ValueError("lever arm: sigma_prior and sigma_rot must be positive (inf: no prior)")
    if not 1 <= c.iters <= 8:
        raise ValueError("lever arm: iters must be in [1, 8]")
    if c.min_rows < 1:
        raise ValueError("lever arm: min_rows must be >= 1")
    if not (c.ratio_max >= 1.0 and c.pivot_min >= 0.0 and c.weak_ratio >= 0.0 and c.conv_tol >= 0.0):
        raise ValueError("lever arm: ratio_max must be >= 1, pivot_min, weak_ratio and conv_tol >= 0")
    return c


class LeverArm:
    """Result of lever_fit_ragged for B tracks (definitions: include/gsf.h, gsf_lever_fit_dev).  Device tensors: l (B,3) = the antenna offset
    in the sensor frame, l_cov (B,3,3), R (B,9), t (B,3), s (B,) = the Sim3 fitted with it, n_rows, n_bad_quat, flags (B,) int32
    (_lib.LEVER_* bits), rms_before, rms_after, last_step (B,); sigma_prior (3 floats) and valid (P,) = the mask of the fit.  A track with
    any of _lib.LEVER_KEPT carries its starting values."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def sigma(self):
        """(B,3): the square roots of the diagonal of l_cov"""
        return torch.sqrt(torch.diagonal(self.l_cov, dim1=1, dim2=2))

    @property
    def observed(self):
        """(B,3) bool: the axis is not flagged WEAK (the data, not the prior, decided it)"""
        bits = torch.tensor([_lib.LEVER_WEAK_X, _lib.LEVER_WEAK_Y, _lib.LEVER_WEAK_Z], dtype=torch.int32, device=self.flags.device)
        return (self.flags[:, None] & bits[None, :]) == 0

    @property
    def fitted(self):
        """(B,) bool: the track carries a fit, not its starting values"""
        return (self.flags & _lib.LEVER_KEPT) == 0

    def table(self):
        """one line per track, on the host: l, sigma, the observed axes, rows, RMS before -> after, flags"""
        l, sg, ob = self.l.cpu().numpy(), self.sigma.cpu().numpy(), self.observed.cpu().numpy()
        n, fl = self.n_rows.cpu().numpy(), self.flags.cpu().numpy()
        rb_, ra = self.rms_before.cpu().numpy(), self.rms_after.cpu().numpy()
        lines = ["track      l_x      l_y      l_z   sigma_x  sigma_y  sigma_z  observed  rows  rms_before  rms_after  flags"]
        for b in range(len(n)):
            axes = "".join(a if o else "-" for a, o in zip("xyz", ob[b]))
            lines.append(f"{b:5d} {l[b, 0]:8.3f} {l[b, 1]:8.3f} {l[b, 2]:8.3f}  {sg[b, 0]:8.3f} {sg[b, 1]:8.3f} {sg[b, 2]:8.3f}  {axes:>8s} {n[b]:5d}  {rb_[b]:10.4f} {ra[b]:10.4f}  {fl[b]:5d}")
        return "\n".join(lines)


def lever_apply_ragged(quat, xyz, offsets, R, l, sign=-1):
    """xyz + sign R (M(quat) l) per pose (gsf_lever_apply_dev): quat (P,4), xyz (P,3), offsets (B+1,) int64, R (B,9), l (B,3).  sign = -1
    moves fixes from the antenna to the camera, +1 from the camera to the antenna; pass the identity as R when quat is already a world
    quaternion (a fused one).  A NaN fix stays NaN; a quaternion that cannot be normalised gives a NaN row and _lib.LVP_BAD_QUAT.  One
    launch on torch's current stream.  Returns xyz_out (P,3), pose_flags (P,) int32."""
    if sign not in (-1, 1):
        raise ValueError("lever_apply_ragged: sign must be -1 (antenna -> camera) or +1 (camera -> antenna)")
    B = _offsets_chk(offsets)
    P = int(xyz.shape[0]) if xyz.dim() == 2 else -1
    _chk(quat, torch.float64, (P, 4), "quat"); _chk(xyz, torch.float64, (P, 3), "xyz")
    _chk(R, torch.float64, (B, 9), "R"); _chk(l, torch.float64, (B, 3), "l")
    out = torch.empty_like(xyz)
    fl = torch.empty((P,), dtype=torch.int32, device=xyz.device)
    check(_lib.load().gsf_lever_apply_dev(context().handle, _p(quat), _p(xyz), _p(offsets), B, _p(R), _p(l), float(sign), _p(out), _p(fl)))
    return out, fl


def lever_fit_ragged(pos, quat, gps, valid, offsets, R, t, s, l0=None, sigma_fix=0.5, sigma_prior=(1.0, 1.0, 1.0), sigma_rot=0.05, fit_scale=True,
                     fit_rotation=True, iters=4, min_rows=8, ratio_max=2.0, pivot_min=1e-10, weak_ratio=0.5, conv_tol=1e-6, run_status=None):
    """The antenna lever arm of B ragged tracks on torch's current stream (gsf_lever_fit_dev; definitions in include/gsf.h): a joint
    Gauss-Newton over scale, translation, lever arm and a rotation increment from the starting values R (B,9), t (B,3), s (B,) -- each
    track's global Sim3 -- and l0 (B,3) (None: zero), `iters` rounds.  pos (P,3), quat (P,4): the original SLAM tracks; gps (P,3) / valid
    (P,) uint8 as the time alignment returns them.  sigma_fix: the noise of a fix; sigma_prior (one number or three, metres; inf: none): the
    prior of l about l0 per sensor axis; sigma_rot (radians; inf: none): the prior of the accumulated rotation.  run_status (B,) int32:
    tracks with a non-zero word are not read (_lib.LEVER_TRACK).  Returns a LeverArm."""
    cfg = _lever_config(sigma_fix, sigma_prior, sigma_rot, fit_scale, fit_rotation, iters, min_rows, ratio_max, pivot_min, weak_ratio, conv_tol)
    B = _offsets_chk(offsets)
    P = int(pos.shape[0]) if pos.dim() == 2 else -1
    _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat"); _chk(gps, torch.float64, (P, 3), "gps")
    _chk(valid, torch.uint8, (P,), "valid")
    _chk(R, torch.float64, (B, 9), "R"); _chk(t, torch.float64, (B, 3), "t"); _chk(s, torch.float64, (B,), "s")
    dev = pos.device
    f = dict(dtype=torch.float64, device=dev)
    i = dict(dtype=torch.int32, device=dev)
    if l0 is None:
        l0 = torch.zeros((B, 3), **f)
    _chk(l0, torch.float64, (B, 3), "l0")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    lv = LeverArm(R=torch.empty((B, 9), **f), t=torch.empty((B, 3), **f), s=torch.empty((B,), **f), l=torch.empty((B, 3), **f),
                  l_cov=torch.empty((B, 3, 3), **f), n_rows=torch.empty((B,), **i), n_bad_quat=torch.empty((B,), **i),
                  rms_before=torch.empty((B,), **f), rms_after=torch.empty((B,), **f), last_step=torch.empty((B,), **f),
                  flags=torch.empty((B,), **i), sigma_prior=tuple(cfg.sigma_prior), sigma_fix=cfg.sigma_fix, valid=valid, l0=l0)
    check(_lib.load().gsf_lever_fit_dev(context().handle, _p(pos), _p(quat), _p(gps), _p(valid), _p(offsets), B, _p(R), _p(t), _p(s), _p(l0),
                                        _p(run_status), C.byref(cfg), _p(lv.R), _p(lv.t), _p(lv.s), _p(lv.l), _p(lv.l_cov), _p(lv.n_rows),
                                        _p(lv.n_bad_quat), _p(lv.rms_before), _p(lv.rms_after), _p(lv.last_step), _p(lv.flags)))
    return lv


def lever_fit_fused(rb, r, valid=None, **kw):
    """lever_fit_ragged on the result r of run_fusion_ragged / run_fusion_batch for the batch rb: the run's global Sim3, the aligned fixes,
    their mask and run_status are r's (valid=: another mask over the same rows, e.g. g.valid(k) of gate_fused, as at smooth_fused)."""
    v = (r.valid.reshape(-1) if valid is None else valid).contiguous()
    return lever_fit_ragged(rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), r.aligned.reshape(-1, 3), v, rb.slam_offsets, r.R, r.t, r.s,
                            run_status=r.run_status, **kw)


def refuse_lever(rb, r, lv, want_cov=False, skip_seconds=5.0, config=None):
    """Fuse again with the fixes moved from the antenna to the camera under the lever arm lv (lever_fit_fused): lever_apply_ragged on
    r.aligned under lv.R / lv.l, the initial pose of every track = row 0 of apply_sim3_batch under lv.R / lv.t / lv.s, the existing
    ekf_fuse_ragged on the ORIGINAL SLAM poses -- no fuse kernel knows of the lever arm --, optionally ekf_covariance_ragged, and step 6's
    nearest-fix error rows for the raw SLAM track, the Sim3-aligned one under lv and the fused one, all against the de-levered fixes.
    A pose whose quaternion cannot be normalised has a NaN fix and is fused as a pose without one.  Returns a RunResult in the shape of
    refuse_local's -- pos, quat, status, valid, err_stats / errors of the fused track, cov, init_pos, init_quat, err_stats3 (3,B,4) /
    errors3 (3,P) -- plus gps_camera (P,3), the de-levered fixes, and lever_flags (P,) int32."""
    ts, pos, quat = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4)
    aligned, valid, offsets = r.aligned.reshape(-1, 3).contiguous(), lv.valid, rb.slam_offsets
    B, P = _offsets_chk(offsets), int(ts.numel())
    dev = ts.device
    gc, lf = lever_apply_ragged(quat, aligned, offsets, lv.R, lv.l, sign=-1)
    sp, _, _ = apply_sim3_batch(pos, quat, offsets, lv.R, lv.t, lv.s)
    if P:
        first = torch.clamp(offsets[:-1], max=P - 1)                      # (an empty track's row is never read)
        one = torch.arange(B + 1, dtype=torch.int64, device=dev)
        ip, iq, _ = apply_sim3_batch(pos[first].contiguous(), quat[first].contiguous(), one, lv.R, lv.t, lv.s)
    else:
        ip, iq = torch.zeros((B, 3), dtype=torch.float64, device=dev), torch.zeros((B, 4), dtype=torch.float64, device=dev)
    po, qo, st = ekf_fuse_ragged(ts, pos, quat, gc, valid, offsets, ip, iq, config=config)
    cov = ekf_covariance_ragged(ts, quat, gc, valid, offsets, config=config, run_status=r.run_status) if want_cov else None
    rows = _step6_rows(ts, offsets, (pos, sp, po), gc, valid, skip_seconds)
    return RunResult(pos=po, quat=qo, status=st, valid=valid, err_stats=rows[2][0], errors=rows[2][1], cov=cov, init_pos=ip, init_quat=iq,
                     err_stats3=torch.stack([x[0] for x in rows]), errors3=torch.stack([x[1] for x in rows]), gps_camera=gc, lever_flags=lf)


class PoseQuery:
    """The fused track at query stamps (query_poses_ragged), flat over the M queries: pos (M,3), quat (M,4), flags (M,) uint8 of _lib.Q_* bits,
    index (M,) int32 = the bracket's first pose relative to its track (-1: none), pose_flags (M,) uint8 or None = the _lib.POSE_* bits of
    the bracket's poses or'ed, track_state (B,) int32 of _lib.QT_* bits (None for a call without queries), q_offsets (B+1,)."""

    def __init__(self, pos, quat, flags, index, pose_flags, track_state, q_offsets):
        self.pos, self.quat, self.flags, self.index, self.pose_flags = pos, quat, flags, index, pose_flags
        self.track_state, self.q_offsets = track_state, q_offsets


class GeorefPoints:
    """Sensor points in the fused track's frame (georef_points_ragged): xyz (M,3), lonlatalt (M,3) rows [lon, lat, alt] or None, flags / index
    / pose_flags / track_state / q_offsets as in PoseQuery."""

    def __init__(self, xyz, lonlatalt, flags, index, pose_flags, track_state, q_offsets):
        self.xyz, self.lonlatalt, self.flags, self.index, self.pose_flags = xyz, lonlatalt, flags, index, pose_flags
        self.track_state, self.q_offsets = track_state, q_offsets


def _query_args(name, ts, pos, quat, offsets, q_t, q_offsets, pose_flags, run_status):
    B = _offsets_chk(offsets)
    if _offsets_chk(q_offsets) != B:
        raise ValueError(f"{name}: offsets and the query offsets must describe the same number of tracks")
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    M = int(q_t.shape[0]) if q_t.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(q_t, torch.float64, (M,), "query stamps")
    if pose_flags is not None:
        _chk(pose_flags, torch.uint8, (P,), "pose_flags")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    return B, P, M


def _query_outputs(B, M, dev, want_pose_flags):
    flags = torch.empty((M,), dtype=torch.uint8, device=dev)
    index = torch.empty((M,), dtype=torch.int32, device=dev)
    pf = torch.empty((M,), dtype=torch.uint8, device=dev) if want_pose_flags else None
    state = torch.empty((B,), dtype=torch.int32, device=dev)
    return flags, index, pf, state


def _unread_rows(ts, pos, quat):
    """a batch without a single pose: the entries want non-NULL arrays, which they then never read"""
    z = torch.zeros((8,), dtype=torch.float64, device=ts.device)
    return (z[:1], z[:3].view(1, 3), z[:4].view(1, 4)) if ts.numel() == 0 else (ts, pos, quat)


def query_poses_ragged(ts, pos, quat, offsets, q_t, q_offsets, pose_flags=None, run_status=None, max_gap=0.0):
    """The fused tracks at any stamps (gsf_pose_query_dev): ts (P,), pos (P,3), quat (P,4), offsets (B+1,) int64 as the ragged entries give
    them; q_t (M,) query stamps in any order, q_offsets (B+1,) int64.  Between two poses the position is interpolated linearly and the
    orientation by quaternion_nlerp (EKFGPSSLAM.py:94-105); a query on a pose's stamp returns that pose bit for bit; before the first /
    after the last stamp, across a bracket wider than max_gap (> 0) and on an unusable track the rows are NaN and flags says why.
    pose_flags (P,) uint8 = FusedCovariance.flags; run_status (B,) int32: tracks with run_status != 0 are not read.  Returns a PoseQuery."""
    B, P, M = _query_args("query_poses_ragged", ts, pos, quat, offsets, q_t, q_offsets, pose_flags, run_status)
    f = dict(dtype=torch.float64, device=ts.device)
    out_pos, out_quat = torch.empty((M, 3), **f), torch.empty((M, 4), **f)
    flags, index, pf, state = _query_outputs(B, M, ts.device, pose_flags is not None)
    if M == 0:                                                           # the entry does nothing without queries: no track_state either
        return PoseQuery(out_pos, out_quat, flags, index, pf, None, q_offsets)
    ts_, pos_, quat_ = _unread_rows(ts, pos, quat)
    check(_lib.load().gsf_pose_query_dev(context().handle, _p(ts_), _p(pos_), _p(quat_), _p(offsets), _p(run_status), _p(pose_flags), B, _p(q_t),
                                         _p(q_offsets), M, float(max_gap), _p(out_pos), _p(out_quat), _p(flags), _p(index), _p(pf), _p(state)))
    return PoseQuery(out_pos, out_quat, flags, index, pf, state, q_offsets)


def georef_points_ragged(ts, pos, quat, offsets, pt_t, pt_xyz, pt_offsets, ext_q=None, ext_t=None, scale=None, pose_flags=None, run_status=None,
                         max_gap=0.0, zone=None, south=None):
    """Sensor points into the fused tracks' frame (gsf_georef_points_dev): pt_xyz (M,3) in the sensor frame stamped by pt_t (M,), pt_offsets
    (B+1,) int64; ext_q (B,4) / ext_t (B,3) = sensor -> body per track (None: identity / zero), scale (B,) (None: 1; map points in SLAM units
    pass the run's s).  xyz = p(t) + R(q(t)) (scale (R(ext_q) x + ext_t)) with the pose of query_poses_ragged.  zone / south (B,) int32
    given: lonlatalt = utm_to_wgs84_ragged(xyz, pt_offsets, zone, south, run_status).  Returns a GeorefPoints."""
    B, P, M = _query_args("georef_points_ragged", ts, pos, quat, offsets, pt_t, pt_offsets, pose_flags, run_status)
    _chk(pt_xyz, torch.float64, (M, 3), "pt_xyz")
    if ext_q is not None:
        _chk(ext_q, torch.float64, (B, 4), "ext_q")
    if ext_t is not None:
        _chk(ext_t, torch.float64, (B, 3), "ext_t")
    if scale is not None:
        _chk(scale, torch.float64, (B,), "scale")
    if (zone is None) != (south is None):
        raise ValueError("georef_points_ragged: zone and south go together")
    xyz = torch.empty((M, 3), dtype=torch.float64, device=ts.device)
    flags, index, pf, state = _query_outputs(B, M, ts.device, pose_flags is not None)
    if M == 0:                                                           # the entry does nothing without points: no track_state either
        return GeorefPoints(xyz, xyz.clone() if zone is not None else None, flags, index, pf, None, pt_offsets)
    ts_, pos_, quat_ = _unread_rows(ts, pos, quat)
    check(_lib.load().gsf_georef_points_dev(context().handle, _p(ts_), _p(pos_), _p(quat_), _p(offsets), _p(run_status), _p(pose_flags), B, _p(pt_t),
                                            _p(pt_offsets), M, float(max_gap), _p(pt_xyz), _p(ext_q), _p(ext_t), _p(scale), _p(xyz), _p(flags),
                                            _p(index), _p(pf), _p(state)))
    lla = utm_to_wgs84_ragged(xyz, pt_offsets, zone, south, run_status) if zone is not None else None
    return GeorefPoints(xyz, lla, flags, index, pf, state, pt_offsets)


def _fused_pose_flags(r):
    cov = getattr(r, "cov", None)
    return cov.flags if cov is not None else None


def query_fused(rb, r, q_t, q_offsets, max_gap=0.0):
    """query_poses_ragged on a run_fusion_ragged result: rb.ts, r.fused.pos / .quat, rb.slam_offsets, r.run_status, and r.cov.flags when the
    run carries them (want_cov=True)."""
    return query_poses_ragged(rb.ts, r.fused.pos, r.fused.quat, rb.slam_offsets, q_t, q_offsets, pose_flags=_fused_pose_flags(r),
                              run_status=r.run_status, max_gap=max_gap)


def georef_fused(rb, r, pt_t, pt_xyz, pt_offsets, ext_q=None, ext_t=None, scale=None, max_gap=0.0, wgs84=False):
    """georef_points_ragged on a run_fusion_ragged result (see query_fused).  wgs84=True: lonlatalt through the run's projector (r.zone /
    r.south); a projected=True run has none and raises ValueError."""
    if wgs84 and (getattr(r, "zone", None) is None or getattr(r, "south", None) is None):
        raise ValueError("georef_fused: wgs84=True needs the run's projector, and a projected=True run has none (ref :1096)")
    return georef_points_ragged(rb.ts, r.fused.pos, r.fused.quat, rb.slam_offsets, pt_t, pt_xyz, pt_offsets, ext_q=ext_q, ext_t=ext_t, scale=scale,
                                pose_flags=_fused_pose_flags(r), run_status=r.run_status, max_gap=max_gap,
                                zone=r.zone if wgs84 else None, south=r.south if wgs84 else None)


# ---- trajectory evaluation against 6-DoF truth (gsf_traj_eval_dev) ----------------------------------------------------------------------------
_TE_ALIGN = {"none": _lib.TE_ALIGN_NONE, "se3": _lib.TE_ALIGN_SE3, "sim3": _lib.TE_ALIGN_SIM3}
_TE_ASSOC = {"nearest": _lib.TE_NEAREST, "interp": _lib.TE_INTERP}
APE_STATS = ("n", "mean", "median", "rmse", "std", "min", "max", "sse")


class RpeScenarios:
    """K relative-error scenarios on the device: kind (K,) int32 of _lib.TE_FRAMES / TE_METRES / TE_SECONDS, value (K,) float64, stride (K,)
    int64 (rpe_scenarios / kitti_scenarios build them)."""

    def __init__(self, kind, value, stride):
        self.kind, self.value, self.stride = kind, value, stride
        self.K = int(kind.numel())
        self.host = (kind.cpu().tolist(), value.cpu().tolist(), stride.cpu().tolist())


def rpe_scenarios(frames=(), metres=(), seconds=(), stride=1, device="cuda"):
    """Relative-error scenarios: one per delta, frames first, then metres, then seconds; stride = the step between first frames (an int, or
    one per scenario).  Returns an RpeScenarios."""
    kinds = [_lib.TE_FRAMES] * len(frames) + [_lib.TE_METRES] * len(metres) + [_lib.TE_SECONDS] * len(seconds)
    values = [float(v) for v in tuple(frames) + tuple(metres) + tuple(seconds)]
    strides = [int(stride)] * len(kinds) if isinstance(stride, int) else [int(v) for v in stride]
    if len(strides) != len(kinds):
        raise ValueError(f"rpe_scenarios: {len(kinds)} scenarios but {len(strides)} strides")
    if any(v < 1 for v in strides):
        raise ValueError("rpe_scenarios: a stride must be at least 1")
    return RpeScenarios(torch.tensor(kinds, dtype=torch.int32, device=device), torch.tensor(values, dtype=torch.float64, device=device),
                        torch.tensor(strides, dtype=torch.int64, device=device))


def kitti_scenarios(device="cuda"):
    """The KITTI odometry benchmark's segments: 100, 200, ... 800 m, a first frame every 10 poses."""
    return rpe_scenarios(metres=tuple(100.0 * k for k in range(1, 9)), stride=10, device=device)


class TrajectoryEval:
    """What evaluate_trajectory_ragged returns.  Per track: R (B,9) / t (B,3) / s (B,) of the alignment, track_state (B,) int32 of
    _lib.TE_TRACK_* bits.  Per pose: flags (P,) uint8 of _lib.TE_* bits, match_index (P,) int32, ape_t / ape_r (P,) (metres / radians, NaN
    where the pose is not matched).  ape_stats (B,2,8): translation / rotation x APE_STATS.  rpe_n (B,K) int64 and rpe_sums (B,K,8) per
    scenario; rpe_last (P,) int32 / rpe_t / rpe_r (P,) of the traced scenario, or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def ape(self, b):
        """{'translation': {n, mean, ...}, 'rotation': {...}} of track b (one device -> host copy)"""
        st = self.ape_stats[b].cpu().tolist()
        return {"translation": dict(zip(APE_STATS, st[0])), "rotation": dict(zip(APE_STATS, st[1]))}

    def ape_table(self):
        """ape_stats on the host: (B,2,8) numpy, columns as APE_STATS"""
        return self.ape_stats.cpu().numpy()

    def rpe(self, k):
        """scenario k per track: {'n' (B,) int64, 'mean_t', 'rmse_t', 'max_t', 'mean_r', 'rmse_r', 'max_r' (B,)}; NaN where a track has no pair"""
        n, sm = self.rpe_n[:, k], self.rpe_sums[:, k]
        nf = torch.where(n > 0, n.to(torch.float64), torch.full_like(sm[:, 0], float("nan")))
        return {"n": n, "mean_t": sm[:, 0] / nf, "rmse_t": torch.sqrt(sm[:, 1] / nf), "max_t": torch.where(n > 0, sm[:, 2], nf),
                "mean_r": sm[:, 3] / nf, "rmse_r": torch.sqrt(sm[:, 4] / nf), "max_r": torch.where(n > 0, sm[:, 5], nf)}

    def kitti(self):
        """KITTI's segment errors over every TE_METRES scenario: t_rel in percent = 100 sum(et / len) / n and r_rel in rad/m = sum(er / len) /
        n, over all tracks and per track (t_rel_track / r_rel_track, NaN without a pair); a length with no pair contributes nothing."""
        kinds = self.scenarios.host[0] if self.scenarios is not None else []
        cols = [k for k, kind in enumerate(kinds) if kind == _lib.TE_METRES]
        if not cols:
            raise ValueError("TrajectoryEval.kitti: the evaluation has no scenario in metres")
        n = self.rpe_n[:, cols].sum(dim=1)
        st, sr = self.rpe_sums[:, cols, 6].sum(dim=1), self.rpe_sums[:, cols, 7].sum(dim=1)
        nf = torch.where(n > 0, n.to(torch.float64), torch.full_like(st, float("nan")))
        tot = int(n.sum())
        return KittiErrors(t_rel=100.0 * float(st.sum()) / tot if tot else float("nan"), r_rel=float(sr.sum()) / tot if tot else float("nan"), n=tot,
                           t_rel_track=100.0 * st / nf, r_rel_track=sr / nf, n_track=n)

    def table(self):
        """one text line per track: state, matched poses, APE rmse / median / max (m, deg)"""
        import math
        st, state = self.ape_table(), self.track_state.cpu().tolist()
        lines = ["track state matched ape_t_rmse ape_t_median ape_t_max ape_r_rmse_deg ape_r_max_deg"]
        for b, row in enumerate(st):
            lines.append(f"{b} {state[b]} {int(row[0][0])} {row[0][3]:.4f} {row[0][2]:.4f} {row[0][6]:.4f} {math.degrees(row[1][3]):.4f} {math.degrees(row[1][6]):.4f}")
        return "\n".join(lines)


class KittiErrors:
    """TrajectoryEval.kitti(): t_rel (percent), r_rel (rad/m), n pairs; the same per track as tensors."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def r_rel_deg_per_100m(self):
        import math
        return math.degrees(self.r_rel) * 100.0


def evaluate_trajectory_ragged(ts, pos, quat, offsets, ref_ts, ref_pos, ref_quat, ref_offsets, align="se3", assoc="nearest", max_diff=0.01, rpe=None,
                               trace=None, run_status=None, check_offsets=True):
    """Grade B tracks against 6-DoF truth (gsf_traj_eval_dev): estimate ts (P,), pos (P,3), quat (P,4), offsets (B+1,) int64; truth ref_ts
    (G,), ref_pos (G,3), ref_quat (G,4), ref_offsets (B+1,) int64.  assoc: "nearest" truth stamp within max_diff, or "interp" = the truth at
    the estimate's stamp by the rule of query_poses_ragged (max_diff = the widest bracket).  align: "none", "se3" or "sim3" over the matched
    pairs.  rpe: an RpeScenarios or None; trace: the scenario whose pairs are returned per first frame.  run_status (B,) int32: tracks with
    run_status != 0 are not read.  check_offsets: both offsets arrays are copied to the host and checked (ascending, inside their arrays: the
    kernels trust them), which waits for the stream; False for offsets already known to be good leaves the call asynchronous.  Returns a
    TrajectoryEval."""
    name = "evaluate_trajectory_ragged"
    if align not in _TE_ALIGN:
        raise ValueError(f"{name}: align must be one of {sorted(_TE_ALIGN)}, got {align!r}")
    if assoc not in _TE_ASSOC:
        raise ValueError(f"{name}: assoc must be one of {sorted(_TE_ASSOC)}, got {assoc!r}")
    if not float(max_diff) == float(max_diff):
        raise ValueError(f"{name}: max_diff is NaN")
    B = _offsets_chk(offsets)
    if _offsets_chk(ref_offsets) != B:
        raise ValueError(f"{name}: offsets and ref_offsets must describe the same number of tracks")
    P = int(ts.shape[0]) if ts.dim() == 1 else -1
    G = int(ref_ts.shape[0]) if ref_ts.dim() == 1 else -1
    _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
    _chk(ref_ts, torch.float64, (G,), "ref_ts"); _chk(ref_pos, torch.float64, (G, 3), "ref_pos"); _chk(ref_quat, torch.float64, (G, 4), "ref_quat")
    if run_status is not None:
        _chk(run_status, torch.int32, (B,), "run_status")
    K = 0
    if rpe is not None:
        K = int(rpe.kind.numel()) if rpe.kind.dim() == 1 else -1
        _chk(rpe.kind, torch.int32, (K,), "rpe.kind"); _chk(rpe.value, torch.float64, (K,), "rpe.value"); _chk(rpe.stride, torch.int64, (K,), "rpe.stride")
    if trace is not None and not 0 <= int(trace) < K:
        raise ValueError(f"{name}: trace = {trace} names none of the {K} scenarios")
    for o, rows, what in ((offsets, P, "offsets"), (ref_offsets, G, "ref_offsets")) if check_offsets else ():
        oh = o.cpu()
        if int(oh[0]) < 0 or int(oh[-1]) > rows or bool((oh[1:] < oh[:-1]).any()):
            raise ValueError(f"{name}: {what} must ascend from >= 0 to <= {rows}, the rows of its arrays")
    dev = ts.device
    f = dict(dtype=torch.float64, device=dev)
    tr = trace is not None
    r = TrajectoryEval(R=torch.empty((B, 9), **f), t=torch.empty((B, 3), **f), s=torch.empty((B,), **f),
                       track_state=torch.empty((B,), dtype=torch.int32, device=dev), flags=torch.empty((P,), dtype=torch.uint8, device=dev),
                       match_index=torch.empty((P,), dtype=torch.int32, device=dev), ape_t=torch.empty((P,), **f), ape_r=torch.empty((P,), **f),
                       ape_stats=torch.empty((B, 2, 8), **f), rpe_n=torch.empty((B, K), dtype=torch.int64, device=dev),
                       rpe_sums=torch.empty((B, K, 8), **f), rpe_last=torch.empty((P,), dtype=torch.int32, device=dev) if tr else None,
                       rpe_t=torch.empty((P,), **f) if tr else None, rpe_r=torch.empty((P,), **f) if tr else None, scenarios=rpe,
                       offsets=offsets, align=align, assoc=assoc)
    if B == 0:
        return r
    ts_, pos_, quat_ = _unread_rows(ts, pos, quat)
    rts_, rpos_, rquat_ = _unread_rows(ref_ts, ref_pos, ref_quat)
    check(_lib.load().gsf_traj_eval_dev(context().handle, _p(ts_), _p(pos_), _p(quat_), _p(offsets), P, _p(rts_), _p(rpos_), _p(rquat_), _p(ref_offsets),
                                        _p(run_status), B, _TE_ASSOC[assoc], float(max_diff), _TE_ALIGN[align], K,
                                        _p(rpe.kind) if K else None, _p(rpe.value) if K else None, _p(rpe.stride) if K else None,
                                        int(trace) if tr else -1, _p(r.R), _p(r.t), _p(r.s), _p(r.track_state), _p(r.flags), _p(r.match_index),
                                        _p(r.ape_t), _p(r.ape_r), _p(r.ape_stats), _p(r.rpe_n) if K else None, _p(r.rpe_sums) if K else None,
                                        _p(r.rpe_last), _p(r.rpe_t), _p(r.rpe_r)))
    return r


def evaluate_fused(rb, r, truth, **kw):
    """Grade a run_fusion_ragged result against truth = (ref_ts, ref_pos, ref_quat, ref_offsets): the Sim3-aligned raw track (apply_sim3_batch
    under r.R / r.t / r.s) and the fused track (r.fused), one evaluate_trajectory_ragged call each with the run's run_status; keyword arguments
    go to both.  Returns (raw, fused), two TrajectoryEval."""
    ref_ts, ref_pos, ref_quat, ref_offsets = truth
    ts, pos, quat = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4)
    sp, sq, _ = apply_sim3_batch(pos, quat, rb.slam_offsets, r.R, r.t, r.s)
    kw.setdefault("run_status", r.run_status)
    raw = evaluate_trajectory_ragged(ts, sp, sq, rb.slam_offsets, ref_ts, ref_pos, ref_quat, ref_offsets, **kw)
    kw["check_offsets"] = False                                           # (the same offsets: checked by the first call, if at all)
    fused = evaluate_trajectory_ragged(ts, r.fused.pos.reshape(-1, 3), r.fused.quat.reshape(-1, 4), rb.slam_offsets, ref_ts, ref_pos, ref_quat,
                                       ref_offsets, **kw)
    return raw, fused


def read_kitti_poses(poses_path, times_path):
    """A KITTI pose file (12 numbers a row: the 3x4 matrix [R | t], row-major) and its stamp file (one number a row) on the host, in NumPy:
    -> {'timestamps' (n,), 'positions' (n,3), 'quaternions' (n,4)} with unit quaternions [x, y, z, w], w >= 0, by the branch on the largest
    of the diagonal and the trace.  ValueError where the row counts differ or a row has another width, as kitti2tum.py refuses them."""
    import numpy as np
    try:
        m, t = np.loadtxt(poses_path, dtype=np.float64, ndmin=2), np.loadtxt(times_path, dtype=np.float64, ndmin=2)
    except OSError as e:
        raise ValueError(f"read_kitti_poses: {e}")
    if m.shape[1] != 12:
        raise ValueError(f"read_kitti_poses: a KITTI pose row holds 12 numbers, {poses_path} has {m.shape[1]}")
    if t.shape[1] != 1 or t.shape[0] != m.shape[0]:
        raise ValueError("read_kitti_poses: the timestamp file must have one column of timestamps and the same number of rows as the pose file")
    return {"timestamps": t[:, 0].copy(), "positions": np.ascontiguousarray(m[:, [3, 7, 11]]), "quaternions": kitti_rotations_to_quat(m)}


def kitti_rotations_to_quat(m):
    """(n,12) KITTI pose rows -> (n,4) unit quaternions [x, y, z, w] with w >= 0 (NumPy, host)"""
    import numpy as np
    R = np.asarray(m, np.float64).reshape(-1, 3, 4)[:, :, :3]
    n = R.shape[0]
    d = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]], axis=1)
    c = np.argmax(d, axis=1)
    q = np.empty((n, 4))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        sel = c == i
        q[sel, i] = 1.0 - d[sel, 3] + 2.0 * R[sel, i, i]
        q[sel, j] = R[sel, j, i] + R[sel, i, j]
        q[sel, k] = R[sel, k, i] + R[sel, i, k]
        q[sel, 3] = R[sel, k, j] - R[sel, j, k]
    sel = c == 3
    q[sel, 0], q[sel, 1], q[sel, 2], q[sel, 3] = R[sel, 2, 1] - R[sel, 1, 2], R[sel, 0, 2] - R[sel, 2, 0], R[sel, 1, 0] - R[sel, 0, 1], 1.0 + d[sel, 3]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1.0
    return q


# ---- streaming fusion: append poses to live tracks (gsf_stream_*) ----------------------------------------------------------------------------
class StreamStep:
    """What FusionStream.append returns: pos (P,3) / quat (P,4) = the fused rows of this call's segments as they stand when the call ends,
    cov (P,7) = the filtered covariance diagonal after each pose; n_total (B,) int64 = poses each track holds; n_final (B,): rows
    [0, n_final) will never be written again; revised_from (B,) = the smallest global index this call wrote; status (B,) int32 = the
    accumulated _lib.ST_* bits as of now | _lib.STREAM_FULL (this segment was refused: NaN rows, track untouched) | _lib.STREAM_BAD_STATE.
    A stream with a lag also fills pos_smooth (P,3) / var_smooth (P,3) / flags_smooth (P,) uint8 = the smoothed rows that BECAME FINAL in
    this call, in the segments' ragged shape: row j of track b's segment is final row smooth_from[b] + j, the rest of the segment's rows
    are NaN (flags 0); flags = _lib.POSE_SMOOTHED | _lib.POSE_SPAN_START; smooth_from / n_smooth_final (B,) int64 = the number of final
    smoothed rows before and after the call.  Without a lag the five are None.  Iteration yields the first seven fields only."""
    __slots__ = ("pos", "quat", "cov", "n_total", "n_final", "revised_from", "status", "pos_smooth", "var_smooth", "flags_smooth", "smooth_from",
                 "n_smooth_final")

    def __init__(self, pos, quat, cov, n_total, n_final, revised_from, status, pos_smooth=None, var_smooth=None, flags_smooth=None, smooth_from=None,
                 n_smooth_final=None):
        self.pos, self.quat, self.cov, self.n_total, self.n_final, self.revised_from, self.status = pos, quat, cov, n_total, n_final, revised_from, status
        self.pos_smooth, self.var_smooth, self.flags_smooth, self.smooth_from, self.n_smooth_final = pos_smooth, var_smooth, flags_smooth, smooth_from, n_smooth_final

    def __iter__(self):
        return iter((self.pos, self.quat, self.cov, self.n_total, self.n_final, self.revised_from, self.status))


def _stream_sizes_chk(B, cap):
    B, cap = int(B), int(cap)
    if B < 0 or cap < 1:
        raise ValueError(f"FusionStream: B >= 0 and cap >= 1 expected, got B = {B}, cap = {cap}")
    return B, cap


class FusionStream:
    """B tracks whose fusion can be continued: the filter state and the last `cap` fused rows of every track live in tensors this object
    owns, an append costs what its new poses cost, and every append says which rows are final.  init_pos (B,3) / init_quat (B,4) are what
    they are at ekf_fuse_ragged: the Sim3-transformed pose 0.  How a track is cut into appends does not change one bit of any output.
    Capacity: a track whose open outage plus new segment exceeds `cap` rows is refused (StreamStep.status & _lib.STREAM_FULL) and left
    untouched; give the stream a larger cap, append shorter segments, or reopen() that track.  Every call is one launch on torch's current
    stream.
    lag = L (1 .. _lib.STREAM_LAG_MAX) adds a fixed-lag RTS smoother: every row is also smoothed with the fixes of the next L rows of its
    span (gsf_stream_append_lag_dev); row i is final once the track holds i + L + 1 poses, the rows above are provisional -- the whole-track
    smoother's answer on what has arrived -- and rewritten by every append.  The stream then owns three more rings (ring_lag, ring_spos,
    ring_svar), an append is two launches and also refuses a track with min(L, n_total) + segment length > cap; everything else an append
    returns is what it returns without a lag, bit for bit."""

    def __init__(self, B, cap, init_pos, init_quat, config=None, device="cuda", lag=None):
        self.B, self.cap = _stream_sizes_chk(B, cap)
        self.lag = None if lag is None else int(lag)
        if self.lag is not None and not 1 <= self.lag <= _lib.STREAM_LAG_MAX:
            raise ValueError(f"FusionStream: lag in 1 .. {_lib.STREAM_LAG_MAX} expected, got {lag}")
        self.config = config or CONFIG
        self._cfg = EkfConfig.from_config(self.config)
        dev = torch.device(device)
        f = dict(dtype=torch.float64, device=dev)
        self.state_f64 = torch.empty((_lib.STREAM_F64, self.B), **f)
        self.state_i64 = torch.empty((_lib.STREAM_I64, self.B), dtype=torch.int64, device=dev)
        self.ring_t, self.ring_pos, self.ring_quat = torch.empty((self.B, self.cap), **f), torch.empty((self.B, self.cap, 3), **f), torch.empty((self.B, self.cap, 4), **f)
        if self.lag is not None:
            self.ring_lag = torch.empty((self.B, self.cap, _lib.STREAM_LAG_F64), **f)
            self.ring_spos, self.ring_svar = torch.empty((self.B, self.cap, 3), **f), torch.empty((self.B, self.cap, 3), **f)
        if init_pos is not None:
            self.reopen(None, init_pos, init_quat)

    @property
    def device(self):
        return self.state_f64.device

    def reopen(self, mask, init_pos, init_quat):
        """(re-)start the tracks with a non-zero byte in mask (B,) uint8 (None: all) from init_pos (B,3) / init_quat (B,4); the others are untouched"""
        dev = self.device
        ip = torch.as_tensor(init_pos, dtype=torch.float64).to(dev).contiguous()
        iq = torch.as_tensor(init_quat, dtype=torch.float64).to(dev).contiguous()
        _chk(ip, torch.float64, (self.B, 3), "init_pos"); _chk(iq, torch.float64, (self.B, 4), "init_quat")
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8).contiguous()
            _chk(mask, torch.uint8, (self.B,), "mask")
        check(_lib.load().gsf_stream_open_dev(context(dev).handle, self.B, self.cap, _p(ip), _p(iq), _p(mask), _p(self.state_f64), _p(self.state_i64)))

    def append(self, ts, pos, quat, gps, valid, seg_offsets, want_cov=True):
        """ts (P,), pos (P,3), quat (P,4) = the new original SLAM poses, gps (P,3) / valid (P,) uint8 = their time-aligned fixes and mask, flat
        over the tracks; track b contributes rows seg_offsets[b] .. seg_offsets[b+1] (int64 (B+1,)), possibly none.  Returns a StreamStep."""
        B = _offsets_chk(seg_offsets)
        if B != self.B:
            raise ValueError(f"seg_offsets: {self.B + 1} entries expected, got {B + 1}")
        P = int(ts.shape[0]) if ts.dim() == 1 else -1
        _chk(ts, torch.float64, (P,), "ts"); _chk(pos, torch.float64, (P, 3), "pos"); _chk(quat, torch.float64, (P, 4), "quat")
        _chk(gps, torch.float64, (P, 3), "gps"); _chk(valid, torch.uint8, (P,), "valid")
        dev = self.device
        f = dict(dtype=torch.float64, device=dev)
        i = dict(dtype=torch.int64, device=dev)
        s = StreamStep(torch.empty((P, 3), **f), torch.empty((P, 4), **f), torch.empty((P, 7), **f) if want_cov else None, torch.empty((B,), **i),
                       torch.empty((B,), **i), torch.empty((B,), **i), torch.empty((B,), dtype=torch.int32, device=dev))
        if self.lag is not None:
            s.pos_smooth, s.var_smooth, s.flags_smooth = torch.empty((P, 3), **f), torch.empty((P, 3), **f), torch.empty((P,), dtype=torch.uint8, device=dev)
            s.smooth_from, s.n_smooth_final = torch.empty((B,), **i), torch.empty((B,), **i)
            check(_lib.load().gsf_stream_append_lag_dev(context(dev).handle, C.byref(self._cfg), B, self.cap, self.lag, _p(self.state_f64), _p(self.state_i64),
                                                        _p(self.ring_t), _p(self.ring_pos), _p(self.ring_quat), _p(self.ring_lag), _p(self.ring_spos),
                                                        _p(self.ring_svar), _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(seg_offsets), _p(s.pos),
                                                        _p(s.quat), _p(s.cov), _p(s.n_total), _p(s.n_final), _p(s.revised_from), _p(s.status),
                                                        _p(s.pos_smooth), _p(s.var_smooth), _p(s.flags_smooth), _p(s.smooth_from), _p(s.n_smooth_final)))
            return s
        check(_lib.load().gsf_stream_append_dev(context(dev).handle, C.byref(self._cfg), B, self.cap, _p(self.state_f64), _p(self.state_i64), _p(self.ring_t),
                                                _p(self.ring_pos), _p(self.ring_quat), _p(ts), _p(pos), _p(quat), _p(gps), _p(valid), _p(seg_offsets),
                                                _p(s.pos), _p(s.quat), _p(s.cov), _p(s.n_total), _p(s.n_final), _p(s.revised_from), _p(s.status)))
        return s

    def rows(self, lo, counts):
        """rows [lo[b], lo[b] + counts[b]) of every track from the ring: ts (P,), pos (P,3), quat (P,4), out_offsets (B+1,); a row the ring
        no longer holds (or does not hold yet) is NaN.  lo / counts: (B,) int64 tensors or sequences (sequences cost no device read)."""
        t, p, q, off = self._gather(lo, counts, self.ring_pos, True)
        return t, p, q, off

    def rows_smoothed(self, lo, counts):
        """the same rows of the smoothed rings of a stream with a lag: ts (P,), pos (P,3), var (P,3), out_offsets (B+1,) -- final below
        n_smooth_final, provisional above (two gathers: the variances' ring has the positions' layout)"""
        if self.lag is None:
            raise ValueError("FusionStream.rows_smoothed: the stream was opened without a lag")
        t, p, _, off = self._gather(lo, counts, self.ring_spos, False)
        _, v, _, _ = self._gather(lo, counts, self.ring_svar, False)
        return t, p, v, off

    def _gather(self, lo, counts, ring_pos, want_quat):
        dev = self.device
        host_counts = not torch.is_tensor(counts)
        lo = torch.as_tensor(lo, dtype=torch.int64).to(dev).contiguous()
        cnt = torch.as_tensor(counts, dtype=torch.int64)
        _chk(lo, torch.int64, (self.B,), "lo")
        if tuple(cnt.shape) != (self.B,):
            raise ValueError(f"counts: shape ({self.B},) expected")
        off_h = torch.zeros(self.B + 1, dtype=torch.int64)
        off_h[1:] = torch.cumsum(cnt.cpu() if not host_counts else cnt, 0)
        if self.B and int(cnt.min()) < 0:
            raise ValueError("counts: negative")
        P = int(off_h[-1])
        off = off_h.to(dev)
        f = dict(dtype=torch.float64, device=dev)
        t, p, q = torch.empty((P,), **f), torch.empty((P, 3), **f), torch.empty((P, 4), **f) if want_quat else None
        check(_lib.load().gsf_stream_gather_dev(context(dev).handle, self.B, self.cap, _p(self.state_i64), _p(self.ring_t), _p(ring_pos),
                                                _p(self.ring_quat), _p(lo), _p(off), _p(t), _p(p), _p(q)))
        return t, p, q, off

    @property
    def n_total(self):
        return self.state_i64[2]

    def state_dict(self):
        """the checkpoint: plain tensors (safe to .cpu() and save) from which from_state continues with the same bits"""
        d = dict(version=_lib.STREAM_LAYOUT_VERSION, B=self.B, cap=self.cap, config=self.config, state_f64=self.state_f64.clone(),
                 state_i64=self.state_i64.clone(), ring_t=self.ring_t.clone(), ring_pos=self.ring_pos.clone(), ring_quat=self.ring_quat.clone())
        if self.lag is not None:                                         # (a stream without a lag: the keys it always had)
            d.update(lag=self.lag, ring_lag=self.ring_lag.clone(), ring_spos=self.ring_spos.clone(), ring_svar=self.ring_svar.clone())
        return d

    @classmethod
    def from_state(cls, d, device="cuda"):
        """a stream that continues the one state_dict() was taken from.  A checkpoint of another layout version is refused (ValueError) before
        anything touches a device."""
        if int(d.get("version", -1)) != _lib.STREAM_LAYOUT_VERSION:
            raise ValueError(f"FusionStream.from_state: layout version {d.get('version')!r}, this library reads version {_lib.STREAM_LAYOUT_VERSION}")
        B, cap = _stream_sizes_chk(d["B"], d["cap"])
        shapes_ = dict(state_f64=(_lib.STREAM_F64, B), state_i64=(_lib.STREAM_I64, B), ring_t=(B, cap), ring_pos=(B, cap, 3), ring_quat=(B, cap, 4))
        lag = d.get("lag")
        if lag is not None:
            shapes_.update(ring_lag=(B, cap, _lib.STREAM_LAG_F64), ring_spos=(B, cap, 3), ring_svar=(B, cap, 3))
        for k, shp in shapes_.items():
            t = d[k]
            want = torch.int64 if k == "state_i64" else torch.float64
            if not torch.is_tensor(t) or t.dtype != want or tuple(t.shape) != shp:
                raise ValueError(f"FusionStream.from_state: {k}: {want} tensor of shape {shp} expected")
        si = d["state_i64"]
        if B and (bool((si[0] != _lib.STREAM_LAYOUT_VERSION).any()) or bool((si[1] != cap).any())):
            raise ValueError("FusionStream.from_state: state_i64 was not written by this layout version for this cap")
        s = cls(B, cap, None, None, config=d.get("config"), device=device, lag=lag)
        for k in shapes_:
            getattr(s, k).copy_(d[k])
        return s

    @classmethod
    def from_run(cls, rb, r, cap=4096, config=None, lag=None):
        """a stream opened from the Sim3-transformed pose 0 of every track of a run_fusion_ragged result r for the batch rb (built as
        gate_fused builds it), on rb's device; feed it rb's poses with r.aligned / r.valid, in pieces"""
        ip, iq = _fused_init_pose(rb, r)
        return cls(int(ip.shape[0]), cap, ip, iq, config=config, device=ip.device, lag=lag)
