"""Whole-track RTS smoothing: gsf_ekf_smooth_ragged_dev against what a caller pays today for the causal track and its covariance, one
ekf_fuse_ragged launch plus one ekf_covariance_ragged launch on the same batch.

Shapes: the synthetic ragged batch of 1 000 tracks x 271 poses (C2's shape) and 1 000 x 1 000.  Per case: warm-up, then the context's timer
(HIP events on the stream, gsf_timer_start / gsf_timer_stop) around one call, median of the repetitions, the smoother and the yardstick
launches alternating inside one process.  Prints one JSON line per shape: ms of the smoother with and without the optional filtered
outputs, ms of the two yardsticks, the ratio smoother / (fuse + covariance), and the share of rows a later fix reaches.
GSF_LIBRARY picks a differently built library (how DESIGN.md 7k's lane reversals and the lone-wave scheduler were compared), whose name is
printed with the row.
usage: python tools/smooth_timing.py [reps]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gps_optimize_slam_amd import batch as B  # noqa: E402
from gps_optimize_slam_amd import _lib  # noqa: E402
from gps_optimize_slam_amd.ekfgpsslam import CONFIG  # noqa: E402


def make(nb, N):
    tb = B.TrajectoryBatch.synthetic(nb, N, layout=B.LAYOUT_TRAJ_MAJOR, seed=7)
    P = nb * N
    offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * N
    return (tb.ts.view(P), tb.pos.view(P, 3), tb.quat.view(P, 4), tb.gps.view(P, 3).clone(), tb.valid.view(P), offsets, tb.init_pos.contiguous(),
            tb.init_quat.contiguous())


def timed(ctx, fn, reps, other):
    ms = []
    for _ in range(reps):
        ctx.timer_start(); fn(); ms.append(ctx.timer_stop())
        other()
    return float(np.median(ms))


def main(reps):
    ctx = B.context()
    L = _lib.load()
    cfg = _lib.EkfConfig.from_config(CONFIG)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f64, i32, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.uint8, device="cuda")
    for nb, N in ((1000, 271), (1000, 1000)):
        d = make(nb, N)
        P = nb * N
        po, qo, st = torch.empty((P, 3), **f64), torch.empty((P, 4), **f64), torch.empty((nb,), **i32)
        cf, co, fl, cst = torch.empty((P, 7), **f64), torch.empty((P, 7), **f64), torch.empty((P,), **u8), torch.empty((nb,), **i32)
        sp, sq, sc, spf, scf = torch.empty((P, 3), **f64), torch.empty((P, 4), **f64), torch.empty((P, 7), **f64), torch.empty((P, 3), **f64), torch.empty((P, 7), **f64)
        sfl, sst = torch.empty((P,), **u8), torch.empty((nb,), **i32)

        def fuse():
            _lib.check(L.gsf_ekf_fuse_ragged_dev(ctx.handle, *[p(x) for x in d], C.byref(cfg), nb, p(po), p(qo), p(st)))

        def cov():
            _lib.check(L.gsf_ekf_cov_ragged_dev(ctx.handle, p(d[0]), p(d[2]), p(d[3]), p(d[4]), p(d[5]), None, C.byref(cfg), nb, p(cf), p(co), p(fl), p(cst)))

        def smooth(filtered=False):
            _lib.check(L.gsf_ekf_smooth_ragged_dev(ctx.handle, *[p(x) for x in d], None, C.byref(cfg), nb, p(sp), p(sq), p(sc), p(spf) if filtered else None,
                                                   p(scf) if filtered else None, p(sfl), p(sst)))

        def smooth_all():
            smooth(True)
        for _ in range(3):
            smooth(); fuse(); cov(); smooth_all()
        ctx.synchronize()
        t_s, t_sa = timed(ctx, smooth, reps, fuse), timed(ctx, smooth_all, reps, cov)
        t_f, t_c = timed(ctx, fuse, reps, smooth), timed(ctx, cov, reps, smooth)
        ctx.synchronize()
        row = {"tracks": nb, "poses": N, "reps": reps, "library": os.path.basename(_lib.library_path()), "smooth_ms": round(t_s, 4),
               "smooth_with_filtered_ms": round(t_sa, 4), "fuse_ms": round(t_f, 4), "cov_ms": round(t_c, 4),
               "smooth_over_fuse_plus_cov": round(t_s / (t_f + t_c), 3), "ns_per_pose": round(1e6 * t_s / P, 3),
               "rows_reached": round(float(((sfl & _lib.POSE_SMOOTHED) != 0).double().mean()), 4),
               "max_correction_m": round(float((sp - spf).abs().max()), 4)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
