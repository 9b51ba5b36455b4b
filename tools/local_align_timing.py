"""Local Sim3 alignment: gsf_sim3_local_fit_dev and gsf_sim3_local_apply_dev next to what one global alignment of the same tracks costs
(gsf_sim3_umeyama_batch_dev on the valid rows + gsf_apply_sim3_batch_dev).

Shapes: 1 000 tracks x 271 poses (C2's shape) and 1 000 x 1 000, spacing 30 s, half-window 30 s, min_rows 8, both modes.  Per entry:
warm-up, then WINDOWS windows of as many back-to-back calls as fill ~0.3 s (sized from the warm-up), each window timed with the context's
timer (HIP events on the stream, gsf_timer_start / gsf_timer_stop); the four entries take turns inside every round of windows, so a
disturbance of the host hits them alike.  Prints one JSON line per shape and mode: ms per call as the median of the windows with the
lowest and highest, the knots per track, and the share of the 8 TB/s HBM peak the blend reaches on its algorithmic bytes (ts, pos, quat
read; pos, quat, scale_at, pose_flags written: 132 B per pose; the knot rows are a few KB).
usage: python tools/local_align_timing.py [windows]"""
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

HBM_PEAK = 8.0e12
APPLY_BYTES_PER_POSE = 8 + 24 + 32 + 24 + 32 + 8 + 4


def window(ctx, fn, calls):
    ctx.timer_start()
    for _ in range(calls):
        fn()
    return ctx.timer_stop() / calls


def main(windows):
    ctx = B.context()
    L = _lib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    for nb, N in ((1000, 271), (1000, 1000)):
        tb = B.TrajectoryBatch.synthetic(nb, N, layout=B.LAYOUT_TRAJ_MAJOR, seed=7)
        P = nb * N
        ts, pos, quat, gps, valid = tb.ts.view(P), tb.pos.view(P, 3), tb.quat.view(P, 4), tb.gps.view(P, 3), tb.valid.view(P)
        offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * N
        R, t, s, st = torch.empty((nb, 9), **f64), torch.empty((nb, 3), **f64), torch.empty((nb,), **f64), torch.empty((nb,), **i32)
        po, qo, bad = torch.empty_like(pos), torch.empty_like(quat), torch.empty((nb,), **i32)
        sc, fl = torch.empty((P,), **f64), torch.empty((P,), **i32)

        def global_fit():
            _lib.check(L.gsf_sim3_umeyama_batch_dev(ctx.handle, p(pos), p(gps), p(valid), p(offsets), nb, p(R), p(t), p(s), p(st)))

        def global_apply():
            _lib.check(L.gsf_apply_sim3_batch_dev(ctx.handle, p(pos), p(quat), p(offsets), nb, p(R), p(t), p(s), p(po), p(qo), p(bad)))
        global_fit()
        ctx.synchronize()
        span = float((ts[N - 1] - ts[0]).item())
        for mode in ("scale", "sim3"):
            cfg = B._local_config(mode, 8, 30.0, 30.0, 1e-3, 2.0)
            Kmax = B._knot_stride(ts, offsets, 30.0, nb, P)
            kR, kt, ks = torch.empty((nb, Kmax, 9), **f64), torch.empty((nb, Kmax, 3), **f64), torch.empty((nb, Kmax), **f64)
            kn, krms, kfl = torch.empty((nb, Kmax), **i32), torch.empty((nb, Kmax), **f64), torch.empty((nb, Kmax), **i32)
            nk, tst = torch.empty((nb,), **i32), torch.empty((nb,), **i32)

            def fit():
                _lib.check(L.gsf_sim3_local_fit_dev(ctx.handle, p(ts), p(pos), p(gps), p(valid), p(offsets), nb, p(R), p(t), p(s), C.byref(cfg), Kmax,
                                                    p(kR), p(kt), p(ks), p(kn), p(krms), p(kfl), p(nk), p(tst)))

            def apply():
                _lib.check(L.gsf_sim3_local_apply_dev(ctx.handle, p(ts), p(pos), p(quat), p(offsets), nb, p(R), p(t), p(s), 30.0, Kmax, p(kR), p(kt), p(ks),
                                                      p(kfl), p(nk), p(tst), p(po), p(qo), p(sc), p(fl)))
            entries = {"local_fit": fit, "local_apply": apply, "global_fit": global_fit, "global_apply": global_apply}
            calls = {}
            for name, fn in entries.items():                              # warm-up, and the calls that fill a window of ~0.3 s
                for _ in range(5):
                    fn()
                ctx.synchronize()
                calls[name] = max(10, int(300.0 / max(window(ctx, fn, 20), 1e-4)))
            ms = {name: [] for name in entries}
            for _ in range(windows):
                for name, fn in entries.items():
                    ms[name].append(window(ctx, fn, calls[name]))
            ctx.synchronize()
            row = {"tracks": nb, "poses": N, "track_seconds": round(span, 2), "mode": mode, "spacing": 30.0, "half_window": 30.0, "knot_stride": Kmax,
                   "valid_knots_per_track": round(float(((kfl[:, :Kmax] & 7) == 0).sum().item()) / nb, 2), "tracks_with_status": int((tst != 0).sum().item()),
                   "windows": windows, "calls_per_window": calls, "library": os.path.basename(_lib.library_path())}
            for name, v in ms.items():
                row[name + "_ms"] = {"median": round(float(np.median(v)), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}
            loc = row["local_fit_ms"]["median"] + row["local_apply_ms"]["median"]
            glo = row["global_fit_ms"]["median"] + row["global_apply_ms"]["median"]
            row.update(local_ms=round(loc, 5), global_ms=round(glo, 5), local_over_global=round(loc / glo, 2),
                       apply_share_of_hbm_peak=round(P * APPLY_BYTES_PER_POSE / (row["local_apply_ms"]["median"] * 1e-3) / HBM_PEAK, 4),
                       global_apply_share_of_hbm_peak=round(P * 112 / (row["global_apply_ms"]["median"] * 1e-3) / HBM_PEAK, 4))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
