"""Antenna lever arm: gsf_lever_fit_dev and gsf_lever_apply_dev next to what one global alignment of the same tracks costs
(gsf_sim3_umeyama_batch_dev on the valid rows + gsf_apply_sim3_batch_dev), the method of tools/local_align_timing.py.

Shapes: 1 000 tracks x 271 poses (C2's shape) and 1 000 x 1 000, the defaults of batch.lever_fit_ragged (4 rounds).  Per entry: warm-up,
then WINDOWS windows of as many back-to-back calls as fill ~0.3 s (sized from the warm-up), each window timed with the context's timer
(HIP events on the stream, gsf_timer_start / gsf_timer_stop); the four entries take turns inside every round of windows, so a
disturbance of the host hits them alike.  Prints one JSON line per shape: ms per call as the median of the windows with the lowest and
highest, how many tracks kept their starting values (a flagged track leaves the rounds early and would flatter the figure), and the share
of the 8 TB/s HBM peak the apply reaches on its algorithmic bytes (quat, xyz read; xyz_out, pose_flags written: 84 B per pose) beside
K3's on its 112 B.
usage: python tools/lever_timing.py [windows]"""
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
APPLY_BYTES_PER_POSE = 32 + 24 + 24 + 4


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
        pos, quat, gps, valid = tb.pos.view(P, 3), tb.quat.view(P, 4), tb.gps.view(P, 3), tb.valid.view(P)
        offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * N
        R, t, s, st = torch.empty((nb, 9), **f64), torch.empty((nb, 3), **f64), torch.empty((nb,), **f64), torch.empty((nb,), **i32)
        po, qo, bad = torch.empty_like(pos), torch.empty_like(quat), torch.empty((nb,), **i32)
        l0 = torch.zeros((nb, 3), **f64)
        Ro, to, so, lo, lc = torch.empty((nb, 9), **f64), torch.empty((nb, 3), **f64), torch.empty((nb,), **f64), torch.empty((nb, 3), **f64), torch.empty((nb, 9), **f64)
        nr, nq, fl = torch.empty((nb,), **i32), torch.empty((nb,), **i32), torch.empty((nb,), **i32)
        r0, r1, ls = torch.empty((nb,), **f64), torch.empty((nb,), **f64), torch.empty((nb,), **f64)
        gc, pf = torch.empty_like(gps), torch.empty((P,), **i32)
        cfg = B._lever_config(0.5, 1.0, 0.05, True, True, 4, 8, 2.0, 1e-10, 0.5, 1e-6)

        def global_fit():
            _lib.check(L.gsf_sim3_umeyama_batch_dev(ctx.handle, p(pos), p(gps), p(valid), p(offsets), nb, p(R), p(t), p(s), p(st)))

        def global_apply():
            _lib.check(L.gsf_apply_sim3_batch_dev(ctx.handle, p(pos), p(quat), p(offsets), nb, p(R), p(t), p(s), p(po), p(qo), p(bad)))

        def fit():
            _lib.check(L.gsf_lever_fit_dev(ctx.handle, p(pos), p(quat), p(gps), p(valid), p(offsets), nb, p(R), p(t), p(s), p(l0), None, C.byref(cfg),
                                           p(Ro), p(to), p(so), p(lo), p(lc), p(nr), p(nq), p(r0), p(r1), p(ls), p(fl)))

        def apply():
            _lib.check(L.gsf_lever_apply_dev(ctx.handle, p(quat), p(gps), p(offsets), nb, p(Ro), p(lo), -1.0, p(gc), p(pf)))
        global_fit()
        ctx.synchronize()
        entries = {"lever_fit": fit, "lever_apply": apply, "global_fit": global_fit, "global_apply": global_apply}
        calls = {}
        for name, fn in entries.items():                                  # warm-up, and the calls that fill a window of ~0.3 s
            for _ in range(5):
                fn()
            ctx.synchronize()
            calls[name] = max(10, int(300.0 / max(window(ctx, fn, 20), 1e-4)))
        ms = {name: [] for name in entries}
        for _ in range(windows):
            for name, fn in entries.items():
                ms[name].append(window(ctx, fn, calls[name]))
        ctx.synchronize()
        row = {"tracks": nb, "poses": N, "iters": int(cfg.iters), "tracks_kept_at_start": int(((fl & _lib.LEVER_KEPT) != 0).sum().item()),
               "tracks_not_converged": int(((fl & _lib.LEVER_NOT_CONVERGED) != 0).sum().item()), "rows_per_track": round(float(nr.double().mean().item()), 1),
               "windows": windows, "calls_per_window": calls, "library": os.path.basename(_lib.library_path())}
        for name, v in ms.items():
            row[name + "_ms"] = {"median": round(float(np.median(v)), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}
        lev = row["lever_fit_ms"]["median"] + row["lever_apply_ms"]["median"]
        glo = row["global_fit_ms"]["median"] + row["global_apply_ms"]["median"]
        row.update(lever_ms=round(lev, 5), global_ms=round(glo, 5), lever_over_global=round(lev / glo, 2),
                   apply_share_of_hbm_peak=round(P * APPLY_BYTES_PER_POSE / (row["lever_apply_ms"]["median"] * 1e-3) / HBM_PEAK, 4),
                   global_apply_share_of_hbm_peak=round(P * 112 / (row["global_apply_ms"]["median"] * 1e-3) / HBM_PEAK, 4))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
