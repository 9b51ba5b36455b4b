"""Per-fix GNSS noise: gsf_ekf_smooth_weighted_dev against gsf_ekf_smooth_ragged_dev on the same rows, the method of tools/lever_timing.py.

Shapes: 1 000 tracks x 271 poses (C2's shape) and 1 000 x 1 000, the default CONFIG.  The weighted entry reads 24 B more per pose and always
runs three variance scans and three d scans, where the unweighted one runs two of each under the default CONFIG (x and y share theirs).
Variances: per-row values that differ between the axes, and per-row values equal on x and y (what an axis-sharing ballot could exploit),
each against the unweighted entry; all optional outputs but nis are written by both.  Per entry: warm-up, then WINDOWS windows of as many
back-to-back calls as fill ~0.3 s (sized from the warm-up) on pre-allocated outputs, each window between two stream events
(gsf_timer_start / gsf_timer_stop); the entries take turns inside every round of windows, so a disturbance of the host hits them alike.
Prints one JSON line per shape: ms per call as the median of the windows with the lowest and highest, and the ratios of the medians.
usage: python tools/weighted_timing.py [windows]"""
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


def window(ctx, fn, calls):
    ctx.timer_start()
    for _ in range(calls):
        fn()
    return ctx.timer_stop() / calls


def main(windows):
    ctx = B.context()
    L = _lib.load()
    cfg = _lib.EkfConfig.from_config(CONFIG)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f64, i32, u8 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.uint8, device="cuda")
    for nb, N in ((1000, 271), (1000, 1000)):
        tb = B.TrajectoryBatch.synthetic(nb, N, layout=B.LAYOUT_TRAJ_MAJOR, seed=7)
        P = nb * N
        offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * N
        d = (tb.ts.view(P), tb.pos.view(P, 3), tb.quat.view(P, 4), tb.gps.view(P, 3), tb.valid.view(P))
        tail = (offsets, tb.init_pos.contiguous(), tb.init_quat.contiguous())
        rng = np.random.default_rng(3)
        differ = torch.as_tensor(10.0 ** rng.uniform(-4, 1, (P, 3)), **f64)
        xy = differ.clone(); xy[:, 1] = xy[:, 0]
        outs = [tuple([torch.empty((P, 3), **f64), torch.empty((P, 4), **f64), torch.empty((P, 7), **f64), torch.empty((P, 3), **f64), torch.empty((P, 7), **f64),
                       torch.empty((P,), **u8), torch.empty((nb,), **i32)]) for _ in range(2)]
        nis = torch.empty((P,), **f64)

        def plain():
            _lib.check(L.gsf_ekf_smooth_ragged_dev(ctx.handle, *[p(x) for x in d + tail], None, C.byref(cfg), nb, *[p(x) for x in outs[0]]))

        def weighted(mv, with_nis):
            _lib.check(L.gsf_ekf_smooth_weighted_dev(ctx.handle, *[p(x) for x in d], p(mv), *[p(x) for x in tail], None, C.byref(cfg), nb,
                                                     *[p(x) for x in outs[1]], p(nis) if with_nis else None))
        entries = {"smooth": plain, "weighted_axes_differ": lambda: weighted(differ, False), "weighted_xy_equal": lambda: weighted(xy, False),
                   "weighted_axes_differ_nis": lambda: weighted(differ, True)}
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
        row = {"tracks": nb, "poses": N, "windows": windows, "calls_per_window": calls, "library": os.path.basename(_lib.library_path()),
               "rows_used": round(float(((outs[1][5] & _lib.POSE_GNSS_USED) != 0).double().mean()), 4),
               "rows_bad_sigma": int(((outs[1][5] & _lib.POSE_BAD_SIGMA) != 0).sum())}
        for name, v in ms.items():
            row[name + "_ms"] = {"median": round(float(np.median(v)), 5), "lowest": round(min(v), 5), "highest": round(max(v), 5)}
        base = row["smooth_ms"]["median"]
        for name in entries:
            if name != "smooth":
                row[name + "_over_smooth"] = round(row[name + "_ms"]["median"] / base, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
