"""GNSS outage study: gsf_outage_study_dev against the only other way to get the same figures, K calls of ekf_fuse_ragged on edited masks.

Shapes: 1 000 tracks x 271 poses (C2's shape) and 1 track x 4 000 poses, each with K = 64 and K = 1 600 windows of 10 s whose starts are
spread evenly over the track.  Per shape: warm-up, then the context's timer (HIP events on the stream, gsf_timer_start / gsf_timer_stop)
around one call, median of the repetitions, the study and the fuse launches alternating inside one process.  Three figures per shape: the
whole entry; the base pass, timed as the entry with ONE scenario whose window is empty (its scenario pass is one wave per track that writes
a row of zeros); and the scenario pass as the difference of the two.  The yardstick is K times one ekf_fuse_ragged launch -- what a user
has to do today, without the host-side mask edit and error pass that go with every such launch.  The fuse kernels are the same code in
this library as in the one before the study was added.  Prints one JSON line per shape.
usage: python tools/outage_study_timing.py [reps]"""
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

WINDOW = 10.0


def make(nb, N):
    tb = B.TrajectoryBatch.synthetic(nb, N, layout=B.LAYOUT_TRAJ_MAJOR, seed=7)
    P = nb * N
    offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * N
    return (tb.ts.view(P), tb.pos.view(P, 3), tb.quat.view(P, 4), tb.gps.view(P, 3), tb.valid.view(P), offsets, tb.init_pos.contiguous(), tb.init_quat.contiguous())


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
    p = lambda t: C.c_void_p(t.data_ptr())
    for nb, N, K in ((1000, 271, 64), (1000, 271, 1600), (1, 4000, 64), (1, 4000, 1600)):
        d = make(nb, N)
        t0 = d[0][:N].cpu().numpy()
        span = float(t0[-1] - t0[0])
        scen = torch.as_tensor(B.outage_scenarios(np.linspace(0.0, max(span - WINDOW, 0.0), K), [WINDOW])).cuda()
        none = torch.as_tensor(np.array([[np.nan, WINDOW]])).cuda()
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        stats, seg, fl = torch.empty((nb, K, 13), **f64), torch.empty((nb, K, 2), **i32), torch.empty((nb, K), **i32)
        po, qo, fst = torch.empty_like(d[1]), torch.empty_like(d[2]), torch.empty((nb,), **i32)

        def entry(sc=scen, k=K):
            _lib.check(L.gsf_outage_study_dev(ctx.handle, *[p(x) for x in d[:6]], None, p(d[6]), p(d[7]), C.byref(cfg), nb, None, None, p(sc), k, -1,
                                              p(stats), p(seg), p(fl), None, None, None))

        def base():
            entry(none, 1)

        def fuse():
            _lib.check(L.gsf_ekf_fuse_ragged_dev(ctx.handle, *[p(x) for x in d[:6]], p(d[6]), p(d[7]), C.byref(cfg), nb, p(po), p(qo), p(fst)))
        for _ in range(3):
            entry(); base(); fuse()
        ctx.synchronize()
        t_entry, t_base, t_fuse = timed(ctx, entry, reps, fuse), timed(ctx, base, reps, fuse), timed(ctx, fuse, reps, entry)
        st = stats.cpu().numpy()
        poses = float(st[..., 2].sum())                                  # poses of all the outages the scenario pass walked
        print(json.dumps({"tracks": nb, "poses": N, "K": K, "window_s": WINDOW, "track_s": round(span, 2), "reps": reps,
                          "library": os.path.basename(_lib.library_path()), "entry_ms": round(t_entry, 4), "base_ms": round(t_base, 4),
                          "scenario_ms": round(t_entry - t_base, 4), "fuse_ms": round(t_fuse, 4), "k_fuse_ms": round(K * t_fuse, 4),
                          "k_fuse_over_entry": round(K * t_fuse / t_entry, 2), "mean_outage_poses": round(poses / (nb * K), 1),
                          "scenario_GBps_read": round(58.0 * poses / max(t_entry - t_base, 1e-9) / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
