"""EKF noise sweep: gsf_ekf_noise_sweep_dev against the only other way to run the filter under K noise settings, K calls of ekf_fuse_ragged.

Shapes: 1 000 tracks x 271 poses (C2's shape) with K in {1, 9, 64}, and 1 track x 4 000 poses with K = 64.  Per shape: warm-up, then the
context's timer (HIP events on the stream, gsf_timer_start / gsf_timer_stop) around one call, median of the repetitions, the sweep and
the fuse launches alternating inside one process.  The sweep is timed with the automatic group size and with noise_sweep_group forced to
1, 8 and 64.  Prints one JSON line per shape: sweep ms (whole entry: sweep, picks, pooled), ms of ONE fuse launch and K times that, their
ratio, the group size and the number of waves, and the achieved bytes/s on the bytes the algorithm reads: 89 B per pose and group.
usage: python tools/noise_sweep_timing.py [reps]"""
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

PEAK = 8.0e12
FILL_WAVES = 2048                                                       # sweep_group() of csrc/gsf_wave_route.hpp, restated for the report


def auto_group(nb, K):
    groups = min(K, -(-FILL_WAVES // nb))
    return min(64, -(-K // groups))


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
    for nb, N, K in ((1000, 271, 1), (1000, 271, 9), (1000, 271, 64), (1, 4000, 64)):
        d = make(nb, N)
        side = int(round(np.sqrt(K)))
        scales = np.logspace(-1, 1, side) if side * side == K and K > 1 else np.ones(1)
        cand = B.noise_candidates(CONFIG, scales, scales)[0] if K > 1 else B.noise_candidates(CONFIG, (1.0,), (1.0,))[0]
        assert len(cand) == K
        dc = torch.as_tensor(cand).cuda()
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        stats, best, pooled = torch.empty((nb, K, 12), **f64), torch.empty((nb, 2), **i32), torch.empty((K, 12), **f64)
        pbest, st = torch.empty((2,), **i32), torch.empty((nb,), **i32)
        po, qo, fst = torch.empty_like(d[1]), torch.empty_like(d[2]), torch.empty((nb,), **i32)

        def sweep():
            _lib.check(L.gsf_ekf_noise_sweep_dev(ctx.handle, *[p(x) for x in d[:6]], None, p(d[6]), p(d[7]), C.byref(cfg), nb, p(dc), K, 0.0, 1, -1,
                                                 p(stats), p(best), p(pooled), p(pbest), p(st), None, None))

        def fuse():
            _lib.check(L.gsf_ekf_fuse_ragged_dev(ctx.handle, *[p(x) for x in d[:6]], p(d[6]), p(d[7]), C.byref(cfg), nb, p(po), p(qo), p(fst)))
        row = {"tracks": nb, "poses": N, "K": K, "reps": reps, "library": os.path.basename(_lib.library_path())}
        try:
            for forced in (0, 1, 8, 64):
                ctx.set_option("noise_sweep_group", forced)
                for _ in range(3):
                    sweep(); fuse()
                ctx.synchronize()
                ms = timed(ctx, sweep, reps, fuse)
                kc = min(forced, K) if forced else auto_group(nb, K)
                groups = -(-K // kc)
                nbytes = 89.0 * nb * N * groups
                row["auto" if forced == 0 else f"group{forced}"] = {"ms": round(ms, 4), "candidates_per_wave": kc, "waves": nb * groups,
                                                                    "GBps_read": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                                                    "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 4)}
        finally:
            ctx.set_option("noise_sweep_group", 0)
        t_fuse = timed(ctx, fuse, reps, sweep)
        row.update(fuse_ms=round(t_fuse, 4), k_fuse_ms=round(K * t_fuse, 4), k_fuse_over_sweep=round(K * t_fuse / row["auto"]["ms"], 2),
                   n_upd_first_track=float(stats[0, 0, 0]))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
