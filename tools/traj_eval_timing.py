"""Trajectory evaluation: gsf_traj_eval_dev next to one fuse launch (gsf_fuse_pipeline_ragged_dev) at the same shape, the method of
tools/lever_timing.py.

Shapes: 1 000 tracks x 271 poses (C2's shape) and 1 000 x 1 000.  The estimate is the fused track of the synthetic batch, the truth its
GNSS positions with the SLAM orientations at the same stamps (every pose is matched).  Nine scenarios: KITTI's eight segment lengths at a
first frame every 10 poses, and the frame-to-frame error.  Entries: nearest association with an SE3 alignment and the nine scenarios; the
same without scenarios (two launches); interpolated association.  Per entry: warm-up, then WINDOWS windows of as many back-to-back calls as
fill ~0.3 s (sized from the warm-up), each window timed with the context's timer (HIP events on the stream); the entries take turns inside
every round of windows, so a disturbance of the host hits them alike.  Prints one JSON line per shape: ms per call as the median of the
windows with the lowest and highest, and the pairs found per scenario.  The entry is not part of bench.py.
usage: python tools/traj_eval_timing.py [windows]"""
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
    scen = B.rpe_scenarios(frames=(1,), metres=tuple(100.0 * k for k in range(1, 9)), stride=[1] + [10] * 8)
    for nb, N in ((1000, 271), (1000, 1000)):
        tb = B.TrajectoryBatch.synthetic(nb, N, layout=B.LAYOUT_TRAJ_MAJOR, seed=7)
        P = nb * N
        ts, pos, quat, gps, valid = tb.ts.view(P), tb.pos.view(P, 3), tb.quat.view(P, 4), tb.gps.view(P, 3), tb.valid.view(P)
        offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * N
        fused_pos, fused_quat, _, _, _, _ = B.fuse_pipeline_ragged(ts, pos, quat, gps, valid, offsets)
        cfg = B.EkfConfig.from_config(B.CONFIG)
        R, t, s, st = torch.empty((nb, 9), **f64), torch.empty((nb, 3), **f64), torch.empty((nb,), **f64), torch.empty((nb,), **i32)
        po, qo = torch.empty_like(pos), torch.empty_like(quat)
        o = dict(R=torch.empty((nb, 9), **f64), t=torch.empty((nb, 3), **f64), s=torch.empty((nb,), **f64), state=torch.empty((nb,), **i32),
                 flags=torch.empty((P,), dtype=torch.uint8, device="cuda"), index=torch.empty((P,), **i32), ape_t=torch.empty((P,), **f64),
                 ape_r=torch.empty((P,), **f64), stats=torch.empty((nb, 2, 8), **f64), rpe_n=torch.empty((nb, scen.K), dtype=torch.int64, device="cuda"),
                 rpe_sums=torch.empty((nb, scen.K, 8), **f64))

        def fuse():
            _lib.check(L.gsf_fuse_pipeline_ragged_dev(ctx.handle, p(ts), p(pos), p(quat), p(gps), p(valid), p(offsets), C.byref(cfg), nb, p(R), p(t), p(s),
                                                      p(po), p(qo), p(st)))

        def evaluate(assoc, K):
            def fn():
                _lib.check(L.gsf_traj_eval_dev(ctx.handle, p(ts), p(fused_pos), p(fused_quat), p(offsets), P, p(ts), p(gps), p(quat), p(offsets), None, nb,
                                               assoc, 0.01 if assoc == _lib.TE_NEAREST else 1.0, _lib.TE_ALIGN_SE3, K, p(scen.kind), p(scen.value),
                                               p(scen.stride), -1, p(o["R"]), p(o["t"]), p(o["s"]), p(o["state"]), p(o["flags"]), p(o["index"]),
                                               p(o["ape_t"]), p(o["ape_r"]), p(o["stats"]), p(o["rpe_n"]), p(o["rpe_sums"]), None, None, None))
            return fn
        entries = {"eval_nearest_se3_9": evaluate(_lib.TE_NEAREST, scen.K), "eval_nearest_se3_0": evaluate(_lib.TE_NEAREST, 0),
                   "eval_interp_se3_9": evaluate(_lib.TE_INTERP, scen.K), "fuse_pipeline": fuse}
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
        entries["eval_nearest_se3_9"]()
        ctx.synchronize()
        row = {"tracks": nb, "poses": N, "scenarios": scen.K, "tracks_evaluated": int((o["state"] == 0).sum().item()),
               "poses_matched": int((o["flags"] == _lib.TE_MATCHED).sum().item()), "pairs_per_scenario": o["rpe_n"].sum(dim=0).tolist(),
               "windows": windows, "calls_per_window": calls, "library": os.path.basename(_lib.library_path())}
        for name, v in ms.items():
            row[name + "_us"] = {"median": round(1e3 * float(np.median(v)), 2), "lowest": round(1e3 * min(v), 2), "highest": round(1e3 * max(v), 2)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
