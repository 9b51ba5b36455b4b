"""Streaming fusion: the time of one append against the only thing a caller could do before it, fusing the whole track again.

B = 1 000 tracks with a history of 271 and of 20 000 poses; appends of 1, 16 and 64 poses per track (gsf_stream_append_dev, cap 256,
outputs pre-allocated, the raw entry so that no tensor is made inside the window); the yardstick is ekf_fuse_ragged's entry on the whole
1 000 x 271 and 1 000 x 20 000 tracks -- an entry this feature does not touch, measured in the same process, the two alternating.
What the design predicts: an append costs the same at either history, the re-fuse does not.

Both histories END AT THE SAME POSE of the same synthetic tracks (the short one starts 271 poses before it), so the appended segments are
the same rows in both cases and carry the same outages: what differs is the history alone.

Method: the stream is brought to its history once and its state and ring are kept; a window restores them (not timed), then runs K
consecutive appends of m poses between two events on the stream (gsf_timer_start / gsf_timer_stop) -- one append is too short for an event
pair -- and a host clock around the same K calls with a synchronise at the end tells whether the launch path or the kernel bounds it.
Every shape is warmed up; REPS windows per case, the median with the lowest and highest as the spread.  One JSON line per history.
usage: python tools/stream_latency.py [reps] [K]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gps_optimize_slam_amd import batch as B  # noqa: E402
from gps_optimize_slam_amd import _lib  # noqa: E402
from gps_optimize_slam_amd.ekfgpsslam import CONFIG  # noqa: E402

NB, CAP, SEGS = 1000, 256, (1, 16, 64)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def main(reps, K):
    ctx = B.context()
    L = _lib.load()
    cfg = _lib.EkfConfig.from_config(CONFIG)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f64, i64 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int64, device="cuda")
    HMAX = 20000
    N = HMAX + K * max(SEGS)
    tb = B.TrajectoryBatch.synthetic(NB, N, layout=B.LAYOUT_TRAJ_MAJOR, seed=7)
    for H in (271, HMAX):
        first = HMAX - H                                                    # the stream's pose 0 is pose `first` of the synthetic track
        ts, pos, quat, gps, valid = (a[:, first:] for a in (tb.ts.view(NB, N), tb.pos.view(NB, N, 3), tb.quat.view(NB, N, 4), tb.gps.view(NB, N, 3), tb.valid.view(NB, N)))
        cut = lambda lo, hi: [a[:, lo:hi].reshape((-1,) + a.shape[2:]).contiguous() for a in (ts, pos, quat, gps, valid)]
        offs = lambda m: torch.arange(NB + 1, **i64) * m
        # ---- the stream at history H
        s = B.FusionStream(NB, CAP, tb.init_pos.contiguous(), tb.init_quat.contiguous())
        for lo in range(0, H, CAP // 2):
            hi = min(H, lo + CAP // 2)
            st = s.append(*cut(lo, hi), offs(hi - lo), want_cov=False)
        assert int(st.n_total.min()) == H and not bool((st.status & (_lib.STREAM_FULL | _lib.STREAM_BAD_STATE)).any())
        keep = {k: getattr(s, k).clone() for k in ("state_f64", "state_i64", "ring_t", "ring_pos", "ring_quat")}
        # ---- the yardstick: the whole H-pose tracks through ekf_fuse_ragged's entry
        whole = cut(0, H) + [offs(H)]
        ip, iq = tb.init_pos.contiguous(), tb.init_quat.contiguous()
        po, qo, fst = torch.empty((NB * H, 3), **f64), torch.empty((NB * H, 4), **f64), torch.empty((NB,), dtype=torch.int32, device="cuda")

        def refuse():
            _lib.check(L.gsf_ekf_fuse_ragged_dev(ctx.handle, *[p(x) for x in whole], p(ip), p(iq), C.byref(cfg), NB, p(po), p(qo), p(fst)))
        row = {"tracks": NB, "history": H, "cap": CAP, "appends_per_window": K, "reps": reps, "library": os.path.basename(_lib.library_path())}
        cases = {}
        for m in SEGS:
            segs = [cut(H + j * m, H + (j + 1) * m) for j in range(K)]
            so = offs(m)
            outs = (torch.empty((NB * m, 3), **f64), torch.empty((NB * m, 4), **f64), torch.empty((NB * m, 7), **f64), torch.empty((NB,), **i64),
                    torch.empty((NB,), **i64), torch.empty((NB,), **i64), torch.empty((NB,), dtype=torch.int32, device="cuda"))

            def window():
                for seg in segs:
                    _lib.check(L.gsf_stream_append_dev(ctx.handle, C.byref(cfg), NB, CAP, p(s.state_f64), p(s.state_i64), p(s.ring_t), p(s.ring_pos),
                                                       p(s.ring_quat), *[p(x) for x in seg], p(so), *[p(x) for x in outs]))

            def restore():
                for k, v in keep.items():
                    getattr(s, k).copy_(v)
            dev_us, host_us = [], []
            for r in range(reps + 2):                                       # (two warm-up windows)
                restore(); ctx.synchronize()
                t0 = time.perf_counter()
                ctx.timer_start(); window(); ms = ctx.timer_stop()          # (timer_stop waits for the second event)
                t1 = time.perf_counter()
                refuse()                                                    # the yardstick between the windows
                if r >= 2:
                    dev_us.append(1e3 * ms / K); host_us.append(1e6 * (t1 - t0) / K)
            assert int(outs[3].min()) == H + K * m and not bool((outs[6] & (_lib.STREAM_FULL | _lib.STREAM_BAD_STATE)).any())
            cases[f"append_{m}"] = {"us_per_append_events": spread(dev_us), "us_per_append_host_clock": spread(host_us)}
        row.update(cases)
        ctx.synchronize()
        KF = K if H < 1000 else 2
        ms_f = []
        for r in range(reps + 2):
            ctx.timer_start()
            for _ in range(KF):
                refuse()
            ms = ctx.timer_stop()
            restore(); window()                                             # an append window between the yardstick's
            if r >= 2:
                ms_f.append(1e3 * ms / KF)
        row["refuse_whole_tracks_us"] = spread(ms_f)
        print(json.dumps(row), flush=True)
        del ts, pos, quat, gps, valid, whole, po, qo, s, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 11, int(sys.argv[2]) if len(sys.argv) > 2 else 50)
