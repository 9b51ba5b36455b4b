"""Streaming fusion with a fixed-lag smoother: the time of one append with a lag against the two things a caller could do before it.

B = 1 000 tracks, cap 512, histories of 271 and of 20 000 poses; appends of 1, 16 and 64 poses per track under the lags 8, 32 and 128
(gsf_stream_append_lag_dev, outputs pre-allocated, the raw entry so that no tensor is made inside a window).  Yardsticks, both entries this
feature does not touch, measured in the same process and alternating with the lag windows:
  (a) the plain append (gsf_stream_append_dev) of the same segments;
  (b) the plain append plus gsf_ekf_smooth_ragged_dev over the whole history -- what a caller who wants a smoothed pose pays today.
What the design predicts: a lag append costs the same at either history, (b) grows with the history.

The method is tools/stream_latency.py's: both histories END AT THE SAME POSE of the same synthetic tracks, so the appended rows and their
outages are the same; a stream is brought to its history once and its state and rings are kept; a window restores them (not timed), then
runs K consecutive appends between two events on the stream; REPS windows per case after two warm-up ones, the median with the lowest and
the highest.  One JSON line per history.
usage: python tools/stream_lag_latency.py [reps] [K]"""
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

NB, CAP, SEGS, LAGS = 1000, 512, (1, 16, 64), (8, 32, 128)
PLAIN = ("state_f64", "state_i64", "ring_t", "ring_pos", "ring_quat")
WITH_LAG = PLAIN + ("ring_lag", "ring_spos", "ring_svar")


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
    ip, iq = tb.init_pos.contiguous(), tb.init_quat.contiguous()
    for H in (271, HMAX):
        first = HMAX - H                                                    # the stream's pose 0 is pose `first` of the synthetic track
        ts, pos, quat, gps, valid = (a[:, first:] for a in (tb.ts.view(NB, N), tb.pos.view(NB, N, 3), tb.quat.view(NB, N, 4), tb.gps.view(NB, N, 3), tb.valid.view(NB, N)))
        cut = lambda lo, hi: [a[:, lo:hi].reshape((-1,) + a.shape[2:]).contiguous() for a in (ts, pos, quat, gps, valid)]
        offs = lambda m: torch.arange(NB + 1, **i64) * m
        # ---- the streams at history H: one without a lag, one per lag
        streams, keep = {}, {}
        for lag in (None,) + LAGS:
            s = B.FusionStream(NB, CAP, ip, iq, lag=lag)
            for lo in range(0, H, CAP // 4):
                hi = min(H, lo + CAP // 4)
                st = s.append(*cut(lo, hi), offs(hi - lo), want_cov=False)
            assert int(st.n_total.min()) == H and not bool((st.status & (_lib.STREAM_FULL | _lib.STREAM_BAD_STATE)).any())
            streams[lag], keep[lag] = s, {k: getattr(s, k).clone() for k in (PLAIN if lag is None else WITH_LAG)}
        # ---- yardstick (b)'s second half: the whole H-pose tracks through the whole-track smoother's entry
        whole = cut(0, H) + [offs(H)]
        po, qo, co = torch.empty((NB * H, 3), **f64), torch.empty((NB * H, 4), **f64), torch.empty((NB * H, 7), **f64)
        fl, sst = torch.empty((NB * H,), dtype=torch.uint8, device="cuda"), torch.empty((NB,), dtype=torch.int32, device="cuda")

        def smooth_whole():
            _lib.check(L.gsf_ekf_smooth_ragged_dev(ctx.handle, *[p(x) for x in whole], p(ip), p(iq), None, C.byref(cfg), NB, p(po), p(qo), p(co), None, None,
                                                   p(fl), p(sst)))
        row = {"tracks": NB, "history": H, "cap": CAP, "appends_per_window": K, "reps": reps, "library": os.path.basename(_lib.library_path())}
        for m in SEGS:
            segs = [cut(H + j * m, H + (j + 1) * m) for j in range(K)]
            so = offs(m)
            outs = (torch.empty((NB * m, 3), **f64), torch.empty((NB * m, 4), **f64), torch.empty((NB * m, 7), **f64), torch.empty((NB,), **i64),
                    torch.empty((NB,), **i64), torch.empty((NB,), **i64), torch.empty((NB,), dtype=torch.int32, device="cuda"))
            souts = (torch.empty((NB * m, 3), **f64), torch.empty((NB * m, 3), **f64), torch.empty((NB * m,), dtype=torch.uint8, device="cuda"),
                     torch.empty((NB,), **i64), torch.empty((NB,), **i64))

            def window(lag, smooth_too=False):
                s = streams[lag]
                for seg in segs:
                    if lag is None:
                        _lib.check(L.gsf_stream_append_dev(ctx.handle, C.byref(cfg), NB, CAP, p(s.state_f64), p(s.state_i64), p(s.ring_t), p(s.ring_pos),
                                                           p(s.ring_quat), *[p(x) for x in seg], p(so), *[p(x) for x in outs]))
                        if smooth_too:
                            smooth_whole()
                    else:
                        _lib.check(L.gsf_stream_append_lag_dev(ctx.handle, C.byref(cfg), NB, CAP, lag, p(s.state_f64), p(s.state_i64), p(s.ring_t),
                                                               p(s.ring_pos), p(s.ring_quat), p(s.ring_lag), p(s.ring_spos), p(s.ring_svar),
                                                               *[p(x) for x in seg], p(so), *[p(x) for x in outs], *[p(x) for x in souts]))

            def restore(lag):
                for k, v in keep[lag].items():
                    getattr(streams[lag], k).copy_(v)

            def timed(lag, smooth_too=False):
                restore(lag); ctx.synchronize()
                ctx.timer_start(); window(lag, smooth_too); ms = ctx.timer_stop()
                return 1e3 * ms / K
            t = {k: [] for k in ("plain",) + LAGS}
            for r in range(reps + 2):                                       # (two warm-up rounds); the cases alternate inside a round
                for k in t:
                    us = timed(None if k == "plain" else k)
                    if r >= 2:
                        t[k].append(us)
                if k != "plain":
                    assert int(souts[4].min()) == H + K * m - k and not bool((outs[6] & (_lib.STREAM_FULL | _lib.STREAM_BAD_STATE)).any())
            case = {"plain_append_us": spread(t["plain"])}
            for lag in LAGS:
                case[f"lag_{lag}_us"] = spread(t[lag])
                case[f"lag_{lag}_over_plain"] = round(float(np.median(t[lag]) / np.median(t["plain"])), 2)
            row[f"append_{m}"] = case
        # ---- yardstick (b): the plain append of 1 pose plus the whole-track smoother over the history, a lag window between its windows
        m = 1
        segs = [cut(H + j, H + j + 1) for j in range(K)]
        KB = K if H < 1000 else 4
        segs = segs[:KB]
        so = offs(1)
        outs = (torch.empty((NB, 3), **f64), torch.empty((NB, 4), **f64), torch.empty((NB, 7), **f64), torch.empty((NB,), **i64), torch.empty((NB,), **i64),
                torch.empty((NB,), **i64), torch.empty((NB,), dtype=torch.int32, device="cuda"))
        souts = (torch.empty((NB, 3), **f64), torch.empty((NB, 3), **f64), torch.empty((NB,), dtype=torch.uint8, device="cuda"), torch.empty((NB,), **i64),
                 torch.empty((NB,), **i64))
        tb_us = []
        for r in range(reps + 2):
            for k, v in keep[None].items():
                getattr(streams[None], k).copy_(v)
            ctx.synchronize()
            ctx.timer_start()
            s = streams[None]
            for seg in segs:
                _lib.check(L.gsf_stream_append_dev(ctx.handle, C.byref(cfg), NB, CAP, p(s.state_f64), p(s.state_i64), p(s.ring_t), p(s.ring_pos), p(s.ring_quat),
                                                   *[p(x) for x in seg], p(so), *[p(x) for x in outs]))
                smooth_whole()
            ms = ctx.timer_stop()
            s = streams[LAGS[0]]
            for k, v in keep[LAGS[0]].items():
                getattr(s, k).copy_(v)
            _lib.check(L.gsf_stream_append_lag_dev(ctx.handle, C.byref(cfg), NB, CAP, LAGS[0], p(s.state_f64), p(s.state_i64), p(s.ring_t), p(s.ring_pos),
                                                   p(s.ring_quat), p(s.ring_lag), p(s.ring_spos), p(s.ring_svar), *[p(x) for x in segs[0]], p(so),
                                                   *[p(x) for x in outs], *[p(x) for x in souts]))
            if r >= 2:
                tb_us.append(1e3 * ms / KB)
        row["plain_append_1_plus_smooth_whole_history_us"] = spread(tb_us)
        print(json.dumps(row), flush=True)
        del ts, pos, quat, gps, valid, whole, po, qo, co, fl, streams, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 11, int(sys.argv[2]) if len(sys.argv) > 2 else 50)
