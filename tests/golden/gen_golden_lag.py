#!/usr/bin/env python3
"""Generate tests/golden/ekf_lag_tracks.npz: the fixed-lag RTS smoother of the streaming fusion, computed by the REFERENCE's own code.

Runs only where the reference is present (see gen_golden.py).  As gen_golden_smooth.py does, the reference's apply_ekf_correction runs on
every track with recorders around ExtendedKalmanFilter.process_step (all four returns of every pose) and is_sharp_turn_in_segment; every
recovery judged a sharp turn starts a new span.  Then, for every lag L and every row i with s(i) the last row of i's span,

    we(i) = min(i + L, s(i), n - 1)

and the reference's OWN rts_smoother_segment is called on the four lists cut to rows [i .. we(i)]; its first row is row i of the fixed-lag
smoother.  The wrappers are this file's own code; nothing of the reference is copied, and only data is stored:

  track_index (T,)  which tracks: indices into the file order of ekf_smooth_tracks.npz (tests/test_smooth_host.py::smooth_tracks serves their
                    inputs, initial poses and configs) -- eight of ekf_random_tracks.npz, every hand-made track of gen_golden_cov.py, the
                    five of gen_golden_smooth.new_tracks()
  offsets (T+1,)    rows of every track in the flat per-pose arrays
  lags (4,)         1, 5, 64 and 512 (>= every track's length)
  filt_pos, filt_var (P,3)      the filter's position and variance (process_step's first two returns; row 0 = the initial pose under P0)
  lag_pos, lag_var (4,P,3)      the smoothed position and variance under each lag
  lag_reached (4,P)             "a fix was applied in rows (i, we(i)]" (GSF_POSE_SMOOTHED)
  span_start (P,)               row 0 and every sharp-turn recovery (GSF_POSE_SPAN_START)

Asserted here: the rows of the largest lag equal ekf_smooth_tracks.npz's smooth_pos / smooth_var bit for bit; rows outside any fix's reach
equal the filtered lists exactly; every off-diagonal element of every smoothed covariance is exactly 0.0.

    python tests/golden/gen_golden_lag.py
"""
import json
import os

import numpy as np

from gen_golden import HERE, AlignRecorder, cfg_copy, quiet, ref, save
from gen_golden_cov import diag_exact, hand_tracks
from gen_golden_smooth import StepRecorder, new_tracks

LAGS = (1, 5, 64, 512)
N_RANDOM_USED = 8


def record(ts, pos, quat, aligned, valid, ip, iq, cfg):
    """the four lists apply_ekf_correction keeps, the span starts and the rows that took a fix"""
    n = len(ts)
    slam = {"timestamps": ts, "positions": pos, "quaternions": quat}
    sp, sq = pos.copy(), quat.copy()
    sp[0], sq[0] = ip, iq
    with quiet(), AlignRecorder(inject=(aligned, valid)), StepRecorder() as rec:
        ref.apply_ekf_correction(slam, {"timestamps": ts, "positions": aligned}, sp, sq, cfg)
    assert len(rec.steps) == n - 1
    x0 = np.concatenate([ip, ref.ExtendedKalmanFilter.normalize_quaternion(np.asarray(iq, float))])
    P0 = np.diag(cfg["ekf"]["initial_cov_diag"]).astype(float)
    sf, cf = [x0] + [s[0] for s in rec.steps], [P0] + [s[1] for s in rec.steps]
    sp_, cp = [x0] + [s[2] for s in rec.steps], [P0] + [s[3] for s in rec.steps]
    starts = [0] + [b for a, b, res in rec.decisions if res]
    fix = np.zeros(n, bool)
    fix[1:] = np.asarray(valid[1:], bool) & ~np.isnan(aligned[1:]).any(axis=1)      # (:867-869; pose 0 takes no update)
    return sf, cf, sp_, cp, starts, fix


def lag_rows(sf, cf, sp_, cp, starts, fix, L):
    n = len(sf)
    span_last = np.empty(n, int)
    for s, e in zip(starts, starts[1:] + [n]):
        span_last[s:e] = e - 1
    xs, Ps, reached = np.empty((n, 3)), np.empty((n, 3)), np.zeros(n, bool)
    for i in range(n):
        we = min(i + L, int(span_last[i]), n - 1)
        with quiet():
            ss, cs = ref.rts_smoother_segment(sf[i:we + 1], cf[i:we + 1], sp_[i:we + 1], cp[i:we + 1])
        xs[i], Ps[i] = ss[0][:3], diag_exact(cs[0])[:3]
        reached[i] = fix[i + 1:we + 1].any()
        if not reached[i]:
            assert (xs[i] == sf[i][:3]).all() and (Ps[i] == np.diag(cf[i])[:3]).all(), "a row no fix reaches moved"
    return xs, Ps, reached


def main():
    sm = np.load(os.path.join(HERE, "ekf_smooth_tracks.npz"), allow_pickle=False)
    g = np.load(os.path.join(HERE, "ekf_random_tracks.npz"), allow_pickle=False)
    cfgs = [json.loads(str(s)) for s in sm["cfgs"]]
    full = [cfg_copy(), cfg_copy(), cfg_copy()]
    for c, k in zip(full, cfgs):                                 # the stored sections over the reference's CONFIG
        for sec in k:
            c[sec] = k[sec]
    nr, nh = int(sm["n_random"]), int(sm["n_hand"])
    hand, new = hand_tracks(), new_tracks()
    assert len(hand) == nh
    ci = sm["cfg_index"]
    tracks = [(b, (g["ts"][b], g["pos"][b], g["quat"][b], g["aligned"][b], g["valid"][b]), g["sp0"][b], g["sq0"][b]) for b in range(N_RANDOM_USED)]
    tracks += [(nr + j, tr, tr[1][0].copy(), tr[2][0].copy()) for j, (name, _, tr) in enumerate(hand + new)]
    so = sm["offsets"]
    offsets, FP, FV, LP, LV, LR, SS = [0], [], [], [], [], [], []
    for idx, (ts, pos, quat, aligned, valid), ip, iq in tracks:
        n = len(ts)
        assert n == so[idx + 1] - so[idx] and n <= LAGS[-1]
        sf, cf, sp_, cp, starts, fix = record(ts, pos, quat, aligned, valid, ip, iq, full[int(ci[idx])])
        assert starts == [int(a) for b, a in sm["span_starts"] if b == idx]
        per = [lag_rows(sf, cf, sp_, cp, starts, fix, L) for L in LAGS]
        sl = slice(so[idx], so[idx + 1])
        assert (per[-1][0] == sm["smooth_pos"][sl]).all() and (per[-1][1] == sm["smooth_var"][sl]).all(), "lag >= length is not the whole-track smoother"
        FP.append(np.array([s[:3] for s in sf])); FV.append(np.array([np.diag(P)[:3] for P in cf]))
        assert (FP[-1] == sm["filt_pos"][sl]).all()
        LP.append(np.stack([p[0] for p in per])); LV.append(np.stack([p[1] for p in per])); LR.append(np.stack([p[2] for p in per]))
        st = np.zeros(n, bool); st[starts] = True
        SS.append(st); offsets.append(offsets[-1] + n)
    save("ekf_lag_tracks.npz", track_index=np.array([t[0] for t in tracks], np.int64), offsets=np.array(offsets, np.int64), lags=np.array(LAGS, np.int64),
         filt_pos=np.concatenate(FP), filt_var=np.concatenate(FV), lag_pos=np.concatenate(LP, axis=1), lag_var=np.concatenate(LV, axis=1),
         lag_reached=np.concatenate(LR, axis=1), span_start=np.concatenate(SS))
    print(f"{len(tracks)} tracks, {offsets[-1]} poses, lags {LAGS}")


if __name__ == "__main__":
    main()
