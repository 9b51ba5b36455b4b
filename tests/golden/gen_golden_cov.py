#!/usr/bin/env python3
"""Generate tests/golden/ekf_cov_tracks.npz: the covariances the REFERENCE computes inside apply_ekf_correction and drops.

Runs only where the reference is present (see gen_golden.py, whose import helpers are used).  The reference's own
apply_ekf_correction runs on every track with recorders wrapped around ExtendedKalmanFilter.process_step (filtered and predicted
covariance of every pose), rts_smoother_segment (smoothed covariances of every segment it rewrites) and is_sharp_turn_in_segment
(its decision per outage).  The wrappers are this file's own code; nothing of the reference is copied, and only data is stored:

  tracks   the 64 inputs of ekf_random_tracks.npz (NOT stored again: `n_random` says how many lead the file order) followed by the
           hand-made tracks below (stored: hand_offsets, hand_ts, hand_quat, hand_aligned, hand_valid, hand_names)
  offsets  (T+1,) rows of every track in the flat per-pose arrays, file order
  filt     (P,7)  diagonal of ekf_covs_filt_hist
  smooth   (P,7)  diagonal of the smoothed covariance on the rows of every smoothed segment [a..b], the filtered one elsewhere
  segments (K,3)  track, a, b of every rts_smoother_segment call (a = outage start, b = recovery), from the recorders' call order
  sharp    (K,3)  track, a, b of every outage a..b-1 whose recovery b was judged a sharp turn
  cfg_index (T,) / cfgs: index into the JSON configs (0 = the reference's CONFIG, 1 = three distinct position axes, 5 transition steps)

Asserted here: every off-diagonal element of every filtered, predicted and smoothed covariance is exactly 0.0, and the largest yaw
rate of every judged outage lies outside 0.9 .. 1.1 x the threshold (computed here with scipy), so no decision hangs on an ulp.

    python tests/golden/gen_golden_cov.py
"""
import json
import os

import numpy as np
from scipy.spatial.transform import Rotation

from gen_golden import HERE, cfg_copy, quiet, ref, save, AlignRecorder


class CovRecorder:
    """Records what process_step / rts_smoother_segment / is_sharp_turn_in_segment return, in call order."""

    def __init__(self):
        self.filt, self.pred, self.segs, self.decisions = [], [], [], []

    def __enter__(self):
        self._ps, self._rts, self._sharp = ref.ExtendedKalmanFilter.process_step, ref.rts_smoother_segment, ref.is_sharp_turn_in_segment
        rec = self

        def process_step(ekf, *a, **k):
            r = rec._ps(ekf, *a, **k)
            rec.filt.append(np.array(r[1])); rec.pred.append(np.array(r[3]))
            return r

        def rts(sf, cf, sp, cp):
            s, c = rec._rts(sf, cf, sp, cp)
            b = len(rec.filt)                                   # process_step has been called for poses 1..b
            rec.segs.append((b - len(sf) + 1, b, [np.array(x) for x in c]))
            return s, c

        def sharp(quats, stamps, thr):
            res = rec._sharp(quats, stamps, thr)
            b = len(rec.filt) + 1                               # asked before the recovery pose's process_step
            rec.decisions.append((b - len(quats), b, bool(res)))
            return res

        ref.ExtendedKalmanFilter.process_step, ref.rts_smoother_segment, ref.is_sharp_turn_in_segment = process_step, rts, sharp
        return self

    def __exit__(self, *a):
        ref.ExtendedKalmanFilter.process_step, ref.rts_smoother_segment, ref.is_sharp_turn_in_segment = self._ps, self._rts, self._sharp


def diag_exact(M):
    M = np.asarray(M)
    assert M.shape == (7, 7)
    assert (M[~np.eye(7, dtype=bool)] == 0.0).all(), "off-diagonal element is not exactly 0"
    return np.diag(M).copy()


def run_track(ts, pos, quat, aligned, valid, cfg):
    n = len(ts)
    slam = {"timestamps": ts, "positions": pos, "quaternions": quat}
    with quiet(), AlignRecorder(inject=(aligned, valid)), CovRecorder() as rec:
        ref.apply_ekf_correction(slam, {"timestamps": ts, "positions": aligned}, pos.copy(), quat.copy(), cfg)
    assert len(rec.filt) == n - 1
    for P in rec.pred:
        diag_exact(P)
    filt = np.array([np.array(cfg["ekf"]["initial_cov_diag"], float)] + [diag_exact(P) for P in rec.filt])
    smooth = filt.copy()
    segs = []
    for a, b, covs in rec.segs:
        assert len(covs) == b - a + 1 and 0 <= a < b < n
        smooth[a:b + 1] = [diag_exact(P) for P in covs]
        assert (smooth[b] == filt[b]).all()
        segs.append((a, b))
    thr = np.deg2rad(cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"])
    sharp = []
    for a, b, res in rec.decisions:                             # the margin of every decision, computed here
        yaw = Rotation.from_quat(quat[a:b]).as_euler("zyx")[:, 0]
        rate = 0.0
        for k in range(1, b - a):
            dt = ts[a + k] - ts[a + k - 1]
            if dt > 0:
                d = yaw[k] - yaw[k - 1]
                rate = max(rate, abs(np.arctan2(np.sin(d), np.cos(d)) / dt))
        assert not (0.9 * thr <= rate <= 1.1 * thr), f"outage [{a}, {b}): max yaw rate {rate} within 10 % of the threshold {thr}"
        assert (rate > thr) == res
        if res:
            sharp.append((a, b))
    assert not (set(sharp) & {(a, b) for a, b in segs})
    return filt, smooth, segs, sharp


def make_track(rng, n, outages=(), sharp=(), nan_rows=(), repeat=(), t0=100.0):
    """n poses turning gently about z (about 2 deg/s), GNSS masked off on [a, b) for every outage; `sharp`: outages whose poses
    turn at about 140 deg/s over three pairs (two pairs for a two-pose outage: its only pair)."""
    ts = t0 + np.cumsum(rng.uniform(0.08, 0.12, n))
    for k in repeat:
        ts[k] = ts[k - 1]
    rate = np.full(n, np.deg2rad(2.0))
    for a, b in sharp:
        rate[a + 1:min(b, a + 4)] = np.deg2rad(140.0)
    dts = np.diff(ts, prepend=ts[0])
    yaw = np.cumsum(rate * dts)
    quat = Rotation.from_euler("z", yaw).as_quat() * rng.choice([-1.0, 1.0], size=(n, 1)) * rng.uniform(0.98, 1.02, size=(n, 1))
    pos = np.cumsum(np.c_[np.cos(yaw), np.sin(yaw), 0.0 * yaw] * 0.8, axis=0)
    valid = np.ones(n, bool)
    for a, b in outages:
        valid[a:b] = False
    aligned = pos + rng.normal(0, 0.3, (n, 3))
    aligned[~valid] = np.nan
    for k, c in nan_rows:
        aligned[k, c] = np.nan                                  # NaN component, mask still set (:868)
    return ts, pos, quat, aligned, valid


def hand_tracks():
    rng = np.random.default_rng(20251017)
    T = []
    add = lambda name, cfg, *a, **k: T.append((name, cfg, make_track(rng, *a, **k)))
    add("clean", 0, 70)
    add("one_pose_valid", 0, 1)
    add("one_pose_outage", 0, 1, outages=[(0, 1)])
    add("two_poses_from_outage", 0, 2, outages=[(0, 1)])
    add("outage_from_pose0", 0, 80, outages=[(0, 5)])
    add("nan_fix_at_pose0_mask_set", 0, 66, nan_rows=[(0, 1)])
    add("outage_to_end", 0, 100, outages=[(90, 100)])
    add("gentle_across_two_boundaries", 0, 200, outages=[(40, 140)])
    add("sharp_across_two_boundaries", 0, 200, outages=[(40, 140)], sharp=[(40, 140)])
    add("recovery_at_lane0_and_lane63", 0, 150, outages=[(50, 64), (100, 127)])
    add("recovery_at_last_pose", 0, 130, outages=[(120, 129)])
    add("one_pose_outage_sharp_and_gentle_in_one_chunk", 0, 64, outages=[(5, 6), (10, 20), (30, 45)], sharp=[(10, 20)])
    add("sharp_outage_of_two_poses", 0, 40, outages=[(10, 12)], sharp=[(10, 12)])
    add("repeated_stamps", 0, 90, outages=[(20, 30)], repeat=[10, 24, 25, 50])
    add("nan_component_mask_set", 0, 70, outages=[(30, 33)], nan_rows=[(12, 0), (40, 2), (41, 1)])
    add("sharp_late_in_carried_outage", 0, 140, outages=[(30, 100)], sharp=[(80, 100)])
    add("axes_differ_gentle_and_sharp", 1, 150, outages=[(0, 4), (20, 40), (60, 75), (90, 91), (140, 150)], sharp=[(60, 75)], nan_rows=[(110, 2)])
    add("axes_differ_across_boundary", 1, 130, outages=[(60, 70)])
    add("axes_differ_sharp_steps5", 1, 66, outages=[(8, 12)], sharp=[(8, 12)])
    return T


def main():
    cfgs = [cfg_copy(), cfg_copy(rts_decision__default_ekf_transition_steps_on_sharp_turn=5)]
    cfgs[1]["ekf"]["initial_cov_diag"] = [0.1, 0.25, 0.05, 0.01, 0.02, 0.03, 0.04]
    cfgs[1]["ekf"]["process_noise_diag"] = [0.1, 0.3, 0.7, 0.01, 0.02, 0.005, 0.03]
    cfgs[1]["ekf"]["meas_noise_diag"] = [0.2, 0.05, 0.6]
    g = np.load(os.path.join(HERE, "ekf_random_tracks.npz"), allow_pickle=False)
    tracks = [(f"random{b}", 0, (g["ts"][b], g["pos"][b], g["quat"][b], g["aligned"][b], g["valid"][b])) for b in range(g["ts"].shape[0])]
    n_random = len(tracks)
    hand = hand_tracks()
    tracks += hand
    offsets, F, S, segs, sharp = [0], [], [], [], []
    for tr, (name, ci, (ts, pos, quat, aligned, valid)) in enumerate(tracks):
        filt, smooth, sg, sh = run_track(ts, pos, quat, aligned, valid, cfgs[ci])
        F.append(filt); S.append(smooth); offsets.append(offsets[-1] + len(ts))
        segs += [(tr, a, b) for a, b in sg]; sharp += [(tr, a, b) for a, b in sh]
    ho = np.cumsum([0] + [len(t[2][0]) for t in hand])
    cat = lambda k, shape: np.concatenate([np.asarray(t[2][k]).reshape(shape) for t in hand])
    keep = {sec: cfgs[0][sec] for sec in ("ekf", "rts_decision")}, {sec: cfgs[1][sec] for sec in ("ekf", "rts_decision")}
    save("ekf_cov_tracks.npz", n_random=np.array(n_random), offsets=np.array(offsets, np.int64), filt=np.concatenate(F), smooth=np.concatenate(S),
         segments=np.array(segs, np.int64).reshape(-1, 3), sharp=np.array(sharp, np.int64).reshape(-1, 3),
         cfg_index=np.array([t[1] for t in tracks], np.int64), cfgs=np.array([json.dumps(c) for c in keep]),
         hand_names=np.array([t[0] for t in hand]), hand_offsets=ho.astype(np.int64), hand_ts=cat(0, (-1,)), hand_quat=cat(2, (-1, 4)),
         hand_aligned=cat(3, (-1, 3)), hand_valid=cat(4, (-1,)).astype(bool))
    print(f"{len(tracks)} tracks, {offsets[-1]} poses, {len(segs)} smoothed segments, {len(sharp)} sharp-turn outages")


if __name__ == "__main__":
    main()
