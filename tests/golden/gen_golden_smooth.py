#!/usr/bin/env python3
"""Generate tests/golden/ekf_smooth_tracks.npz: the fixed-interval RTS smoother over whole fused tracks, computed by the REFERENCE's own code.

Runs only where the reference is present (see gen_golden.py, whose import helpers are used).  The reference's apply_ekf_correction runs on
every track with recorders around ExtendedKalmanFilter.process_step (ALL FOUR returns of every pose: filtered and predicted state and
covariance) and is_sharp_turn_in_segment (its decision per outage, as gen_golden_cov.py records it).  Every recovery judged a sharp turn
starts a new span; each span [s..e] is then handed, as the lists the reference itself keeps (ekf_states_filt_hist, ekf_covs_filt_hist,
ekf_states_pred_hist, ekf_covs_pred_hist), to the reference's own rts_smoother_segment -- the call apply_ekf_correction never makes.
The wrappers are this file's own code; nothing of the reference is copied, and only data is stored:

  tracks    file order: the 64 inputs of ekf_random_tracks.npz (NOT stored again; initial pose sp0 / sq0 of that file), the hand-made tracks
            of gen_golden_cov.py (ts / quat / aligned / valid are in ekf_cov_tracks.npz; their positions are stored HERE as hand_pos; initial
            pose = pose 0), then the tracks made below (stored whole: new_offsets, new_ts, new_pos, new_quat, new_aligned, new_valid, new_names;
            initial pose = pose 0)
  offsets   (T+1,) rows of every track in the flat per-pose arrays
  filt_pos  (P,3)  the filter's position (process_step's first return; row 0 = the initial position)
  smooth_pos (P,3) the smoothed position
  smooth_var (P,3) the smoothed position variances (the diagonal's first three entries)
  span_starts (K,2) track, first row of every span (row 0 of every non-empty track included)
  cfg_index (T,) / cfgs: JSON configs (0 = the reference's CONFIG, 1 = gen_golden_cov.py's three distinct axes, 2 = a zero-variance z axis)

Asserted here: every off-diagonal element of every filtered, predicted and smoothed covariance is exactly 0.0; the smoothed variances of
axes 3-6 equal the filtered ones; the smoothed quaternion is the filter's within 1e-15; the largest yaw rate of every judged outage lies
outside 0.9 .. 1.1 x the threshold.

    python tests/golden/gen_golden_smooth.py
"""
import json
import os

import numpy as np
from scipy.spatial.transform import Rotation

from gen_golden import HERE, cfg_copy, quiet, ref, save, AlignRecorder
from gen_golden_cov import diag_exact, hand_tracks, make_track


class StepRecorder:
    """Records the four returns of every process_step and every is_sharp_turn_in_segment decision, in call order."""

    def __init__(self):
        self.steps, self.decisions = [], []

    def __enter__(self):
        self._ps, self._sharp = ref.ExtendedKalmanFilter.process_step, ref.is_sharp_turn_in_segment
        rec = self

        def process_step(ekf, *a, **k):
            r = rec._ps(ekf, *a, **k)
            rec.steps.append(tuple(np.array(x, dtype=float) for x in r))
            return r

        def sharp(quats, stamps, thr):
            res = rec._sharp(quats, stamps, thr)
            b = len(rec.steps) + 1                              # asked before the recovery pose's process_step
            rec.decisions.append((b - len(quats), b, bool(res)))
            return res

        ref.ExtendedKalmanFilter.process_step, ref.is_sharp_turn_in_segment = process_step, sharp
        return self

    def __exit__(self, *a):
        ref.ExtendedKalmanFilter.process_step, ref.is_sharp_turn_in_segment = self._ps, self._sharp


def run_track(ts, pos, quat, aligned, valid, ip, iq, cfg):
    n = len(ts)
    if n == 0:
        z = np.empty((0, 3))
        return z, z, z, []
    slam = {"timestamps": ts, "positions": pos, "quaternions": quat}
    sp, sq = pos.copy(), quat.copy()
    sp[0], sq[0] = ip, iq
    with quiet(), AlignRecorder(inject=(aligned, valid)), StepRecorder() as rec:
        ref.apply_ekf_correction(slam, {"timestamps": ts, "positions": aligned}, sp, sq, cfg)
    assert len(rec.steps) == n - 1
    x0 = np.concatenate([ip, ref.ExtendedKalmanFilter.normalize_quaternion(np.asarray(iq, float))])
    P0 = np.diag(cfg["ekf"]["initial_cov_diag"]).astype(float)
    sf, cf = [x0] + [s[0] for s in rec.steps], [P0] + [s[1] for s in rec.steps]       # what apply_ekf_correction keeps (:852-853, :902-903)
    sp_, cp = [x0] + [s[2] for s in rec.steps], [P0] + [s[3] for s in rec.steps]
    for P in cf + cp:
        diag_exact(P)
    thr = np.deg2rad(cfg["rts_decision"]["sharp_turn_yaw_rate_threshold_deg_per_sec"])
    starts = [0]
    for a, b, res in rec.decisions:                              # the margin of every decision (as gen_golden_cov.py)
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
            starts.append(b)
    xs, Ps = np.empty((n, 7)), np.empty((n, 7))
    for s, e in zip(starts, starts[1:] + [n]):                   # span [s .. e-1]: the reference's own smoother on the reference's own lists
        with quiet():
            ss, cs = ref.rts_smoother_segment(sf[s:e], cf[s:e], sp_[s:e], cp[s:e])
        xs[s:e] = ss
        Ps[s:e] = [diag_exact(P) for P in cs]
    F, Cf = np.array(sf), np.array([np.diag(P) for P in cf])
    assert (Ps[:, 3:] == Cf[:, 3:]).all(), "a quaternion axis was smoothed"
    assert np.abs(xs[:, 3:] - F[:, 3:]).max() <= 1e-15
    return F[:, :3], xs[:, :3], Ps[:, :3], starts


def new_tracks():
    rng = np.random.default_rng(20261020)
    T = []
    add = lambda name, cfg, *a, **k: T.append((name, cfg, make_track(rng, *a, **k)))
    add("zero_variance_z", 2, 90, outages=[(20, 30), (50, 58)], sharp=[(50, 58)])
    # spans that start at lane 63 of chunk 0, lane 0 of chunk 2, lane 63 of chunk 2 and row 256 (lane 0 = pose 64 x 4), a gentle outage between
    add("span_starts_at_lanes_0_63_64", 0, 330, outages=[(55, 63), (90, 100), (120, 128), (185, 191), (250, 256)],
        sharp=[(55, 63), (120, 128), (185, 191), (250, 256)])
    add("last_update_three_chunks_before_the_end", 0, 300, outages=[(30, 40), (100, 300)])
    add("span_start_then_outage_to_the_end", 1, 200, outages=[(60, 70), (130, 200)], sharp=[(60, 70)])
    ts, pos, quat, aligned, valid = make_track(rng, 140, outages=[(20, 30), (100, 104)], sharp=[(100, 104)])
    shift = np.array([4.6e5, 5.4e6, 120.0])
    pos[70:] += shift; aligned[70:] += shift                      # half of the track at UTM size
    T.append(("half_shifted_to_utm_size", 0, (ts, pos, quat, aligned, valid)))
    return T


def main():
    cfgs = [cfg_copy(), cfg_copy(rts_decision__default_ekf_transition_steps_on_sharp_turn=5), cfg_copy()]
    cfgs[1]["ekf"]["initial_cov_diag"] = [0.1, 0.25, 0.05, 0.01, 0.02, 0.03, 0.04]
    cfgs[1]["ekf"]["process_noise_diag"] = [0.1, 0.3, 0.7, 0.01, 0.02, 0.005, 0.03]
    cfgs[1]["ekf"]["meas_noise_diag"] = [0.2, 0.05, 0.6]
    cfgs[2]["ekf"]["initial_cov_diag"] = list(cfgs[2]["ekf"]["initial_cov_diag"]); cfgs[2]["ekf"]["initial_cov_diag"][2] = 0.0
    cfgs[2]["ekf"]["process_noise_diag"] = list(cfgs[2]["ekf"]["process_noise_diag"]); cfgs[2]["ekf"]["process_noise_diag"][2] = 0.0
    g = np.load(os.path.join(HERE, "ekf_random_tracks.npz"), allow_pickle=False)
    c = np.load(os.path.join(HERE, "ekf_cov_tracks.npz"), allow_pickle=False)
    tracks = [(f"random{b}", 0, (g["ts"][b], g["pos"][b], g["quat"][b], g["aligned"][b], g["valid"][b]), g["sp0"][b], g["sq0"][b])
              for b in range(g["ts"].shape[0])]
    hand = hand_tracks()
    assert [t[0] for t in hand] == [str(s) for s in c["hand_names"]]
    assert (np.concatenate([t[2][0] for t in hand]) == c["hand_ts"]).all()        # the same hand-made tracks as ekf_cov_tracks.npz holds
    new = new_tracks()
    tracks += [(name, ci, tr, tr[1][0].copy(), tr[2][0].copy()) for name, ci, tr in hand + new if len(tr[0])]
    assert len(tracks) == 64 + len(hand) + len(new)
    offsets, F, S, V, starts = [0], [], [], [], []
    for tr, (name, ci, (ts, pos, quat, aligned, valid), ip, iq) in enumerate(tracks):
        f, s, v, st = run_track(ts, pos, quat, aligned, valid, ip, iq, cfgs[ci])
        F.append(f); S.append(s); V.append(v); offsets.append(offsets[-1] + len(ts))
        starts += [(tr, a) for a in st]
    no = np.cumsum([0] + [len(t[2][0]) for t in new])
    cat = lambda T, k, shape: np.concatenate([np.asarray(t[2][k]).reshape(shape) for t in T])
    keep = [{sec: cf[sec] for sec in ("ekf", "rts_decision")} for cf in cfgs]
    save("ekf_smooth_tracks.npz", n_random=np.array(64), n_hand=np.array(len(hand)), offsets=np.array(offsets, np.int64),
         filt_pos=np.concatenate(F), smooth_pos=np.concatenate(S), smooth_var=np.concatenate(V),
         span_starts=np.array(starts, np.int64).reshape(-1, 2), cfg_index=np.array([t[1] for t in tracks], np.int64),
         cfgs=np.array([json.dumps(cf) for cf in keep]), hand_pos=cat(hand, 1, (-1, 3)),
         new_names=np.array([t[0] for t in new]), new_offsets=no.astype(np.int64), new_ts=cat(new, 0, (-1,)), new_pos=cat(new, 1, (-1, 3)),
         new_quat=cat(new, 2, (-1, 4)), new_aligned=cat(new, 3, (-1, 3)), new_valid=cat(new, 4, (-1,)).astype(bool))
    n_sharp = len(starts) - len(tracks)
    print(f"{len(tracks)} tracks, {offsets[-1]} poses, {len(starts)} spans ({n_sharp} start at a sharp-turn recovery)")


if __name__ == "__main__":
    main()
