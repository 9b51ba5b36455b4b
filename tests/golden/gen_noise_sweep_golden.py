#!/usr/bin/env python3
"""Generate tests/golden/noise_sweep_tracks.npz: the innovations of the REFERENCE's own filter for several noise settings per track.

Runs only where the reference is present (see gen_golden.py, whose import helpers are used).  The reference's apply_ekf_correction runs
once per case and per candidate with a recorder wrapped around ExtendedKalmanFilter.process_step; the recorder calls the original and
keeps, per call, the measurement it was handed, the predicted position pred_state[:3], diag(pred_cov)[:3] and whether an update was
applied.  The wrapper is this file's own code; nothing of the reference is copied, and only data is stored:

  names      (T,)   case names; the first two are the bundled runs (yolotum04.txt with each bundled GNSS file), whose inputs are NOT stored
                    again: ts / pos / quat are kat_bundled.npz's, aligned / valid / the initial pose c1_<tag>.npz's (bundled_tags)
  offsets    (T+1,) rows of every case in the flat per-pose arrays
  cfg_index  (T,) / cfgs: index into the JSON configs (0 = the reference's CONFIG, 1 = 5 transition steps on a sharp turn)
  cand       (3,9)  the candidates {P0, Q, R} x 3 axes every case is run with: the default, three distinct axes, P0 and Q x 16 with R / 16
  hand_*            inputs of the synthetic cases (ts, pos, quat, aligned, valid), flat over hand_offsets
  meas       (P,3)  the measurement handed to process_step (NaN where none), the same for every candidate
  upd        (P,)   an update was applied (never at pose 0)
  pred_pos   (3,P,3) / pred_var (3,P,3): predicted position and its variance per candidate (NaN at pose 0: no step)

    python tests/golden/gen_noise_sweep_golden.py
"""
import copy
import json
import os

import numpy as np

from gen_golden import HERE, cfg_copy, quiet, ref, save, AlignRecorder
from gen_golden_cov import make_track


class StepRecorder:
    def __init__(self):
        self.meas, self.pred, self.var, self.upd = [], [], [], []

    def __enter__(self):
        self._ps = ref.ExtendedKalmanFilter.process_step
        rec = self

        def process_step(ekf, motion, gps_measurement, gnss_is_available, delta_time, override_transition_steps=None):
            r = rec._ps(ekf, motion, gps_measurement, gnss_is_available, delta_time, override_transition_steps=override_transition_steps)
            z = np.full(3, np.nan) if gps_measurement is None else np.array(gps_measurement, float)
            rec.meas.append(z); rec.pred.append(np.array(r[2][:3], float)); rec.var.append(np.diag(np.array(r[3]))[:3].copy())
            rec.upd.append(bool(gnss_is_available) and gps_measurement is not None and not np.isnan(z).any())
            return r
        ref.ExtendedKalmanFilter.process_step = process_step
        return self

    def __exit__(self, *a):
        ref.ExtendedKalmanFilter.process_step = self._ps


def with_candidate(cfg, c):
    g = copy.deepcopy(cfg)
    for name, lo in (("initial_cov_diag", 0), ("process_noise_diag", 3), ("meas_noise_diag", 6)):
        v = [float(x) for x in g["ekf"][name]]
        v[0:3] = [float(x) for x in c[lo:lo + 3]]
        g["ekf"][name] = v
    return g


def run_case(ts, pos, quat, aligned, valid, sim3_pos, sim3_quat, cfg, cand):
    n = len(ts)
    slam = {"timestamps": ts, "positions": pos, "quaternions": quat}
    meas = upd = None
    P, V = [], []
    for c in cand:
        with quiet(), AlignRecorder(inject=(aligned, valid)), StepRecorder() as rec:
            ref.apply_ekf_correction(slam, {"timestamps": ts, "positions": aligned}, sim3_pos, sim3_quat, with_candidate(cfg, c))
        assert len(rec.meas) == max(n - 1, 0)
        nan = np.full((1, 3), np.nan)
        m = np.concatenate([nan] + [x[None] for x in rec.meas]) if n else np.empty((0, 3))
        u = np.array([False] + rec.upd, bool) if n else np.empty(0, bool)
        if meas is None:
            meas, upd = m, u
        assert np.array_equal(m, meas, equal_nan=True) and np.array_equal(u, upd)
        P.append(np.concatenate([nan] + [x[None] for x in rec.pred])); V.append(np.concatenate([nan] + [x[None] for x in rec.var]))
    return meas, upd, np.array(P), np.array(V)


def hand_cases():
    rng = np.random.default_rng(20261019)
    T = []
    add = lambda name, cfg, *a, **k: T.append((name, cfg, make_track(rng, *a, **k)))
    for n in (1, 2, 3, 63, 64, 65, 129):
        add(f"clean_{n}", 0, n)
    add("straight_outage_rts", 0, 90, outages=[(30, 42)])
    sharp = make_track(rng, 100, outages=[(40, 52)], sharp=[(40, 52)])
    T.append(("sharp_outage_steps0", 0, sharp))
    T.append(("sharp_outage_steps5_blend", 1, sharp))
    add("outage_from_pose0", 0, 70, outages=[(0, 6)])
    add("outage_at_the_end", 0, 80, outages=[(71, 80)])
    add("mask_set_on_nan_fix", 0, 70, nan_rows=[(0, 1), (12, 0), (40, 2), (41, 1)])
    add("repeated_stamps", 1, 90, outages=[(20, 30)], repeat=[10, 24, 25, 50])
    add("outage_of_one_pose", 1, 66, outages=[(5, 6), (64, 65)])
    return T


def main():
    cfgs = [cfg_copy(), cfg_copy(rts_decision__default_ekf_transition_steps_on_sharp_turn=5)]
    e = cfgs[0]["ekf"]
    d = np.array([float(x) for x in e["initial_cov_diag"][:3]] + [float(x) for x in e["process_noise_diag"][:3]]
                 + [float(x) for x in e["meas_noise_diag"][:3]])
    cand = np.array([d, [0.1, 0.25, 0.05, 0.1, 0.3, 0.7, 0.2, 0.05, 0.6], np.r_[d[0:3] * 16.0, d[3:6] * 16.0, d[6:9] / 16.0]])
    kat = np.load(os.path.join(HERE, "kat_bundled.npz"), allow_pickle=False)
    tags = ["kitti04gps", "combined"]
    cases = []
    for tag in tags:
        c1 = np.load(os.path.join(HERE, f"c1_{tag}.npz"), allow_pickle=False)
        cases.append((f"bundled_{tag}", 0, (kat["ts"], kat["pos"], kat["quat"], c1["ekf_aligned"], c1["ekf_valid"]), c1["sim3_pos"], c1["sim3_quat"]))
    hand = hand_cases()
    cases += [(name, ci, tr, tr[1].copy(), tr[2].copy()) for name, ci, tr in hand]
    offsets, M, U, PP, PV = [0], [], [], [], []
    for name, ci, (ts, pos, quat, aligned, valid), sp, sq in cases:
        m, u, pp, pv = run_case(ts, pos, quat, aligned, valid, sp, sq, cfgs[ci], cand)
        M.append(m); U.append(u); PP.append(pp); PV.append(pv); offsets.append(offsets[-1] + len(ts))
    ho = np.cumsum([0] + [len(t[2][0]) for t in hand])
    cat = lambda k, shape: np.concatenate([np.asarray(t[2][k]).reshape(shape) for t in hand])
    keep = [{sec: c[sec] for sec in ("ekf", "rts_decision")} for c in cfgs]
    save("noise_sweep_tracks.npz", names=np.array([c[0] for c in cases]), bundled_tags=np.array(tags), offsets=np.array(offsets, np.int64),
         cfg_index=np.array([c[1] for c in cases], np.int64), cfgs=np.array([json.dumps(c) for c in keep]), cand=cand,
         hand_offsets=ho.astype(np.int64), hand_ts=cat(0, (-1,)), hand_pos=cat(1, (-1, 3)), hand_quat=cat(2, (-1, 4)),
         hand_aligned=cat(3, (-1, 3)), hand_valid=cat(4, (-1,)).astype(bool),
         meas=np.concatenate(M), upd=np.concatenate(U), pred_pos=np.concatenate(PP, axis=1), pred_var=np.concatenate(PV, axis=1))
    print(f"{len(cases)} cases, {offsets[-1]} poses, {int(np.concatenate(U).sum())} updates per candidate")


if __name__ == "__main__":
    main()
