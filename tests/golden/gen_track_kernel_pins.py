"""Writes tests/golden/track_kernel_pins.npz: every output array of the five entries whose kernels run the filter "one wave per track, 64
poses per chunk" -- gsf_ekf_smooth_ragged_dev, gsf_ekf_smooth_weighted_dev, gsf_ekf_noise_sweep_dev, gsf_innovation_gate_dev and
gsf_outage_study_dev -- as the library of ONE commit computes them.  tests/test_track_kernel_pins.py builds the same inputs with the
functions below and asks the library under test for the same words.

usage (on the GPU, with the library of the commit to pin built in the tree or named by GSF_LIBRARY):
    python tests/golden/gen_track_kernel_pins.py --commit <hash of the commit the library was built from>

One ragged batch of ten tracks (LENGTHS), the smallest shapes at which every branch of the shared chunk body is taken:
  0, 1, 2   an empty track, a track of pose 0 alone, one step (valid[0] = 0 on the track of two)
  63        valid[0] = 0, a valid row whose fix holds a NaN
  64        ends in an outage (rows 55 .. 63)
  65        an outage over rows 58 .. 63 that recovers at row 64, the first row of the next chunk, no pair over the yaw threshold: rows of
            the earlier chunk are NOT re-flagged; two equal stamps (the 1e-6 clamp)
  129       a zero quaternion at row 5 and a NaN one at row 64: the scanned orientation route, the return to the telescoped one, and the
            carry across a chunk boundary; a row whose three variances are +inf; ends in an outage
  200       an outage over rows 50 .. 69 (recovery in the next chunk) with a 30 degree step of yaw between rows 60 and 61: a sharp-turn
            recovery that re-flags rows of the earlier chunk; an outage over rows 120 .. 134 without one; a NaN fix; three equal stamps;
            a row with an unusable variance
  70        run_status = 1: NaN rows, inputs not read
  66        a NaN in init_quat (the normalisation returns the identity) and a zero quaternion at row 3, so that the first chunk takes the
            scanned orientation route with pose 0 on a lane that does not step; the second chunk telescopes
The smoother and the outage study run under four noise configs (all axes shared / x = y != z, the default / y = z != x / three different
axes; the last three with a four-step blend at a sharp-turn recovery)."""
import argparse
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]
PATH = os.path.join(HERE, "track_kernel_pins.npz")

LENGTHS = [0, 1, 2, 63, 64, 65, 129, 200, 70, 66]
STOPPED = 8                                                                 # the track with run_status != 0
UTM = np.array([4.5e5, 5.4e6, 110.0])
CONFIGS = ("shared", "default", "yz", "three")
GATES = [float("inf"), 3.0, 0.5]
SCENARIOS = [[2.0, 1.5], [5.5, 2.0], [11.0, 3.0]]                           # rows 20 .. 34 / 55 .. 74 (crosses row 64) / 110 .. 139 (crosses row 128)


def _quat(yaw, roll, pitch):
    cy, sy, cr, sr, cp, sp = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=1)


def inputs():
    """name -> host array: ts, pos, quat, gps, valid, offsets, init_pos, init_quat, run_status, meas_scale (P,3), and the rows with planted variances"""
    rng = np.random.default_rng(20261021)
    ts, pos, quat, gps, valid, ip, iq = [], [], [], [], [], [], []
    for b, n in enumerate(LENGTHS):
        k = np.arange(n, dtype=np.float64)
        t = 1.7e9 + 100.0 * b + 0.1 * k
        yaw = 0.3 * b + np.deg2rad(5.0) * 0.1 * k
        if n == 200:
            yaw[61:] += np.deg2rad(30.0)                                    # 300 deg/s between rows 60 and 61
            t[150:153] = t[150]
        if n == 65:
            t[31] = t[30]
        q = _quat(yaw, 0.02 * np.sin(0.05 * k), 0.03 * np.cos(0.07 * k))
        step = np.stack([np.cos(yaw), np.sin(yaw), 0.02 * np.sin(0.1 * k)], axis=1) * 0.8
        w = np.cumsum(step, axis=0) - step[:1] if n else np.zeros((0, 3))
        a0 = 0.4 + 0.1 * b                                                  # the SLAM frame: the world frame turned about z, scaled positions
        Rz = np.array([[np.cos(a0), -np.sin(a0), 0.0], [np.sin(a0), np.cos(a0), 0.0], [0.0, 0.0, 1.0]])
        p = w @ Rz + rng.normal(0.0, 0.01, (n, 3))
        z = UTM + np.array([37.0 * b, -11.0 * b, 0.5 * b]) + w + rng.normal(0.0, 0.3, (n, 3))
        v = np.ones(n, np.uint8)
        if n == 2:
            v[0] = 0
        if n == 63:
            v[0] = 0; z[10, 1] = np.nan
        if n == 64:
            v[55:] = 0
        if n == 65:
            v[58:64] = 0
        if n == 129:
            q[5] = 0.0; q[64] = [np.nan, 0.0, np.inf, 1.0]; v[120:] = 0
        if n == 200:
            v[50:70] = 0; v[120:135] = 0; z[20, 2] = np.nan
        if n == 66:
            q[3] = 0.0
        ts.append(t); pos.append(p); quat.append(q); gps.append(z); valid.append(v)
        ip.append(z[0] if n else UTM); iq.append(_quat(np.array([a0 + 0.3 * b]), np.array([0.01]), np.array([-0.02]))[0] * 1.5)   # (not normalised)
    iq[9][1] = np.nan
    offsets = np.zeros(len(LENGTHS) + 1, np.int64); offsets[1:] = np.cumsum(LENGTHS)
    P = int(offsets[-1])
    run_status = np.zeros(len(LENGTHS), np.int32); run_status[STOPPED] = 1
    scale = rng.uniform(0.5, 2.0, (P, 3))
    return dict(ts=np.concatenate(ts), pos=np.concatenate(pos), quat=np.concatenate(quat), gps=np.concatenate(gps), valid=np.concatenate(valid),
                offsets=offsets, init_pos=np.array(ip), init_quat=np.array(iq), run_status=run_status, meas_scale=scale,
                row_bad_var=np.array(int(offsets[7]) + 90), row_inf_var=np.array(int(offsets[6]) + 30))


def config(name):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = copy.deepcopy(E.CONFIG)
    e = cfg["ekf"]
    if name == "shared":
        e["process_noise_diag"][:3] = [0.1, 0.1, 0.1]
    elif name == "yz":
        e["initial_cov_diag"][:3] = [0.3, 0.1, 0.1]; e["process_noise_diag"][:3] = [0.1, 0.7, 0.7]; e["meas_noise_diag"] = [0.2, 0.5, 0.5]
    elif name == "three":
        e["initial_cov_diag"][:3] = [0.3, 0.1, 0.2]; e["process_noise_diag"][:3] = [0.1, 0.7, 0.05]; e["meas_noise_diag"] = [0.2, 0.5, 1.0]
    else:
        assert name == "default"
    if name != "default":
        cfg["rts_decision"]["default_ekf_transition_steps_on_sharp_turn"] = 4
    return cfg


def candidates():
    """K = 5 rows [P0 Q R] x 3 axes: all axes shared, x = y, y = z, three different, shared again at another scale"""
    return np.array([[0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.2, 0.2, 0.2],
                     [0.1, 0.1, 0.1, 0.1, 0.1, 0.7, 0.2, 0.2, 0.2],
                     [0.3, 0.1, 0.1, 0.1, 0.7, 0.7, 0.2, 0.5, 0.5],
                     [0.3, 0.1, 0.2, 0.1, 0.7, 0.05, 0.2, 0.5, 1.0],
                     [1.0, 1.0, 1.0, 0.02, 0.02, 0.02, 2.0, 2.0, 2.0]])


def _put(out, tag, r, names):
    for k in names:
        v = getattr(r, k, None)
        assert v is not None, (tag, k)
        out[f"{tag}/{k}"] = v.cpu().numpy()


def run_all(B):
    """name -> host array: every output array of the five entries, on the library that is loaded"""
    import torch
    h = inputs()
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    a8 = [d(h[k]) for k in ("ts", "pos", "quat", "gps", "valid", "offsets", "init_pos", "init_quat")]
    rs = d(h["run_status"])
    out = {}
    track = ("pos", "quat", "cov", "flags", "status")
    filt = ("pos_filt", "cov_filt")
    for name in CONFIGS:
        cfg = config(name)
        wf = name == "default"
        _put(out, f"smooth_{name}", B.ekf_smooth_ragged(*a8, config=cfg, run_status=rs, want_filtered=wf), track + (filt if wf else ()))
        _put(out, f"outage_{name}", B.outage_study_ragged(*a8, SCENARIOS, config=cfg, run_status=rs, trace=1),
             ("stats", "seg", "flags", "err_dr", "err_fused", "trace_pos"))
    # the weighted smoother: the config's R on every row; varied per row with one unusable variance and one row of three +inf
    for name, varied in (("default", False), ("default", True), ("three", True)):
        cfg = config(name)
        mv = np.tile(np.asarray(cfg["ekf"]["meas_noise_diag"], np.float64), (len(h["ts"]), 1))
        if varied:
            mv = mv * h["meas_scale"]
            mv[int(h["row_bad_var"]), 1] = 1e-9
            mv[int(h["row_inf_var"])] = np.inf
        wf = name == "default" and varied
        r = B.ekf_smooth_weighted_ragged(*a8[:5], d(mv), *a8[5:], config=cfg, run_status=rs, want_filtered=wf, want_nis=True)
        _put(out, f"weighted_{name}_{'rows' if varied else 'R'}", r, track + ("nis",) + (filt if wf else ()))
    ctx = B.context()
    try:
        for group, trace, skip in ((4, 1, 0.0), (2, 4, 1.0)):               # groups of {4, 1} and of {2, 2, 1} candidates
            ctx.set_option("noise_sweep_group", group)
            r = B.ekf_noise_sweep_ragged(*a8, candidates(), config=config("three"), run_status=rs, skip_seconds=skip, min_updates=2, trace=trace)
            _put(out, f"sweep_g{group}", r, ("stats", "best_k", "pooled", "pooled_best", "status", "innov", "innov_var"))
    finally:
        ctx.set_option("noise_sweep_group", 0)
    r = B.innovation_gate_ragged(*a8, GATES, config=config("default"), run_status=rs, arm_seconds=1.0, max_run=3, want_nis=True)
    _put(out, "gate", r, ("valid_out", "stats", "status", "nis_out"))
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    from gps_optimize_slam_amd import batch
    arrays = run_all(batch)
    print("smooth status", arrays["smooth_default/status"].tolist())
    print("gate stats[:, :, 2]", arrays["gate/stats"][:, :, 2].tolist())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, commit=np.array(a.commit), **arrays)
    print(f"wrote {a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")
