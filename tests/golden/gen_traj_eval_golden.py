#!/usr/bin/env python3
"""Generate tests/golden/traj_eval_kitti04.npz: the KITTI 04 ground truth and the SLAM estimate of the same 271 frames that the reference
ships, with the yardstick's KITTI segment errors of the estimate.

Runs only where the reference's data files are present; their folder is the first argument (or the environment variable GSF_REFERENCE).
Only data is stored:

  truth_ts (271,) / truth_pos (271,3) / truth_quat (271,4)   04.txt (rows of 3x4 matrices) and times04.txt; the quaternions [x, y, z, w] are
                                                             scipy's Rotation.from_matrix of each row's rotation, w >= 0
  truth_rows (271,12)                                        04.txt as it stands (what batch.read_kitti_poses is checked against)
  est_ts / est_pos / est_quat                                yolotum04.txt (TUM rows: stamp, position, quaternion)
  path_length                                                the truth path in metres
  lengths (8,) / stride                                      KITTI's segments: 100 ... 800 m, a first frame every 10 poses
  n_pairs (8,)                                               pairs per length (tests/traj_eval_ref.py, no alignment, nearest stamps within 0.01 s)
  pair_k / pair_f / pair_l                                   every pair: its length's number, first and last frame
  pair_et / pair_er / pair_bt / pair_br                      its errors in 50 digits rounded once, and their bounds
  t_rel / r_rel                                              100 sum(et / len) / n in percent, sum(er / len) / n in rad/m

    python tests/golden/gen_traj_eval_golden.py <folder of the reference>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import traj_eval_ref as ref                                              # noqa: E402

MAX_DIFF = 0.01


def main():
    from scipy.spatial.transform import Rotation
    folder = sys.argv[1] if len(sys.argv) > 1 else os.environ["GSF_REFERENCE"]
    rows = np.loadtxt(os.path.join(folder, "04.txt"))
    times = np.loadtxt(os.path.join(folder, "times04.txt"))
    est = np.loadtxt(os.path.join(folder, "yolotum04.txt"))
    assert rows.shape == (271, 12) and times.shape == (271,) and est.shape == (271, 8)
    q = Rotation.from_matrix(rows.reshape(-1, 3, 4)[:, :, :3]).as_quat()
    q[q[:, 3] < 0] *= -1.0
    truth = (times, np.ascontiguousarray(rows[:, [3, 7, 11]]), np.ascontiguousarray(q))
    lengths = np.array([100.0 * k for k in range(1, 9)])
    scen = tuple((ref.METRES, float(v), 10) for v in lengths)
    w = ref.evaluate_track(est[:, 0].copy(), np.ascontiguousarray(est[:, 1:4]), np.ascontiguousarray(est[:, 4:8]), *truth, False, ref.NEAREST,
                           ref.ALIGN_NONE, MAX_DIFF, scen, tuple(range(8)))
    assert w.state == 0 and w.M == 271
    k_, f_, l_, et, er, bt, br = [], [], [], [], [], [], []
    for k in range(8):
        for j, (f, l) in enumerate(w.pairs[k]):
            k_.append(k); f_.append(f); l_.append(l)
            et.append(w.rpe_t[k][j]); er.append(w.rpe_r[k][j]); bt.append(w.b_rpe_t[k][j]); br.append(w.b_rpe_r[k][j])
    k_ = np.array(k_, np.int32)
    n = len(k_)
    t_rel = 100.0 * float(np.sum(np.array(et, np.longdouble) / lengths[k_])) / n
    r_rel = float(np.sum(np.array(er, np.longdouble) / lengths[k_])) / n
    out = os.path.join(HERE, "traj_eval_kitti04.npz")
    np.savez_compressed(out, truth_ts=truth[0], truth_pos=truth[1], truth_quat=truth[2], truth_rows=rows, est_ts=est[:, 0], est_pos=est[:, 1:4],
                        est_quat=est[:, 4:8], path_length=float(w.d[-1]), lengths=lengths, stride=10, n_pairs=np.array([len(p) for p in w.pairs]),
                        pair_k=k_, pair_f=np.array(f_, np.int32), pair_l=np.array(l_, np.int32), pair_et=np.array(et), pair_er=np.array(er),
                        pair_bt=np.array(bt), pair_br=np.array(br), t_rel=t_rel, r_rel=r_rel)
    print(f"{out}: path {float(w.d[-1]):.1f} m, pairs {[len(p) for p in w.pairs]}, t_rel {t_rel:.4f} %, r_rel {r_rel:.3e} rad/m, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
