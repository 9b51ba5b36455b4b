"""Writes tests/golden/run_chain_pinned.npz: every output array and the final generator states of one dense and two ragged whole-run
calls (gsf_run_fusion_batch_dev / gsf_run_fusion_ragged_dev), as the library of ONE commit computes them.  tests/test_run_chain_pinned.py
builds the same inputs with the functions below and asks the library under test for the same words.

usage (on the GPU, with the library of the commit to pin built in the tree or named by GSF_LIBRARY):
    python tests/golden/gen_run_chain_pinned.py --commit <hash of the commit the library was built from>

The shapes are the smallest at which every branch of the chain is taken:
  dense   16 tracks x 130 poses (three 64-pose chunks, the last one two poses), logs of test_buffer_hygiene.dense_run_batch: fixes 60 m off,
          rows the loader drops, a log of three fixes, of one fix, with nothing in range, an empty one;
  ragged  nine tracks of 0, 1, 5, 64, 65 and 200 poses (RAGGED_LENGTHS), called once with ground-truth logs (their filter enabled) and once
          without: ground truth present / absent (an empty range) / thinned below two fixes by its filter (GT_FEW), a primary log of one fix
          and one with nothing in range next to a ground truth (the runs stop there: the ground-truth leg is gated off), an empty SLAM track."""
import argparse
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]
PATH = os.path.join(HERE, "run_chain_pinned.npz")

RAGGED_LENGTHS = [0, 1, 5, 64, 65, 200, 65, 64, 5]
FIELDS = ("R", "t", "s", "n_inliers", "zone", "south", "gps_utm", "gps_keep", "aligned", "valid", "sim3_pos", "gt_zone", "gt_south", "gt_utm", "gt_keep",
          "gt_aligned", "gt_valid", "err_stats", "plot_ref", "run_status", "inlier_mask", "trial_info")


def ragged_inputs(orc):
    """(tracks, logs, ground-truth logs) of RAGGED_LENGTHS, made like test_run_ragged._make_batch's"""
    from test_run_ragged import _log, _synthetic_case
    rng = np.random.default_rng(33)
    tracks, logs, gts = [], [], []
    for b, n in enumerate(RAGGED_LENGTHS):
        tt, pp, qq, uu = _synthetic_case(orc, max(n, 50), b)                # (the logs of the shortest tracks run on past them)
        log = _log(orc, tt, uu, rng, 0.3, 0.03)
        m = len(log)
        if b in (3, 5):                                                     # fixes thrown 60 m off
            for r_ in rng.choice(m, size=3, replace=False):
                log[r_, 1] += 60.0 / 111200.0 * rng.choice([-1, 1]); log[r_, 2] += 60.0 / 73000.0 * rng.choice([-1, 1])
        if b == 4:                                                          # rows the loader removes
            rr = rng.choice(m, size=4, replace=False)
            log[rr[0], 1] = 0.0; log[rr[1], 2] = 0.0; log[rr[2], 1] = 91.0; log[rr[3], 2] = -181.0
        gt = _log(orc, tt[::2], uu[::2], rng, 0.15, 0.05)                   # an independent, sparser log
        if b == 4: gt = None                                                # no ground truth: an empty range
        if b == 6: log = log[[m // 2]]                                      # the primary log stops the run (one fix): ground-truth leg gated off
        if b == 7:                                                          # GT_FEW under the enabled filter: 7 fixes scattered by 300 m
            gt = gt[:7].copy(); gt[:, 1] += rng.uniform(-1, 1, 7) * 300.0 / 111200.0; gt[:, 2] += rng.uniform(-1, 1, 7) * 300.0 / 73000.0
            gt[:, 3] += rng.uniform(-300, 300, 7); gt[:, 0] = tt[0] + np.arange(7) * 1.0
        if b == 8: log[:, 1] = 0.0                                          # nothing in range: GPS_EMPTY, gated as well
        tracks.append((tt[:n], pp[:n], qq[:n])); logs.append(log); gts.append(gt)
    return tracks, logs, gts


def _arrays(tag, r, st, out):
    out[f"{tag}/mt_state"] = st.cpu().numpy()
    out[f"{tag}/pos"], out[f"{tag}/quat"], out[f"{tag}/status"] = (x.cpu().numpy() for x in (r.fused.pos, r.fused.quat, r.fused.status))
    for k in FIELDS:
        v = getattr(r, k, None)
        if v is not None:
            out[f"{tag}/{k}"] = v.cpu().numpy()


def run_all(B, orc):
    """name -> host array: every output and the final generator state of the three calls, on the library that is loaded"""
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    from test_buffer_hygiene import dense_run_batch
    ctx = B.context()
    before = ctx.options.get("ransac_early_exit", 0)
    out = {}
    gb = dense_run_batch(B, 16, 130, 77)
    st = B.mt19937_seed(np.arange(16) + 500)
    _arrays("dense", B.run_fusion_batch(gb, st, copy.deepcopy(E.CONFIG)), st, out)
    ctx.set_option("ransac_early_exit", before)                             # (the dense function leaves it on)
    tracks, logs, gts = ragged_inputs(orc)
    cfg = copy.deepcopy(E.CONFIG)
    cfg["ground_truth_gps_filtering"]["enabled"] = True
    for tag, g, ee in (("ragged_gt", gts, True), ("ragged", None, False)):
        rb = B.RaggedGeodeticBatch.from_host(tracks, logs, g)
        st = B.mt19937_seed(np.arange(rb.B) + 100)
        _arrays(tag, B.run_fusion_ragged(rb, st, cfg, early_exit=ee), st, out)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    from gps_optimize_slam_amd import batch
    from oracle import oracle
    oracle.build()
    arrays = run_all(batch, oracle)
    for tag in ("dense", "ragged_gt", "ragged"):
        print(tag, "run_status", arrays[f"{tag}/run_status"].tolist())
    np.savez_compressed(a.out, commit=np.array(a.commit), **arrays)
    print(f"wrote {a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")
