"""Device time of the ragged whole-run entry (gsf_run_fusion_ragged_dev) against the dense one (gsf_run_fusion_batch_dev), with device events
after warm-up and the two sides alternating repeat by repeat:
  * equal lengths, dense vs ragged: 1 000 x 271 and 10 000 x 271 (the same GeodeticBatch.synthetic batch fed to both);
  * a mixed-length batch (1 000 tracks, lengths drawn from 100 .. 3 000; ragged only);
  * the ground-truth leg on and off (1 000 x 271, its filter disabled as in CONFIG, and enabled).
usage: python tools/time_run_ragged.py [--reps 20] [--warmup 3]   -> one JSON object on stdout (milliseconds, median and min per case)"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gps_optimize_slam_amd import batch as Bm  # noqa: E402
from gps_optimize_slam_amd.ekfgpsslam import CONFIG  # noqa: E402


def ragged_of(gb, lens=None, gt=False):
    """a RaggedGeodeticBatch over the device tensors of a dense GeodeticBatch (tracks cut to `lens`), optionally with a ground-truth log
    = the primary log with its stamps shifted by 50 ms"""
    if lens is None:
        so = gb.slam_offsets
        ts, pos, quat, mp = gb.ts.reshape(-1), gb.pos.reshape(-1, 3), gb.quat.reshape(-1, 4), gb.N
    else:
        lens_t = torch.as_tensor(lens, dtype=torch.int64, device=gb.ts.device)
        keep = torch.arange(gb.N, device=gb.ts.device)[None, :] < lens_t[:, None]
        ts, pos, quat = gb.ts[keep].contiguous(), gb.pos[keep].contiguous(), gb.quat[keep].contiguous()
        so = torch.zeros(gb.B + 1, dtype=torch.int64, device=gb.ts.device)
        so[1:] = torch.cumsum(lens_t, 0)
        mp = int(max(lens))
    kw = {}
    if gt:
        kw = dict(gt_t=(gb.gps_t + 0.05).contiguous(), gt_llh=gb.gps_llh, gt_offsets=gb.gps_offsets, gt_max_fixes=gb.max_fixes)
    return Bm.RaggedGeodeticBatch(ts, pos, quat, so, gb.gps_t, gb.gps_llh, gb.gps_offsets, max_poses=mp, max_fixes=gb.max_fixes, **kw)


def timed(fns, reps, warmup):
    """fns: name -> callable(); alternating repeats; device time per call in ms"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v))} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {}
    for B, N in ((1000, 271), (10000, 271)):
        gb = Bm.GeodeticBatch.synthetic(B, N)
        rb = ragged_of(gb)
        st = Bm.mt19937_seed(np.arange(B))
        st0 = st.clone()

        def dense():
            st.copy_(st0); Bm.run_fusion_batch(gb, st, CONFIG)

        def ragged():
            st.copy_(st0); Bm.run_fusion_ragged(rb, st, CONFIG)
        res[f"equal_{B}x{N}"] = timed({"dense": dense, "ragged": ragged}, a.reps, a.warmup)
        r = res[f"equal_{B}x{N}"]
        r["ragged_over_dense"] = r["ragged"]["median_ms"] / r["dense"]["median_ms"]
    # mixed lengths: 1 000 tracks of 100 .. 3 000 poses (cut from a 3 000-pose synthetic batch)
    B = 1000
    gb = Bm.GeodeticBatch.synthetic(B, 3000, seed=5)
    lens = np.random.default_rng(1).integers(100, 3001, B)
    rb_mix = ragged_of(gb, lens)
    st = Bm.mt19937_seed(np.arange(B)); st0 = st.clone()

    def mixed():
        st.copy_(st0); Bm.run_fusion_ragged(rb_mix, st, CONFIG)
    res["mixed_1000_100..3000"] = timed({"ragged": mixed}, a.reps, a.warmup)
    res["mixed_1000_100..3000"]["poses"] = int(lens.sum())
    # ground-truth leg off / on (filter disabled as in CONFIG) / on with its filter enabled
    gb = Bm.GeodeticBatch.synthetic(1000, 271)
    rb0, rb1 = ragged_of(gb), ragged_of(gb, gt=True)
    cfg_f = copy.deepcopy(CONFIG); cfg_f["ground_truth_gps_filtering"]["enabled"] = True
    st = Bm.mt19937_seed(np.arange(1000)); st0 = st.clone()

    def run(rb, cfg):
        def f():
            st.copy_(st0); Bm.run_fusion_ragged(rb, st, cfg)
        return f
    g = timed({"no_gt": run(rb0, CONFIG), "gt_filter_off": run(rb1, CONFIG), "gt_filter_on": run(rb1, cfg_f)}, a.reps, a.warmup)
    g["gt_leg_share_filter_off"] = (g["gt_filter_off"]["median_ms"] - g["no_gt"]["median_ms"]) / g["no_gt"]["median_ms"]
    res["ground_truth_1000x271"] = g
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
