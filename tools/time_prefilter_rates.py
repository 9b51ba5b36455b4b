"""Device time of the whole-run chain (run_fusion_batch: gsf_run_fusion_batch_dev) on 1 000 x 271-pose tracks with 10 Hz GNSS logs and with
50 Hz logs -- 15 s pre-filter windows of 150 and of 750 fixes: scikit-learn's sampler takes its permutation route on the first, its tracking-
selection route on the second (min_samples / n <= 0.01).  Device events after warm-up, the two rates alternating repeat by repeat.  Then,
in runs of their own (one child process per rate), rocprofv3 --kernel-trace --stats: the pre-filter kernel's (gps_prefilter_chain_kernel)
time per launch and per log, and the chain's other kernels.
usage: python tools/time_prefilter_rates.py [--reps 20] [--warmup 3] [--trace-dir DIR]   -> one JSON object on stdout (milliseconds)
       python tools/time_prefilter_rates.py --only-rate 50 --reps 3 --warmup 1          (what the traced child runs)"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gps_optimize_slam_amd import batch as Bm  # noqa: E402
from gps_optimize_slam_amd.ekfgpsslam import CONFIG  # noqa: E402

NB, N = 1000, 271


def batch_at(rate, seed=20250523):
    """GeodeticBatch.synthetic's tracks with their logs resampled to `rate` Hz (fixes interpolated along the log, 0.3 m noise)"""
    src = Bm.GeodeticBatch.synthetic(NB, N, seed=seed)
    offs = src.gps_offsets.cpu().numpy()
    gt, llh = src.gps_t.cpu().numpy(), src.gps_llh.cpu().numpy()
    ts, pos, quat = src.ts.cpu().numpy(), src.pos.cpu().numpy(), src.quat.cpu().numpy()
    rng = np.random.default_rng(seed)
    logs = []
    for b in range(NB):
        t0, l0 = gt[offs[b]:offs[b + 1]], llh[offs[b]:offs[b + 1]]
        t = t0[0] + np.arange(int((t0[-1] - t0[0]) * rate) + 1) / rate
        cols = [np.interp(t, t0, l0[:, c]) for c in range(3)]
        noise = rng.normal(0, 0.3, (len(t), 3))
        logs.append(np.column_stack((t, cols[0] + noise[:, 0] / 111200.0, cols[1] + noise[:, 1] / 73000.0, cols[2] + noise[:, 2])))
    return Bm.GeodeticBatch.from_host(ts, pos, quat, logs), int(np.mean([len(x) for x in logs]))


def timed(cases, reps, warmup):
    ms = {k: [] for k in cases}
    for r in range(warmup + reps):
        for k, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v))} for k, v in ms.items()}


def kernel_stats(rate, trace_dir, reps, warmup):
    """one rocprofv3 --kernel-trace --stats run of this script at one rate; per-kernel calls / average ns from its stats CSV"""
    d = os.path.join(trace_dir, f"rate{rate}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--only-rate", str(rate), "--reps", str(reps), "--warmup", str(warmup)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    f = sorted(glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True), key=os.path.getmtime)[-1]
    out = {}
    for row in csv.DictReader(open(f)):
        name = row["Name"].replace("(anonymous namespace)::", "")
        name = (name[5:] if name.startswith("void ") else name).split("(")[0]
        out[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-rate", type=int, default=0)
    ap.add_argument("--trace-dir", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rates = [a.only_rate] if a.only_rate else [10, 50]
    cases, fixes, status = {}, {}, {}
    for rate in rates:
        gb, fixes[rate] = batch_at(rate)
        st0 = Bm.mt19937_seed(np.arange(NB) + 1)

        def run(gb=gb, st0=st0, rate=rate):
            r = Bm.run_fusion_batch(gb, st0.clone(), CONFIG, want_mask=False)
            status[rate] = r.run_status
        cases[f"{rate}hz"] = run
    res = timed(cases, a.reps, a.warmup)
    if a.only_rate:
        return
    doc = {"tracks": NB, "poses": N, "fixes_per_log": {f"{k}hz": v for k, v in fixes.items()}, "run_fusion_batch": res,
           "run_status_nonzero": {f"{k}hz": int((v != 0).sum()) for k, v in status.items()},
           "prefilter_unhandled": {f"{k}hz": int(((v & 4) != 0).sum()) for k, v in status.items()}}
    if a.trace_dir:
        doc["kernels"] = {}
        for rate in rates:
            ks = kernel_stats(rate, a.trace_dir, 3, 1)
            doc["kernels"][f"{rate}hz"] = ks
            pf = ks.get("gps_prefilter_chain_kernel")
            if pf:
                doc.setdefault("prefilter_us_per_log", {})[f"{rate}hz"] = pf["avg_us"] / NB
                doc.setdefault("prefilter_us_per_launch", {})[f"{rate}hz"] = pf["avg_us"]
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
