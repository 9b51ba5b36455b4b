"""The launch sequence of the whole-run chain: one dense call (16 x 130) and one ragged call with ground truth (nine tracks of 0 .. 200 poses),
the sizes of tests/test_run_chain_pinned.py on synthetic batches.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/run_chain_launches.py      (a run of its own, no counters)
    python tools/run_chain_launches.py --list <dir>/**/*_kernel_trace.csv > launches.txt

--list prints one line per dispatch in start order: kernel name, grid, workgroup, LDS bytes.  Two commits launch the same chain when their
lists are the same text (diff)."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def listing(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0].replace("void ", "")
        xyz = lambda stem: "x".join(str(int(r.get(f"{stem}_{a}", 1) or 1)) for a in "XYZ")
        print(f"{name} grid={xyz('Grid_Size')} block={xyz('Workgroup_Size')} lds={int(r.get('LDS_Block_Size', 0) or 0)}")


def main():
    sys.path.insert(0, ROOT)
    import copy
    import numpy as np
    import torch
    from gps_optimize_slam_amd import batch as B
    from gps_optimize_slam_amd.ekfgpsslam import CONFIG
    from time_run_ragged import ragged_of
    B.run_fusion_batch(B.GeodeticBatch.synthetic(16, 130, seed=77), B.mt19937_seed(np.arange(16) + 500), CONFIG)
    cfg = copy.deepcopy(CONFIG)
    cfg["ground_truth_gps_filtering"]["enabled"] = True
    rb = ragged_of(B.GeodeticBatch.synthetic(9, 200, seed=3), [0, 1, 5, 64, 65, 200, 65, 64, 5], gt=True)
    B.run_fusion_ragged(rb, B.mt19937_seed(np.arange(rb.B) + 100), cfg)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        main()
