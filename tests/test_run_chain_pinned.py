"""The whole-run chain computes what the pinned commit computed: every output word and the final generator states of one dense call
(16 x 130) and two ragged calls (nine tracks of 0 .. 200 poses, with and without ground truth) against tests/golden/run_chain_pinned.npz,
which tests/golden/gen_run_chain_pinned.py wrote with the library of the commit the file names.  Equality of words, no tolerance.

A pull request that changes the chain's results on purpose regenerates the file with that generator (at its own commit) and says so."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_run_chain_pinned as gen  # noqa: E402

pytestmark = pytest.mark.gpu


def test_whole_run_outputs_are_the_pinned_words():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    from oracle import oracle
    oracle.build()
    want = np.load(gen.PATH)
    assert len(str(want["commit"])) == 40
    got = gen.run_all(batch, oracle)
    assert sorted(got) == sorted(k for k in want.files if k != "commit")
    # a batch that stops everywhere would compare equal as well: each call holds runs that complete and runs that do not
    for tag in ("dense", "ragged_gt", "ragged"):
        rs = want[f"{tag}/run_status"]
        print(tag, "run_status", rs.tolist())
        assert (rs != 0).sum() >= 3 and (rs == 0).sum() >= 3, (tag, rs)
    assert (want["ragged_gt/run_status"] != want["ragged/run_status"]).any()       # the ground-truth leg stops runs of its own
    diff = []
    for k, g in got.items():
        w = want[k]
        if g.dtype != w.dtype or g.shape != w.shape:
            diff.append(f"{k}: {g.dtype} {g.shape}, pinned {w.dtype} {w.shape}")
        elif g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)) // g.itemsize
            diff.append(f"{k}: {np.unique(bad).size} of {g.size} words differ, first at flat index {int(bad[0])}")
    assert not diff, f"against commit {want['commit']}:\n" + "\n".join(diff)
