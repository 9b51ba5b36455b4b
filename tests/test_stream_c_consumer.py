"""The streaming fusion from plain C (examples/stream_track.c): one track fused in three appends on device buffers the program owns, the
consumer keeping its own copy of the track by the rules of the contract (rows of the append, rows revised, rows final).
CPU tier: it builds warning-free as C99 against libgsf.so and fails loudly without a device.  GPU tier: the track it ends up with is the
track of one append of everything, bit for bit, and of batch.ekf_fuse_ragged within the project's gates."""
import os
import subprocess

import numpy as np
import pytest

import gate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gps_optimize_slam_amd")
BUILD = os.path.join(ROOT, "tests", "_build")
HIP_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")      # the runtime libgsf.so itself is linked against


@pytest.fixture(scope="module")
def exe():
    from gps_optimize_slam_amd import _lib
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "stream_track")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "stream_track.c"), "-o", out, "-L" + PKG, "-lgsf", "-Wl,-rpath," + PKG,
                           "-L" + HIP_LIB, "-lamdhip64", "-Wl,-rpath," + HIP_LIB])
    return out


def _track():
    from gps_optimize_slam_amd import ekfgpsslam as E
    # an outage across the first cut (pose 43), one inside the second segment, one that the track ends in
    return R.withhold(R.synthetic_track(130, 70, E.CONFIG), list(range(38, 50)) + [60, 61] + list(range(120, 130)))


def _write(path, tr):
    with open(path, "wb") as f:
        np.array([len(tr[0])], dtype=np.int64).tofile(f)
        for a in tr[:4]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        np.ascontiguousarray(tr[4], dtype=np.uint8).tofile(f)
        np.ascontiguousarray(tr[5], dtype=np.float64).tofile(f); np.ascontiguousarray(tr[6], dtype=np.float64).tofile(f)


def test_consumer_builds_and_fails_loudly_without_a_device(exe, tmp_path):
    from gps_optimize_slam_amd import _lib
    _write(tmp_path / "in.bin", _track())
    if _lib.load().gsf_device_count() > 0:
        return                                                              # (the GPU tier below runs it)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr and not (tmp_path / "out.bin").exists()


@pytest.mark.gpu
def test_three_appends_from_c_equal_one_append(exe, tmp_path):
    import torch
    from gps_optimize_slam_amd import batch as B, ekfgpsslam as E, _lib
    tr = _track()
    n = len(tr[0])
    _write(tmp_path / "in.bin", tr)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "gfx950" in r.stdout and f"streamed {n} poses in three appends" in r.stdout
    raw = open(tmp_path / "out.bin", "rb").read()
    fl = np.frombuffer(raw[:8 * n * 7], dtype=np.float64)
    pc, qc = fl[:n * 3].reshape(n, 3), fl[n * 3:].reshape(n, 4)
    marks = np.frombuffer(raw[8 * n * 7:8 * n * 7 + 72], dtype=np.int64).reshape(3, 3)
    status = np.frombuffer(raw[8 * n * 7 + 72:], dtype=np.int32)
    np.testing.assert_array_equal(marks[0], [43, 86, 130])                  # n_total
    np.testing.assert_array_equal(marks[1], [38, 86, 120])                  # n_final: the open outage's first pose
    np.testing.assert_array_equal(marks[2], [0, 38, 86])                    # revised_from: the second append's back-pass reached pose 38
    assert status[0] & _lib.ST_ENDED_IN_OUTAGE and status[1] & _lib.ST_RTS_APPLIED and not status[1] & _lib.ST_ENDED_IN_OUTAGE and status[2] & _lib.ST_ENDED_IN_OUTAGE
    s = E.FusionSession(tr[5], tr[6], E.CONFIG, cap=256)
    one = s.push(*tr[:5])
    np.testing.assert_array_equal(pc.view(np.uint64), one["pos"].view(np.uint64))
    np.testing.assert_array_equal(qc.view(np.uint64), one["quat"].view(np.uint64))
    assert one["status"] == status[2] and one["n_final"] == 120
    d = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    po, qo, st = B.ekf_fuse_ragged(d(tr[0]), d(tr[1]), d(tr[2]), d(tr[3]), d(tr[4], torch.uint8), d(np.array([0, n])), d(tr[5][None]), d(tr[6][None]))
    assert np.abs(pc - po.cpu().numpy()).max() < 1e-7 and np.abs(qc - qo.cpu().numpy()).max() < 1e-9 and int(st[0]) == int(status[2])
