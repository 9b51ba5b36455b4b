"""Shared by tests/test_stream_lag_host.py and tests/test_stream_lag.py: the stand-alone host harness of the stream's fixed-lag smoother
(tests/host_harness_stream_lag.cpp: gsf_stream_lag_core.hpp under g++), its job / result files, and the tracks of
tests/golden/ekf_lag_tracks.npz with their configs.  The NumPy statement the provisional rows are held to is
test_smooth_host.restate on the prefix."""
import os
import subprocess
import tempfile

import numpy as np

import stream_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
SMOOTHED, SPAN_START = 4, 16                       # GSF_POSE_*
LAG_F64, LAG_MAX = 12, 512
POS_TOL, VAR_TOL = 1e-7, 1e-12                     # the CPU gates of the whole-track smoother (tests/test_smooth_host.py)
_built = {}


def build(flags=("-O2",), tag=""):
    if tag not in _built:
        bdir = os.path.join(HERE, "_build")
        os.makedirs(bdir, exist_ok=True)
        exe = os.path.join(bdir, f"host_harness_stream_lag{tag}")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(HERE, "host_harness_stream_lag.cpp")])
        _built[tag] = exe
    return _built[tag]


def run(tracks, seg_lengths, cap, lag, config, exe=None):
    """tracks as stream_ref.flat takes them; seg_lengths: [v[B]] per append call, on a stream just opened over NaN garbage.
    -> dict(rep (ncalls,B,5) = n_total, status, smooth_from, n_smooth_final, new rings untouched; rows[c][b] (m,7) = spos, svar, sflags of the
    segment; tail[c][b] (k,6) = rows [smooth_from, n_total) of the smoothed rings after the call; violations; superset_diff;
    mirror[b] (n,6); ring_lag (B,cap,12), ring_spos, ring_svar (B,cap,3))"""
    exe = exe or build()
    B = len(tracks)
    f = S.flat(tracks)
    c18, steps = S.cfg_numbers(config)
    P = int(f["offsets"][-1])
    job = [np.array([B, cap, len(seg_lengths), P, steps, lag], dtype=np.float64), np.array(c18), f["init_pos"].ravel(), f["init_quat"].ravel(),
           f["offsets"].astype(np.float64), f["ts"], f["pos"].ravel(), f["quat"].ravel(), f["gps"].ravel(), f["valid"].astype(np.float64)]
    job += [np.asarray(v, dtype=np.float64) for v in seg_lengths]
    with tempfile.TemporaryDirectory() as d:
        jp, rp = os.path.join(d, "job.bin"), os.path.join(d, "result.bin")
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in job]).tofile(jp)
        p = subprocess.run([exe, jp, rp], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.startswith("OK"), (p.stdout, p.stderr)
        out = np.fromfile(rp, dtype=np.float64)
    at = 0
    rep, rows, tails = np.empty((len(seg_lengths), B, 5)), [], []
    for c, v in enumerate(seg_lengths):
        rep[c] = out[at:at + B * 5].reshape(B, 5); at += B * 5
        rc = []
        for b in range(B):
            m = int(v[b])
            rc.append(out[at:at + m * 7].reshape(m, 7)); at += m * 7
        rows.append(rc)
        tc = []
        for b in range(B):
            k = int(out[at]); at += 1
            tc.append(out[at:at + k * 6].reshape(k, 6)); at += k * 6
        tails.append(tc)
    violations, superset = int(out[at]), int(out[at + 1]); at += 2
    mirror = []
    for b in range(B):
        n = int(out[at]); at += 1
        mirror.append(out[at:at + n * 6].reshape(n, 6)); at += n * 6
    ring_lag = out[at:at + B * cap * LAG_F64].reshape(B, cap, LAG_F64); at += B * cap * LAG_F64
    ring_spos = out[at:at + B * cap * 3].reshape(B, cap, 3); at += B * cap * 3
    ring_svar = out[at:at + B * cap * 3].reshape(B, cap, 3); at += B * cap * 3
    assert at == out.size
    return dict(rep=rep, rows=rows, tail=tails, violations=violations, superset_diff=superset, mirror=mirror, ring_lag=ring_lag, ring_spos=ring_spos,
                ring_svar=ring_svar, stdout=p.stdout.strip())


def final_rows(res, b):
    """the rows that became final, call by call, concatenated: (k,7) = spos, svar, sflags"""
    parts = []
    for c in range(len(res["rows"])):
        k = int(res["rep"][c, b, 3] - res["rep"][c, b, 2])
        if not (int(res["rep"][c, b, 1]) & (S.STREAM_FULL | S.STREAM_BAD_STATE)):
            parts.append(res["rows"][c][b][:k])
            assert np.isnan(res["rows"][c][b][k:, :6]).all() and (res["rows"][c][b][k:, 6] == 0).all()
    return np.concatenate(parts) if parts else np.empty((0, 7))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


def var_err(got, want):
    """largest relative deviation; where the expected variance is exactly 0 the value must be 0 as well"""
    got, want = np.asarray(got), np.asarray(want)
    zero = want == 0.0
    assert (got[zero] == 0.0).all()
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]), initial=0.0))


# ------------------------------------------------------------------------------------------------ the fixture's tracks
def fixture_tracks(golden):
    """-> (g, [(name, stream track [ts, pos, quat, aligned, valid, init_pos, init_quat], cfg, slice into the fixture's rows)])"""
    import test_smooth_host as H
    g = golden("ekf_lag_tracks.npz")
    all_tracks, _ = H.smooth_tracks(golden)
    out = []
    for j, idx in enumerate(g["track_index"]):
        name, ts, pos, quat, aligned, valid, ip, iq, cfg = all_tracks[int(idx)]
        out.append((name, [ts, pos, quat, aligned, valid, ip, iq], cfg, slice(int(g["offsets"][j]), int(g["offsets"][j + 1]))))
    return g, out


def by_config(named):
    """the fixture's tracks grouped by their config (a stream has one): [(cfg, [positions in `named`])]"""
    import json
    groups = {}
    for k, (_, _, cfg, _) in enumerate(named):
        groups.setdefault(json.dumps(cfg, sort_keys=True), (cfg, []))[1].append(k)
    return list(groups.values())
