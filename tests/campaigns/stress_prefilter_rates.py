"""Randomised campaign for the GPS pre-filter at any receiver rate, inside the whole-run chain (gsf_run_fusion_batch_dev) on the GPU box: per
round one random CONFIG of the pre-filter (sliding or global, window length / step, min_samples, degree, threshold, trial cap) and 48 tracks
whose logs run at random rates of 1 .. 100 Hz -- windows on both sides of 100 x min_samples rows, i.e. both routes of scikit-learn's sampler
(permutation, tracking selection) -- with planted outliers.  Every track against the oracle's composition of the flow under ONE seeded generator
(tests/test_run_chain.py:_oracle_run, scikit-learn's sampler live): run_status, kept fixes and the final generator state exactly, n_inliers,
R, s and fused poses to the gates of tests/test_run_ragged.py.  No sorted log may be flagged PREFILTER_UNHANDLED.
usage: stress_prefilter_rates.py [ROUNDS] [SEED] [TRACKS]   (the issue's run: 15 rounds)"""
import copy, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from gps_optimize_slam_amd import batch as B, ekfgpsslam as E
from oracle import oracle as orc
from test_run_chain import _oracle_run, np_state
from test_run_ragged import _synthetic_case, _log

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
nb = int(sys.argv[3]) if len(sys.argv) > 3 else 48
orc.build()
tot = dict(tracks=0, ok=0, unhandled=0, other_status=0, filtered=0, tracking_logs=0, both_route_logs=0)
worst_p = 0.0
t0 = time.time()
for r in range(rounds):
    rng = np.random.default_rng(seed0 + r)
    N = 271
    cfg = copy.deepcopy(E.CONFIG)
    f = cfg["gps_filtering_ransac"]
    f["use_sliding_window"] = bool(rng.random() < 0.7)
    f["window_duration_seconds"] = float(rng.choice([8.0, 15.0, 15.0, 25.0]))
    f["window_step_factor"] = float(rng.choice([0.25, 0.5, 0.5, 1.0]))
    f["polynomial_degree"] = int(rng.choice([1, 2, 2, 3]))
    f["min_samples"] = int(rng.choice([4, 6, 6, 8]))
    f["residual_threshold_meters"] = float(rng.choice([3.0, 10.0, 10.0]))
    f["max_trials"] = int(rng.choice([20, 50, 50, 120]))
    ms = f["min_samples"]
    ts, pos, quat, logs = [], [], [], []
    for b in range(nb):
        tt, pp, qq, uu = _synthetic_case(orc, N, int(rng.integers(1000)))      # (its seed also places the track: near 450 km E)
        rate = float(rng.uniform(1.0, 100.0))
        tg = tt[0] + np.arange(int((tt[-1] - tt[0]) * rate) + 1) / rate
        ug = np.column_stack([np.interp(tg, tt, uu[:, c]) for c in range(3)])
        log = _log(orc, tg, ug, rng, 0.3, 0.003)
        m = len(log)
        if rng.random() < 0.6 and m > 10:                                  # fixes thrown 15 .. 80 m off
            for r_ in rng.choice(m, size=int(rng.integers(1, max(2, m // 50))), replace=False):
                d = rng.uniform(15.0, 80.0)
                log[r_, 1] += d / 111200.0 * rng.choice([-1, 1]); log[r_, 2] += d / 73000.0 * rng.choice([-1, 1])
        per_window = rate * (f["window_duration_seconds"] if f["use_sliding_window"] else tt[-1] - tt[0])
        tot["tracking_logs"] += int(per_window >= 100 * ms)
        tot["both_route_logs"] += int(f["use_sliding_window"] and 0.6 * per_window < 100 * ms <= per_window)
        ts.append(tt); pos.append(pp); quat.append(qq); logs.append(log)
    ts, pos, quat = np.stack(ts), np.stack(pos), np.stack(quat)
    gb = B.GeodeticBatch.from_host(ts, pos, quat, logs)
    seeds = rng.integers(1, 1 << 31, size=nb)
    st = B.mt19937_seed(seeds)
    res = B.run_fusion_batch(gb, st, cfg, early_exit=False)
    p, q, status = res.fused.host_traj_major()
    o2 = gb.gps_offsets.cpu().numpy()
    keep, rs = res.gps_keep.cpu().numpy().astype(bool), res.run_status.cpu().numpy()
    for b in range(nb):
        tot["tracks"] += 1
        ctx_ = (r, b, {k: f[k] for k in ("use_sliding_window", "window_duration_seconds", "window_step_factor", "min_samples", "max_trials")}, len(logs[b]))
        if rs[b] & 4:
            tot["unhandled"] += 1
            continue
        o = _oracle_run(orc, ts[b], pos[b], quat[b], logs[b], cfg, int(seeds[b]))
        key, ppos = np.random.get_state()[1:3]
        gk, gp = np_state(st[b])
        assert (gk == key).all() and gp == int(ppos), ("generator", ctx_)
        assert rs[b] == o["status"], ("run_status", ctx_, rs[b], o["status"])
        if o["status"] == 1:
            tot["other_status"] += 1; continue
        assert (keep[o2[b]:o2[b + 1]] == o["keep"]).all(), ("kept fixes", ctx_)
        tot["filtered"] += int(o["keep"].sum() < o["loaded"].sum())
        if o["status"] != 0:
            tot["other_status"] += 1
            assert np.isnan(p[b]).all(); continue
        tot["ok"] += 1
        assert int(res.n_inliers[b]) == o["n_inliers"], ("n_inliers", ctx_)
        fr = o["fit_rows"]
        sv = np.linalg.svd((pos[b][fr] - pos[b][fr].mean(0)).T @ (o["aligned"][fr] - o["aligned"][fr].mean(0)), compute_uv=False)
        k = max(1.0, float(sv[0] / max(sv[1] + sv[2], 1e-300)) / 100.0)
        assert np.abs(res.R[b].cpu().numpy().reshape(3, 3) - o["R"]).max() < 2e-9 * k, ("R", ctx_)
        assert abs(float(res.s[b]) - o["s"]) < 1e-11 * k, ("s", ctx_)
        dp = float(np.abs(p[b] - o["pos"]).max())
        assert dp < 1e-6 * k and np.abs(q[b] - o["quat"]).max() < 1e-8 * k, ("pose", ctx_, dp)
        worst_p = max(worst_p, dp / k)
    print(f"round {r}: {dict(tot)} ({time.time() - t0:.0f} s)", flush=True)
assert tot["unhandled"] == 0, tot
print(dict(tot, worst_pos_m=worst_p, seconds=round(time.time() - t0, 1)))
