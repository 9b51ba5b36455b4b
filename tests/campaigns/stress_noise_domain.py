"""Randomised campaign over the stated noise range of the EKF routes (GPU box; not collected by pytest): log-uniform draws of P0, Q, R per
position axis and of the time unit of the stamps inside  0 <= P0 <= 1e8, 1e-8 <= R <= 1e8, 0 <= Q dt <= 1e14,  the host-made tracks of
tests/test_ekf_noise_domain_host.py, and the comparisons of tests/test_ekf_noise_domain.py: every pose route against the oracle, the
covariance kernel against the longdouble restatement.  usage: stress_noise_domain.py [ROUNDS] [SEED]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from gps_optimize_slam_amd import batch as B
from oracle import oracle as orc
import test_ekf_noise_domain as T
import test_ekf_noise_domain_host as H

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed0)
t0 = time.time()
for r in range(rounds):
    tscale = float(10.0 ** rng.integers(0, 10))                         # stamps in s .. ns
    alike = rng.random() < 0.5
    draw = lambda lo, hi: [float(10.0 ** rng.uniform(lo, hi))] * 3 if alike else [float(10.0 ** rng.uniform(lo, hi)) for _ in range(3)]
    qmax = 14.0 - np.log10(0.12 * tscale)                               # Q dt <= 1e14 at the longest step
    case = H._case(f"campaign-{seed0}-{r}", P0=draw(-8, 8), Q=draw(-8, min(8.0, qmax)), R=draw(-8, 8), tscale=tscale)
    if rng.random() < 0.1:
        case["Q"] = [0.0, 0.0, 0.0]
    case["seed"] = 1000 + r
    H.CASES[case["name"]] = case
    for route in T.ROUTES:
        T.test_pose_routes_on_the_grid(B, orc, route, case["name"])
    T.test_covariance_kernel_on_the_grid(B, case["name"])
    big, small, _ = H.scan_product_range(case, 200)
    print(f"round {r}: P0 {case['P0']} Q {case['Q']} R {case['R']} stamps x{tscale:g}: ok (unscaled product {small:.3g} .. {big:.3g}), {time.time() - t0:.0f} s", flush=True)
print(f"{rounds} rounds passed")
