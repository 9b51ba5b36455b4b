"""CPU tier of the clock-offset search: the yardstick itself (tests/clock_offset_ref.py, the oracle's composition) finds a planted offset
with a margin that makes "same best_k" a fair demand of the device, calls a straight constant-velocity track flat, and the batches'
with_clock_offset shifts stamps bit for bit."""
import numpy as np
import pytest

import clock_offset_ref as ref


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def planted(orc):
    """the three planted-offset shapes on the grid -1 .. 1 / 0.05, swept once"""
    out = []
    for n, ng in ref.PLANTED_SHAPES:
        tr = ref.make_track(n, ng)
        out.append((n, ng) + ref.sweep(orc, tr["ts"], tr["pos"], tr["gps_t"], tr["gps_p"], None, -1.0, 0.05, 41))
    return out


def test_yardstick_recovers_the_planted_offset(planted):
    for n, ng, J, nr, tau in planted:
        k, tau_best, tau_ref, st = ref.pick(J, tau, 0.05)
        print(f"poses {n} fixes {ng}: best tau {tau_best:.2f}  J {J[k]:.3g} m  margin {ref.margin(J) * 1e3:.3g} mm  refined {tau_ref:.6f}")
        assert np.isfinite(J).all() and (nr >= 4).all()
        assert k == int(np.argmin(np.abs(tau - ref.TAU_TRUE))) and st == 0, (n, ng, k)
        assert abs(tau_ref - ref.TAU_TRUE) < 1e-3, (n, ng, tau_ref)


def test_margin_to_the_runner_up_is_at_least_a_millimetre(planted):
    for n, ng, J, nr, tau in planted:
        assert ref.margin(J) >= 1e-3, (n, ng, ref.margin(J))


def test_straight_constant_velocity_track_is_flat(orc):
    tr = ref.make_track(130, 65, straight=True)
    J, nr, tau = ref.sweep(orc, tr["ts"], tr["pos"], tr["gps_t"], tr["gps_p"], None, -1.0, 0.05, 41)
    spread = np.nanmax(J) - np.nanmin(J)
    print(f"straight track: J spread {spread:.3g} m, max J {np.nanmax(J):.3g} m")
    assert np.isfinite(J).all() and spread < 1e-9
    assert ref.pick(J, tau, 0.05, flat_threshold=1e-3)[3] & ref.CLK_FLAT


def test_with_clock_offset_shifts_stamps_bit_for_bit():
    import torch
    from gps_optimize_slam_amd import batch as B
    rng = np.random.default_rng(3)
    tracks = [(np.arange(n) * 0.1, rng.normal(size=(n, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))) for n in (5, 0, 9)]
    logs = [np.column_stack((1.7e9 + np.sort(rng.uniform(0, 9, m)), rng.normal(size=(m, 3)))) for m in (7, 3, 0)]
    gts = [logs[0][:4], None, logs[1]]
    rb = B.RaggedGeodeticBatch.from_host(tracks, logs, gts, device="cpu")
    gps_t0, gt_t0 = rb.gps_t.clone(), rb.gt_t.clone()
    tau = torch.tensor([0.3, -1.25, 7.0], dtype=torch.float64)
    sh = rb.with_clock_offset(tau)
    want = rb.gps_t.numpy() + np.repeat(tau.numpy(), [7, 3, 0])
    assert sh.gps_t.numpy().tobytes() == want.tobytes()
    assert sh.gt_t is rb.gt_t and sh.gps_llh is rb.gps_llh and sh.ts is rb.ts and sh.max_fixes == rb.max_fixes
    sh2 = rb.with_clock_offset(tau, gt_tau=[0.5, 0.0, -2.0])
    want_gt = rb.gt_t.numpy() + np.repeat([0.5, 0.0, -2.0], [4, 0, 3])
    assert sh2.gt_t.numpy().tobytes() == want_gt.tobytes() and sh2.gps_t.numpy().tobytes() == want.tobytes()
    assert torch.equal(rb.gps_t, gps_t0) and torch.equal(rb.gt_t, gt_t0)                       # the source batch is untouched
    assert rb.with_clock_offset(0.0 * tau).gps_t.numpy().tobytes() == gps_t0.numpy().tobytes()   # a zero shift changes nothing
    with pytest.raises(ValueError):
        rb.with_clock_offset(tau[:2])
    # the dense batch's GNSS log
    gb = B.GeodeticBatch.from_host(np.zeros((2, 4)), np.zeros((2, 4, 3)), np.zeros((2, 4, 4)), logs[:2], device="cpu")
    g2 = gb.with_clock_offset([1.0, 2.0])
    assert g2.gps_t.numpy().tobytes() == (gb.gps_t.numpy() + np.repeat([1.0, 2.0], [7, 3])).tobytes() and g2.gps_llh is gb.gps_llh
