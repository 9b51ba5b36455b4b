"""GPU tier of the innovation gate (gsf_innovation_gate_dev; definitions in include/gsf.h).

The kernel against tests/gate_ref.py, the per-pose restatement that tests/test_innovation_gate_host.py pins to the oracle.  The tracks are
gate_ref.edge_batch: lengths 0, 1, 2, 63, 64, 65, 129 and 200, planted so that a rejection falls into lane 0 and lane 63 of a chunk, at pose
1 and at the last pose, in a run across the 63 / 64 boundary, next to an outage of the data on either side, into a one-pose outage that
then counts as a sharp turn; a gate of 0 rejects all 64 lanes of a chunk; plus a stopped and an unsorted track.

 1. exact properties: an infinite gate changes nothing; a gate's rows are the same bytes alone, among five and in reversed order; up to
    and including the first rejection the NIS is the ungated run's, bit for bit; no output depends on stale buffers or workspaces.
 2. the mask against the restatement.  A decision can only differ where |nis / gate - 1| is within the NIS discrepancy of two float64
    evaluations (y within 1.7e-9 m); a (track, gate) case with a tested pose within 1e-6 of the gate BY THE RESTATEMENT ALONE is
    left out (the host tier asserts that these are under 5 % of the cases), on every other case valid_out, the six counts and gate_status
    are exact and the NIS figures lie within the first-order bound from the project's 1e-6 m / 1e-10 gates.
 3. composition: ekf_fuse_ragged on valid_out gives the gated track (1e-6 m), ekf_covariance_ragged on it flags exactly the poses without
    an applied fix.
 4. it does what it is for: planted 30 m outliers are all rejected at the 0.999 quantile, under 1 % of the clean fixes are, and the fused
    track is closer to the planted truth."""
import numpy as np
import pytest

import gate_ref as R
import hygiene
from test_cov_gpu import file_batch, small_dirt
from test_noise_sweep import dev, flat, same

pytestmark = pytest.mark.gpu

EXACT = [0, 1, 2, 3, 4, 5]                                              # the six counts of a stats row


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def edge():
    """gate_ref.gpu_cases() and the flat batch of its tracks with a stopped and an unsorted track appended:
    (cases, flat host arrays, run_status, index of the stopped track, index of the unsorted one)"""
    cases = R.gpu_cases()
    tracks = [t for _, t in cases[0]["tracks"]]
    stopped = [np.array(x, copy=True) for x in tracks[14]]
    unsorted = [np.array(x, copy=True) for x in tracks[14]]
    unsorted[0][10], unsorted[0][11] = unsorted[0][11], unsorted[0][10]
    allt = tracks + [stopped, unsorted]
    assert len(allt) <= 32 and {len(t[0]) for t in allt} == {0, 1, 2, 63, 64, 65, 129, 200}
    rs = np.zeros(len(allt), np.int32); rs[len(tracks)] = 3
    return cases, flat(allt), rs, len(tracks), len(tracks) + 1


def gate(B, f, gates, cfg, rs=None, **kw):
    """f = flat(...) host arrays (or device tensors already) -> InnovationGate, synchronised"""
    import torch
    d = [x if torch.is_tensor(x) else dev(x) for x in f]
    g = B.innovation_gate_ragged(*d, gates, config=cfg, run_status=None if rs is None else dev(rs), **kw)
    torch.cuda.synchronize()
    return g


def h(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


# ------------------------------------------------------------------------------------------------ 1. exact properties
def test_infinite_gate_changes_nothing(B, edge):
    cases, f, rs, i_stop, i_uns = edge
    g = gate(B, f, [np.inf], cases[0]["cfg"], rs, want_nis=True)
    vo, st, offs = h(g.valid_out)[0], h(g.stats), f[5]
    want = f[4].copy(); want[offs[i_stop]:offs[i_stop + 1]] = 0          # a stopped track: bytes 0
    np.testing.assert_array_equal(vo, want)
    ran = [b for b in range(len(rs)) if b not in (i_stop, i_uns)]
    assert (st[ran, 0, 2] == 0).all() and (st[ran, 0, 3] == 0).all() and (st[ran, 0, 5] == -1).all()
    assert not h(g.rejected(0)).any()
    status = h(g.status)
    assert status[i_stop] == R.GATE_SKIPPED and status[i_uns] == R.GATE_UNSORTED and np.isnan(st[[i_stop, i_uns]]).all()
    empty = [b for b in ran if offs[b + 1] == offs[b]]
    assert empty and (status[empty] == R.GATE_EMPTY).all() and (status[[b for b in ran if b not in empty]] == 0).all()
    assert st[empty[0], 0].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]
    nis = h(g.nis_out)[0]
    assert np.isnan(nis[offs[i_stop]:offs[i_stop + 1]]).all() and np.isnan(nis[offs[i_uns]:offs[i_uns + 1]]).all()
    np.testing.assert_array_equal(vo[offs[i_uns]:offs[i_uns + 1]], f[4][offs[i_uns]:offs[i_uns + 1]])     # unsorted: the mask as it came


def test_a_gates_rows_do_not_depend_on_its_neighbours(B, edge):
    cases, f, rs, _, _ = edge
    import torch
    d = [dev(x) for x in f]
    for c in (cases[0], cases[2]):
        kw = dict(arm_seconds=c["arm_seconds"], max_run=c["max_run"], want_nis=True)
        gates = list(R.GPU_GATES)
        five = gate(B, d, gates, c["cfg"], rs, **kw)
        rev = gate(B, d, gates[::-1], c["cfg"], rs, **kw)
        K = len(gates)
        for k in range(K):
            alone = gate(B, d, [gates[k]], c["cfg"], rs, **kw)
            for other, ko in ((five, k), (rev, K - 1 - k)):
                assert torch.equal(alone.valid_out[0], other.valid_out[ko]), (k, ko)
                assert same(alone.stats[:, 0], other.stats[:, ko]), (k, ko)
                assert same(alone.nis_out[0], other.nis_out[ko]), (k, ko)


def test_nis_up_to_the_first_rejection_is_the_ungated_runs(B, edge):
    cases, f, rs, i_stop, i_uns = edge
    offs = f[5]
    checked = 0
    for c in (cases[0], cases[1], cases[4]):
        g = gate(B, f, list(R.GPU_GATES), c["cfg"], rs, arm_seconds=c["arm_seconds"], max_run=c["max_run"], want_nis=True)
        nis, st = h(g.nis_out), h(g.stats)
        inf_k = len(R.GPU_GATES) - 1
        for b in range(len(rs)):
            if b in (i_stop, i_uns) or offs[b + 1] == offs[b]:
                continue
            for k in range(inf_k):
                first = int(st[b, k, 5])
                upto = offs[b + 1] if first < 0 else offs[b] + first + 1
                np.testing.assert_array_equal(bits(nis[k, offs[b]:upto]), bits(nis[inf_k, offs[b]:upto]), err_msg=str((b, k)))
                checked += first >= 0
    assert checked > 100


def test_outputs_do_not_depend_on_stale_buffers(B, monkeypatch, edge):
    """outputs prefilled with two byte patterns, workspaces poisoned and not: the same bytes, with and without the NIS rows"""
    cases, f, rs, _, _ = edge
    c = cases[2]
    d, drs, gates = [dev(x) for x in f], dev(rs), list(R.GPU_GATES)
    kw = dict(config=c["cfg"], run_status=drs, max_run=c["max_run"])
    res = hygiene.same_bytes_under_dirt(monkeypatch, B.context(), lambda: B.innovation_gate_ragged(*d, gates, want_nis=True, **kw), small_dirt(B))
    res2 = hygiene.same_bytes_under_dirt(monkeypatch, B.context(), lambda: B.innovation_gate_ragged(*d, gates, **kw), small_dirt(B))
    assert same(res.stats, res2.stats) and same(res.valid_out, res2.valid_out) and same(res.status, res2.status)
    assert res2.nis_out is None and tuple(res.nis_out.shape) == (len(gates), int(f[5][-1]))


def test_null_outputs_and_argument_errors(B, edge):
    """every output NULL in turn leaves the others' bytes unchanged; B = 0 returns GSF_OK; K outside 1..64 is refused by the library too"""
    import ctypes as C
    import torch
    from gps_optimize_slam_amd import _lib
    cases, f, rs, _, _ = edge
    cfg = cases[0]["cfg"]
    d, drs = [dev(x) for x in f], dev(rs)
    gates = dev(np.array(R.GPU_GATES))
    nb, K, P = len(rs), len(R.GPU_GATES), int(f[5][-1])
    want = gate(B, d, gates, cfg, rs, want_nis=True)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    c = _lib.EkfConfig.from_config(cfg)

    def call(outs, nb_=nb, K_=K):
        return _lib.load().gsf_innovation_gate_dev(B.context().handle, *[p(x) for x in d[:6]], p(drs), p(d[6]), p(d[7]), C.byref(c), nb_, p(gates),
                                                   K_, 0.0, 0, *[p(o) for o in outs])
    names = ("valid_out", "nis_out", "stats", "status")
    for skip in range(4):
        outs = [torch.empty_like(getattr(want, n)) for n in names]
        outs[skip] = None
        assert call(outs) == 0
        torch.cuda.synchronize()
        for j, n in enumerate(names):
            if j != skip:
                assert same(outs[j], getattr(want, n)), (skip, n)
    assert call([None] * 4, nb_=0) == 0
    for bad in (0, 65):
        assert call([None] * 4, K_=bad) != 0


# ------------------------------------------------------------------------------------------------ 2. the mask against the restatement
@pytest.mark.parametrize("ci", range(len(R.GPU_CONFIGS)))
def test_mask_counts_and_nis_against_the_restatement(B, edge, ci):
    cases, f, rs, i_stop, i_uns = edge
    c = cases[ci]
    offs = f[5]
    g = gate(B, f, list(R.GPU_GATES), c["cfg"], rs, arm_seconds=c["arm_seconds"], max_run=c["max_run"], want_nis=True)
    vo, nis, st, status = h(g.valid_out), h(g.nis_out), h(g.stats), h(g.status)
    kept = left_out = 0
    worst_nis = worst_sum = 0.0
    for b, ((name, _), refs) in enumerate(zip(c["tracks"], c["ref"])):
        sl = slice(offs[b], offs[b + 1])
        all_kept = True
        for k, r in enumerate(refs):
            what = (name, R.GPU_GATES[k], c["max_run"], c["arm_seconds"])
            if r["near"]:
                left_out += 1; all_kept = False
                continue
            kept += 1
            print(f"{what}: rejected {int(st[b, k, 2])} / {int(r['stats'][2])}, forced {int(st[b, k, 3])} / {int(r['stats'][3])}, "
                  f"longest {int(st[b, k, 4])}, first {int(st[b, k, 5])}")
            np.testing.assert_array_equal(vo[k, sl], r["valid_out"], err_msg=str(what))
            np.testing.assert_array_equal(st[b, k, EXACT], r["stats"][EXACT], err_msg=str(what))
            np.testing.assert_array_equal(np.isnan(nis[k, sl]), ~r["avail"], err_msg=str(what))
            av = r["avail"]
            if av.any():
                bound = R.nis_bound(r)
                share = np.abs(nis[k, sl][av] - r["nis"][av]) / bound[av]
                worst_nis = max(worst_nis, float(share.max()))
                at = R.applied_tested(r)
                bmax = float(bound[at].max()) if at.any() else 0.0
                bsum = float(bound[at].sum()) + 1e-12 * float(r["stats"][7])
                for j, bd in ((6, bmax), (7, bsum)):
                    dlt = abs(st[b, k, j] - r["stats"][j])
                    if dlt > 0.0:
                        assert bd > 0.0, (what, j)
                        worst_sum = max(worst_sum, dlt / bd)
            else:
                assert st[b, k, 6] == 0.0 and st[b, k, 7] == 0.0
        if all_kept:
            want = 0
            for r in refs:
                want |= r["status"]
            assert status[b] == want, (name, status[b], want)
    print(f"config {ci}: {kept} cases kept, {left_out} left out; NIS within {worst_nis:.2e} of its bound, the two NIS figures of stats within {worst_sum:.2e}")
    assert left_out <= 0.05 * (kept + left_out)
    assert worst_nis <= 1.0 and worst_sum <= 1.0
    assert status[i_stop] == R.GATE_SKIPPED and status[i_uns] == R.GATE_UNSORTED


# ------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("ci", [0, 2, 4])
def test_existing_entries_on_valid_out_give_the_gated_fusion(B, edge, ci):
    """ekf_fuse_ragged on valid_out: the gated filter's positions wherever RTS rewrites nothing (the restatement's p), and the oracle's
    apply_ekf_correction on the restatement's mask everywhere (the host tier pins the two to each other); POSE_IN_OUTAGE of
    ekf_covariance_ragged on valid_out is set on exactly the poses that lack a valid fix or were rejected"""
    import torch
    from gps_optimize_slam_amd import _lib
    from oracle import oracle as orc
    cases, f, rs, i_stop, i_uns = edge
    c = cases[ci]
    offs = f[5]
    d = [dev(x) for x in f]
    g = gate(B, d, list(R.GPU_GATES), c["cfg"], rs, arm_seconds=c["arm_seconds"], max_run=c["max_run"])
    worst_p = worst_o = 0.0
    for k in (0, 1, 3):
        vk = g.valid(k).contiguous()
        po, _, _ = B.ekf_fuse_ragged(d[0], d[1], d[2], d[3], vk, d[5], d[6], d[7], config=c["cfg"])
        cov = B.ekf_covariance_ragged(d[0], d[2], d[3], vk, d[5], config=c["cfg"], run_status=dev(rs))
        torch.cuda.synchronize()
        po, fl = h(po), h(cov.flags)
        for b, ((name, tr), refs) in enumerate(zip(c["tracks"], c["ref"])):
            r = refs[k]
            n = len(tr[0])
            if r["near"] or n == 0:
                continue
            sl = slice(offs[b], offs[b + 1])
            applied = r["avail"] & ~r["rejected"]
            if applied.any():
                worst_p = max(worst_p, float(np.abs(po[sl][applied] - r["p"][applied]).max()))
            want = orc.apply_ekf_correction_aligned(tr[0], tr[1], tr[2], tr[3], r["valid_out"], tr[5], tr[6], c["cfg"])[0]
            worst_o = max(worst_o, float(np.abs(po[sl] - want).max()))
            in_outage = ~applied
            in_outage[0] = not bool(tr[4][0])                            # pose 0: the raw mask byte
            np.testing.assert_array_equal((fl[sl] & _lib.POSE_IN_OUTAGE) != 0, in_outage, err_msg=str((name, k)))
    print(f"config {ci}: ekf_fuse_ragged on valid_out vs the restatement's filter {worst_p:.2e} m, vs the oracle on the restatement's mask {worst_o:.2e} m")
    assert worst_p <= 1e-6 and worst_o <= 1e-6


# ------------------------------------------------------------------------------------------------ 4. it does what it is for
@pytest.mark.parametrize("seed", range(8))
def test_planted_outliers_are_rejected_and_the_fused_track_improves(B, seed):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    tracks, disp = R.planted_outlier_batch(cfg, seed)
    truth = np.concatenate(R.planted_truth(cfg, seed))
    f = flat(tracks)
    d = [dev(x) for x in f]
    g = gate(B, d, [B.chi2_gate(0.999)], cfg, want_nis=True)
    rej = h(g.rejected(0))
    nis = h(g.nis_out)[0]
    dm = np.concatenate(disp)
    avail = ~np.isnan(nis)
    assert rej[dm].all()                                                  # arm_seconds = 0: every displaced fix is tested
    clean = avail & ~dm
    false_rej = int((rej & clean).sum())
    pg, _, _ = B.ekf_fuse_ragged(d[0], d[1], d[2], d[3], g.valid(0).contiguous(), d[5], d[6], d[7], config=cfg)
    pu, _, _ = B.ekf_fuse_ragged(*d, config=cfg)
    torch.cuda.synchronize()
    rms_g, rms_u = (float(np.sqrt(((h(p) - truth) ** 2).sum(axis=1).mean())) for p in (pg, pu))
    print(f"seed {seed}: {int(dm.sum())} displaced fixes all rejected, {false_rej} of {int(clean.sum())} clean ones rejected "
          f"({100.0 * false_rej / clean.sum():.2f} %), fused rms against the truth {rms_g:.3f} m gated, {rms_u:.3f} m ungated")
    assert false_rej < 0.01 * clean.sum()
    assert rms_g < rms_u
    t = g.table()
    assert float(t["rejected"][0]) == rej.sum() and float(t["tested"][0]) == avail.sum()
    np.testing.assert_allclose(h(g.reject_rate)[:, 0], h(g.stats)[:, 0, 2] / h(g.stats)[:, 0, 1])


# ------------------------------------------------------------------------------------------------ 5. the workflow
def test_gate_on_a_whole_run_and_fuse_again(B, golden, tmp_path):
    """run_fusion_ragged on the bundled track's files -> gate_fused -> refuse_gated: with an infinite gate the second fusion is the
    run's own (1e-6 m); with the 0.999 quantile it runs, flags the stopped track and reports the error rows of the tracks that ran"""
    import torch
    from gps_optimize_slam_amd import _lib, ekfgpsslam as E
    rb = file_batch(B, golden, tmp_path)
    r = B.run_fusion_ragged(rb, B.mt19937_seed([3, 4, 5, 6]), E.CONFIG)
    g = B.gate_fused(rb, r, [np.inf, B.chi2_gate(0.999)], arm_seconds=5.0, max_run=10, want_nis=True)
    torch.cuda.synchronize()
    rs, so = h(r.run_status), h(rb.slam_offsets)
    status = h(g.status)
    assert rs[2] != 0 and status[2] == _lib.GATE_SKIPPED and (status[[0, 1, 3]] & (_lib.GATE_SKIPPED | _lib.GATE_EMPTY | _lib.GATE_UNSORTED) == 0).all()
    same_run = B.refuse_gated(rb, r, g, k=0)
    gated = B.refuse_gated(rb, r, g, k=1, want_cov=True)
    torch.cuda.synchronize()
    for b in (0, 1, 3):
        sl = slice(so[b], so[b + 1])
        assert float(np.abs(h(same_run.pos)[sl] - h(r.fused.pos)[sl]).max()) <= 1e-6, b
        assert np.isfinite(h(gated.pos)[sl]).all() and np.isfinite(h(gated.err_stats)[b]).all()
        np.testing.assert_array_equal(h(gated.valid)[sl] != 0, (h(r.valid)[sl] != 0) & ~h(g.rejected(1))[sl])
    assert gated.cov is not None and tuple(gated.errors.shape) == (int(so[-1]),)
    print("whole run:", {k: h(v).round(3).tolist() for k, v in g.table().items()})


def test_single_track_entry_agrees_with_the_batch_entry(B):
    """ekfgpsslam.gate_gnss_fixes: the same alignment call as apply_ekf_correction, then the batch entry on that one track"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    tr = R.plant(R.synthetic_track(129, 21, E.CONFIG), [40, 41, 90])
    slam = {"timestamps": tr[0], "positions": tr[1], "quaternions": tr[2]}
    gps = {"timestamps": tr[0][::2].copy(), "positions": tr[3][::2].copy()}      # a 5 Hz log against 10 Hz poses: every other fix interpolated
    sim3_pos, sim3_quat = np.tile(tr[5], (129, 1)), np.tile(tr[6], (129, 1))
    gates = [np.inf, B.chi2_gate(0.999)]
    out = E.gate_gnss_fixes(slam, gps, sim3_pos, sim3_quat, E.CONFIG, gates, arm_seconds=1.0, max_run=5, want_nis=True)
    aligned, valid = E.dynamic_time_alignment(slam, gps, E.CONFIG["time_alignment"])
    np.testing.assert_array_equal(out["aligned"], aligned)
    f = flat([(tr[0], tr[1], tr[2], aligned, valid, tr[5], tr[6])])
    g = gate(B, f, gates, E.CONFIG, arm_seconds=1.0, max_run=5, want_nis=True)
    np.testing.assert_array_equal(out["valid"], h(g.valid_out))
    np.testing.assert_array_equal(bits(out["stats"]), bits(h(g.stats)[0]))
    np.testing.assert_array_equal(bits(out["nis"]), bits(h(g.nis_out)))
    assert out["status"] == int(g.status[0]) == R.GATE_ANY_REJECTED
    assert out["rejected"].shape == (2, 129) and not out["rejected"][0].any() and out["rejected"][1][[40, 90]].all()
    want = R.gated(tr[0], tr[1], tr[2], aligned, valid, tr[5], tr[6], gates[1], E.CONFIG, arm_seconds=1.0, max_run=5)
    assert not want["near"]
    np.testing.assert_array_equal(out["valid"][1], want["valid_out"])
    with pytest.raises(ValueError):
        E.gate_gnss_fixes(slam, gps, sim3_pos[:5], sim3_quat[:5], E.CONFIG, gates)
    with pytest.raises(ValueError, match="gates"):
        E.gate_gnss_fixes(slam, gps, sim3_pos, sim3_quat, E.CONFIG, [])
