"""Scans of a track's last chunk sized by its last active lane (gsf_set_option "tail_scan_stages", gsf_wave_common.hpp GSF_SCAN_STAGES_N).

A last chunk of at most 16 / 32 poses runs its Moebius, affine and quaternion scans with 4 / 5 of the 6 DPP stages: the cross-row stages
cannot reach its lanes.  The claim is BITS, not a tolerance: with the option at 1 (sized, the default) and at 0 (always six stages) every
output byte of K4 and of the fused pipeline is the same, in the one-wave build, the forced two-wave build and the big-batch build; and the
sized path agrees with the CPU oracle inside the tolerances tests/test_gpu_parity.py uses for the same outputs.  The -0.0 / non-finite
corner of a skipped stage (al * 0.0 + be) is kept by code -- the stage is replaced by its identity form, not dropped -- so no byte is
excused here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py: what the wave kernels are held to against the oracle
POS_TOL = 1e-7       # positions (the stated gate is 1e-6 m)
Q_TOL = 1e-9         # quaternion components
S_TOL = 1e-10        # scale of the pipeline's fit
SYN_POS_TOL, SYN_Q_TOL = 1e-6, 1e-8   # pipeline on the synthetic generator's short straight tracks (fit conditioned ~1e3-1e4)

LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 96, 97, 271, 335, 1000, 1039]
NB_SMALL, NB_BIG = 256, 2304         # one-wave / two-wave builds; big-batch build (B > 2 048)


@pytest.fixture(scope="module")
def B():
    from gps_optimize_slam_amd import batch
    return batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def planted_batch(nb, N, seed):
    """Host-made tracks, eight kinds in turn (track b is of kind b % 8): clean; outage at the start; outage at the end; outage across the
    last chunk boundary, recovered inside the tail chunk; NaN fixes with the mask still set (tail chunk included); an invalid quaternion in
    the tail chunk (generic orientation path); duplicate consecutive poses through the tail chunk, in and out of an outage (predicted
    displacements of +-0.0: the corner of the skipped stages); several random outages with a yaw burst (sharp-turn recoveries)."""
    rng = np.random.default_rng(seed)
    dt = 0.1 + rng.uniform(-0.004, 0.004, size=(nb, N)); dt[:, 0] = 0.0
    ts = 1000.0 + np.cumsum(dt, axis=1)
    head = np.cumsum(rng.normal(0, 0.01, size=(nb, N)), axis=1)
    valid = np.ones((nb, N), dtype=np.uint8)
    yaw_extra = np.zeros((nb, N))
    tail0 = ((N - 1) // 64) * 64                       # first pose of the last chunk
    for b in range(nb):
        kind = b % 8
        if kind == 1:
            valid[b, :int(rng.integers(1, max(2, min(N, 70))))] = 0
        elif kind == 2:
            valid[b, N - int(rng.integers(1, max(2, min(N, 70)))):] = 0
        elif kind == 3:
            lo = max(1, tail0 - int(rng.integers(1, 40))); hi = min(N - 1, tail0 + int(rng.integers(1, 12)))
            valid[b, lo:hi] = 0
        elif kind == 7:
            for _ in range(int(rng.integers(1, 4))):
                L = int(rng.choice([1, 2, 3, 7, 20, 64, 65]))
                s = int(rng.integers(0, max(1, N - L)))
                valid[b, s:s + L] = 0
                if L >= 3 and s + L < N:
                    k = s + 1 + int(rng.integers(0, L - 2))
                    yaw_extra[b, k:] += rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.2)
    step = 1.4 * np.stack([np.cos(head), np.sin(head), 0.01 * np.ones_like(head)], -1) * (dt[..., None] / 0.1)
    pos = np.cumsum(step, axis=1) + rng.normal(0, 0.01, size=(nb, N, 3))
    yaw = head + yaw_extra
    quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], -1) * rng.uniform(0.5, 2.0, size=(nb, N, 1))
    for b in range(6, nb, 8):                          # duplicates: the pose repeats from somewhere before the tail chunk to the end
        d0 = max(1, tail0 - int(rng.integers(0, 12))) if tail0 > 0 else max(1, N // 2)   # (never the whole track: one repeated point leaves the fit's rotation undefined)
        pos[b, d0:] = pos[b, d0 - 1]; quat[b, d0:] = quat[b, d0 - 1]
        if (b // 8) % 2 == 0 and N - d0 > 2:           # ... half of them inside an outage that runs to the end, or is recovered in the tail
            valid[b, d0:N - int(rng.integers(0, 3))] = 0
    for b in range(5, nb, 8):
        quat[b, int(rng.integers(tail0, N))] = 0.0
    gps = pos * 1.03 + np.array([4.5e5, 5.4e6, 110.0]) + rng.normal(0, 0.4, size=(nb, N, 3))
    gps[valid == 0] = np.nan
    for b in range(4, nb, 8):
        for i in set([int(rng.integers(tail0, N)), int(rng.integers(0, N)), N - 1]):
            gps[b, i, int(rng.integers(0, 3))] = np.nan
    init_pos = gps[:, 0].copy(); bad0 = np.isnan(init_pos).any(axis=1)
    init_pos[bad0] = pos[bad0, 0] * 1.03 + np.array([4.5e5, 5.4e6, 110.0])
    with np.errstate(invalid="ignore", divide="ignore"):
        init_quat = quat[:, 0] / np.linalg.norm(quat[:, 0], axis=1, keepdims=True)
    bq = ~np.isfinite(init_quat).all(axis=1); init_quat[bq] = np.array([0.0, 0.0, 0.0, 1.0])
    return ts, pos, quat, gps, valid, init_pos, init_quat


def as_bytes(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def run_all(B, batch, rules=("reference", "all")):
    """K4 and the fused pipeline under both row rules: name -> array, as the caller gets them"""
    res = {}
    p, q, st = B.ekf_fuse_batch(batch).host_traj_major()
    res["k4.pos"], res["k4.quat"], res["k4.status"] = p, q, st
    for rows in rules:
        out, R, t, s = B.fuse_pipeline_batch(batch, fit_rows=rows)
        p, q, st = out.host_traj_major()
        res[f"{rows}.pos"], res[f"{rows}.quat"], res[f"{rows}.status"] = p, q, st
        res[f"{rows}.R"], res[f"{rows}.t"], res[f"{rows}.s"] = R.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy()
    return res


def with_options(B, opts, fn):
    ctx = B.context()
    defaults = {"tail_scan_stages": 1, "duo_kernel": -1}
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            ctx.set_option(k, defaults[k])


def builds_for(N):
    """(name, trajectories, duo_kernel): the one-wave build, the forced two-wave build where it applies (pipeline, 64 < N <= 640), the big-batch build"""
    r = [("one-wave", NB_SMALL, 0)]
    if 64 < N <= 640:
        r.append(("two-wave", NB_SMALL, 1))
    r.append(("big-batch", NB_BIG, 0))
    return r


def inputs_for(B, N, nb):
    """name -> device batch: the synthetic generator (both variants) and the planted tracks (tiled up to nb from NB_SMALL distinct ones)"""
    host = planted_batch(NB_SMALL, N, 7000 + N)
    reps = (nb + NB_SMALL - 1) // NB_SMALL
    tiled = tuple(np.concatenate([a] * reps, axis=0)[:nb] for a in host)
    return {"synthetic v0": B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=77 + N, variant=0),
            "synthetic v1": B.TrajectoryBatch.synthetic(nb, N, layout=0, seed=78 + N, variant=1),
            "planted": B.TrajectoryBatch.from_host(*tiled, layout=0)}, host


@pytest.mark.parametrize("N", LENGTHS)
def test_sized_tail_scans_give_the_same_bytes(B, N):
    """option 1 against option 0, raw bytes of pos / quat / status (K4) and pos / quat / status / R / t / s (pipeline, both row rules)"""
    total = 0
    for build, nb, duo in builds_for(N):
        batches, _ = inputs_for(B, N, nb)
        for iname, batch in batches.items():
            got = {v: with_options(B, {"tail_scan_stages": v, "duo_kernel": duo}, lambda: run_all(B, batch)) for v in (1, 0)}
            for key in got[0]:
                a, b = as_bytes(got[1][key]), as_bytes(got[0][key])
                assert a.shape == b.shape
                differing = int((a != b).sum())
                total += differing
                print(f"N={N} {build} {iname} {key}: {differing} differing bytes of {a.size}")
                assert differing == 0, (N, build, iname, key, differing)
    assert total == 0


@pytest.mark.parametrize("N", LENGTHS)
def test_sized_tail_scans_against_the_oracle(B, orc, N):
    """the sized path (option 1, the default) against oracle.fuse_batch / oracle.fuse_pipeline_batch: status words equal, positions and
    quaternions inside the tolerances of tests/test_gpu_parity.py -- every build, the planted tracks and the synthetic generator"""
    for build, nb, duo in builds_for(N):
        batches, host = inputs_for(B, N, nb)
        for iname, batch in batches.items():
            if iname == "planted":
                ts, pos, quat, gps, valid, ip, iq = host                  # the oracle runs the NB_SMALL distinct tracks once; the batch tiles them
                sel = np.arange(nb) % NB_SMALL
                ptol, qtol = POS_TOL, Q_TOL
            else:
                h = batch.host_traj_major()
                k = min(nb, NB_SMALL)                                     # a slice of the generator's tracks is enough for the CPU side
                ts, pos, quat, gps, valid, ip, iq = (h[n][:k] for n in ("ts", "pos", "quat", "gps", "valid", "init_pos", "init_quat"))
                sel = None
                ptol, qtol = SYN_POS_TOL, SYN_Q_TOL
            got = with_options(B, {"tail_scan_stages": 1, "duo_kernel": duo}, lambda: run_all(B, batch))
            pick = (lambda a: a[:len(ts)]) if sel is None else (lambda a: a)
            tile = (lambda a: a) if sel is None else (lambda a: a[sel])
            po, qo, sto = orc.fuse_batch(ts, pos, quat, gps, valid, ip, iq)
            p, q, st = pick(got["k4.pos"]), pick(got["k4.quat"]), pick(got["k4.status"])
            ok = np.isfinite(tile(po)).all(axis=(1, 2))
            ep, eq = np.abs(p[ok] - tile(po)[ok]).max(initial=0.0), np.abs(q[ok] - tile(qo)[ok]).max(initial=0.0)
            print(f"N={N} {build} {iname} K4: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, {int((~ok).sum())} non-finite tracks")
            assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, build, iname)
            np.testing.assert_array_equal(st, tile(sto), err_msg=f"N={N} {build} {iname} K4 status")
            assert ep < POS_TOL and eq < Q_TOL, (N, build, iname, ep, eq)
            for rows in ("reference", "all"):
                pr, qr, str_, Rr, tr, sr = orc.fuse_pipeline_batch(ts, pos, quat, gps, valid, fit_rows=rows)
                p, q, st, s = (pick(got[f"{rows}.{n}"]) for n in ("pos", "quat", "status", "s"))
                ok = np.isfinite(tile(pr)).all(axis=(1, 2))
                ep, eq = np.abs(p[ok] - tile(pr)[ok]).max(initial=0.0), np.abs(q[ok] - tile(qr)[ok]).max(initial=0.0)
                es = np.abs(s[ok] - tile(sr)[ok]).max(initial=0.0)
                print(f"N={N} {build} {iname} pipeline/{rows}: max |dp| {ep:.2e} m, max |dq| {eq:.2e}, max |ds| {es:.2e}, {int((~ok).sum())} non-finite tracks")
                assert (np.isfinite(p).all(axis=(1, 2)) == ok).all(), (N, build, iname, rows)
                # (a track whose pose-0 quaternion is invalid has NaN poses on both sides -- SciPy would raise -- and no status the reference
                # defines: as in tests/test_gpu_parity.py the words are compared where the oracle has poses)
                bad = np.nonzero(((st & ~(16 << 8)) != tile(str_)) & ok)[0]
                assert len(bad) == 0, (N, build, iname, rows, bad[:8].tolist(), st[bad[:8]].tolist(), tile(str_)[bad[:8]].tolist())
                assert ep < ptol and eq < qtol and es < S_TOL, (N, build, iname, rows, ep, eq, es)
