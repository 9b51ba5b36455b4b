"""Clock-offset search: the fused entry (gsf_clock_offset_search_dev: B x K workgroups, two numbers written per candidate) against the
composition of the entry points that existed before it, run on the materialised B x K virtual batch -- shift the stamps, gsf_time_align_batch_dev,
gsf_sim3_fit_rows_batch_dev, gsf_sim3_umeyama_batch_dev with the row mask, gsf_apply_sim3_batch_dev, residual reduce.

Two shapes: 1 000 tracks x 271 poses with 90 fixes, and 100 tracks x 1 000 poses with 330 fixes, K = 41 both.  Warm-up, then HIP events on
torch's current stream around every phase, medians over the repetitions; the two routes alternate inside one process.  Prints one JSON line
per shape: times in ms, the ratio, the bytes the composition allocates beyond its inputs, and max |J_fused - J_composition|.
usage: python tools/clock_offset_timing.py [reps]"""
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import clock_offset_ref as ref  # noqa: E402  (the planted-offset generator)
from gps_optimize_slam_amd import batch as B  # noqa: E402
from gps_optimize_slam_amd import _lib  # noqa: E402

GAP, K, TAU0, DTAU = 5.0, 41, -1.0, 0.05


def median_ms(events):
    """events: list over repetitions of [e0, e1, ..., en] -> per-phase medians (n,) and the median of the totals"""
    ph = np.array([[a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])] for ev in events])
    return np.median(ph, axis=0), float(np.median(ph.sum(axis=1)))


def run_shape(Bn, N, ng, reps):
    dev = "cuda"
    tr = ref.make_track(N, ng)
    rng = np.random.default_rng(1)
    f = dict(dtype=torch.float64, device=dev)
    # B tracks: the same path, each with its own SLAM-frame noise (1 mm) so that no two problems are the same numbers
    ts = torch.as_tensor(np.tile(tr["ts"], Bn), **f)
    pos = torch.as_tensor(np.tile(tr["pos"], (Bn, 1)) + rng.normal(scale=1e-3, size=(Bn * N, 3)), **f)
    gps_t = torch.as_tensor(np.tile(tr["gps_t"], Bn), **f)
    gps_p = torch.as_tensor(np.tile(tr["gps_p"], (Bn, 1)), **f)
    so = torch.arange(Bn + 1, dtype=torch.int64, device=dev) * N
    go = torch.arange(Bn + 1, dtype=torch.int64, device=dev) * ng
    L, ctx = _lib.load(), B.context()
    p = B._p

    # (the batch form: max_fixes is known to the host, so the call reads nothing back)
    log = SimpleNamespace(ts=ts, pos=pos, slam_offsets=so, gps_t=gps_t, gps_offsets=go, max_fixes=ng)
    projected = SimpleNamespace(gps_utm=gps_p, gps_keep=None)

    def fused():
        return B.estimate_clock_offset(log, tau0=TAU0, dtau=DTAU, K=K, run=projected)

    # ---- the virtual batch of the composition: problem (b, k) is track b * K + k (set-up, not timed; its bytes are counted)
    V = Bn * K
    tau = (TAU0 + torch.arange(K, **f) * DTAU).repeat(Bn)                         # (V,)
    v_ts = ts.view(Bn, 1, N).expand(Bn, K, N).reshape(-1).contiguous()
    v_pos = pos.view(Bn, 1, N, 3).expand(Bn, K, N, 3).reshape(-1, 3).contiguous()
    v_quat = torch.zeros((V * N, 4), **f); v_quat[:, 3] = 1.0
    v_gp = gps_p.view(Bn, 1, ng, 3).expand(Bn, K, ng, 3).reshape(-1, 3).contiguous()
    v_gt0 = gps_t.view(Bn, 1, ng).expand(Bn, K, ng)
    v_so = torch.arange(V + 1, dtype=torch.int64, device=dev) * N
    v_go = torch.arange(V + 1, dtype=torch.int64, device=dev) * ng
    aligned, valid = torch.empty((V * N, 3), **f), torch.empty((V * N,), dtype=torch.uint8, device=dev)
    extra = sum(t.numel() * t.element_size() for t in (v_ts, v_pos, v_quat, v_gp, aligned, valid))
    extra += V * ng * 8 + V * N * (1 + 24 + 32) + V * (72 + 24 + 8 + 4 + 4 + 4)      # shifted stamps, row mask, applied poses, fits and counts

    def composition(ev=None):
        mark = (lambda: ev.append(_event())) if ev is not None else (lambda: None)
        mark()
        v_gt = (v_gt0 + tau.view(Bn, K, 1)).reshape(-1)
        mark()
        _lib.check(L.gsf_time_align_batch_dev(ctx.handle, p(v_ts), p(v_so), p(v_gt), p(v_gp), p(v_go), V, ng, GAP, p(aligned), p(valid), None))
        mark()
        mask, n_rows, _ = B.sim3_fit_rows_batch(v_ts, aligned, valid, offsets=v_so)
        mark()
        R, t, s, _ = B.sim3_umeyama_batch(v_pos, aligned, v_so, mask)
        mark()
        po, _, _ = B.apply_sim3_batch(v_pos, v_quat, v_so, R, t, s)
        mark()
        d2 = torch.where(mask.bool(), ((aligned - po) ** 2).sum(dim=1), torch.zeros((), **f))
        J = torch.sqrt(d2.view(V, N).sum(dim=1) / n_rows.clamp(min=1))
        mark()
        return J.view(Bn, K)

    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    for _ in range(3):                                                            # warm-up of both routes at this shape
        rf, Jc = fused(), composition()
    torch.cuda.synchronize()
    diff = float((rf.J - Jc).abs().max())
    ev_f, ev_c = [], []
    for _ in range(reps):                                                         # alternating
        e = [_event()]; fused(); e.append(_event()); ev_f.append(e)
        e = []; composition(e); ev_c.append(e)
    torch.cuda.synchronize()
    _, t_f = median_ms(ev_f)
    ph, t_c = median_ms(ev_c)
    names = ("shift", "time_align", "sim3_fit_rows", "sim3_umeyama", "apply_sim3", "residual_reduce")
    return {"shape": f"{Bn} x {N} poses, {ng} fixes, K = {K}", "fused_ms": round(t_f, 4), "composition_ms": round(t_c, 4),
            "composition_over_fused": round(t_c / t_f, 3), "composition_phases_ms": {n: round(float(v), 4) for n, v in zip(names, ph)},
            "composition_extra_bytes": int(extra), "fused_output_bytes": int(Bn * K * 12), "max_abs_J_diff_m": diff, "reps": reps}


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    for shape in ((1000, 271, 90), (100, 1000, 330)):
        print(json.dumps(run_shape(*shape, reps)), flush=True)
