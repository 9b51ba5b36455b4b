"""Pose queries: gsf_pose_query_dev / gsf_georef_points_dev against the torch composition a user writes without them (torch.searchsorted +
gathers + lerp + nlerp + rotate, track by track).

Shape: 16 tracks x 4 096 poses, M = 2^24 queries, (a) time-sorted inside each track (the window route), (b) shuffled inside each track (the
general route).  Warm-up, then HIP events on torch's current stream, medians over the repetitions; the library's two routes and the
composition alternate inside one process.  Prints one JSON line per entry: ms, GB/s on the algorithmic bytes (georef 8 + 24 read, 24 + 1
written = 57 B per point; poses 8 read, 56 + 1 written = 65 B per query; no optional output is asked for), the fraction of 8 TB/s, the same
for the composition with the bytes it allocates beyond its inputs and outputs, and max |delta| between the two.
GSF_LIBRARY=... times another build of the library (the form that moved the 24- / 32-byte rows as 16-byte pieces through LDS was measured
this way and retired: tools/experiments/README.md).
usage: python tools/pose_query_timing.py [reps] [log2 M]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gps_optimize_slam_amd import batch as B  # noqa: E402
from gps_optimize_slam_amd import _lib  # noqa: E402

TRACKS, POSES, PEAK = 16, 4096, 8.0e12


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def make(M):
    g = torch.Generator(device="cuda").manual_seed(1)
    f = dict(dtype=torch.float64, device="cuda")
    P = TRACKS * POSES
    ts = (1.3e9 + torch.cumsum(0.08 + 0.06 * torch.rand((TRACKS, POSES), generator=g, **f), dim=1)).reshape(-1)
    pos = torch.tensor([4.5e5, 9.4e6, 120.0], **f) + torch.cumsum(torch.rand((TRACKS, POSES, 3), generator=g, **f), dim=1)
    ang = torch.cumsum(0.05 + 0.1 * torch.rand((TRACKS, POSES), generator=g, **f), dim=1)
    quat = torch.stack((torch.zeros_like(ang), torch.zeros_like(ang), torch.sin(ang / 2), torch.cos(ang / 2)), dim=2)
    offsets = torch.arange(TRACKS + 1, dtype=torch.int64, device="cuda") * POSES
    per = M // TRACKS
    q_offsets = torch.arange(TRACKS + 1, dtype=torch.int64, device="cuda") * per
    t2 = ts.view(TRACKS, POSES)
    u = torch.rand((TRACKS, per), generator=g, **f)
    q_shuffled = (t2[:, :1] + u * (t2[:, -1:] - t2[:, :1])).clamp(t2[:, :1], t2[:, -1:]).contiguous()
    q_sorted = torch.sort(q_shuffled, dim=1).values.contiguous()
    x = 140.0 * (torch.rand((TRACKS * per, 3), generator=g, **f) - 0.5)
    return dict(ts=ts.contiguous(), pos=pos.reshape(P, 3).contiguous(), quat=quat.reshape(P, 4).contiguous(), offsets=offsets, q_offsets=q_offsets,
                sorted=q_sorted.reshape(-1), shuffled=q_shuffled.reshape(-1), x=x, per=per)


def torch_poses(d, q):
    """the composition: per track searchsorted -> gathers -> lerp -> nlerp (ref :94-105 without its degenerate branch)"""
    out_p, out_q = [], []
    for b in range(TRACKS):
        sl, ql = slice(b * POSES, (b + 1) * POSES), slice(b * d["per"], (b + 1) * d["per"])
        t, tau = d["ts"][sl], q[ql]
        i = (torch.searchsorted(t, tau, right=True) - 1).clamp(0, POSES - 2)
        ti, tj = t[i], t[i + 1]
        w = ((tau - ti) / (tj - ti)).unsqueeze(1)
        pi, pj, qi, qj = d["pos"][sl][i], d["pos"][sl][i + 1], d["quat"][sl][i], d["quat"][sl][i + 1]
        qj = torch.where((qi * qj).sum(dim=1, keepdim=True) < 0, -qj, qj)
        qm = (1.0 - w) * qi + w * qj
        out_p.append(pi + w * (pj - pi)); out_q.append(qm / qm.norm(dim=1, keepdim=True))
    return torch.cat(out_p), torch.cat(out_q)


def torch_points(d, q):
    p, qu = torch_poses(d, q)
    u, w = qu[:, :3], qu[:, 3:]
    t = 2.0 * torch.linalg.cross(u, d["x"])
    return p + d["x"] + w * t + torch.linalg.cross(u, t)


def timed(fn, reps, others):
    """median ms of fn over reps, the other callables run in between (alternating)"""
    ev = []
    for _ in range(reps):
        a = _event(); fn(); b = _event()
        ev.append((a, b))
        for o in others:
            o()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main(reps, log2m):
    M = 1 << log2m
    d = make(M)
    args = (d["ts"], d["pos"], d["quat"], d["offsets"])
    lib = {
        ("poses", "sorted"): lambda: B.query_poses_ragged(*args, d["sorted"], d["q_offsets"]),
        ("poses", "shuffled"): lambda: B.query_poses_ragged(*args, d["shuffled"], d["q_offsets"]),
        ("georef", "sorted"): lambda: B.georef_points_ragged(*args, d["sorted"], d["x"], d["q_offsets"]),
        ("georef", "shuffled"): lambda: B.georef_points_ragged(*args, d["shuffled"], d["x"], d["q_offsets"]),
    }
    comp = {"poses": lambda q: torch_poses(d, q), "georef": lambda q: torch_points(d, q)}
    nbytes = {"poses": 65, "georef": 57}
    for entry in ("georef", "poses"):
        for order in ("sorted", "shuffled"):
            ours, q = lib[(entry, order)], d[order]
            theirs = lambda: comp[entry](q)
            for _ in range(2):
                r, c = ours(), theirs()
            torch.cuda.synchronize()
            got = r.xyz if entry == "georef" else r.pos
            want = c if entry == "georef" else c[0]
            diff = float((got - want).abs().max())
            dq = float((r.quat - c[1]).abs().max()) if entry == "poses" else None
            clean = int((r.flags == 0).sum()) + int((r.flags == _lib.Q_EXACT).sum())
            del r, c
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            c = theirs(); torch.cuda.synchronize()
            keep = sum(t.numel() * t.element_size() for t in ((c,) if entry == "georef" else c))
            extra = torch.cuda.max_memory_allocated() - base - keep
            del c
            t_o = timed(ours, reps, (theirs,))
            t_c = timed(theirs, reps, (ours,))
            gbs = lambda ms: M * nbytes[entry] / (ms * 1e-3) / 1e9
            print(json.dumps({"entry": entry, "order": order, "M": M, "tracks": TRACKS, "poses_per_track": POSES, "library": os.path.basename(_lib.library_path()),
                              "ms": round(t_o, 4), "GBps": round(gbs(t_o), 1), "fraction_of_8TBps": round(gbs(t_o) * 1e9 / PEAK, 3),
                              "torch_ms": round(t_c, 4), "torch_GBps": round(gbs(t_c), 1), "torch_fraction_of_8TBps": round(gbs(t_c) * 1e9 / PEAK, 3),
                              "torch_over_library": round(t_c / t_o, 2), "torch_extra_bytes": int(extra), "max_abs_diff_pos_m": diff,
                              "max_abs_diff_quat": dq, "queries_with_a_pose": clean, "reps": reps}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 24)
