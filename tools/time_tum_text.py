"""Step 7's text on the device (gsf_tum_text_dev) against np.savetxt on the same rows, same host.

Device side, with HIP events on torch's stream: the size call and the write call per format (GSF_TUM_UTM, GSF_TUM_WGS84) and the copy of the
text into pinned host memory.  Host side: np.savetxt with the reference's fmt lists (EKFGPSSLAM.py:1091-1092, :1098-1101) into a file under
the temp dir -- all rows at C2, a stated sample of the large shape.  Shapes: C2 = 1 000 x 271 and 100 000 x 1 000 (the copy and np.savetxt are
taken at C2 and on the sample only: the large shape's text is ~10 GB per format).  Bytes/s count 64 B read per row and pass plus the text
written; per-kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script.
usage: python tools/time_tum_text.py [--c2-only] [--no-host] [--reps R]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gps_optimize_slam_amd import _lib, batch as B  # noqa: E402
from gps_optimize_slam_amd import ekfgpsslam as E  # noqa: E402

HBM_BPS = 8.0e12


def rows_on_device(nb, n, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = nb * n
    f = dict(dtype=torch.float64, device="cuda")
    ts = 1.6e9 + torch.arange(P, **f) % n * 0.1 + torch.rand(P, generator=g, **f) * 1e-3
    xyz = torch.rand((P, 3), generator=g, **f) * torch.tensor([6e5, 5e6, 500.0], **f) + torch.tensor([2e5, 4e6, -50.0], **f)
    quat = torch.randn((P, 4), generator=g, **f)
    quat /= quat.norm(dim=1, keepdim=True)
    offsets = torch.arange(nb + 1, dtype=torch.int64, device="cuda") * n
    zone = torch.full((nb,), 32, dtype=torch.int32, device="cuda")
    south = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    return ts, xyz, quat, offsets, zone, south


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        s.record(); fn(); e.record(); e.synchronize()
        best.append(s.elapsed_time(e))
    return float(np.median(best)), float(min(best))


def device_side(nb, n, reps, d2h):
    ts, xyz, quat, offsets, zone, south = rows_on_device(nb, n)
    P = nb * n
    lla = B.utm_to_wgs84_ragged(xyz, offsets, zone, south)
    L, h = _lib.load(), B.context().handle
    out = {"shape": [nb, n], "rows": P}
    p = B._p
    for name, form, cols in (("utm", _lib.TUM_UTM, xyz), ("wgs84", _lib.TUM_WGS84, lla)):
        toff = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
        st = torch.empty(nb, dtype=torch.int32, device="cuda")
        size = lambda: _lib.check(L.gsf_tum_text_dev(h, form, p(ts), p(cols), p(quat), p(offsets), None, nb, P, p(toff), p(st), None))
        size()
        torch.cuda.synchronize()
        total = int(toff[-1])
        assert int((st != 0).sum()) == 0
        text = torch.empty(total, dtype=torch.uint8, device="cuda")
        write = lambda: _lib.check(L.gsf_tum_text_dev(h, form, p(ts), p(cols), p(quat), p(offsets), None, nb, P, p(toff), p(st), p(text)))
        ms_size, best_size = timed(size, reps)
        ms_write, best_write = timed(write, reps)
        r = {"text_bytes": total, "bytes_per_row": total / P, "size_ms": ms_size, "size_ms_best": best_size, "write_ms": ms_write,
             "write_ms_best": best_write,
             "size_GBps": 64.0 * P / (ms_size * 1e-3) / 1e9, "write_GBps": (64.0 * P + total) / (ms_write * 1e-3) / 1e9}
        r["write_frac_of_8TBps"] = r["write_GBps"] * 1e9 / HBM_BPS
        if d2h:
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            r["d2h_ms"], _ = timed(lambda: host.copy_(text, non_blocking=True), reps)
            r["d2h_GBps"] = total / (r["d2h_ms"] * 1e-3) / 1e9
            r["device_route_ms"] = ms_size + ms_write + r["d2h_ms"]
            if name == "utm":                                             # the device text is np.savetxt's, checked on a few tracks
                hb, ho = host.numpy(), toff.cpu().numpy()
                for b in (0, nb // 2, nb - 1):
                    sl = slice(b * n, (b + 1) * n)
                    f = tempfile.TemporaryFile()
                    E.save_tum_utm(f, ts[sl].cpu().numpy(), xyz[sl].cpu().numpy(), quat[sl].cpu().numpy())
                    f.seek(0)
                    assert f.read() == hb[ho[b]:ho[b + 1]].tobytes(), b
        out[name] = r
        del text
    out["wgs84_rows_ms"], _ = timed(lambda: B.utm_to_wgs84_ragged(xyz, offsets, zone, south), reps)
    return out, (ts, xyz, quat, lla)


def host_side(arrs, rows):
    ts, xyz, quat, lla = (a[:rows].cpu().numpy() for a in arrs)
    res = {"rows": rows}
    with tempfile.TemporaryDirectory() as d:
        for name, writer, cols in (("utm", E.save_tum_utm, xyz), ("wgs84", E.save_tum_wgs84, lla)):
            best = []
            for _ in range(2):
                t0 = time.perf_counter()
                writer(os.path.join(d, f"{name}.txt"), ts, cols, quat)
                best.append(time.perf_counter() - t0)
            res[f"{name}_s"] = min(best)
            res[f"{name}_rows_per_s"] = rows / min(best)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=200_000, help="rows of the large shape np.savetxt writes (extrapolated linearly)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    c2, arrs = device_side(1000, 271, a.reps, d2h=True)
    res["c2"] = c2
    if not a.no_host:
        hs = host_side(arrs, 1000 * 271)
        res["c2"]["np_savetxt"] = hs
        dev_ms = c2["utm"]["device_route_ms"] + c2["wgs84"]["device_route_ms"]
        res["c2"]["speedup_both_formats"] = (hs["utm_s"] + hs["wgs84_s"]) * 1e3 / dev_ms
    del arrs
    torch.cuda.empty_cache()
    if not a.c2_only:
        big, arrs = device_side(100_000, 1000, max(3, a.reps // 4), d2h=False)
        res["large"] = big
        if not a.no_host:
            hs = host_side(arrs, a.sample)
            hs["extrapolated_s_per_format"] = {k: 1e8 * hs[f"{k}_s"] / a.sample for k in ("utm", "wgs84")}
            res["large"]["np_savetxt_sample"] = hs
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
