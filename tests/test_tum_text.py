"""Step 7 of main_process_gui (EKFGPSSLAM.py:1085-1104) on the device: utm_to_wgs84_ragged (gsf_utm_to_wgs84_rows_dev), tum_text_ragged
(gsf_tum_text_dev) and save_fusion_ragged.

Against: np.savetxt on the same float64 rows, byte for byte (random ragged batches with 0- and 1-row tracks, a skipped track, a track the
device leaves to the host); the drop-in's utm_to_wgs84 / UtmProjector, bit for bit; the drop-in's writers on the same device outputs and
ekfgpsslam.run_fusion(..., out_path_utm=) on six file triples."""
import ctypes as C
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UTM_FMT = ["%.6f"] + ["%.6f"] * 3 + ["%.8f"] * 4
WGS_FMT = ["%.6f"] + ["%.8f", "%.8f", "%.3f"] + ["%.8f"] * 4
HEADERS = {"utm": "timestamp x y z qx qy qz qw (UTM)", "wgs84": "timestamp lon lat alt qx qy qz qw (WGS84)"}


@pytest.fixture(scope="module")
def B():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def savetxt_bytes(rows, fmt):
    f = io.BytesIO()
    np.savetxt(f, rows, fmt=UTM_FMT if fmt == "utm" else WGS_FMT, header=HEADERS[fmt], comments="")
    return f.getvalue()


def random_batch(rng, lens):
    """ragged rows of run-like magnitudes, with random bit patterns, signed zeros, NaN and inf sprinkled in"""
    P = int(sum(lens))
    ts = rng.uniform(1.2e9, 1.8e9, P)
    xyz = np.column_stack([rng.uniform(1e5, 9e5, P), rng.uniform(-1e7, 1e7, P), rng.uniform(-400, 9000, P)])
    quat = rng.normal(size=(P, 4))
    rows = np.column_stack([ts, xyz, quat])
    pick = rng.random(rows.shape) < 0.03
    bits = (rng.integers(0, 1 << 52, int(pick.sum()), dtype=np.uint64) | (rng.integers(0, 1086, int(pick.sum()), dtype=np.uint64) << np.uint64(52))
            | (rng.integers(0, 2, int(pick.sum()), dtype=np.uint64) << np.uint64(63)))
    rows[pick] = bits.view(np.float64)
    rows[rng.random(rows.shape) < 0.003] = -0.0
    if P > 10:
        rows[3, 1], rows[4, 5], rows[5, 7], rows[6, 0], rows[7, 2] = np.nan, np.inf, -np.inf, 9.9999995, 0.0078125
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    return rows, offs


def to_dev(rows, offs):
    import torch
    f = dict(dtype=torch.float64, device="cuda")
    return (torch.tensor(rows[:, 0].copy(), **f), torch.tensor(rows[:, 1:4].copy(), **f), torch.tensor(rows[:, 4:8].copy(), **f),
            torch.tensor(offs, device="cuda"))


@pytest.mark.parametrize("fmt", ["utm", "wgs84"])
def test_text_equals_savetxt(B, fmt):
    import torch
    from gps_optimize_slam_amd import _lib
    rng = np.random.default_rng(11 if fmt == "utm" else 12)
    lens = [0, 1, 271, 5, 0, 1000, 64, 65, 1, 130, 3, 777]
    rows, offs = random_batch(rng, lens)
    rows[offs[9] + 2, 3] = 1e300                                      # track 9: a finite value above 2^63 -> the host writes it
    ts, xyz, quat, o = to_dev(rows, offs)
    nb = len(lens)
    status = torch.zeros(nb, dtype=torch.int32, device="cuda")
    status[3] = 8                                                     # track 3 failed: skipped
    texts, st = B.tum_text_ragged(ts, xyz, quat, o, fmt=fmt, run_status=status)
    assert list(st) == [0, 0, 0, 1, 0, 0, 0, 0, 0, 2, 0, 0]
    for b in range(nb):
        if b == 3:
            assert texts[b] is None
        else:
            assert texts[b] == savetxt_bytes(rows[offs[b]:offs[b + 1]], fmt), b
    # chunks: the tracks from b0 on, through offsets + b0
    texts2, st2 = B.tum_text_ragged(ts, xyz, quat, o[5:], fmt=fmt, run_status=status[5:])
    assert texts2 == texts[5:] and list(st2) == list(st[5:])
    # the raw entry: every byte of [0, text_offsets[B]) and nothing past it (canary bytes survive)
    L, h = _lib.load(), B.context().handle
    form = _lib.TUM_UTM if fmt == "utm" else _lib.TUM_WGS84
    toff = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    tst = torch.empty(nb, dtype=torch.int32, device="cuda")
    P = int(ts.numel())
    _lib.check(L.gsf_tum_text_dev(h, form, C.c_void_p(ts.data_ptr()), C.c_void_p(xyz.data_ptr()), C.c_void_p(quat.data_ptr()),
                                  C.c_void_p(o.data_ptr()), None, nb, P, C.c_void_p(toff.data_ptr()), C.c_void_p(tst.data_ptr()), None))
    total = int(toff[-1])
    buf = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(L.gsf_tum_text_dev(h, form, C.c_void_p(ts.data_ptr()), C.c_void_p(xyz.data_ptr()), C.c_void_p(quat.data_ptr()),
                                  C.c_void_p(o.data_ptr()), None, nb, P, C.c_void_p(toff.data_ptr()), C.c_void_p(tst.data_ptr()),
                                  C.c_void_p(buf.data_ptr())))
    torch.cuda.synchronize()
    hb, ho = buf.cpu().numpy(), toff.cpu().numpy()
    assert (hb[total:] == 0xA5).all()
    for b in range(nb):
        if b != 9:
            assert hb[ho[b]:ho[b + 1]].tobytes() == savetxt_bytes(rows[offs[b]:offs[b + 1]], fmt), b
    assert ho[10] == ho[9]


def test_wgs84_rows_bit_identical_to_the_drop_in(B):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    rng = np.random.default_rng(5)
    zones = [1, 32, 60, 1, 32, 60, 17, 44]
    south = [0, 0, 0, 1, 1, 1, 0, 1]
    lens = [300, 271, 1, 0, 500, 129, 64, 200]
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    P = int(offs[-1])
    pos = np.column_stack([rng.uniform(2e5, 8e5, P), rng.uniform(1e5, 9.3e6, P), rng.uniform(-100, 4000, P)])
    status = np.zeros(len(lens), np.int32)
    status[6] = 1
    zs = np.array(zones, np.int32)
    zs[6] = -123456                                                   # a failed track's zone / hemisphere hold garbage
    so = np.array(south, np.int32)
    so[6] = 77
    t = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    out = B.utm_to_wgs84_ragged(t(pos, torch.float64), t(offs, torch.int64), t(zs, torch.int32), t(so, torch.int32),
                                t(status, torch.int32)).cpu().numpy()
    for b in range(len(lens)):
        sl = slice(offs[b], offs[b + 1])
        if b == 6:
            assert np.isnan(out[sl]).all()
            continue
        want = E.utm_to_wgs84(pos[sl], E.UtmProjector(zones[b], south[b]))
        np.testing.assert_array_equal(out[sl].view(np.uint64), want.view(np.uint64), err_msg=str(b))
    # without run_status every track is converted
    out2 = B.utm_to_wgs84_ragged(t(pos, torch.float64), t(offs, torch.int64), t(np.array(zones, np.int32), torch.int32),
                                 t(np.array(south, np.int32), torch.int32)).cpu().numpy()
    sl = slice(offs[6], offs[7])
    np.testing.assert_array_equal(out2[sl].view(np.uint64), E.utm_to_wgs84(pos[sl], E.UtmProjector(17, 0)).view(np.uint64))


def six_triples(golden, d):
    g, k, s6 = golden("c1_combined.npz"), golden("kat_bundled.npz"), golden("step6_gt.npz")
    fill = lambda n: (np.full(n, 4), np.full(n, 5))
    slam_p, gps_p, gt_p = [], [], []
    prim = np.column_stack((g["gps_t_raw"], g["lat"], g["lon"], g["alt"], *fill(len(g["lat"]))))
    grnd = np.column_stack((s6["gt_t_raw"], s6["gt_lat"], s6["gt_lon"], s6["gt_alt"], *fill(len(s6["gt_lat"]))))
    for j, cut in enumerate((271, 240, 200, 180, 160, 120)):
        sf, gf, tf = d / f"traj{j}.txt", d / f"gps{j}.txt", d / f"gt{j}.txt"
        np.savetxt(sf, np.column_stack((k["ts"], k["pos"], k["quat"]))[:cut], fmt="%.18e")
        np.savetxt(gf, prim[:min(len(prim), cut + 8 - j)], fmt="%.18e", delimiter="," if j % 2 else " ")
        np.savetxt(tf, grnd[:min(len(grnd), cut - 10 + 3 * j)], fmt="%.18e")
        slam_p.append(str(sf)); gps_p.append(str(gf)); gt_p.append(str(tf))
    return slam_p, gps_p, gt_p


def test_files_to_files(B, golden, tmp_path):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    slam_p, gps_p, gt_p = six_triples(golden, tmp_path)
    rb = B.RaggedGeodeticBatch.from_files(slam_p, gps_p, gt_p)
    seeds = [3, 4, 5, 6, 7, 8]
    r = B.run_fusion_ragged(rb, B.mt19937_seed(seeds), E.CONFIG, early_exit=False)
    dev_dir, ref_dir, host_dir = tmp_path / "dev", tmp_path / "ref", tmp_path / "host"
    for d in (dev_dir, ref_dir, host_dir):
        d.mkdir()
    names = [B.corrected_utm_name(p) for p in slam_p]
    assert names == [f"traj{j}_corrected_utm.txt" for j in range(6)]
    wrote = B.save_fusion_ragged(rb, r, [str(dev_dir / n) for n in names])
    torch.cuda.synchronize()
    so = rb.slam_offsets.cpu().numpy()
    ts, pos, quat = rb.ts.cpu().numpy(), r.fused.pos.cpu().numpy(), r.fused.quat.cpu().numpy()
    zone, south = r.zone.cpu().numpy(), r.south.cpu().numpy()
    for j in range(6):
        assert int(r.run_status[j]) == 0
        utm, wgs = dev_dir / names[j], dev_dir / names[j].replace("_utm.txt", "_wgs84.txt")
        assert wrote[j] == (str(utm), str(wgs))
        sl = slice(so[j], so[j + 1])
        # the drop-in's writers on the same device outputs: byte for byte
        hu, hw = host_dir / names[j], host_dir / E.wgs84_path(names[j])
        E.save_tum_utm(str(hu), ts[sl], pos[sl], quat[sl])
        E.save_tum_wgs84(str(hw), ts[sl], E.utm_to_wgs84(pos[sl], E.UtmProjector(int(zone[j]), bool(south[j]))), quat[sl])
        assert utm.read_bytes() == hu.read_bytes(), j
        assert wgs.read_bytes() == hw.read_bytes(), j
        # the drop-in run: same names, headers, line counts and stamps; other fields within one unit of the last printed digit
        np.random.seed(seeds[j])
        E.run_fusion(slam_p[j], gps_p[j], out_path_utm=str(ref_dir / names[j]), gt_gps_path=gt_p[j])
        for mine, prec in ((utm, [6] * 4 + [8] * 4), (wgs, [6, 8, 8, 3] + [8] * 4)):
            ref = ref_dir / mine.name
            assert ref.exists(), ref
            a, b = mine.read_text().splitlines(), ref.read_text().splitlines()
            assert a[0] == b[0] and len(a) == len(b) == so[j + 1] - so[j] + 1
            va, vb = np.array([l.split() for l in a[1:]]), np.array([l.split() for l in b[1:]])
            np.testing.assert_array_equal(va[:, 0], vb[:, 0])
            fa, fb = va.astype(float), vb.astype(float)
            for c in range(1, 8):
                assert np.abs(fa[:, c] - fb[:, c]).max() <= 1.001 * 10.0 ** -prec[c], (j, mine.name, c)
    assert sorted(os.listdir(dev_dir)) == sorted(os.listdir(ref_dir))


def test_failed_track_and_projected_input(B, golden, tmp_path):
    import torch
    from gps_optimize_slam_amd import ekfgpsslam as E
    slam_p, gps_p, gt_p = six_triples(golden, tmp_path)
    # track 1's log has no usable fix (lat = lon = 0 are dropped by the loader, ref :259): its run fails, no file is written for it
    raw = np.loadtxt(gps_p[1], delimiter=",")
    raw[:, 1:3] = 0.0
    np.savetxt(gps_p[1], raw, fmt="%.18e", delimiter=",")
    rb = B.RaggedGeodeticBatch.from_files(slam_p[:3], gps_p[:3])
    r = B.run_fusion_ragged(rb, B.mt19937_seed([3, 4, 5]), E.CONFIG)
    st = r.run_status.cpu().numpy()
    assert st[1] != 0 and st[0] == 0 and st[2] == 0
    out = tmp_path / "out"
    out.mkdir()
    paths = [str(out / f"t{j}_corrected_utm.txt") for j in range(3)]
    paths[2] = None                                                   # the user declined to save track 2 (:1086-1090)
    wrote = B.save_fusion_ragged(rb, r, paths)
    assert wrote == [(paths[0], paths[0].replace("_utm.txt", "_wgs84.txt")), (), ()]
    assert sorted(os.listdir(out)) == ["t0_corrected_utm.txt", "t0_corrected_wgs84.txt"]
    # projected input (no projector, :1096): the UTM file only
    r.zone = r.south = None
    out2 = tmp_path / "out2"
    out2.mkdir()
    wrote = B.save_fusion_ragged(rb, r, [str(out2 / "a.txt"), str(out2 / "b.txt"), str(out2 / "c")])
    assert wrote == [(str(out2 / "a.txt"),), (), (str(out2 / "c"),)]
    assert sorted(os.listdir(out2)) == ["a.txt", "c"]
    assert (out2 / "a.txt").read_bytes() == (out / "t0_corrected_utm.txt").read_bytes()
    torch.cuda.synchronize()
