"""Every host-pointer entry of the C ABI against its device form, word for word (no tolerance): the host form declares its arrays to
gsf::Staging, which lays them out, packs, uploads, calls the `_dev` form and copies back; the device form gets the same inputs in
buffers of the test's own.  Every output is compared, generator states and status words included.

Shapes are the smallest that exercise the layout: tracks / sets of 0, 5 and 70 rows (an empty one, one that crosses a 64-row chunk), a
batch whose total is 0, logs of 0 and 40 fixes, every optional array once present and once NULL, every NULL-allowed required output
once NULL.  Outputs of both forms start as the same sentinel words (the host form's arena through "poison_workspaces"), so a byte a
kernel leaves alone compares equal and an early return (B = 0, N = 0) must leave the sentinel in the caller's arrays.

TABLE is complete by construction: every function of _lib.SIGNATURES that takes host arrays is in it or in GOLDEN_COVERED, the
entries without a device twin, which tests/test_gpu_parity.py compares with goldens through the drop-in."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORD = 0x5A                                   # "poison_workspaces" word: the bytes 5A 00 00 00 00 00 00 00 repeated
LENS, EMPTY = (0, 5, 70), (0, 0, 0)
f8, i8, i4, u1, u4 = np.float64, np.int64, np.int32, np.uint8, np.uint32

# no device twin: where each one is compared with the reference's recorded results (all through gps_optimize_slam_amd.ekfgpsslam)
GOLDEN_COVERED = {
    "gsf_relative_pose_batch": "tests/test_gpu_parity.py::test_relative_pose_and_nlerp",
    "gsf_quaternion_nlerp_batch": "tests/test_gpu_parity.py::test_relative_pose_and_nlerp",
    "gsf_is_sharp_turn_batch": "tests/test_gpu_parity.py::test_sharp_turn_function",
    "gsf_rts_smoother_segment_batch": "tests/test_gpu_parity.py::test_rts_smoother_segment_function",
    "gsf_ekf_process_step": "tests/test_gpu_parity.py::test_extended_kalman_filter_class",
    "gsf_sim3_ransac_mt_batch": "tests/test_gpu_parity.py::test_ransac_cases",
}
# functions of the table that take no host arrays (context plumbing, the communicator)
NO_ARRAYS = {"gsf_version", "gsf_abi_version", "gsf_last_error", "gsf_device_count", "gsf_create", "gsf_create_on_stream", "gsf_destroy",
             "gsf_synchronize", "gsf_trim", "gsf_set_option", "gsf_set_sim3_rows", "gsf_timer_start", "gsf_timer_stop", "gsf_comm_unique_id",
             "gsf_comm_rccl_version", "gsf_comm_init_rank", "gsf_comm_destroy", "gsf_allgather_poses"}


def sentinel(nbytes):
    return np.resize(np.array([WORD, 0, 0, 0, 0, 0, 0, 0], u1), nbytes)


class Arr:
    """one array argument: the host form gets a numpy array, the device form a buffer of its own with the same bytes"""

    def __init__(self, role, data, host_null=False):
        self.role, self.data, self.host_null, self.h, self.d = role, np.ascontiguousarray(data), host_null, None, None

    def start(self):
        return sentinel(self.data.nbytes) if self.role == "out" else self.data.reshape(-1).view(u1)

    def host(self):
        self.h = self.start().copy()
        return None if self.host_null else C.c_void_p(self.h.ctypes.data)

    def dev(self):
        import torch
        self.d = torch.zeros(self.data.nbytes + 8, dtype=torch.uint8, device="cuda")       # (never NULL, also for 0 elements)
        self.d[:self.data.nbytes] = torch.as_tensor(self.start().copy())
        return C.c_void_p(self.d.data_ptr())

    def dev_bytes(self):
        return self.d[:self.data.nbytes].cpu().numpy()


def I(a, dtype=None):
    return Arr("in", np.asarray(a, dtype))


def O(shape, dtype, host_null=False):
    return Arr("out", np.empty(shape, dtype), host_null)


def IO(a):
    return Arr("io", a)


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(i8)


class Inputs:
    """the fixed inputs every case draws from, built once"""

    def __init__(self):
        from gps_optimize_slam_amd import _lib
        from gps_optimize_slam_amd import ekfgpsslam as E
        rng = np.random.default_rng(29)
        self.ekf = _lib.EkfConfig.from_config(E.CONFIG)
        self.run = _lib.RunConfig.from_config(E.CONFIG)
        self.gtf = _lib.PrefilterConfig.from_config(E.CONFIG["ground_truth_gps_filtering"])
        self.sim3 = E.CONFIG["sim3_ransac"]
        self.gap = float(E.CONFIG["time_alignment"]["max_gps_gap_threshold"])
        P = 3 * 70                                                    # rows for every case: ragged ones take the first offsets[-1]
        self.ts = np.tile(100.0 + 0.1 * np.arange(70), 3)
        self.pos = np.cumsum(rng.normal(size=(P, 3)) * 0.3, axis=0)
        q = rng.normal(size=(P, 4))
        self.quat = q / np.linalg.norm(q, axis=1, keepdims=True)
        c, s = np.cos(0.3), np.sin(0.3)
        self.gps = 1.02 * self.pos @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + np.array([4.5e5, 5.4e6, 110.0]) + rng.normal(size=(P, 3)) * 0.05
        self.valid = (rng.random(P) < 0.85).astype(u1)
        self.R, self.t, self.s = np.tile(np.eye(3).reshape(9), (3, 1)), rng.normal(size=(3, 3)), rng.uniform(0.5, 2.0, 3)
        self.idx = np.stack([np.stack([rng.choice(max(n, 4), 4, replace=False) for _ in range(8)]) for n in LENS]).astype(i4)
        # GNSS logs of 40 fixes over the tracks' seven seconds: stamps, WGS84 rows, UTM-like rows
        self.log_t = np.tile(np.sort(rng.uniform(99.5, 107.5, 40)), 3)
        self.llh = np.column_stack((49.0 + rng.uniform(0, 1e-3, 120), 8.4 + rng.uniform(0, 1e-3, 120), rng.uniform(100, 120, 120)))
        self.utm = np.array([4.5e5, 5.4e6, 110.0]) + np.cumsum(rng.normal(size=(120, 3)) * 0.4, axis=0)
        self.keep = (rng.random(120) < 0.9).astype(u1)
        q_t = rng.uniform(99.0, 108.0, 75)
        self.q_t = np.concatenate([np.sort(q_t[:5]), np.sort(q_t[5:])])             # query sets of 5, 70 and 0 stamps, each sorted
        self.x = rng.normal(size=(75, 3))
        self.states = np.stack([_lib_seed(k) for k in (5, 6, 7)])

    def rows(self, lens):
        n = int(sum(lens))
        pick = np.concatenate([np.arange(b * 70, b * 70 + k) for b, k in enumerate(lens)]).astype(int) if n else np.zeros(0, int)
        return {k: np.ascontiguousarray(getattr(self, k)[pick]) for k in ("ts", "pos", "quat", "gps", "valid")}, offsets(lens), n


def _lib_seed(seed):
    """NumPy's legacy generator state as the entries take it: 624 key words + the position"""
    st = np.random.RandomState(seed).get_state()
    return np.concatenate([st[1].astype(u4), np.array([st[2]], u4)])


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import _lib
    ctx = _lib.Context(0)
    yield _lib, _lib.load(), ctx, Inputs()
    ctx.close()


# ------------------------------------------------------------------------------------------------ the table
# name -> function(inputs, variant) -> (host arguments, device function, device arguments).  variant: "full" (every optional array
# present), "null" (every optional array and every NULL-allowed required output NULL), "empty" (a batch whose total is 0).
def ragged(v, variant):
    return v.rows(EMPTY if variant == "empty" else LENS)


def case_utm(inverse):
    def build(v, variant):
        n = 0 if variant == "empty" else 75
        a, b = (v.utm[:n, 0], v.utm[:n, 1]) if inverse else (v.llh[:n, 0], v.llh[:n, 1])
        a, b, oa, ob = I(a, f8), I(b, f8), O(n, f8), O(n, f8)
        dev = [a, b, I([0, n], i8), I([32], i4), I([0], i4), 1, oa, ob]
        return [a, b, n, 32, 0, oa, ob], "gsf_utm_inverse_batch_dev" if inverse else "gsf_utm_forward_batch_dev", dev
    return build


def case_umeyama_batch(v, variant):
    r, o, n = ragged(v, variant)
    a = [I(r["pos"]), I(r["gps"]), I(r["valid"]) if variant == "full" else None, I(o), 3, O((3, 9), f8), O((3, 3), f8), O(3, f8), O(3, i4)]
    return a, "gsf_sim3_umeyama_batch_dev", a


def case_ransac_batch(v, variant):
    r, o, n = ragged(v, variant)
    src, dst, off, idx = I(r["pos"]), I(r["gps"]), I(o), I(np.minimum(v.idx, 3) if n == 0 else v.idx)
    outs = [O((3, 9), f8), O((3, 3), f8), O(3, f8), O(3, i4), O(n, u1), O(3, i4)]
    return [src, dst, off, 3, idx, 8, 4, 2.0, 4] + outs, "gsf_sim3_ransac_batch_rows_dev", [src, dst, off, n, 3, idx, 8, 4, 2.0, 4] + outs


def case_apply_sim3(v, variant):
    r, o, n = ragged(v, variant)
    a = [I(r["pos"]), I(r["quat"]), I(o), 3, I(v.R), I(v.t), I(v.s), O((n, 3), f8), O((n, 4), f8), O(3, i4, host_null=variant == "null")]
    return a, "gsf_apply_sim3_batch_dev", a


def dense(v):
    return [I(v.ts), I(v.pos), I(v.quat), I(v.gps), I(v.valid)]


def case_ekf_fuse_batch(v, variant):
    a = [0] + dense(v) + [I(v.pos[::70]), I(v.quat[::70]), C.byref(v.ekf), 3, 70, O((210, 3), f8), O((210, 4), f8), O(3, i4, host_null=variant == "null")]
    return a, "gsf_ekf_fuse_batch_dev", a


def case_fuse_pipeline_batch(v, variant):
    a = [0] + dense(v) + [C.byref(v.ekf), 3, 70, O((3, 9), f8), O((3, 3), f8), O(3, f8), O((210, 3), f8), O((210, 4), f8), O(3, i4)]
    return a, "gsf_fuse_pipeline_batch_dev", a


def case_fit_rows(v, variant):
    if variant == "null":                                             # no offsets: the dense form; no fixes array, no status
        a = [I(v.ts), None, I(v.valid), None, 3, 70, 4, v.gap, 180.0, O(210, u1), O(3, i4), None]
    else:
        r, o, n = ragged(v, variant)
        a = [I(r["ts"]), I(r["gps"]), I(r["valid"]), I(o), 3, 70, 4, v.gap, 180.0, O(n, u1), O(3, i4), O(3, i4)]
    return a, "gsf_sim3_fit_rows_batch_dev", a


def case_robust_batch(v, variant):
    m = v.sim3
    a = dense(v) + [C.byref(v.ekf), 3, 70, int(m["min_samples"]), float(m["residual_threshold"]), 24, int(m["min_inliers_needed"]), IO(v.states),
                    O((3, 9), f8), O((3, 3), f8), O(3, f8), O((210, 3), f8), O((210, 4), f8), O(3, i4), O(3, i4), O(210, u1) if variant == "full" else None]
    return a, "gsf_fuse_pipeline_robust_batch_dev", a


def case_ekf_fuse_ragged(v, variant):
    r, o, n = ragged(v, variant)
    a = [I(r[k]) for k in ("ts", "pos", "quat", "gps", "valid")] + [I(o), I(v.pos[::70]), I(v.quat[::70]), C.byref(v.ekf), 3, O((n, 3), f8), O((n, 4), f8), O(3, i4)]
    return a, "gsf_ekf_fuse_ragged_dev", a


def case_fuse_pipeline_ragged(v, variant):
    r, o, n = ragged(v, variant)
    a = [I(r[k]) for k in ("ts", "pos", "quat", "gps", "valid")] + [I(o), C.byref(v.ekf), 3, O((3, 9), f8), O((3, 3), f8), O(3, f8), O((n, 3), f8), O((n, 4), f8),
                                                                     O(3, i4)]
    return a, "gsf_fuse_pipeline_ragged_dev", a


def case_cov_ragged(v, variant):
    r, o, n = ragged(v, variant)
    full = variant != "null"
    a = [I(r[k]) for k in ("ts", "quat", "gps", "valid")] + [I(o), I([0, 0, 8], i4) if full else None, C.byref(v.ekf), 3, O((n, 7), f8) if full else None,
                                                             O((n, 7), f8), O(n, u1) if full else None, O(3, i4) if full else None]
    return a, "gsf_ekf_cov_ragged_dev", a


def case_windows(v, variant):
    a = [I(v.pos), I(v.gps), I(v.valid) if variant == "full" else None, 3, 70, O((3, 9), f8), O((3, 3), f8), O(3, f8), O(3, i4)]
    return a, "gsf_sim3_umeyama_windows_dev", a


def logs(variant):
    """logs of 40, 0 and 40 fixes (total 0: none at all): row offsets into the 120 rows"""
    return offsets((0, 0, 0) if variant == "empty" else (40, 0, 40))


def case_enu(v, variant):
    o = logs(variant); n = int(o[-1])
    a = [I(v.llh[:n, 0]), I(v.llh[:n, 1]), I(v.llh[:n, 2]), I(o), I(v.llh[:3]), 3, O(n, f8), O(n, f8), O(n, f8)]
    return a, "gsf_geodetic_to_enu_batch_dev", a


def case_rows_to_utm(v, variant):
    o = logs(variant); n = int(o[-1])
    a = [I(v.llh[:n]), I(o), 3, O((n, 3), f8), O(3, i4), O(3, i4)]
    return a, "gsf_gps_rows_to_utm_batch_dev", a


def case_ransac_poly(v, variant):
    r, o, n = ragged(v, variant)
    y = 3.0 + 0.5 * r["ts"] + r["pos"][:, 0] * 0.1 if n else np.zeros(0)
    a = [I(r["ts"]), I(y), I(o), 3, I(np.minimum(v.idx, 3) if n == 0 else v.idx), 8, 4, 2, 1.0, 0.99, O(n, u1), O(3, i4), O(3, i4), O(3, i4)]
    return a, "gsf_ransac_poly_batch_dev", a


def case_prefilter_chain(v, variant):
    o = logs(variant); n = int(o[-1])
    wins = np.array([[0, 40], [5, 35]] * 2, i4) if n else np.zeros((0, 2), i4)          # two windows per non-empty log
    wo = offsets((2, 0, 2) if n else (0, 0, 0))
    a = [I(v.log_t[:n]), I(v.utm[:n]), I(o), 3, I(wins), I(wo), 40, 20, 4, 2, 1.0, 0.99, IO(v.states), O(n, u1), O(len(wins), i4), O(3, i4)]
    return a, "gsf_gps_prefilter_chain_dev", a


def case_time_align(v, variant):
    r, so, ns = v.rows(LENS)
    go = logs(variant); ng = int(go[-1])
    head = [I(r["ts"]), I(so), I(v.log_t[:ng]), I(v.utm[:ng]), I(go), 3]
    outs = [O((ns, 3), f8), O(ns, u1), O(3, i4, host_null=variant == "null")]
    return head + [v.gap] + outs, "gsf_time_align_batch_dev", head + [max(2, 40 if ng else 0), v.gap] + outs


def case_clock_offset(v, variant):
    r, so, ns = v.rows(LENS)
    go = logs(variant); ng = int(go[-1])
    full, K = variant != "null", 5
    head = [I(r["ts"]), I(r["pos"]), I(so), I(v.log_t[:ng]), I(v.utm[:ng]), I(v.keep[:ng]) if full else None, I(go), 3]
    tail = [I([0.0, 0.1, -0.1], f8) if full else None, 0.05, K, v.gap, 4, 1e-3, O((3, K), f8), O((3, K), i4) if full else None, O(3, i4), O(3, f8), O(3, f8),
            O((3, 9), f8) if full else None, O((3, 3), f8) if full else None, O(3, f8) if full else None, O(3, i4)]
    return head + tail, "gsf_clock_offset_search_dev", head + [40 if ng else 0] + tail


def case_eval_errors(v, variant):
    a = [I(v.ts), I(v.pos), I(v.gps), I(v.valid), 3, 70, 1.0, O((3, 4), f8), O(210, f8, host_null=variant == "null")]
    return a, "gsf_eval_errors_batch_dev", a


def queries(v, variant):
    r, o, n = ragged(v, variant)
    if n == 0:                                                       # no poses at all: one unread zero row stands in, as in the host form
        r = {"ts": np.zeros(1), "pos": np.zeros(3), "quat": np.zeros(4)}
    full = variant == "full"
    head = [I(r["ts"]), I(r["pos"]), I(r["quat"]), I(o), I([0, 0, 8], i4) if full else None, I(np.arange(n) % 16, u1) if full and n else None, 3]
    return head, I(v.q_t), I(offsets((5, 70, 0))), full


def case_pose_query(v, variant):
    head, qt, qo, full = queries(v, variant)
    a = head + [qt, qo, 75, 0.5, O((75, 3), f8), O((75, 4), f8), O(75, u1), O(75, i4) if full else None, O(75, u1) if full else None, O(3, i4)]
    return a, "gsf_pose_query_dev", a


def case_georef(v, variant):
    head, qt, qo, full = queries(v, variant)
    ext = [I(v.quat[:3]), I(v.t), I(v.s)] if full else [None, None, None]
    a = head + [qt, qo, 75, 0.5, I(v.x)] + ext + [O((75, 3), f8), O(75, u1), O(75, i4) if full else None, O(75, u1) if full else None, O(3, i4)]
    return a, "gsf_georef_points_dev", a


def case_run_batch(v, variant):
    go = logs(variant); T = int(go[-1])
    full = variant == "full"
    ins = [I(v.ts), I(v.pos), I(v.quat), 3, 70, I(v.log_t[:T]), I(v.llh[:T]), I(go)]
    outs = [IO(v.states), O((3, 9), f8), O((3, 3), f8), O(3, f8), O((210, 3), f8), O((210, 4), f8), O(3, i4), O(3, i4), O(3, i4), O(3, i4), O((T, 3), f8), O(T, u1),
            O((210, 3), f8), O(210, u1), O((210, 3), f8) if full else None, O((3, 3, 4), f8), O(3, i4), O(210, u1) if full else None, O((3, 2), i4) if full else None]
    return ins + [C.byref(v.run)] + outs, "gsf_run_fusion_batch_dev", ins + [T, 40 if T else 0, C.byref(v.run)] + outs


def case_run_ragged(v, variant):
    r, so, P = ragged(v, variant)
    full = variant == "full"
    go = logs("full"); T = int(go[-1])
    to = offsets((0, 40, 40)) if full else None; Tg = 80 if full else 0                  # "null": no ground-truth leg
    gt_in = [I(v.log_t[:Tg]), I(v.llh[40:40 + Tg]), I(to)] if full else [None, None, None]
    gt_out = [O(3, i4), O(3, i4), O((Tg, 3), f8), O(Tg, u1), O((P, 3), f8), O(P, u1)] if full else [None] * 6
    slam, gps = [I(r["ts"]), I(r["pos"]), I(r["quat"]), I(so), 3], [I(v.log_t[:T]), I(v.llh[:T]), I(go)]
    outs = [IO(v.states), O((3, 9), f8), O((3, 3), f8), O(3, f8), O((P, 3), f8), O((P, 4), f8), O(3, i4), O(3, i4), O(3, i4), O(3, i4), O((T, 3), f8), O(T, u1),
            O((P, 3), f8), O(P, u1), O((P, 3), f8) if full else None] + gt_out + [O((2, 3, 3, 4), f8), O(3, i4) if full else None, O(3, i4),
                                                                                 O(P, u1) if full else None, O((3, 2), i4) if full else None]
    cfgs = [C.byref(v.run), C.byref(v.gtf)]
    longest = int(np.diff(so).max())
    return (slam + gps + gt_in + cfgs + outs, "gsf_run_fusion_ragged_dev",
            slam + [P, longest] + gps + [T, 40] + gt_in + [Tg, 40 if full else 0] + cfgs + outs)


RAGGED3 = ("full", "null", "empty")
TABLE = {
    "gsf_utm_forward": (case_utm(False), ("full",)), "gsf_utm_inverse": (case_utm(True), ("full",)),
    "gsf_sim3_umeyama_batch": (case_umeyama_batch, RAGGED3), "gsf_sim3_ransac_batch": (case_ransac_batch, ("full", "empty")),
    "gsf_apply_sim3_batch": (case_apply_sim3, RAGGED3), "gsf_ekf_fuse_batch": (case_ekf_fuse_batch, ("full", "null")),
    "gsf_fuse_pipeline_batch": (case_fuse_pipeline_batch, ("full",)), "gsf_sim3_fit_rows_batch": (case_fit_rows, RAGGED3),
    "gsf_fuse_pipeline_robust_batch": (case_robust_batch, ("full", "null")), "gsf_ekf_fuse_ragged": (case_ekf_fuse_ragged, ("full", "empty")),
    "gsf_fuse_pipeline_ragged": (case_fuse_pipeline_ragged, ("full", "empty")), "gsf_ekf_cov_ragged": (case_cov_ragged, RAGGED3),
    "gsf_sim3_umeyama_windows": (case_windows, ("full", "null")), "gsf_geodetic_to_enu_batch": (case_enu, ("full", "empty")),
    "gsf_gps_rows_to_utm_batch": (case_rows_to_utm, ("full", "empty")), "gsf_ransac_poly_batch": (case_ransac_poly, ("full", "empty")),
    "gsf_gps_prefilter_chain": (case_prefilter_chain, ("full", "empty")), "gsf_time_align_batch": (case_time_align, RAGGED3),
    "gsf_clock_offset_search": (case_clock_offset, RAGGED3), "gsf_eval_errors_batch": (case_eval_errors, ("full", "null")),
    "gsf_pose_query": (case_pose_query, RAGGED3), "gsf_georef_points": (case_georef, RAGGED3),
    "gsf_run_fusion_batch": (case_run_batch, RAGGED3), "gsf_run_fusion_ragged": (case_run_ragged, RAGGED3),
}


def conv(args, mode):
    return [getattr(a, mode)() if isinstance(a, Arr) else a for a in args]


def host_call(env, ctx, name, hargs):
    _lib, L = env[0], env[1]
    ctx.set_option("poison_workspaces", WORD)                          # what the arena holds now (and after it grows) is the sentinel
    _lib.check(getattr(L, name)(ctx.handle, *conv(hargs, "host")))
    return [a for a in hargs if isinstance(a, Arr) and a.role != "in" and not a.host_null]


def both_forms(env, ctx, name, variant):
    import torch
    _lib, L, _, v = env
    hargs, dname, dargs = TABLE[name][0](v, variant)
    outs = host_call(env, ctx, name, hargs)
    dconv = conv(dargs, "dev")
    torch.cuda.synchronize()
    _lib.check(getattr(L, dname)(ctx.handle, *dconv))
    ctx.synchronize()
    assert outs
    for k, a in enumerate(outs):
        got, want = a.h, a.dev_bytes()
        assert (got == want).all(), f"{name}[{variant}]: output {k} ({a.data.dtype}{a.data.shape}) differs from {dname} in {int((got != want).sum())} bytes"
    return [a.h.copy() for a in outs]


def test_table_is_complete(env):
    _lib = env[0]
    host_entries = {n for n in _lib.SIGNATURES if not n.endswith("_dev")} - NO_ARRAYS
    assert host_entries == set(TABLE) | set(GOLDEN_COVERED) and not set(TABLE) & set(GOLDEN_COVERED)
    for name, (build, variants) in TABLE.items():                      # every case fills every argument of both signatures
        for variant in variants:
            hargs, dname, dargs = build(env[3], variant)
            assert dname.endswith("_dev") and len(hargs) + 1 == len(_lib.SIGNATURES[name][1]) and len(dargs) + 1 == len(_lib.SIGNATURES[dname][1]), (name, variant)


@pytest.mark.parametrize("name,variant", [(n, var) for n, (_, variants) in TABLE.items() for var in variants])
def test_host_form_equals_device_form(env, name, variant):
    both_forms(env, env[2], name, variant)


# B = 0 / N = 0 / n = 0: the scalar arguments that make each entry return before it touches the device
EARLY = {
    "gsf_utm_forward": {2: 0}, "gsf_utm_inverse": {2: 0}, "gsf_sim3_umeyama_batch": {4: 0}, "gsf_sim3_ransac_batch": {3: 0}, "gsf_apply_sim3_batch": {3: 0},
    "gsf_ekf_fuse_batch": {10: 0}, "gsf_fuse_pipeline_batch": {8: 0}, "gsf_sim3_fit_rows_batch": {4: 0}, "gsf_fuse_pipeline_robust_batch": {7: 0},
    "gsf_ekf_fuse_ragged": {9: 0}, "gsf_fuse_pipeline_ragged": {7: 0}, "gsf_ekf_cov_ragged": {7: 0}, "gsf_sim3_umeyama_windows": {3: 0},
    "gsf_geodetic_to_enu_batch": {5: 0}, "gsf_gps_rows_to_utm_batch": {2: 0}, "gsf_ransac_poly_batch": {3: 0}, "gsf_gps_prefilter_chain": {3: 0},
    "gsf_time_align_batch": {5: 0}, "gsf_clock_offset_search": {7: 0}, "gsf_eval_errors_batch": {5: 0}, "gsf_pose_query": {9: 0}, "gsf_georef_points": {9: 0},
    "gsf_run_fusion_batch": {4: 0}, "gsf_run_fusion_ragged": {4: 0},
}


@pytest.mark.parametrize("name", list(TABLE))
def test_early_return_leaves_the_outputs_alone(env, name):
    hargs, _, _ = TABLE[name][0](env[3], "full")
    for k, val in EARLY[name].items():
        assert isinstance(hargs[k], int) and hargs[k] > 0, (name, k, hargs[k])       # the slot is the count it is meant to be
        hargs[k] = val
    for a in host_call(env, env[2], name, hargs):
        assert (a.h == a.start()).all(), f"{name}: an output was written on an early return"


def utm_large(env, ctx, n=1_200_000):
    """gsf_utm_forward on n points: 4 arrays of 8 n bytes, 38 MB laid out at n = 1.2 M -- above Staging's 32 MiB, the direct route"""
    import torch
    _lib, L = env[0], env[1]
    rng = np.random.default_rng(3)
    lat, lon = I(rng.uniform(-80, 84, n)), I(rng.uniform(6, 12, n))
    e, nn = O(n, f8), O(n, f8)
    outs = host_call(env, ctx, "gsf_utm_forward", [lat, lon, n, 32, 0, e, nn])
    dconv = conv([lat, lon, I([0, n], i8), I([32], i4), I([0], i4), 1, e, nn], "dev")
    torch.cuda.synchronize()
    _lib.check(L.gsf_utm_forward_batch_dev(ctx.handle, *dconv))
    ctx.synchronize()
    for a in outs:
        assert (a.h == a.dev_bytes()).all(), "direct route differs from gsf_utm_forward_batch_dev"


SMALL = [("gsf_fuse_pipeline_robust_batch", "full"), ("gsf_pose_query", "full"), ("gsf_run_fusion_ragged", "full")]


def test_direct_route_then_reuse_and_trim(env):
    """one call above 32 MiB equals the device form; the small calls after it (the arena has grown), and after a gsf_trim and a second
    large call, give the words a fresh context gives"""
    _lib = env[0]
    fresh = _lib.Context(0)
    try:
        first = [both_forms(env, fresh, n, var) for n, var in SMALL]
    finally:
        fresh.close()
    ctx = env[2]
    utm_large(env, ctx)
    for stage in ("after growth", "after trim", "after trim and growth"):
        if stage == "after trim":
            ctx.trim()
        if stage == "after trim and growth":
            utm_large(env, ctx)
        for (n, var), want in zip(SMALL, first):
            got = both_forms(env, ctx, n, var)
            assert len(got) == len(want) and all((g == w).all() for g, w in zip(got, want)), f"{n} {stage}: differs from a fresh context"
