"""CPU tier of the streaming fusion (gsf_stream_*; contract in include/gsf.h, "streaming fusion").

gsf_stream_core.hpp -- the state's pack / unpack, the ring as EkfTraj's Out, the capacity rule, the n_final / revised_from bookkeeping and
the per-track body of an append -- is compiled with gsf_ekf_core.hpp by g++ into a stand-alone program (tests/host_harness_stream.cpp) that
runs a stream through a list of calls and plays its consumer.  Here: one segment is the oracle's filter; how a track is cut changes no bit;
rows below n_final stay; the capacity rule refuses exactly what it says; a ring that has wrapped gives the bits of one that has not; the
same program once more under the address and undefined-behaviour sanitizers; and the bindings without a device.
tests/test_stream.py holds the kernel to the same rows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gate_ref as R
import stream_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ST_HAD_OUTAGE, ST_RTS_APPLIED, ST_SHARP_TURN = 1, 2, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. one segment is the oracle's filter
@pytest.mark.parametrize("cfg_name", ["default", "steps5"])
def test_one_segment_agrees_with_the_oracle(cfg_name):
    """every edge track in one append against oracle.apply_ekf_correction_aligned: 1e-9 m / 1e-12, the gates of tests/test_oracle_golden.py"""
    from oracle import oracle as orc
    ref = S.reference(cfg_name)
    res = ref["res"]
    worst_p = worst_q = 0.0
    seen = 0
    for b, (name, t) in enumerate(zip(ref["names"], ref["tracks"])):
        n = len(t[0])
        rep = res["rep"][0, b]
        assert rep[0] == n, name
        if n == 0:
            assert rep[1] == 0 and rep[2] == 0 and rep[3] == 0 and res["mirror"][b].shape[0] == 0
            continue
        po, qo, st = orc.apply_ekf_correction_aligned(*t[:7], ref["cfg"], return_status=True)
        m = res["mirror"][b]
        np.testing.assert_array_equal(bits(m[:, 0]), bits(t[0]), err_msg=name)              # the ring's stamps
        np.testing.assert_array_equal(bits(m[:, 1:]), bits(res["rows"][0][b][:, :7]), err_msg=name)   # the call's rows are the ring's
        worst_p = max(worst_p, float(np.abs(m[:, 1:4] - po).max())); worst_q = max(worst_q, float(np.abs(m[:, 4:8] - qo).max()))
        assert int(rep[3]) == int(st), (name, int(rep[3]), int(st))
        open_ = bool(int(st) & S.ST_ENDED_IN_OUTAGE)
        assert rep[1] == (S.first_outage_open(t[4]) if open_ else n), name
        assert rep[2] == 0, name                                           # everything this call wrote is new
        seen |= int(st)
        cov = res["rows"][0][b][:, 7:]
        np.testing.assert_array_equal(cov[0], np.asarray(ref["cfg"]["ekf"]["initial_cov_diag"], dtype=np.float64))
        assert (cov > 0).all()
    print(f"{cfg_name}: one segment vs the oracle over {len(ref['tracks'])} tracks: |dp| {worst_p:.2e} m, |dq| {worst_q:.2e}")
    assert worst_p < 1e-9 and worst_q < 1e-12
    assert seen & ST_RTS_APPLIED and seen & ST_SHARP_TURN and seen & S.ST_ENDED_IN_OUTAGE


# ------------------------------------------------------------------------------------------------ 2. + 3. split invariance and finality
def _check_against_whole(ref, res, cuts, tag):
    whole = ref["res"]
    assert res["violations"] == 0, tag                                     # no row below a reported n_final ever changed its bits
    for b, name in enumerate(ref["names"]):
        n = len(ref["tracks"][b][0])
        np.testing.assert_array_equal(bits(res["mirror"][b]), bits(whole["mirror"][b]), err_msg=f"{tag} {name}: final rows")
        last = res["rep"][-1, b]
        np.testing.assert_array_equal(last[[0, 1, 3]], whole["rep"][-1, b][[0, 1, 3]], err_msg=f"{tag} {name}: n_total, n_final, status")
        np.testing.assert_array_equal(bits(S.concat_rows(res, b)[:, 7:]), bits(whole["rows"][0][b][:, 7:]), err_msg=f"{tag} {name}: cov_out")
        n_before = 0
        for c in range(res["rep"].shape[0]):
            nt, nf, rf, st, mc, same = res["rep"][c, b]
            m = cuts[b][c] if c < len(cuts[b]) else 0
            assert nt == n_before + m and 0 <= nf <= nt and rf <= n_before, (tag, name, c)
            if m == 0:
                assert same == 1 and rf == n_before and mc == -1, (tag, name, c)      # the no-op
            if mc >= 0:
                assert rf == mc, (tag, name, c, rf, mc)                    # a back-pass ran: revised_from IS the smallest changed index
            else:
                assert rf == n_before, (tag, name, c, rf)
            n_before = int(nt)
        assert n_before == n


@pytest.mark.parametrize("cfg_name", ["default", "steps5"])
def test_split_invariance_and_finality(cfg_name):
    """whole track; one pose per call; a cut at pose 1; at the first pose of an outage, inside it, on the recovery pose and one pose after
    it; 20 seeded random cuts per track with empty segments: the final ring, n_final, status and the concatenated cov_out, bit for bit"""
    ref = S.reference(cfg_name)
    pats = [S.cut_patterns(t, seed=b) for b, t in enumerate(ref["tracks"])]
    names = sorted({k for p in pats for k in p})
    assert sum(k.startswith("random_") for k in names) == 20 and "cut_on_recovery" in names and "cut_inside_outage" in names
    n_back = 0
    for k in names:
        cuts = [p.get(k, p["whole"]) for p in pats]
        res = S.run(ref["tracks"], S.calls_from_cuts(cuts), 256, ref["cfg"])
        _check_against_whole(ref, res, cuts, k)
        n_back += int((res["rep"][:, :, 4] >= 0).sum())
    print(f"{cfg_name}: {len(names)} cut patterns x {len(ref['tracks'])} tracks; {n_back} calls whose back-pass rewrote rows of an earlier call")
    assert n_back > 50


# ------------------------------------------------------------------------------------------------ 4. capacity
def _capacity_case(cfg):
    """three tracks; track 1 has a 12-pose outage (poses 20..31, recovery at 32) and is fed in segments of 8"""
    tracks = [R.synthetic_track(48, 40, cfg), R.withhold(R.synthetic_track(48, 41, cfg), list(range(20, 32))), R.withhold(R.synthetic_track(48, 42, cfg), [9, 10])]
    cuts = [[8] * 6] * 3
    return tracks, cuts


def test_capacity_rule():
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    tracks, cuts = _capacity_case(cfg)
    calls = S.calls_from_cuts(cuts)
    # the largest (open outage + segment) any call of track 1 meets: the call of poses 32..39 finds poses 20..31 open: 12 + 8
    need = 12 + 8
    big = S.run(tracks, calls, 256, cfg)
    ok = S.run(tracks, calls, need, cfg)
    assert not (ok["rep"][:, :, 3].astype(np.int64) & S.STREAM_FULL).any() and ok["violations"] == 0
    for b in range(3):
        np.testing.assert_array_equal(bits(ok["mirror"][b]), bits(big["mirror"][b]))
        np.testing.assert_array_equal(bits(S.concat_rows(ok, b)), bits(S.concat_rows(big, b)))
    # one less: exactly the offending call is refused, and only for that track
    tight = S.run(tracks, calls + [(S.REOPEN, [0, 1, 0])] + [(S.APPEND, [0, 8, 0])] * 6, need - 1, cfg)
    full = (tight["rep"][:6, :, 3].astype(np.int64) & S.STREAM_FULL) != 0
    want = np.zeros((6, 3), dtype=bool)
    want[4:, 1] = True                                                      # the call of poses 32..39, and (nothing having changed) the one after it
    np.testing.assert_array_equal(full, want)
    for c in (4, 5):
        rep = tight["rep"][c, 1]
        assert rep[5] == 1, "state and ring bytes of a refused track must be unchanged"
        assert rep[0] == 32 and rep[1] == 20 and rep[2] == 32 and int(rep[3]) & S.ST_ENDED_IN_OUTAGE
        assert np.isnan(tight["rows"][c][1]).all() and tight["rows"][c][1].shape == (8, 14)
    for b in (0, 2):                                                        # the neighbours proceed, with the bits they have without the refusal
        np.testing.assert_array_equal(bits(S.concat_rows(tight, b)[:48]), bits(S.concat_rows(big, b)))
    # re-sending after a reopen works: the re-opened track runs from pose 0 again -- and is refused at the same call again, as it must be
    assert tight["rep"][6, 1, 0] == -1 and tight["rep"][6, 0, 5] == 1 and tight["rep"][6, 2, 5] == 1 and tight["rep"][6, 1, 5] == 0
    again = tight["rep"][7:, 1]
    np.testing.assert_array_equal(again[:4, 0], [8, 16, 24, 32])
    np.testing.assert_array_equal(bits(np.concatenate([tight["rows"][7 + c][1] for c in range(4)])), bits(S.concat_rows(big, 1)[:32]))
    assert int(again[4, 3]) & S.STREAM_FULL
    # ... and with segments that fit (4 poses: 12 + 4 <= 19) the same ring takes the whole track, with the bits of the large ring
    fit = S.run(tracks, S.calls_from_cuts([[4] * 12] * 3), need - 1, cfg)
    assert not (fit["rep"][:, :, 3].astype(np.int64) & S.STREAM_FULL).any()
    np.testing.assert_array_equal(bits(S.concat_rows(fit, 1)), bits(S.concat_rows(big, 1)))


def test_wrapped_ring_gives_the_bits_of_a_large_one():
    """cap = 16, a 200-pose track with outages under 8 poses, segments of up to 8 poses: the ring wraps twelve times"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    out = [i for a in (5, 30, 61, 90, 127, 160, 190) for i in range(a, a + 7)]
    tracks = [R.withhold(R.synthetic_track(200, 50, cfg), out), R.withhold(R.synthetic_track(200, 51, cfg, turn=True), out[:14]), R.synthetic_track(130, 52, cfg)]
    rng = np.random.default_rng(77)
    cuts = []
    for t in tracks:
        n, seg = len(t[0]), []
        while sum(seg) < n:
            seg.append(int(min(rng.integers(0, 9), n - sum(seg))))
        cuts.append(seg)
    calls = S.calls_from_cuts(cuts)
    small, big = S.run(tracks, calls, 16, cfg), S.run(tracks, calls, 256, cfg)
    assert small["violations"] == 0 and big["violations"] == 0
    assert not (small["rep"][:, :, 3].astype(np.int64) & (S.STREAM_FULL | S.STREAM_BAD_STATE)).any()
    np.testing.assert_array_equal(small["rep"][:, :, :5], big["rep"][:, :, :5])
    for b in range(3):
        np.testing.assert_array_equal(bits(small["mirror"][b]), bits(big["mirror"][b]))
        np.testing.assert_array_equal(bits(S.concat_rows(small, b)), bits(S.concat_rows(big, b)))
    assert int(big["rep"][-1, 0, 3]) & ST_RTS_APPLIED


# ------------------------------------------------------------------------------------------------ 5. under the sanitizers
def test_harness_under_sanitizers():
    """the same stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into python): cuts at every
    outage edge, a wrapped ring, a refusal, a re-open and a state of another version"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    exe = S.build(("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "_san")
    ref = S.reference("default")
    pats = [S.cut_patterns(t, seed=b, n_random=2) for b, t in enumerate(ref["tracks"])]
    for k in ("cut_all_four", "random_0", "one_pose_per_call"):
        cuts = [p.get(k, p["whole"]) for p in pats]
        res = S.run(ref["tracks"], S.calls_from_cuts(cuts), 256, ref["cfg"], exe=exe)
        _check_against_whole(ref, res, cuts, k + " (sanitizers)")
    tracks, cuts = _capacity_case(E.CONFIG)
    calls = S.calls_from_cuts(cuts)
    res = S.run(tracks, calls + [(S.REOPEN, [0, 1, 0]), (S.CORRUPT, [1, 0, 0])] + [(S.APPEND, [0, 8, 0])] * 6, 19, E.CONFIG, exe=exe)
    assert int(res["rep"][4, 1, 3]) & S.STREAM_FULL and int(res["rep"][8, 0, 3]) == S.STREAM_BAD_STATE


# ------------------------------------------------------------------------------------------------ 6. the surface, without a device
def test_wrong_layout_version_is_refused():
    from gps_optimize_slam_amd import ekfgpsslam as E
    tracks, cuts = _capacity_case(E.CONFIG)
    calls = S.calls_from_cuts(cuts)
    res = S.run(tracks, calls[:2] + [(S.CORRUPT, [0, 0, 1])] + calls[2:], 64, E.CONFIG)
    for c in range(3, 7):
        rep = res["rep"][c, 2]
        assert int(rep[3]) == S.STREAM_BAD_STATE and rep[5] == 1 and (rep[:3] == 0).all()      # refused, nothing written
        assert np.isnan(res["rows"][c][2]).all()
        assert int(res["rep"][c, 0, 3]) == 0 and res["rep"][c, 0, 0] == 8 * (c - 0)            # the neighbours proceed
    # ... and a ring of another size than the state was opened for is the same refusal (the harness opens for its own cap; FusionStream checks both)
    import torch
    from gps_optimize_slam_amd import batch as GB, _lib
    B, cap = 3, 8
    d = dict(version=_lib.STREAM_LAYOUT_VERSION, B=B, cap=cap, config=None, state_f64=torch.zeros((_lib.STREAM_F64, B), dtype=torch.float64),
             state_i64=torch.zeros((_lib.STREAM_I64, B), dtype=torch.int64), ring_t=torch.zeros((B, cap), dtype=torch.float64),
             ring_pos=torch.zeros((B, cap, 3), dtype=torch.float64), ring_quat=torch.zeros((B, cap, 4), dtype=torch.float64))
    d["state_i64"][0] = _lib.STREAM_LAYOUT_VERSION
    d["state_i64"][1] = cap
    for bad in (dict(version=2), dict(cap=9), dict(state_f64=torch.zeros((21, B), dtype=torch.float64)), dict(state_i64=d["state_i64"].to(torch.int32))):
        with pytest.raises(ValueError):
            GB.FusionStream.from_state({**d, **bad}, device="cpu")
    wrong = d["state_i64"].clone()
    wrong[0, 1] = 7
    with pytest.raises(ValueError, match="layout version"):
        GB.FusionStream.from_state({**d, "state_i64": wrong}, device="cpu")
    with pytest.raises(ValueError):
        GB.FusionStream(3, 0, None, None, device="cpu")


def test_entries_are_declared_bound_and_exported(tmp_path):
    from gps_optimize_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsf.h")).read()
    n_args = {"gsf_stream_open": 8, "gsf_stream_append": 22, "gsf_stream_gather": 12}
    for base, n in n_args.items():
        assert f"{base}(" not in hdr and base not in _lib.SIGNATURES      # device forms only: the ring stays on the device, a binding uploads its segment
        for name in (base + "_dev",):
            m = re.search(rf"GSF_API int {name}\(([^;]*)\);", hdr)
            assert m, f"{name} is not declared in include/gsf.h"
            params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
            res, args = _lib.SIGNATURES[name]
            assert res is C.c_int and len(args) == len(params) == n, name
            for p, a in zip(params, args):
                want = C.POINTER(_lib.EkfConfig) if "gsf_ekf_config" in p else (C.c_void_p if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32}[p.split()[0]])
                assert a is want, (name, p, a)
    # the published constants == what gcc makes of the core header's structs == the binding's
    core = os.path.join(ROOT, "gps_optimize_slam_amd", "csrc")
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include "gsf.h"\n#include "gsf_stream_core.hpp"\nint main() {\n'
                   'printf("%zu %zu %d %d %d %d %d %d %d\\n", sizeof(gsf::StreamF64) / sizeof(double), sizeof(gsf::StreamI64) / sizeof(int64_t), GSF_STREAM_F64, GSF_STREAM_I64,\n'
                   '       GSF_STREAM_LAYOUT_VERSION, (int)gsf::STREAM_LAYOUT_VERSION, GSF_STREAM_FULL == gsf::STREAM_FULL, GSF_STREAM_BAD_STATE == gsf::STREAM_BAD_STATE,\n'
                   '       GSF_ST_ENDED_IN_OUTAGE == gsf::ST_ENDED_IN_OUTAGE);\nreturn 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + core, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [_lib.STREAM_F64, _lib.STREAM_I64, _lib.STREAM_F64, _lib.STREAM_I64, _lib.STREAM_LAYOUT_VERSION, _lib.STREAM_LAYOUT_VERSION, 1, 1, 1], got
    assert (_lib.STREAM_FULL, _lib.STREAM_BAD_STATE) == (S.STREAM_FULL, S.STREAM_BAD_STATE) == (256, 512)
    assert re.search(r"#define GSF_STREAM_FULL 256\b", hdr) and re.search(r"#define GSF_STREAM_BAD_STATE 512\b", hdr)
    assert re.search(r"#define GSF_ABI_VERSION 1\b", hdr)
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    L = C.CDLL(_lib.library_path())
    for base in n_args:
        assert hasattr(L, base + "_dev")


def test_argument_errors_need_no_device():
    import torch
    from gps_optimize_slam_amd import batch as GB
    s = GB.FusionStream(2, 8, None, None, device="cpu")                     # (tensors only: nothing is launched)
    f = lambda *sh: torch.zeros(sh, dtype=torch.float64)
    with pytest.raises(ValueError):
        s.append(f(3), f(3, 3), f(3, 4), f(3, 3), torch.zeros(3, dtype=torch.uint8), torch.tensor([0, 1, 3]))      # host tensors
    with pytest.raises(ValueError):
        s.rows([0, 0], [1, 2, 3])
    d = s.state_dict()
    assert set(d) == {"version", "B", "cap", "config", "state_f64", "state_i64", "ring_t", "ring_pos", "ring_quat"}
    assert d["state_f64"].shape == (22, 2) and d["state_i64"].shape == (6, 2) and d["ring_quat"].shape == (2, 8, 4)
