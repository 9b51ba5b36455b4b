"""GPU tier of the streaming fusion (gsf_stream_*; batch.FusionStream, ekfgpsslam.FusionSession).

The kernel is held to the rows of the stand-alone host harness (tests/stream_ref.py; the CPU tier holds that one to the oracle), to its own
bits under every way of cutting a track, to batch.ekf_fuse_ragged / ekf_covariance_ragged on the concatenated tracks, and to the contract's
bookkeeping: n_final, revised_from, refusals, the checkpoint, and independence of whatever the buffers held before."""
import numpy as np
import pytest

import gate_ref as R
import hygiene
import stream_ref as S

pytestmark = pytest.mark.gpu

POS_TOL, Q_TOL, VAR_RTOL = 1e-7, 1e-9, 1e-10          # the gates of tests/test_gpu_parity.py and tests/test_cov_gpu.py
ST_RTS_APPLIED, ST_SHARP_TURN = 2, 4


@pytest.fixture(scope="module")
def GB():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gps_optimize_slam_amd import batch
    return batch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class DeviceTracks:
    """the flat arrays of a list of tracks on the device, and the segment tensors of one call"""

    def __init__(self, tracks):
        import torch
        self.f = S.flat(tracks)
        self.B = len(tracks)
        self.cursor = np.zeros(self.B, dtype=np.int64)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        self.dev = {k: d(self.f[k]) for k in ("ts", "pos", "quat", "gps", "valid", "init_pos", "init_quat", "offsets")}

    def segment(self, counts, advance=True):
        import torch
        counts = np.asarray(counts, dtype=np.int64)
        idx = np.concatenate([np.arange(c, dtype=np.int64) + self.f["offsets"][b] + self.cursor[b] for b, c in enumerate(counts)]) if counts.sum() else np.empty(0, np.int64)
        so = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if advance:
            self.cursor += counts
        i = torch.as_tensor(idx).cuda()
        return [self.dev[k][i].contiguous() for k in ("ts", "pos", "quat", "gps", "valid")] + [torch.as_tensor(so).cuda()]


def run_device(GB, tracks, calls, cap, cfg, mirror=False, stream=None):
    """the calls of stream_ref.run on a FusionStream -> the same dict (rep columns 0..3, and 4 / violations when mirror=True)"""
    import torch
    dt = DeviceTracks(tracks)
    B = dt.B
    s = stream or GB.FusionStream(B, cap, dt.dev["init_pos"], dt.dev["init_quat"], config=cfg)
    rep, rows = np.full((len(calls), B, 6), -1.0), []
    hist = [np.empty((0, 8)) for _ in range(B)]
    final = np.zeros(B, dtype=np.int64)
    violations = 0
    for c, (typ, v) in enumerate(calls):
        if typ == S.REOPEN:
            s.reopen(np.asarray(v, dtype=np.uint8), dt.dev["init_pos"], dt.dev["init_quat"])
            for b in np.flatnonzero(v):
                dt.cursor[b] = 0; hist[b] = np.empty((0, 8)); final[b] = 0
            rows.append([np.empty((0, 14))] * B)
            continue
        n_before = s.n_total.cpu().numpy().copy()
        seg = dt.segment(v, advance=False)
        st = s.append(*seg)
        so = seg[5].cpu().numpy()
        out = np.concatenate([st.pos.cpu().numpy(), st.quat.cpu().numpy(), st.cov.cpu().numpy()], axis=1)
        rep[c, :, 0], rep[c, :, 1], rep[c, :, 2], rep[c, :, 3] = st.n_total.cpu().numpy(), st.n_final.cpu().numpy(), st.revised_from.cpu().numpy(), st.status.cpu().numpy()
        taken = (rep[c, :, 3].astype(np.int64) & (S.STREAM_FULL | S.STREAM_BAD_STATE)) == 0
        dt.cursor += np.where(taken, np.asarray(v, dtype=np.int64), 0)
        rows.append([out[so[b]:so[b + 1]] for b in range(B)])
        if mirror:
            n = rep[c, :, 0].astype(np.int64)
            lo = np.maximum(0, n - cap)
            t, p, q, off = s.rows(lo.tolist(), (n - lo).tolist())
            got = np.concatenate([t.cpu().numpy()[:, None], p.cpu().numpy(), q.cpu().numpy()], axis=1)
            off = off.cpu().numpy()
            for b in range(B):
                if not taken[b]:
                    continue
                g = got[off[b]:off[b + 1]]
                new = np.empty((n[b], 8)); new[:min(len(hist[b]), n[b])] = hist[b][:n[b]]
                new[lo[b]:] = g
                k = min(len(hist[b]), n_before[b])
                ch = np.flatnonzero((bits(new[:k]) != bits(hist[b][:k])).any(axis=1))
                rep[c, b, 4] = ch[0] if ch.size else -1
                violations += int((ch < final[b]).sum()) + int(rep[c, b, 1] < final[b])
                final[b] = int(rep[c, b, 1])
                # the rows a call returns are the ring's rows right after it
                m = int(v[b])
                assert (bits(new[n[b] - m:, 1:]) == bits(rows[-1][b][:, :7])).all(), (c, b)
                hist[b] = new
    torch.cuda.synchronize()
    return dict(rep=rep, rows=rows, mirror=hist, violations=violations, stream=s, tracks=dt)


def final_rows(GB, s, n):
    t, p, q, off = s.rows([0] * s.B, [int(x) for x in n])
    got = np.concatenate([t.cpu().numpy()[:, None], p.cpu().numpy(), q.cpu().numpy()], axis=1)
    off = off.cpu().numpy()
    return [got[off[b]:off[b + 1]] for b in range(s.B)]


def close(res, ref, tag, exact_cols=(0, 1, 2, 3)):
    """device result against the host harness's: reports exact, rows within the gates"""
    np.testing.assert_array_equal(res["rep"][:, :, list(exact_cols)], ref["rep"][:, :, list(exact_cols)], err_msg=tag)
    w = [0.0, 0.0, 0.0]
    for c in range(len(ref["rows"])):
        for b in range(len(ref["rows"][c])):
            a, h = res["rows"][c][b], ref["rows"][c][b]
            assert a.shape == h.shape, (tag, c, b)
            if a.size == 0:
                continue
            np.testing.assert_array_equal(np.isnan(a), np.isnan(h), err_msg=tag)
            if np.isnan(h).all():
                continue
            w[0] = max(w[0], float(np.abs(a[:, :3] - h[:, :3]).max())); w[1] = max(w[1], float(np.abs(a[:, 3:7] - h[:, 3:7]).max()))
            w[2] = max(w[2], float(np.abs(a[:, 7:] / h[:, 7:] - 1.0).max()))
    return w


# ------------------------------------------------------------------------------------------------ 1. the kernel against the host harness
@pytest.mark.parametrize("cfg_name", ["default", "steps5"])
def test_kernel_agrees_with_the_host_harness(GB, cfg_name):
    ref = S.reference(cfg_name)
    pats = [S.cut_patterns(t, seed=b) for b, t in enumerate(ref["tracks"])]
    names = sorted({k for p in pats for k in p})
    worst = [0.0, 0.0, 0.0]
    for k in names:
        cuts = [p.get(k, p["whole"]) for p in pats]
        calls = S.calls_from_cuts(cuts)
        host = S.run(ref["tracks"], calls, 256, ref["cfg"])
        dev = run_device(GB, ref["tracks"], calls, 256, ref["cfg"])
        w = close(dev, host, f"{cfg_name} {k}")
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"{cfg_name}: kernel vs host harness over {len(names)} cut patterns x {len(ref['tracks'])} tracks: |dp| {worst[0]:.2e} m, |dq| {worst[1]:.2e}, "
          f"|dvar|/var {worst[2]:.2e}")
    assert worst[0] < POS_TOL and worst[1] < Q_TOL and worst[2] < VAR_RTOL


# ------------------------------------------------------------------------------------------------ 2. split invariance on the device
_b130 = {}


def batch130(cfg):
    """130 tracks (two full waves and a partial third): lane k's outage starts at pose k mod 7 and lasts k mod 11 poses, a second one follows
    later in the track, and lanes 5, 69 and 129 turn at 60 deg/s, so each wave has a track that recovers through a sharp turn"""
    if not _b130:
        tracks = []
        for k in range(130):
            n = 140 + k % 61
            t = R.synthetic_track(n, 100 + k, cfg, turn=k in (5, 69, 129))
            a, a2 = k % 7, 70 + k % 13
            tracks.append(R.withhold(t, list(range(a, a + k % 11)) + list(range(a2, a2 + 1 + k % 5))))
        _b130["tracks"] = tracks
    return _b130["tracks"]


def mixed_schedule(tracks, phase, long=65):
    """every call mixes tracks with empty, 1-pose and `long`-pose segments"""
    left = np.array([len(t[0]) for t in tracks], dtype=np.int64)
    calls, c = [], 0
    while left.sum():
        kind = (np.arange(len(tracks)) * phase + c) % 3
        m = np.minimum(left, np.where(kind == 0, 0, np.where(kind == 1, 1, long)))
        calls.append((S.APPEND, m.tolist()))
        left -= m
        c += 1
    return calls


def test_split_invariance_on_the_device(GB):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = S.steps5(E.CONFIG)
    tracks = batch130(cfg)
    n = [len(t[0]) for t in tracks]
    whole = run_device(GB, tracks, [(S.APPEND, n)], 256, cfg)
    want = final_rows(GB, whole["stream"], n)
    st = whole["rep"][0, :, 3].astype(np.int64)
    for k in (5, 69, 129):
        assert st[k] & ST_SHARP_TURN, k
    assert (st & ST_RTS_APPLIED).sum() > 60
    for phase, long in ((1, 65), (2, 65), (1, 64), (5, 7)):
        calls = mixed_schedule(tracks, phase, long)
        kinds = {tuple(sorted(set(v))) for _, v in calls[:3]}
        assert all(0 in k and 1 in k and long in k for k in kinds)
        res = run_device(GB, tracks, calls, 256, cfg)
        got = final_rows(GB, res["stream"], n)
        for b in range(130):
            assert (bits(got[b]) == bits(want[b])).all(), (phase, long, b)
            assert (bits(S.concat_rows(res, b)[:, 7:]) == bits(whole["rows"][0][b][:, 7:])).all(), (phase, long, b)
        np.testing.assert_array_equal(res["rep"][-1][:, [0, 1, 3]], whole["rep"][-1][:, [0, 1, 3]])


# ------------------------------------------------------------------------------------------------ 3. against the whole-track kernels
@pytest.mark.parametrize("which", ["edge", "b130"])
def test_agrees_with_the_whole_track_kernels(GB, which):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    tracks = S.reference("default")["tracks"] if which == "edge" else batch130(cfg)
    n = [len(t[0]) for t in tracks]
    res = run_device(GB, tracks, mixed_schedule(tracks, 1, 33), 256, cfg)
    got = final_rows(GB, res["stream"], n)
    d = res["tracks"].dev
    po, qo, st = GB.ekf_fuse_ragged(d["ts"], d["pos"], d["quat"], d["gps"], d["valid"], d["offsets"], d["init_pos"], d["init_quat"], config=cfg)
    cov = GB.ekf_covariance_ragged(d["ts"], d["quat"], d["gps"], d["valid"], d["offsets"], config=cfg).filtered.cpu().numpy()
    po, qo, st, off = po.cpu().numpy(), qo.cpu().numpy(), st.cpu().numpy(), res["tracks"].f["offsets"]
    w = [0.0, 0.0, 0.0]
    for b in range(len(tracks)):
        if n[b] == 0:
            assert int(res["rep"][-1, b, 3]) == 0
            continue
        lo, hi = off[b], off[b + 1]
        w[0] = max(w[0], float(np.abs(got[b][:, 1:4] - po[lo:hi]).max())); w[1] = max(w[1], float(np.abs(got[b][:, 4:8] - qo[lo:hi]).max()))
        w[2] = max(w[2], float(np.abs(S.concat_rows(res, b)[:, 7:] / cov[lo:hi] - 1.0).max()))
        assert int(res["rep"][-1, b, 3]) == int(st[b]), (b, int(res["rep"][-1, b, 3]), int(st[b]))
    print(f"{which}: stream vs ekf_fuse_ragged / ekf_covariance_ragged: |dp| {w[0]:.2e} m, |dq| {w[1]:.2e}, |dvar|/var {w[2]:.2e}")
    assert w[0] < POS_TOL and w[1] < Q_TOL and w[2] < VAR_RTOL


# ------------------------------------------------------------------------------------------------ 4. finality, revised_from, rows == ring
def test_finality_and_revised_from(GB):
    ref = S.reference("default")
    pats = [S.cut_patterns(t, seed=b, n_random=3) for b, t in enumerate(ref["tracks"])]
    n_back = 0
    for k in ("cut_all_four", "cut_inside_outage", "random_0", "random_1", "random_2"):
        cuts = [p.get(k, p["whole"]) for p in pats]
        calls = S.calls_from_cuts(cuts)
        res = run_device(GB, ref["tracks"], calls, 256, ref["cfg"], mirror=True)
        assert res["violations"] == 0, k
        n_before = np.zeros(len(cuts), dtype=np.int64)
        for c in range(len(calls)):
            nt, nf, rf, mc = (res["rep"][c, :, j].astype(np.int64) for j in (0, 1, 2, 4))
            back = mc >= 0
            assert (rf[back] == mc[back]).all() and (rf[~back] == n_before[~back]).all(), (k, c)
            assert (nf <= nt).all()
            n_before = nt
            n_back += int(back.sum())
        want = final_rows(GB, res["stream"], [len(t[0]) for t in ref["tracks"]])
        for b, m in enumerate(res["mirror"]):                               # the consumer's mirror is the ring
            assert (bits(m) == bits(want[b])).all(), (k, b)
    assert n_back > 10


# ------------------------------------------------------------------------------------------------ 5. a refused track and its neighbours
def test_a_refused_track_leaves_its_neighbours_alone(GB):
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    tracks = [R.synthetic_track(48, 40, cfg), R.withhold(R.synthetic_track(48, 41, cfg), list(range(20, 32))), R.withhold(R.synthetic_track(48, 42, cfg), [9, 10])]
    calls = S.calls_from_cuts([[8] * 6] * 3)
    tight = run_device(GB, tracks, calls, 19, cfg)
    host = S.run(tracks, calls, 19, cfg)
    close(tight, host, "cap 19")
    full = (tight["rep"][:, :, 3].astype(np.int64) & S.STREAM_FULL) != 0
    assert full[4:, 1].all() and full.sum() == 2
    assert np.isnan(tight["rows"][4][1]).all()
    alone = run_device(GB, [tracks[0], tracks[2]], S.calls_from_cuts([[8] * 6] * 2), 19, cfg)
    for b, a in ((0, 0), (2, 1)):
        assert (bits(S.concat_rows(tight, b)) == bits(S.concat_rows(alone, a))).all()
        np.testing.assert_array_equal(tight["rep"][:, b, :4], alone["rep"][:, a, :4])
    # state and ring of the refused track: the bytes they had before the refused call
    s = tight["stream"]
    before = run_device(GB, tracks, calls[:4], 19, cfg)["stream"]
    assert (bits(s.state_f64[:, 1].cpu().numpy()) == bits(before.state_f64[:, 1].cpu().numpy())).all()
    assert (s.state_i64[:, 1] == before.state_i64[:, 1]).all()
    for name in ("ring_t", "ring_pos", "ring_quat"):
        assert (bits(getattr(s, name)[1].cpu().numpy()) == bits(getattr(before, name)[1].cpu().numpy())).all(), name
    # re-sending after a reopen: the track runs again from pose 0, in segments that fit
    s.reopen([0, 1, 0], tight["tracks"].dev["init_pos"], tight["tracks"].dev["init_quat"])
    again = run_device(GB, tracks, [(S.APPEND, [0, 4, 0])] * 12, 19, cfg, stream=s)
    big = run_device(GB, tracks, calls, 256, cfg)
    assert not (again["rep"][:, 1, 3].astype(np.int64) & S.STREAM_FULL).any()
    assert (bits(S.concat_rows(again, 1)) == bits(S.concat_rows(big, 1))).all()


# ------------------------------------------------------------------------------------------------ 6. the checkpoint
def test_checkpoint_continues_with_the_same_bits(GB):
    import torch
    ref = S.reference("default")
    tracks = ref["tracks"]
    calls = mixed_schedule(tracks, 1, 30)[:5]
    straight = run_device(GB, tracks, calls, 64, ref["cfg"])
    first = run_device(GB, tracks, calls[:3], 64, ref["cfg"])
    d = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in first["stream"].state_dict().items()}
    assert all(not v.is_cuda for v in d.values() if torch.is_tensor(v))
    main_ctx = GB.context()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                           # a new context: batch.context() is per (device, stream)
        assert GB.context() is not main_ctx
        s2 = GB.FusionStream.from_state(d)
        dt = DeviceTracks(tracks)
        dt.cursor[:] = first["tracks"].cursor
        outs = []
        for _, v in calls[3:]:
            seg = dt.segment(v)
            outs.append(s2.append(*seg))
        side.synchronize()
    for c, st in zip((3, 4), outs):
        got = np.concatenate([st.pos.cpu().numpy(), st.quat.cpu().numpy(), st.cov.cpu().numpy()], axis=1)
        assert (bits(got) == bits(np.concatenate(straight["rows"][c]))).all(), c
        np.testing.assert_array_equal(st.n_final.cpu().numpy(), straight["rep"][c, :, 1])
        np.testing.assert_array_equal(st.status.cpu().numpy(), straight["rep"][c, :, 3])
    for name in ("state_f64", "ring_t", "ring_pos", "ring_quat"):
        a, b = getattr(s2, name).cpu().numpy(), getattr(straight["stream"], name).cpu().numpy()
        n = straight["rep"][-1, :, 0].astype(np.int64)
        if name.startswith("ring"):                                         # (slots no pose has reached hold whatever the allocation held)
            a, b = a.copy(), b.copy()
            for t in range(len(tracks)):
                a[t, n[t]:] = 0; b[t, n[t]:] = 0
        assert (bits(a) == bits(b)).all(), name
    assert (s2.state_i64.cpu() == straight["stream"].state_i64.cpu()).all()


# ------------------------------------------------------------------------------------------------ 7. nothing depends on stale memory
@pytest.mark.parametrize("side_stream", [False, True])
def test_outputs_do_not_depend_on_stale_memory(GB, monkeypatch, side_stream):
    """state, ring and every output allocated over a sentinel word (0, then 3: a layout version, a count and a flag that could pass for
    real ones); a second stream interleaved on the same context; the default and a non-default torch stream"""
    import contextlib
    import torch
    ref = S.reference("default")
    tracks = ref["tracks"]
    n = [len(t[0]) for t in tracks]
    calls = mixed_schedule(tracks, 2, 40)
    base = run_device(GB, tracks, calls, 64, ref["cfg"])
    want = np.concatenate([np.concatenate(r) for r in base["rows"]])
    side = torch.cuda.Stream() if side_stream else None
    for sentinel in (0, 3, 0x7ff8000000000001):
        alloc = hygiene.GuardedAllocator(sentinel)
        with (torch.cuda.stream(side) if side_stream else contextlib.nullcontext()):
            with alloc.installed(monkeypatch):
                other = run_device(GB, tracks[::-1], mixed_schedule(tracks[::-1], 1, 9)[:4], 64, ref["cfg"])      # a second stream on the same context
                res = run_device(GB, tracks, calls, 64, ref["cfg"])
                run_device(GB, tracks[::-1], mixed_schedule(tracks[::-1], 1, 9)[4:6], 64, ref["cfg"], stream=other["stream"])
            torch.cuda.synchronize()
        alloc.assert_guards_intact()
        got = np.concatenate([np.concatenate(r) for r in res["rows"]])
        assert (bits(got) == bits(want)).all(), sentinel
        np.testing.assert_array_equal(res["rep"][:, :, :4], base["rep"][:, :, :4])
        lo = [max(0, x - 64) for x in n]
        a, b = res["stream"].rows(lo, [x - l for x, l in zip(n, lo)]), base["stream"].rows(lo, [x - l for x, l in zip(n, lo)])
        for x, y in zip(a[:3], b[:3]):
            assert (bits(x.cpu().numpy()) == bits(y.cpu().numpy())).all(), sentinel
        assert (bits(res["stream"].state_f64.cpu().numpy()) == bits(base["stream"].state_f64.cpu().numpy())).all()
        assert (res["stream"].state_i64 == base["stream"].state_i64).all()
    # rows the ring does not hold are NaN whatever the memory holds
    t, p, q, off = base["stream"].rows([x - 70 for x in n], [80] * len(n))
    t = t.cpu().numpy().reshape(len(n), 80)
    for b, x in enumerate(n):
        held = np.zeros(80, dtype=bool)
        g = np.arange(80) + x - 70
        held[(g >= max(0, x - 64)) & (g < x)] = True
        np.testing.assert_array_equal(~np.isnan(t[b]), held)


# ------------------------------------------------------------------------------------------------ 8. longer than the whole-run chain takes
def test_a_28001_pose_track_through_a_small_ring(GB):
    """one pose more than the whole-run chain accepts, pushed 400 poses at a time (FusionSession hands a push to the device in pieces of
    cap // 2 poses): the rows through a 256-row ring are the rows through a 32 768-row one, bit for bit"""
    from gps_optimize_slam_amd import ekfgpsslam as E
    cfg = E.CONFIG
    n = 28001
    gaps = [i for j, a in enumerate(range(50, n - 120, 230)) for i in range(a, a + 1 + (j * 37) % 99)]      # outages of 1 .. 99 poses, apart
    ts, pos, quat, al, valid, ip, iq = R.withhold(R.synthetic_track(n, 60, cfg), gaps)
    runs = []
    for cap in (256, 32768):
        s = E.FusionSession(ip, iq, cfg, cap=cap)
        parts, marks = [], []
        for lo in range(0, n, 400):
            hi = min(n, lo + 400)
            r = s.push(ts[lo:hi], pos[lo:hi], quat[lo:hi], al[lo:hi], valid[lo:hi])
            parts.append(np.concatenate([r["pos"], r["quat"], r["cov"]], axis=1))
            marks.append((r["n_total"], r["n_final"], r["revised_from"], r["status"]))
            assert r["n_total"] == hi and r["n_final"] <= hi and r["revised_from"] <= lo
        runs.append((np.concatenate(parts), marks))
    assert np.isfinite(runs[0][0]).all()
    assert (bits(runs[0][0]) == bits(runs[1][0])).all()
    assert runs[0][1] == runs[1][1]
    assert runs[0][1][-1][3] & ST_RTS_APPLIED and any(m[1] < m[0] for m in runs[0][1]) and any(m[2] < 400 * i for i, m in enumerate(runs[0][1]))


# ------------------------------------------------------------------------------------------------ 9. a stream opened from a whole run
def test_stream_opened_from_a_whole_run(GB, golden, tmp_path):
    """run_fusion_ragged on the bundled track's files -> FusionStream.from_run -> the same poses with the run's aligned fixes in 100-pose
    appends: the run's own fused tracks (its EKF is the whole-track wave kernel: 1e-7 m / 1e-9), status words equal; the track whose run
    stopped sends nothing"""
    import torch
    from test_cov_gpu import file_batch
    from gps_optimize_slam_amd import ekfgpsslam as E
    rb = file_batch(GB, golden, tmp_path)
    r = GB.run_fusion_ragged(rb, GB.mt19937_seed([3, 4, 5, 6]), E.CONFIG)
    s = GB.FusionStream.from_run(rb, r, cap=512)
    off = rb.slam_offsets.cpu().numpy()
    n = np.diff(off)
    ok = r.run_status.cpu().numpy() == 0
    assert ok.tolist() == [True, True, False, True] and s.B == 4
    ts, pos, quat, al, va = rb.ts.reshape(-1), rb.pos.reshape(-1, 3), rb.quat.reshape(-1, 4), r.aligned.reshape(-1, 3), r.valid.reshape(-1)
    for lo in range(0, int(n.max()), 100):
        counts = np.clip(n - lo, 0, 100) * ok
        idx = np.concatenate([np.arange(c, dtype=np.int64) + off[b] + lo for b, c in enumerate(counts)])
        i = torch.as_tensor(idx).cuda()
        so = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda()
        st = s.append(ts[i].contiguous(), pos[i].contiguous(), quat[i].contiguous(), al[i].contiguous(), va[i].contiguous(), so)
        assert not bool((st.status & (S.STREAM_FULL | S.STREAM_BAD_STATE)).any())
    t, p, q, o = s.rows([0] * 4, (n * ok).tolist())
    p, q, o = p.cpu().numpy(), q.cpu().numpy(), o.cpu().numpy()
    fp, fq, fs = r.fused.pos.cpu().numpy(), r.fused.quat.cpu().numpy(), r.fused.status.cpu().numpy()
    for b in np.flatnonzero(ok):
        assert np.abs(p[o[b]:o[b + 1]] - fp[off[b]:off[b + 1]]).max() < POS_TOL and np.abs(q[o[b]:o[b + 1]] - fq[off[b]:off[b + 1]]).max() < Q_TOL, b
        assert int(st.status[b]) == int(fs[b]) & 0xff, b
    assert int(st.n_total[2]) == 0 and int(st.status[2]) == 0
