"""The yardstick of the pose-query entries (gsf_pose_query[_dev], gsf_georef_points[_dev]): a NumPy restatement of the contract in
include/gsf.h ("pose queries"), with every value evaluated in np.longdouble (80-bit on x86-64: 64 significand bits, so its own rounding is
2^-11 of a float64 ulp).  Classification, indices and flags are comparisons of float64 numbers and therefore exact.

Also here: the bounds the tests hold the float64 code to, computed from the inputs (never from what the code under test returns), and the
generator of the test tracks -- UTM-sized coordinates, stamps near 1.3e9 s, consecutive poses >= 0.1 m and a few degrees apart, so that the
smallest real mistake (the neighbouring bracket, the weight of the other side) moves a result by more than 1e-3."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52

QT_EMPTY, QT_UNSORTED, QT_SKIPPED, QT_BAD_EXTRINSIC = 1, 2, 4, 8
Q_EXACT, Q_BEFORE, Q_AFTER, Q_GAP, Q_NAN, Q_TRACK, Q_BAD_QUAT = 1, 2, 4, 8, 16, 32, 64


def can_normalise(q):
    """quat_unit's test (gsf_math.hpp): the squared norm is a number in [1e-280, 1e280]"""
    n2 = float(np.sum(np.asarray(q, dtype=np.float64) ** 2))
    return bool(n2 >= 1e-280 and n2 <= 1e280)


def nlerp(q1, q2, weight_q2):
    """quaternion_nlerp, EKFGPSSLAM.py:94-105, line by line in long double"""
    q1, q2, weight_q2 = np.asarray(q1, dtype=LD), np.asarray(q2, dtype=LD), LD(weight_q2)
    dot = np.dot(q1, q2)
    if dot < 0.0:
        q2 = -q2
    w = np.clip(weight_q2, LD(0.0), LD(1.0))
    q_interp = (LD(1.0) - w) * q1 + w * q2
    norm = np.sqrt(np.sum(q_interp * q_interp))
    if norm < 1e-9:
        return q1 if weight_q2 < 0.5 else q2
    return q_interp / norm


def rotate(q_unit, v):
    """Rotation.apply of a unit quaternion [x y z w], long double: v + w t + u x t, t = 2 u x v"""
    u, w = q_unit[:3], q_unit[3]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def unit(q):
    q = np.asarray(q, dtype=LD)
    return q / np.sqrt(np.sum(q * q))


def track_states(ts, offsets, run_status=None, ext_q=None):
    B = len(offsets) - 1
    st = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if run_status is not None and run_status[b] != 0:
            st[b] = QT_SKIPPED
            continue
        t = ts[offsets[b]:offsets[b + 1]]
        if len(t) == 0:
            st[b] |= QT_EMPTY
        elif np.isnan(t[0]) or not np.all(t[1:] >= t[:-1]):
            st[b] |= QT_UNSORTED
        if ext_q is not None and not can_normalise(ext_q[b]):
            st[b] |= QT_BAD_EXTRINSIC
    return st


def query(ts, pos, quat, offsets, q_t, q_offsets, pose_flags=None, run_status=None, max_gap=0.0, ext_q=None):
    """-> dict: pos (M,3) / quat (M,4) long double, flags (M,) uint8, index (M,) int32, pose_flags (M,) uint8, track_state (B,) int32"""
    M, B = len(q_t), len(offsets) - 1
    out_p, out_q = np.full((M, 3), np.nan, dtype=LD), np.full((M, 4), np.nan, dtype=LD)
    flags, index, pf = np.zeros(M, dtype=np.uint8), np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.uint8)
    state = track_states(ts, offsets, run_status, ext_q)
    for b in range(B):
        t, p, q = ts[offsets[b]:offsets[b + 1]], pos[offsets[b]:offsets[b + 1]], quat[offsets[b]:offsets[b + 1]]
        fl_b = None if pose_flags is None else pose_flags[offsets[b]:offsets[b + 1]]
        for m in range(q_offsets[b], q_offsets[b + 1]):
            tau = q_t[m]
            if state[b] != 0:
                flags[m] = Q_TRACK
            elif np.isnan(tau):
                flags[m] = Q_NAN
            elif tau < t[0]:
                flags[m] = Q_BEFORE
            elif tau > t[-1]:
                flags[m] = Q_AFTER
            else:
                i = int(np.searchsorted(t, tau, side="right")) - 1
                index[m] = i
                if t[i] == tau:
                    out_p[m], out_q[m], flags[m] = p[i], q[i], Q_EXACT
                    if fl_b is not None:
                        pf[m] = fl_b[i]
                    continue
                j = i + 1
                if fl_b is not None:
                    pf[m] = fl_b[i] | fl_b[j]
                gap = t[j] - t[i]                                        # float64, as the contract has it
                if max_gap > 0 and gap > max_gap:
                    flags[m] = Q_GAP
                    continue
                w = (LD(tau) - LD(t[i])) / (LD(t[j]) - LD(t[i]))
                out_p[m] = p[i].astype(LD) + w * (p[j].astype(LD) - p[i].astype(LD))
                out_q[m] = nlerp(q[i], q[j], w)
    return dict(pos=out_p, quat=out_q, flags=flags, index=index, pose_flags=pf, track_state=state)


def georef(ts, pos, quat, offsets, q_t, x, q_offsets, ext_q=None, ext_t=None, scale=None, pose_flags=None, run_status=None, max_gap=0.0):
    """-> dict: xyz (M,3) long double, flags, index, pose_flags, track_state"""
    r = query(ts, pos, quat, offsets, q_t, q_offsets, pose_flags, run_status, max_gap, ext_q)
    M, B = len(q_t), len(offsets) - 1
    xyz, flags = np.full((M, 3), np.nan, dtype=LD), r["flags"].copy()
    for b in range(B):
        if r["track_state"][b] != 0:
            continue
        e = unit(ext_q[b]) if ext_q is not None else np.array([0, 0, 0, 1], dtype=LD)
        et = ext_t[b].astype(LD) if ext_t is not None else np.zeros(3, dtype=LD)
        s = LD(scale[b]) if scale is not None else LD(1.0)
        for m in range(q_offsets[b], q_offsets[b + 1]):
            if r["index"][m] < 0 or (flags[m] & Q_GAP):
                continue
            if not can_normalise(np.asarray(r["quat"][m], dtype=np.float64)):
                flags[m] |= Q_BAD_QUAT
                continue
            y = s * (rotate(e, x[m].astype(LD)) + et)
            xyz[m] = r["pos"][m] + rotate(unit(r["quat"][m]), y)
    return dict(xyz=xyz, flags=flags, index=r["index"], pose_flags=r["pose_flags"], track_state=r["track_state"])


# ------------------------------------------------------------------------------------------------ bounds (derived from the inputs)
def bracket_rows(offsets, q_offsets, index, flags):
    """global pose rows (i, j) of every query with a bracket (j = i on an exact hit); -1 elsewhere"""
    M = len(index)
    gi, gj = np.full(M, -1, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    for b in range(len(offsets) - 1):
        sl = slice(q_offsets[b], q_offsets[b + 1])
        has = index[sl] >= 0
        gi[sl] = np.where(has, offsets[b] + index[sl], -1)
        gj[sl] = np.where(has, offsets[b] + index[sl] + np.where(flags[sl] & Q_EXACT, 0, 1), -1)
    return gi, gj


def pos_bound(pos, gi, gj):
    """per component: 2 spacing(max(|p_i,c|, |p_j,c|)); rows without a bracket get 0 (they are compared as NaN patterns)"""
    has = gi >= 0
    big = np.maximum(np.abs(pos[np.maximum(gi, 0)]), np.abs(pos[np.maximum(gj, 0)]))
    with np.errstate(invalid="ignore"):
        b = 2.0 * np.spacing(big)
    return np.where(has[:, None], b, 0.0)


QUAT_BOUND = 10 * EPS                                                    # ten roundings of magnitude <= 1 in lerp, norm and division


def point_bound(pos, gi, gj, x, scale_q, ext_t_q):
    """the position bound + 32 * 2^-52 * (|scale| * ||x|| + ||ext_t||), scale_q (M,) / ext_t_q (M,3) = the query's track's values"""
    return pos_bound(pos, gi, gj) + (32 * EPS * (np.abs(scale_q) * np.linalg.norm(x, axis=1) + np.linalg.norm(ext_t_q, axis=1)))[:, None]


def same_nan_pattern(got, want):
    return np.array_equal(np.isnan(got), np.isnan(np.asarray(want, dtype=np.float64)))


def max_excess(got, want, bound):
    """max of |got - want| - bound over the finite entries of want (<= 0: within the bound), and max |got - want| itself"""
    d = np.abs(got.astype(LD) - want)
    fin = np.isfinite(np.asarray(want, dtype=np.float64))
    if not fin.any():
        return -np.inf, 0.0
    bound = np.broadcast_to(bound, d.shape)
    return float(np.max((d - bound)[fin])), float(np.max(d[fin]))


# ------------------------------------------------------------------------------------------------ test tracks
def make_track(n, rng, t0=1.3e9, e0=4.5e5, n0=9.4e6):
    """n poses: stamps t0 + irregular steps of 0.08 .. 0.14 s, positions a walk of 0.2 .. 1 m steps at UTM-sized coordinates, orientations
    turning 3 .. 8 degrees per pose about a tilted axis (unit quaternions, both hemispheres: every third pose is stored negated, so the
    sign flip of nlerp is exercised)"""
    ts = t0 + np.cumsum(rng.uniform(0.08, 0.14, n))
    step = rng.uniform(0.2, 1.0, (n, 3)) * np.array([1.0, 1.0, 0.05]) * rng.choice([-1.0, 1.0], (n, 3))
    step[:, 0] = np.abs(step[:, 0])                                      # it keeps moving east: >= 0.2 m between consecutive poses
    pos = np.array([e0, n0, 120.0]) + np.cumsum(step, axis=0)
    ang = np.cumsum(np.deg2rad(rng.uniform(3.0, 8.0, n)))
    axis = np.array([0.2, -0.1, 1.0]); axis /= np.linalg.norm(axis)
    quat = np.column_stack((np.sin(ang / 2)[:, None] * axis, np.cos(ang / 2)))
    quat[2::3] *= -1.0
    return ts, pos, quat


def inner_queries(ts, count, rng):
    """`count` stamps strictly inside brackets of ts (n >= 2), each at least 1 % of its gap away from both ends"""
    i = rng.integers(0, len(ts) - 1, count)
    return ts[i] + rng.uniform(0.01, 0.99, count) * (ts[i + 1] - ts[i])


MAX_GAP = 1.0                                                            # s; the tracks' own steps are <= 0.14 s, the planted loss is 5 s


def build_cases(seed=7):
    """The batch both tiers run: tracks of 0, 1, 2, 3, 63, 64, 65 and 130 poses, three equal stamps in a row, an unsorted track, a NaN stamp,
    a skipped track, a track of special poses, a track with a dead extrinsic quaternion; query counts from {0, 1, 63, 64, 65, 257} laid out
    so that waves of 64 straddle track boundaries.  Queries are time-sorted inside each track (NaN last).  -> dict of host arrays."""
    rng = np.random.default_rng(seed)
    tracks, queries, notes = [], [], {}

    def specials(ts):
        return [ts[0], ts[-1], ts[len(ts) // 2], np.nextafter(ts[0], -np.inf), np.nextafter(ts[-1], np.inf), np.nan]

    def add(name, trk, count, extra=()):
        ts = trk[0]
        q = list(extra)
        usable = len(ts) >= 1 and not np.isnan(ts).any() and np.all(np.diff(ts) >= 0)
        if usable and count >= 6 + len(q):
            q += specials(ts)
        if usable and len(ts) >= 2:
            q += list(inner_queries(ts, max(count - len(q), 0), rng))
        elif len(ts) >= 1:
            q += list(np.nanmin(ts) + rng.uniform(-0.5, 0.5, max(count - len(q), 0)))
        else:
            q += list(1.3e9 + rng.uniform(0, 1, max(count - len(q), 0)))
        q = np.sort(np.asarray(q[:count], dtype=np.float64))
        assert len(q) == count, (name, len(q), count)
        notes[name] = len(tracks)
        tracks.append(trk); queries.append(q)

    empty = tuple(a[:0] for a in make_track(1, rng))
    add("n0", empty, 1)
    for n, c in ((1, 63), (2, 64), (3, 65), (63, 257), (64, 0), (65, 63)):
        add(f"n{n}", make_track(n, rng), c)
    # 130 poses: 257 queries packed inside three poses (two brackets: the window route), then 64 spread over the whole track (a wave whose
    # span exceeds 64 poses: the general route).  Sorted by segment, not as a whole, so that the spread ones share waves.
    t130 = make_track(130, rng)
    packed = np.sort(np.r_[t130[0][40:43], t130[0][40] + rng.uniform(0.01, 0.99, 254) * (t130[0][42] - t130[0][40])])
    packed = packed[(np.abs(packed[:, None] - t130[0][None, 40:43]).min(axis=1) == 0) | (np.abs(packed[:, None] - t130[0][None, 40:43]).min(axis=1) > 2e-3)]
    packed = np.sort(np.r_[packed, inner_queries(t130[0][40:43], 257 - len(packed), rng)])
    spread = np.sort(np.r_[t130[0][0], t130[0][-1], inner_queries(t130[0], 62, rng)])
    notes["n130"] = len(tracks)
    tracks.append(t130); queries.append(np.r_[packed, spread])
    # three equal stamps in a row: a query on them must return the LAST of the three, bit for bit
    rep = make_track(10, rng)
    rep[0][5] = rep[0][6] = rep[0][4]
    add("repeated", rep, 65, extra=[rep[0][4]])
    uns = make_track(5, rng); uns[0][3] = uns[0][1] - 0.01
    add("unsorted", uns, 1)
    nan_t = make_track(5, rng); nan_t[0][2] = np.nan
    add("nan_stamp", nan_t, 64)
    add("skipped", make_track(7, rng), 63)
    # special poses: 2 has a NaN position (exact hits on 1 and 3 must not see it), 5 -> 6 is a tracking loss of 5 s, 8 / 9 are quaternions of
    # norm 1e-10 at right angles (their blend has a norm below 1e-9: the reference returns q_i or q_j by the weight), 11 is a zero quaternion
    sp = make_track(13, rng)
    sp[0][6:] += 5.0
    sp[1][2] = np.nan
    sp[2][8] = [0.0, 0.0, 0.0, 1e-10]; sp[2][9] = [0.0, 0.0, 1e-10, 0.0]
    sp[2][11] = 0.0
    ts = sp[0]
    extra = [ts[1], ts[3], ts[1] + 0.5 * (ts[2] - ts[1]), ts[2], ts[5] + 2.0, ts[8] + 0.25 * (ts[9] - ts[8]), ts[8] + 0.75 * (ts[9] - ts[8]), ts[11],
             ts[10] + 0.5 * (ts[11] - ts[10])]
    add("special", sp, 64, extra=extra)
    add("dead_extrinsic", make_track(3, rng), 1)

    B = len(tracks)
    offsets = np.zeros(B + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(t[0]) for t in tracks])
    q_offsets = np.zeros(B + 1, dtype=np.int64); q_offsets[1:] = np.cumsum([len(q) for q in queries])
    cat = lambda k, cols: np.ascontiguousarray(np.concatenate([t[k].reshape(-1, cols) for t in tracks]).reshape((-1, cols) if cols > 1 else -1))
    P, M = int(offsets[-1]), int(q_offsets[-1])
    run_status = np.zeros(B, dtype=np.int32); run_status[notes["skipped"]] = 8
    ext_q = rng.normal(size=(B, 4)); ext_q *= (2.0 / np.linalg.norm(ext_q, axis=1))[:, None]
    ext_q[notes["dead_extrinsic"]] = 0.0
    x = rng.normal(size=(M, 3)); x *= (rng.uniform(0.5, 140.0, M) / np.linalg.norm(x, axis=1))[:, None]
    return dict(ts=cat(0, 1), pos=cat(1, 3), quat=cat(2, 4), offsets=offsets, q_t=np.ascontiguousarray(np.concatenate(queries)), q_offsets=q_offsets,
                pose_flags=rng.integers(0, 16, P).astype(np.uint8), run_status=run_status, ext_q=np.ascontiguousarray(ext_q),
                ext_t=rng.uniform(-1.0, 1.0, (B, 3)), scale=rng.uniform(0.5, 2.0, B), x=np.ascontiguousarray(x), notes=notes, B=B, P=P, M=M)
