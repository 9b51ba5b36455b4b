"""CPU tier of the staging layout (gps_optimize_slam_amd/csrc/gsf_stage_plan.hpp): the planner gsf::Staging calls for every host-pointer
entry, compiled with g++ into a test-only harness (tests/host_stage_harness.cpp) and compared with the restatement below: inputs first in
the order declared, then outputs and temporaries in the order declared, every block on a 256-byte boundary.  The properties the entries
rely on are asserted on their own as well.  The same harness, with its own main, is built under -fsanitize=address,undefined and run once
as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_stage_harness.cpp")
IN, OUT, TMP = 0, 1, 2
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
GUARD = -7777


@pytest.fixture(scope="module")
def hs():
    bdir = os.path.join(HERE, "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libhost_stage_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, SRC])
    L = C.CDLL(so)
    L.hs_plan.restype = C.c_int
    L.hs_plan.argtypes = [i64p, i32p, u8p, C.c_int, i64p, i64p]
    L.hs_max_blocks.restype = C.c_int
    return L


def restated(blocks):
    """the layout in ten lines: (offsets, in_end, d2h_lo, d2h_hi, cap) of [(bytes, kind, host-backed)]"""
    off, end, in_end, span = [0] * len(blocks), 0, 0, []
    for first in (True, False):
        for i, (nbytes, kind, host) in enumerate(blocks):
            if (kind == IN) == first:
                off[i] = -(-end // 256) * 256
                end = off[i] + nbytes
                in_end = end if first else in_end
                span += [off[i], end] if (kind == OUT and host and nbytes) else []
    return off, in_end, min(span, default=0), max(span, default=0), end


def plan(hs, blocks):
    """the harness on a list; the offsets array is guarded behind the table's size"""
    n, m = len(blocks), min(len(blocks), hs.hs_max_blocks())
    nbytes = np.array([b[0] for b in blocks], np.int64)
    kind = np.array([b[1] for b in blocks], np.int32)
    host = np.array([b[2] for b in blocks], np.uint8)
    off = np.full(m + 8, GUARD, np.int64)
    p = np.zeros(4, np.int64)
    refused = hs.hs_plan(nbytes, kind, host, n, off, p)
    assert (off[m:] == GUARD).all()
    return off[:m].tolist(), [int(v) for v in p], refused


def check(hs, blocks):
    off, (in_end, lo, hi, cap), refused = plan(hs, blocks)
    assert refused == 0
    want = restated(blocks)
    assert (off, in_end, lo, hi, cap) == want, (blocks, off, (in_end, lo, hi, cap), want)
    ends = [o + b[0] for o, b in zip(off, blocks)]
    assert all(o % 256 == 0 for o in off)
    live = sorted((o, e) for o, e, b in zip(off, ends, blocks) if b[0])
    assert all(a[1] <= b[0] for a, b in zip(live, live[1:])), "blocks overlap"
    ins = [e for e, b in zip(ends, blocks) if b[1] == IN]
    rest = [o for o, b in zip(off, blocks) if b[1] != IN]
    assert not ins or not rest or max(ins) <= min(rest), "an input above an output"
    assert in_end == max(ins, default=0)
    for o, e, b in zip(off, ends, blocks):
        if b[1] == OUT and b[2] and b[0]:
            assert lo <= o and e <= hi, "a host-backed output outside the D2H span"
    assert cap == max(ends, default=0)
    return off, in_end, lo, hi, cap


def test_named_lists(hs):
    # zero-byte arrays keep their place and take no room
    off, in_end, lo, hi, cap = check(hs, [(0, IN, True), (24, IN, True), (0, OUT, True), (8, OUT, True), (0, TMP, False)])
    assert off == [0, 0, 256, 256, 512] and (in_end, lo, hi, cap) == (24, 256, 264, 512)
    # a NULL-host required output between two host-backed ones: inside the span, and the span is still one copy
    off, in_end, lo, hi, cap = check(hs, [(100, IN, True), (300, OUT, True), (40, OUT, False), (7, OUT, True)])
    assert off == [0, 256, 768, 1024] and (lo, hi, cap) == (256, 1031, 1031)
    # a NULL-host output / a temporary at either end does not widen the span
    _, _, lo, hi, cap = check(hs, [(40, OUT, False), (300, OUT, True), (7, OUT, True), (64, TMP, False)])
    assert (lo, hi, cap) == (256, 775, 1088)
    # outputs declared before inputs: the inputs still come first
    off, in_end, _, _, _ = check(hs, [(10, OUT, True), (20, IN, True), (30, TMP, False), (40, IN, False)])
    assert off == [512, 0, 768, 256] and in_end == 296
    # only inputs, only outputs, nothing at all
    assert check(hs, [(5, IN, True), (5, IN, True)])[1:] == (261, 0, 0, 261)
    assert check(hs, [(5, OUT, True), (5, OUT, True)])[1:] == (0, 0, 261, 261)
    assert check(hs, [])[1:] == (0, 0, 0, 0)
    # above 4 GiB
    check(hs, [(5 << 30, IN, True), (3, IN, True), (6 << 30, OUT, True), (1, OUT, True)])


def test_full_table_and_one_more(hs):
    m = hs.hs_max_blocks()
    assert m >= 41                                                          # the ragged whole run with every optional array declares 41
    full = [(i * 37 % 900, (IN, OUT, TMP)[i % 3], i % 2 == 0) for i in range(m)]
    check(hs, full)
    off, p, refused = plan(hs, full + [(123, OUT, True)])                   # (plan() asserts that nothing is written past the table)
    assert refused == 1
    assert (off, *p) == restated(full)                                      # the refused array is not part of the layout
    assert plan(hs, full + [(1, IN, True)] * 5)[2] == 5


def test_random_lists(hs):
    rng = np.random.default_rng(256)
    m = hs.hs_max_blocks()
    for _ in range(4000):
        n = int(rng.integers(0, m + 1))
        nbytes = np.where(rng.random(n) < 0.15, 0, rng.integers(1, rng.choice([300, 70000, 40 << 20]), n))
        check(hs, list(zip(nbytes.tolist(), rng.integers(0, 3, n).tolist(), (rng.random(n) < 0.7).tolist())))


def test_standalone_program_under_sanitizers():
    """the harness's own main (5000 random lists, the same properties, the table plus two), address + undefined-behaviour sanitizers"""
    exe = os.path.join(HERE, "_build", "host_stage_harness_san")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DHS_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "5000 lists ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
