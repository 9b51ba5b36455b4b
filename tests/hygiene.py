"""Helpers of tests/test_buffer_hygiene.py: outputs that must not depend on what memory held before the call.

batch.py obtains every output through `torch.empty` / `torch.empty_like`, and PyTorch's caching allocator hands a freed block straight back
to the next request of the same size -- often with the previous, correct, answer still in it.  `GuardedAllocator` replaces the two
functions for the duration of one product call: every CUDA request becomes a view into a larger uint8 block with GUARD bytes of GUARD_BYTE
on both sides and a payload pre-filled with a chosen 64-bit sentinel word.  `HostAllocator` hands out numpy arrays of the same make for the
host-pointer entry points.  `same_bytes_under_dirt` runs one call three times -- fresh workspaces, then twice on workspaces that hold
another call's data overwritten by gsf_set_option "poison_workspaces" -- and asks for the same payload bytes every time.  Byte equality
only: there is no tolerance anywhere in this module."""
import contextlib
import sys

import numpy as np

GUARD = 4096
GUARD_BYTE = 0xC3
ALIGN = 256


def _count(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def _site(depth):
    f = sys._getframe(depth)
    return f"{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno}"


class Allocation:
    def __init__(self, order, block, off, nbytes, shape, dtype, itemsize, site):
        self.order, self.block, self.off, self.nbytes, self.shape = order, block, off, nbytes, tuple(int(v) for v in shape)
        self.dtype, self.itemsize, self.site = dtype, itemsize, site

    def label(self):
        return f"allocation #{self.order} {self.shape} {str(self.dtype).replace('torch.', '')} ({self.site})"


def _guard_damage(rec, host):
    """None, or the text naming the first damaged guard byte of one allocation (host = the whole block as numpy bytes)"""
    for name, lo, hi in (("before", 0, rec.off), ("after", rec.off + rec.nbytes, host.size)):
        bad = np.flatnonzero(host[lo:hi] != GUARD_BYTE)
        if bad.size:
            at = int(bad[0]) - (rec.off if name == "before" else 0)         # from the payload's first byte (negative) / from the byte after its last
            return (f"guard bytes {name} {rec.label()} overwritten: {bad.size} byte(s), first at offset {at:+d} from the payload's "
                    f"{'start' if name == 'before' else 'end'} (value 0x{int(host[lo + int(bad[0])]):02x})")
    return None


class GuardedAllocator:
    """torch.empty / torch.empty_like for one product call (see the module text).  CPU requests (pinned ones included) pass through."""

    def __init__(self, sentinel):
        import torch
        self.torch, self.sentinel, self.records = torch, int(sentinel), []
        self._empty, self._empty_like = torch.empty, torch.empty_like

    def _is_cuda(self, device):
        return device is not None and self.torch.device(device).type == "cuda"

    def _make(self, shape, dtype, device, site):
        torch = self.torch
        dtype = dtype or torch.get_default_dtype()
        itemsize = self._empty((), dtype=dtype).element_size()
        nbytes = _count(shape) * itemsize
        padded = (nbytes + 7) // 8 * 8
        block = self._empty((GUARD + ALIGN + padded + GUARD,), dtype=torch.uint8, device=device)
        off = GUARD + (-(block.data_ptr() + GUARD)) % ALIGN
        block.fill_(GUARD_BYTE)
        if padded:
            block[off:off + padded].view(torch.int64).fill_(self.sentinel)
            if padded > nbytes:
                block[off + nbytes:off + padded].fill_(GUARD_BYTE)
        self.records.append(Allocation(len(self.records), block, off, nbytes, shape, dtype, itemsize, site))
        return block[off:off + nbytes].view(dtype).view(tuple(shape))

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._is_cuda(device):
            return self._empty(*size, dtype=dtype, device=device, **kw)
        assert not any(kw.values()), f"torch.empty on the device with {kw}: not modelled by the guarded allocator"
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(int(v) for v in size)
        return self._make(shape, dtype, device, _site(2))

    def empty_like(self, t, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if not self._is_cuda(device):
            return self._empty_like(t, dtype=dtype, device=device, **kw)
        assert not kw, f"torch.empty_like on the device with {kw}: not modelled by the guarded allocator"
        return self._make(tuple(t.shape), dtype or t.dtype, device, _site(2))

    @contextlib.contextmanager
    def installed(self, monkeypatch):
        """both functions replaced through `monkeypatch` inside the block, restored after it"""
        with monkeypatch.context() as m:
            m.setattr(self.torch, "empty", self.empty)
            m.setattr(self.torch, "empty_like", self.empty_like)
            yield self

    # ---- after torch.cuda.synchronize()
    def payloads(self):
        """the recorded payload bytes on the host, in call order"""
        return [r.block[r.off:r.off + r.nbytes].cpu().numpy().copy() for r in self.records]

    def assert_guards_intact(self):
        for r in self.records:
            text = _guard_damage(r, r.block.cpu().numpy())
            assert text is None, text

    def find(self, tensor):
        """the allocation a returned tensor lives in (by address), or None"""
        if tensor is None:
            return None
        p = tensor.data_ptr()
        for r in self.records:
            lo = r.block.data_ptr() + r.off
            if lo <= p < lo + max(r.nbytes, 1):
                return r
        return None


class HostAllocator:
    """numpy outputs of a host-pointer entry point, made like GuardedAllocator's: guards of GUARD_BYTE, payload = the sentinel word repeated"""

    def __init__(self, sentinel):
        self.sentinel, self.records = int(sentinel), []

    def new(self, shape, dtype):
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
        dt = np.dtype(dtype)
        nbytes = _count(shape) * dt.itemsize
        padded = (nbytes + 7) // 8 * 8
        block = np.full(GUARD + ALIGN + padded + GUARD, GUARD_BYTE, dtype=np.uint8)
        off = GUARD + (-(block.ctypes.data + GUARD)) % ALIGN
        block[off:off + padded].view(np.int64)[:] = self.sentinel
        block[off + nbytes:off + padded] = GUARD_BYTE
        self.records.append(Allocation(len(self.records), block, off, nbytes, shape, dt, dt.itemsize, _site(2)))
        return block[off:off + nbytes].view(dt).reshape(shape)

    @contextlib.contextmanager
    def installed(self, monkeypatch):
        yield self

    def payloads(self):
        return [r.block[r.off:r.off + r.nbytes].copy() for r in self.records]

    def assert_guards_intact(self):
        for r in self.records:
            text = _guard_damage(r, r.block)
            assert text is None, text


def _decode(rec, byte_index, rows_of=None):
    """where a payload byte lies: element index, and (track, row, column) where the shape allows; rows_of = the offsets of a ragged batch
    (flat per-row payloads of as many rows are then decoded through them)"""
    el = byte_index // rec.itemsize
    idx = tuple(int(v) for v in np.unravel_index(el, rec.shape)) if rec.shape and all(rec.shape) else (int(el),)
    text = f"element {idx}"
    if rows_of is not None and len(rec.shape) >= 1 and rows_of[-1] > 0 and rec.shape[0] == int(rows_of[-1]):
        b = int(np.searchsorted(rows_of, idx[0], side="right") - 1)
        text += f" = track {b}, row {idx[0] - int(rows_of[b])}" + (f", column {idx[1:]}" if len(idx) > 1 else "")
    elif len(idx) >= 2:
        text += f" = track {idx[0]}, row / column {idx[1:]}"
    else:
        text += f" = track {idx[0]}"
    return text


def _tracks(rec, where, rows_of):
    """'; tracks [...]' for the payload bytes `where`, when the payload's first axis is the track or the rows of a ragged batch"""
    if not rec.shape or not all(rec.shape):
        return ""
    lead = np.unique(where // (rec.nbytes // rec.shape[0]))
    if rows_of is not None and rows_of[-1] > 0 and rec.shape[0] == int(rows_of[-1]):
        lead = np.unique(np.searchsorted(rows_of, lead, side="right") - 1)
    return f"; tracks {lead[:24].tolist()}{' ...' if lead.size > 24 else ''} ({lead.size})"


def compare_runs(runs, names, masks=None, rows_of=None):
    """runs: [(records, payloads)] of the same call; payload k must hold the same bytes in all of them as in the first, but for the bytes
    masks[k] excludes.  Returns the differences as text (empty = equal)."""
    problems = []
    recs0, pay0 = runs[0]
    for (recs, pay), name in zip(runs[1:], names[1:]):
        if len(pay) != len(pay0):
            problems.append(f"{name}: {len(pay)} allocations, {names[0]} made {len(pay0)}")
            continue
        for k, (a, b) in enumerate(zip(pay0, pay)):
            if a.size != b.size:
                problems.append(f"{name}: {recs[k].label()} has {b.size} bytes, {names[0]} {a.size}")
                continue
            diff = a != b
            if masks and k in masks:
                diff &= ~masks[k]
            if diff.any():
                where = np.flatnonzero(diff)
                es = recs[k].itemsize
                e0 = int(where[0]) // es * es
                problems.append(f"{names[0]} vs {name}: {recs[k].label()}: {int(np.unique(where // es).size)} element(s) differ ({where.size} bytes), "
                                f"first at {_decode(recs[k], int(where[0]), rows_of)}: bytes {a[e0:e0 + es].tobytes().hex()} vs {b[e0:e0 + es].tobytes().hex()}"
                                f"{_tracks(recs[k], where, rows_of)}")
    return problems


RUNS = ((-1, 0, "fresh (workspaces released, poison off, sentinel 0)"), (0, 0, "dirty A (poison 0, sentinel 0)"), (3, 3, "dirty B (poison 3, sentinel 3)"))


def same_bytes_under_dirt(monkeypatch, ctx, fn, dirty, states=(), masks_of=None, rows_of=None, host=False):
    """fn(*states) is one product call on fixed inputs (states: generator states that are inputs AND outputs, cloned per run; host=True:
    fn(allocator, *states) with a HostAllocator for its numpy outputs); `dirty()` a different, larger call on the same context.  Three
    runs, see RUNS.  Every payload byte must be the same in dirty A and dirty B -- a byte that differs was not written by the call, or
    depends on memory it did not write -- and the same as in the fresh run; states likewise; guards intact in all three.
    masks_of(result, allocator) -> {order number: (excluded bytes as a bool array over the payload, the count its definition implies)} for
    what the header says is not written; the count is asserted.  Returns the fresh run's result."""
    import torch
    runs, results, ends = [], [], []
    try:
        for poison, sentinel, _ in RUNS:
            torch.cuda.synchronize()
            if poison < 0:
                ctx.set_option("poison_workspaces", -1)
                ctx.trim()
            else:
                dirty()
                ctx.set_option("poison_workspaces", poison)
            st = tuple(s.clone() for s in states)
            alloc = HostAllocator(sentinel) if host else GuardedAllocator(sentinel)
            with alloc.installed(monkeypatch):
                res = fn(alloc, *st) if host else fn(*st)
            torch.cuda.synchronize()
            alloc.assert_guards_intact()
            runs.append((alloc.records, alloc.payloads()))
            results.append((res, alloc))
            ends.append(tuple(s.cpu().numpy().copy() for s in st))
    finally:
        ctx.set_option("poison_workspaces", -1)
    masks = None
    if masks_of is not None:
        per_run = []
        for res, alloc in results:
            m = masks_of(res, alloc)
            for k, (mask, implied) in m.items():
                assert mask.dtype == np.bool_ and mask.size == alloc.records[k].nbytes
                assert int(mask.sum()) == int(implied), f"{alloc.records[k].label()}: the mask excludes {int(mask.sum())} bytes, its definition implies {int(implied)}"
            per_run.append({k: v[0] for k, v in m.items()})
        for other in per_run[1:]:
            assert other.keys() == per_run[0].keys() and all((other[k] == per_run[0][k]).all() for k in other), "the exception masks differ between the runs"
        masks = per_run[0]
    order = (1, 2, 0)                                                       # A vs B first: that difference names an unwritten byte
    problems = compare_runs([runs[i] for i in order], [RUNS[i][2] for i in order], masks, rows_of)
    for j, (f, a, b) in enumerate(zip(*ends)):
        if not (np.array_equal(a, b) and np.array_equal(a, f)):
            rows = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1) | (a != f).reshape(a.shape[0], -1).any(1))
            problems.append(f"generator state {j}: differs between the runs for tracks {rows[:16].tolist()} ({rows.size} in all)")
    assert not problems, "\n".join(problems)
    return results[0][0]
