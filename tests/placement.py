"""Placement harness: the buffers of ONE library call inside one arena, each at its exact size between guard bands.

Why: every launcher chooses a 16-byte (float4) or a scalar form from the size and the address of every buffer, and the
suite's buffers are all torch.empty allocations -- 16-byte aligned, with allocator slack behind them.  A float4 tail, a ragged
last tile or a partials row that writes a few words past its buffer lands in memory the process owns and no test reads.

The arena is one uint8 tensor filled with byte 0xFF before every call: every fp32 word is then a NaN, every int64 is -1,
every uint8 is 255.  Each buffer lies at its exact byte size (a workspace at exactly the bytes its size query returned)
between guard bands of GUARD bytes, on the 16-byte grid plus a per-buffer byte offset (0; 4 for fp32; 1 for a byte buffer).
Inputs are copied in after the fill.  After the call, `violations` reports

  (a) every guard byte that is no longer 0xFF                                  ("guard")
  (b) after success: every output element that still holds the fill            ("unwritten")
  (c) after a refusal: every byte of the arena that changed                    ("written after refusal")

What this sees and what it does not: a WRITE outside a buffer is seen as long as it lands inside the arena (a band is
4 KiB; every overrun looked for -- a float4 tail, a tile edge, a partials row -- is far shorter).  A READ outside an input
returns fill (NaN / -1 / 255) or a neighbour's data; it is seen only if it reaches a result, as a NaN or a mismatch in the
caller's comparison with its reference.  A stray read that reaches no result is not detectable this way.  An output element
whose correct value has every byte 0xFF (an fp32 NaN with that exact payload, the int64 -1, the byte 255) would be reported
as unwritten: no entry point produces one on the suite's inputs (the library's NaNs are the canonical 0x7fc00000 or come
from its inputs).

The harness is device-agnostic: tests/test_placement_cpu.py proves each check on CPU tensors with planted violations."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

FILL = 0xFF
GUARD = 4096

# role: "in" (copied in, never checked for the fill), "out" (every element must be written on success), "inout" (the
# caller initialises it and the call rewrites part or all of it: g_model_out's zeroed variance half), "ws" (a workspace: the
# call may leave any part of it untouched)
Buf = namedtuple("Buf", "name shape dtype role")


def nbytes_of(b):
    return int(np.prod(b.shape, dtype=np.int64)) * torch.empty((), dtype=b.dtype).element_size()


class Arena:
    def __init__(self, bufs, offsets=None, device="cpu"):
        """bufs: Buf records in layout order; offsets: {name: bytes off the 16-byte grid} (absent = 0)"""
        offsets = dict(offsets or {})
        unknown = set(offsets) - {b.name for b in bufs}
        assert not unknown, f"offsets for unknown buffers {sorted(unknown)}"
        self.bufs = {b.name: b for b in bufs}
        self.offsets = offsets
        total = GUARD + 32 + sum(((nbytes_of(b) + 15) // 16) * 16 + 16 + GUARD for b in bufs)
        self.mem = torch.empty(total, dtype=torch.uint8, device=device)
        base, cur = self.mem.data_ptr(), 0
        self.span = {}
        for b in bufs:
            off = int(offsets.get(b.name, 0))
            assert 0 <= off < 16 and off % min(torch.empty((), dtype=b.dtype).element_size(), 4) == 0, (b.name, off)
            start = (base + cur + GUARD + 15) // 16 * 16 - base + off      # the ABSOLUTE address is on the grid, plus off
            assert (base + start) % 16 == off and start - cur >= GUARD
            self.span[b.name] = (start, start + nbytes_of(b))
            cur = start + nbytes_of(b)
        assert cur + GUARD <= total
        guard = torch.ones(total, dtype=torch.bool)
        for lo, hi in self.span.values():
            guard[lo:hi] = False
        self.guard = guard.to(device)
        self.fill()

    # ------------------------------------------------------------------ contents
    def fill(self):
        self.mem.fill_(FILL)

    def put(self, name, value):
        """copy an input (numpy array or tensor of the buffer's dtype and element count) into its buffer"""
        b = self.bufs[name]
        t = torch.as_tensor(np.ascontiguousarray(value) if isinstance(value, np.ndarray) else value).contiguous()
        assert t.dtype == b.dtype and t.numel() == int(np.prod(b.shape, dtype=np.int64)), (name, t.dtype, tuple(t.shape))
        lo, hi = self.span[name]
        self.mem[lo:hi].copy_(t.reshape(-1).view(torch.uint8).to(self.mem.device))

    def get(self, name):
        """a copy of the buffer's contents as a tensor of its dtype and shape"""
        b = self.bufs[name]
        lo, hi = self.span[name]
        return self.mem[lo:hi].clone().view(b.dtype).reshape(b.shape)

    def addr(self, name):
        return self.mem.data_ptr() + self.span[name][0]

    def ptr(self, name):
        return None if name is None else ctypes.c_void_p(self.addr(name))

    def nbytes(self, name):
        lo, hi = self.span[name]
        return hi - lo

    def snapshot(self):
        return self.mem.clone()

    # ------------------------------------------------------------------ the three checks
    def _where(self, pos):
        """byte position -> 'k bytes before/after/inside <buffer>'"""
        best = None
        for name, (lo, hi) in self.span.items():
            if lo <= pos < hi:
                return f"byte {pos - lo} of {name}"
            d, txt = (lo - pos, f"{lo - pos} bytes before {name}") if pos < lo else (pos - hi + 1, f"{pos - hi + 1} bytes after {name}")
            if best is None or d < best[0]:
                best = (d, txt)
        return best[1]

    def violations(self, ok, written=(), before=None):
        """ok: the call returned success.  written: the outputs that call must have written in full (default: none; pass
        the names).  before: the snapshot taken just before a call that refused.  -> list of strings, empty when clean"""
        out = []
        bad = torch.nonzero((self.mem != FILL) & self.guard).reshape(-1)
        if bad.numel():
            out.append(f"guard: {bad.numel()} guard bytes changed, first {self._where(int(bad[0]))}")
        if ok:
            for name in written:
                b = self.bufs[name]
                assert b.role == "out", f"{name} is not an output"
                lo, hi = self.span[name]
                size = torch.empty((), dtype=b.dtype).element_size()
                still = (self.mem[lo:hi].reshape(-1, size) == FILL).all(dim=1)
                if bool(still.any()):
                    idx = torch.nonzero(still).reshape(-1)
                    out.append(f"unwritten: {idx.numel()} of {still.numel()} elements of {name} still hold the fill, "
                               f"first element {int(idx[0])}")
        else:
            assert before is not None, "a refusal is checked against the snapshot taken before the call"
            diff = torch.nonzero((self.mem != before) & ~self.guard).reshape(-1)
            if diff.numel():
                out.append(f"written after refusal: {diff.numel()} bytes changed, first {self._where(int(diff[0]))}")
        return out


def placements(names, offset_of):
    """the placements of one case: all aligned, every named pointer offset, each offset alone.
    names: the buffers whose address enters the call's choice of form; offset_of(name) -> its offset (4, or 1 for bytes)"""
    names = list(names)
    out = [("aligned", {})]
    if len(names) > 1:
        out.append(("all", {n: offset_of(n) for n in names}))
    out += [(n, {n: offset_of(n)}) for n in names]
    return out
