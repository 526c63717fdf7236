"""Guarded, poisoned device buffers for the buffer-contract tests (a helper module like ``graph_cases.py``: no tests here).

``GuardedAlloc`` is a context manager.  Inside its block ``torch.empty`` and ``torch.empty_like`` are replaced: every
contiguous allocation on the guarded device type is carved out of a larger ``uint8`` buffer laid out as

    [ band | exactly the requested bytes | band ]

and the whole buffer is filled with byte 0xFF before it is handed out (NaN as fp32 and fp16, -1 as int32 and int64).  A
kernel that writes a few rows past the end of a workspace, graph view or output lands in a band, where ``check()`` finds
it; a kernel that reads a word nobody wrote gets NaN / -1 instead of the zeros of a fresh allocator block.  The payload
is exact: the caching allocator's rounding to 512 bytes, which normally hides an overrun in slack, is gone.

The band is 64 KiB on each side: four times the largest single tile store in the library (16 rows of 256 floats,
16 KiB), and a multiple of 512, so the 256-byte alignment the plans and workspaces require is kept.

Calls pass through unchanged for tensors on another device type, for results that are not contiguous (``empty_like`` of
a strided tensor, a ``memory_format``), for ``out=`` and while the current stream is capturing: a captured step
(``GraphedTrainStep``, ``torch.cuda.graph``) allocates from the graph's pool and is out of this harness's reach.
Allocations made by torch's C++ side (``torch.zeros``, ``clone``, the results of operators) are not replaced either.

``guarded_copy(t)`` puts a test input into the same kind of buffer: 0xFF bands for floating-point inputs (a read past
``x[n_nodes]`` comes back NaN), bands of zero bytes for index inputs (a stray read of an index is the valid index 0: a
wrong value, never a wild address).
"""
from __future__ import annotations

import os
import sys

import torch

BAND = 64 * 1024
POISON = 0xFF


class GuardError(AssertionError):
    """A byte of a guard band changed."""


class Allocation:
    """One guarded buffer: ``raw`` (uint8, band + payload + band), the payload's bytes and the requested shape / dtype."""
    __slots__ = ("index", "raw", "nbytes", "shape", "dtype", "fill", "kind", "band", "site")

    def __init__(self, index, raw, nbytes, shape, dtype, fill, kind, band, site):
        self.index, self.raw, self.nbytes, self.shape, self.dtype = index, raw, nbytes, tuple(shape), dtype
        self.fill, self.kind, self.band, self.site = fill, kind, band, site

    def payload(self):
        """The payload as the tensor that was handed out (a view of ``raw``)."""
        return self.raw[self.band:self.band + self.nbytes].view(self.dtype).view(self.shape)

    def data_ptr(self):
        return self.raw.data_ptr() + self.band

    def describe(self):
        return (f"allocation #{self.index} ({self.kind}) shape={self.shape} dtype={self.dtype} bytes={self.nbytes}"
                f" from {self.site}")


class GuardedAlloc:
    def __init__(self, device_type="cuda", band=BAND):
        assert band > 0 and band % 512 == 0, "the band keeps the allocator's 512-byte alignment"
        self.device_type = device_type
        self.band = band
        self.allocations = []
        self._saved = []

    # -- the interposer -------------------------------------------------------------------------------------------------
    def _capturing(self):
        return self.device_type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    @staticmethod
    def _site():
        """directory/file:line of the first caller outside this module."""
        f = sys._getframe(1)
        while f is not None and f.f_code.co_filename == __file__:
            f = f.f_back
        if f is None:
            return "?"
        return f"{os.sep.join(f.f_code.co_filename.split(os.sep)[-2:])}:{f.f_lineno}"

    def _carve(self, empty, shape, dtype, device, fill, kind):
        nbytes = dtype.itemsize
        for s in shape:
            nbytes *= int(s)
        raw = empty(2 * self.band + nbytes, dtype=torch.uint8, device=device)
        raw.fill_(fill)
        rec = Allocation(len(self.allocations), raw, nbytes, shape, dtype, fill, kind, self.band, self._site())
        self.allocations.append(rec)
        return rec

    def _guard(self, empty, plain, kind):
        """``plain``: what the original call returned.  Its guarded twin, or ``plain`` itself where the call passes through."""
        if (plain.device.type != self.device_type or plain.layout != torch.strided or not plain.is_contiguous()
                or self._capturing()):
            return plain
        rec = self._carve(empty, plain.shape, plain.dtype, plain.device, POISON, kind)
        out = rec.payload()
        if plain.requires_grad:
            out.requires_grad_(True)
        return out

    def __enter__(self):
        empty, empty_like = torch.empty, torch.empty_like
        self._saved.append((empty, empty_like))

        def guarded_empty(*args, **kwargs):
            plain = empty(*args, **kwargs)
            return plain if kwargs.get("out") is not None else self._guard(empty, plain, "empty")

        def guarded_empty_like(*args, **kwargs):
            return self._guard(empty, empty_like(*args, **kwargs), "empty_like")

        torch.empty, torch.empty_like = guarded_empty, guarded_empty_like
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self._saved.pop()
        return False

    # -- inputs -----------------------------------------------------------------------------------------------------------
    def guarded_copy(self, t):
        """``t`` (contiguous copy) in a guarded buffer on its own device: NaN bands for floats, zero bands for indices."""
        empty = self._saved[-1][0] if self._saved else torch.empty
        t = t.detach().contiguous()
        fill = POISON if (t.dtype.is_floating_point or t.dtype.is_complex) else 0
        rec = self._carve(empty, t.shape, t.dtype, t.device, fill, "input")
        out = rec.payload()
        out.copy_(t)
        return out

    # -- bookkeeping ------------------------------------------------------------------------------------------------------
    def sizes(self, kind=None):
        """Payload byte counts of the recorded allocations (``kind``: 'empty', 'empty_like' or 'input'; None: all)."""
        return [a.nbytes for a in self.allocations if kind is None or a.kind == kind]

    def find(self, nbytes=None, shape=None, dtype=None):
        """The recorded allocations (inputs excluded) that match every given property."""
        return [a for a in self.allocations if a.kind != "input"
                and (nbytes is None or a.nbytes == nbytes)
                and (shape is None or a.shape == tuple(shape))
                and (dtype is None or a.dtype == dtype)]

    def holds(self, t):
        """The allocation whose payload starts where ``t`` does and has its size, or None."""
        for a in self.allocations:
            if a.data_ptr() == t.data_ptr() and a.nbytes == t.numel() * t.element_size():
                return a
        return None

    def check(self):
        """Synchronise, then assert that every byte of both bands of every recorded allocation still holds its fill."""
        if self.device_type == "cuda" and torch.cuda.is_available():
            torch.cuda.synchronize()
        if not self.allocations:
            return
        counts = []
        for a in self.allocations:
            b, n = a.band, a.nbytes
            counts.append(torch.stack([(a.raw[:b] != a.fill).sum(), (a.raw[b + n:] != a.fill).sum()]).cpu())
        problems = []
        for a, c in zip(self.allocations, counts):
            b, n = a.band, a.nbytes
            for side, cnt, band, base in (("below", int(c[0]), a.raw[:b], -b), ("above", int(c[1]), a.raw[b + n:], n)):
                if cnt:
                    hit = (band != a.fill).nonzero().view(-1)
                    first, last = int(hit[0]) + base, int(hit[-1]) + base
                    problems.append(f"{a.describe()}: {cnt} byte(s) of the band {side} the payload changed, payload-relative "
                                    f"offsets {first}..{last} (payload is [0, {n}))")
        if problems:
            raise GuardError("guard band overwritten:\n  " + "\n  ".join(problems))
