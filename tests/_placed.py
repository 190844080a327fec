"""Arrays at a chosen byte offset inside guard bands: the one helper of the placement tests.

include/ccx.h asks little of a pointer (16 bytes for observation, compact, logit and Q rows, 8 for f64, 4 for most f32
arrays, nothing for u8), while ``torch.empty`` hands out 512-byte boundaries.  ``place`` puts a view at ``base + guard +
offset`` of one u8 allocation whose base is a multiple of 128 and whose every byte holds a sentinel, so that a test
chooses the residue of the address mod 128 and sees every byte written in front of the view or behind it.  Works on
CPU tensors as well (tests/test_placed_host.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

SENTINEL = 0xA5
GUARD = 4096
LINE = 128


@dataclass
class Placed:
    """The whole allocation of one placed view."""

    buf: torch.Tensor      # u8 [guard + 128 + nbytes + guard]
    view: torch.Tensor     # the view handed to the library
    start: int             # byte offset of the view inside buf (guard + offset)
    nbytes: int
    offset: int

    def front(self) -> torch.Tensor:
        return self.buf[:self.start]

    def back(self) -> torch.Tensor:
        return self.buf[self.start + self.nbytes:]

    def body(self) -> torch.Tensor:
        return self.buf[self.start:self.start + self.nbytes]


def _aligned_u8(total: int, device) -> torch.Tensor:
    """A u8 buffer of ``total`` bytes whose base is a multiple of 128 (the allocators give that; CPU memory is cut to it)."""
    raw = torch.empty(total + LINE, dtype=torch.uint8, device=device)
    buf = raw[(-raw.data_ptr()) % LINE:][:total]
    assert buf.data_ptr() % LINE == 0, hex(buf.data_ptr())
    return buf


def place(shape, dtype, offset: int, guard: int = GUARD, device="cuda"):
    """-> (view, handle): a contiguous ``shape`` / ``dtype`` view at ``base + guard + offset``, base % 128 == 0, every
    byte of the allocation (the view's included) set to the sentinel.  ``offset`` in bytes, 0 <= offset < 128, a
    multiple of the dtype's size."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    assert 0 <= offset < LINE and offset % item == 0, (offset, dtype)
    assert guard % LINE == 0 and guard > 0, guard
    n = 1
    for s in shape:
        n *= s
    nbytes = n * item
    buf = _aligned_u8(guard + LINE + nbytes + guard, device)
    buf.fill_(SENTINEL)
    start = guard + offset
    view = buf[start:start + nbytes].view(dtype).view(shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + start
    assert view.data_ptr() % LINE == offset
    return view, Placed(buf, view, start, nbytes, offset)


def placed_like(t: torch.Tensor, offset: int, guard: int = GUARD):
    """``place`` with the contents of ``t`` copied in (for inputs)."""
    view, handle = place(t.shape, t.dtype, offset, guard, device=t.device)
    view.copy_(t)
    return view, handle


def _touched(part: torch.Tensor):
    idx = torch.nonzero(part != SENTINEL).flatten()
    return None if idx.numel() == 0 else (int(idx[0]), int(idx[-1]), int(idx.numel()))


def assert_guards(handle: Placed, what: str) -> None:
    """Every byte in front of the view and behind it still holds the sentinel; the message names the array and the first
    and last touched byte offsets relative to the view's first byte."""
    f, b = _touched(handle.front()), _touched(handle.back())
    msgs = []
    if f is not None:
        msgs.append(f"{f[2]} byte(s) written IN FRONT of {what}: offsets {f[0] - handle.start} .. {f[1] - handle.start} "
                    f"relative to the view")
    if b is not None:
        msgs.append(f"{b[2]} byte(s) written BEHIND {what}: offsets {handle.nbytes + b[0]} .. {handle.nbytes + b[1]} relative "
                    f"to the view ({b[0]} .. {b[1]} behind its end)")
    assert not msgs, f"{what} ({handle.nbytes} bytes placed at +{handle.offset}): " + "; ".join(msgs)


def assert_unchanged(handle: Placed, original: torch.Tensor, what: str) -> None:
    """An input's own bytes are those of ``original`` and its guards are intact."""
    assert_guards(handle, what)
    same = torch.equal(handle.body(), original.contiguous().view(-1).view(torch.uint8).to(handle.buf.device))
    assert same, f"input {what} placed at +{handle.offset} was written by the call"


def assert_residue(t: torch.Tensor, offset: int, align: int, what: str) -> None:
    """The premise of a case: the address has the residue asked for mod 128 and satisfies the alignment the header
    states for that pointer -- and, for offsets that are not a multiple of the next power of two, no stricter one."""
    p = t.data_ptr()
    assert p % LINE == offset, f"{what}: address {p:#x} is at +{p % LINE} of its line, wanted +{offset}"
    assert p % align == 0, f"{what}: address {p:#x} breaks the {align}-byte alignment of include/ccx.h"


class PlacedCall:
    """The placed arrays of one library call: every output and every input with its handle, the premise (residue mod 128,
    the alignment the header states) asserted as each is made.  ``check`` is what every placement test ends a call with."""

    def __init__(self, ctx: str, device="cuda"):
        self.ctx, self.device, self.outs, self.ins, self.scratches = ctx, device, {}, {}, {}

    def out(self, name, shape, dtype, offset, align):
        view, h = place(shape, dtype, offset, device=self.device)
        assert_residue(view, offset, align, f"{self.ctx}: {name}")
        assert name not in self.outs, name
        self.outs[name] = (view, h)
        return view

    def scratch(self, name, nbytes, offset, align):
        """A u8 workspace whose contents mean nothing after the call: only its guards are checked."""
        view, h = place((max(int(nbytes), 1),), torch.uint8, offset, device=self.device)
        assert_residue(view, offset, align, f"{self.ctx}: {name}")
        assert name not in self.scratches, name
        self.scratches[name] = (view, h)
        return view

    def inp(self, name, array, offset, align):
        """``array`` (NumPy or tensor; ``None`` passes through) copied to a placed view; the original is kept to compare."""
        if array is None:
            return None
        src = array.detach() if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        src = src.to(self.device).contiguous()
        view, h = placed_like(src, offset)
        assert_residue(view, offset, align, f"{self.ctx}: {name}")
        assert name not in self.ins, name
        self.ins[name] = (view, h, src)
        return view

    def check(self, expected: dict) -> None:
        """Every output equals ``expected[name]`` byte for byte, the guards of outputs and inputs are intact, and the
        inputs' own bytes are unchanged.  The messages name the array, its offset and the byte range."""
        if self.device != "cpu":
            torch.cuda.synchronize()
        assert set(expected) == set(self.outs), (self.ctx, sorted(expected), sorted(self.outs))
        for name, (_view, h) in self.outs.items():
            assert_guards(h, f"{self.ctx}: output {name}")
            got = h.body().cpu().numpy()
            want = expected[name]
            want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.ascontiguousarray(want)
            want = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
            assert got.shape == want.shape, (self.ctx, name, got.shape, want.shape)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"{self.ctx}: output {name} placed at +{h.offset} differs from the expected bits in "
                                     f"{bad.size} of {got.size} bytes, byte offsets {bad[0]} .. {bad[-1]}")
        for name, (_view, h) in self.scratches.items():
            assert_guards(h, f"{self.ctx}: workspace {name}")
        for name, (_view, h, src) in self.ins.items():
            assert_unchanged(h, src, f"{self.ctx}: input {name}")
