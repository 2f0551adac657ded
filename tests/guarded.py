"""Test infrastructure: guard-banded, poisoned, strided buffers for calls through the C ABI.

A kernel promises which elements it writes (include/brepgen_hip.h: "only columns < N are written", "entries past offsets[B] are
not written", "0-padded" ...).  With an exactly sized ``torch.empty`` output and ``ldc == N`` none of that is visible: a store to
column N of row m lands on row m + 1 where the rightful writer overwrites it, a store past the last row lands in the allocator's
slack, and a skipped tile still holds the previous call's (correct) result.  ``guarded`` makes all three visible:

    front guard | rows x ld elements (cols logical + ld - cols padding per row) | rear guard

everything pre-filled with one sentinel bit pattern -- a NaN with a recognisable payload for the floating types, 0xA5 bytes for the
integer types.  Checks reinterpret the buffer as integers of the same width and compare bits; floats are never compared (NaN != NaN),
and no torch arithmetic touches the data.
"""
import math

import torch

# (integer view dtype, sentinel as a signed value of that type)
_SENTINEL = {
    torch.float32: (torch.int32, 0x7FC0A5A5),                                   # quiet NaN, payload 0x00A5A5
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
    torch.bfloat16: (torch.int16, 0x7FE5),                                      # 0 11111111 1100101
    torch.float16: (torch.int16, 0x7EA5),                                       # 0 11111 1010100101
    torch.int64: (torch.int64, 0xA5A5A5A5A5A5A5A5 - (1 << 64)),
    torch.int32: (torch.int32, 0xA5A5A5A5 - (1 << 32)),
    torch.int16: (torch.int16, 0xA5A5 - (1 << 16)),
    torch.uint8: (torch.uint8, 0xA5),
    torch.int8: (torch.int8, 0xA5 - (1 << 8)),
}


def sentinel_bits(dtype):
    """(integer dtype of the same width, sentinel value) for `dtype`."""
    try:
        return _SENTINEL[dtype]
    except KeyError:
        raise TypeError(f"guarded: no sentinel for {dtype}") from None


class Guarded:
    def __init__(self, shape, dtype, device, ld=None, guard=256):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.cols = shape[-1]
        self.rows = math.prod(shape[:-1])
        self.ld = self.cols if ld is None else ld
        assert self.ld >= self.cols and guard >= 0 and self.rows >= 0
        self.guard, self.dtype = guard, dtype
        self._idt, self._bits = sentinel_bits(dtype)
        n = self.rows * self.ld
        self.flat = torch.empty(2 * guard + n, dtype=dtype, device=device)
        self._ibuf = self.flat.view(self._idt)
        self._ibuf.fill_(self._bits)
        # 16-byte alignment of the logical origin: torch allocations are at least 64-byte aligned, so the guard decides
        assert (self.flat.data_ptr() + guard * self.flat.element_size()) % 16 == 0, \
            "guarded: choose `guard` so that guard * element size is a multiple of 16 bytes"
        self.view = self.flat.as_strided((self.rows, self.cols), (self.ld, 1), guard)

    def _body(self):
        return self._ibuf[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)

    def assert_untouched(self, what="buffer"):
        """Front guard, rear guard and the padding of every row still hold the sentinel, bit for bit."""
        g, n = self.guard, self.rows * self.ld
        for name, part in (("front", self._ibuf[:g]), ("rear", self._ibuf[g + n:])):
            bad = (part != self._bits).nonzero()
            if bad.numel():
                off = int(bad[0])
                rel = off - g if name == "front" else off
                raise AssertionError(f"{what}: {name} guard written at offset {rel} "
                                     f"({'elements before the first' if name == 'front' else 'elements past the last'} row; "
                                     f"{bad.shape[0]} stray elements, bits {int(part[off]) & ((1 << 8 * part.element_size()) - 1):#x})")
        if self.ld > self.cols and self.rows:
            bad = (self._body()[:, self.cols:] != self._bits).nonzero()
            if bad.numel():
                r, c = int(bad[0, 0]), int(bad[0, 1]) + self.cols
                raise AssertionError(f"{what}: row padding written at (row {r}, column {c}) of a [{self.rows}, {self.cols}] "
                                     f"tensor with row stride {self.ld} ({bad.shape[0]} stray elements)")

    def assert_fully_written(self, what="buffer"):
        """No logical element still carries the sentinel bits."""
        if not self.rows:
            return
        bad = (self._body()[:, :self.cols] == self._bits).nonzero()
        if bad.numel():
            raise AssertionError(f"{what}: element (row {int(bad[0, 0])}, column {int(bad[0, 1])}) of a [{self.rows}, {self.cols}] "
                                 f"tensor with row stride {self.ld} was not written ({bad.shape[0]} unwritten elements)")

    def written_mask(self):
        """bool [rows, cols]: True where the logical element no longer carries the sentinel."""
        return self._body()[:, :self.cols] != self._bits


def guarded(shape, dtype, device, ld=None, guard=256):
    """One flat sentinel-filled buffer: `guard` elements, rows x ld elements, `guard` elements; see the module docstring.
    shape [..., cols]: the leading dimensions are flattened into rows.  Members: .view ([rows, cols], row stride ld, 16-byte
    aligned origin), .ld, .assert_untouched(), .assert_fully_written()."""
    return Guarded(shape, dtype, device, ld, guard)


def strided_input(t, ld, guard=256):
    """A copy of the 2-D tensor `t` with row stride `ld` whose row padding (and guard bands) hold the sentinel: a kernel that reads
    with the wrong stride, or that sums the padding, produces NaN (or 0xA5A5.. garbage for integers)."""
    assert t.dim() == 2
    g = Guarded(t.shape, t.dtype, t.device, ld, guard)
    g.view.copy_(t)
    return g.view
