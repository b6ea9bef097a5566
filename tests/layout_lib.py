"""Guarded buffer placements for the device-buffer layout contract
(include/algodsp.h, "Device buffers").

A test places a [C][len] array at a chosen base offset and row stride inside
one flat allocation it owns whole: a front guard, `base_off` elements, C rows
of `len` at stride `len + stride_pad` with nothing after the last row (a
buffer of C rows is (C-1)*stride + len elements), a back guard.  Every element
that is not payload holds a quiet NaN whose mantissa carries the element's own
index, compared as int64: a kernel that reads one poisons its result, a kernel
that writes one -- or copies one guard slot over another -- changes its bits.
The guards (16384 elements each side, more than the largest FFT block) keep a
one-block overrun inside memory the test owns, so a wrong kernel is found by
inspection and never by a fault.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

GUARD = 16384  # elements before the base and after the last row (even: keeps the 16-byte phase)

_QNAN = 0x7FF8_0000_0000_0000  # float64 quiet NaN; the low 51 bits are free
_OUT_TAG = 1 << 40             # payload slots of an output placement: index NaNs of their own range
_QNAN16 = 0x7E00               # float16 quiet NaN; 9 free bits

Layout = namedtuple("Layout", "base_off stride_pad")

L0 = Layout(0, 0)     # contiguous; 16-byte aligned rows when len is even
L1 = Layout(0, 3)     # stride parity flips against len: row alignment alternates when the stride is odd
L3 = Layout(1, 1001)  # base 8 bytes off 16-byte alignment, wide padding


def L2(length: int) -> Layout:
    """Base 8 bytes off 16-byte alignment and an even stride: every row is unaligned."""
    return Layout(1, 2 + (length & 1))


def LA(length: int) -> Layout:
    """The reference placement: base and every row 16-byte aligned (L0 itself
    when len is even; one element of padding when it is odd)."""
    return Layout(0, length & 1)


def variants(length: int):
    """Every placement a case runs besides the reference LA(length)."""
    out = [L1, L2(length), L3]
    return out if LA(length) == L0 else [L0] + out


class Buf:
    """One placement: `flat` (the whole allocation), geometry, and `expect`, the
    int64 image of `flat` as placed."""

    def __init__(self, flat, expect, C, length, stride, base, itemsize):
        self.flat, self.expect = flat, expect
        self.C, self.len, self.stride, self.base, self.itemsize = C, length, stride, base, itemsize

    @property
    def ptr(self) -> int:
        """Device (or host) address of row 0, column 0."""
        return self.flat.data_ptr() + self.itemsize * self.base

    @property
    def end(self) -> int:
        return self.base + (self.C - 1) * self.stride + self.len

    def payload_mask(self) -> np.ndarray:
        m = np.zeros(self.expect.size, dtype=bool)
        for c in range(self.C):
            m[self.base + c * self.stride:self.base + c * self.stride + self.len] = True
        return m


def _guard_image(total: int, dtype) -> np.ndarray:
    idx = np.arange(total, dtype=np.int64)
    if dtype == np.float64:
        return idx + _QNAN
    if dtype == np.uint16:
        return ((idx % 511) + 1 + _QNAN16).astype(np.int64)
    raise TypeError(f"layout_lib: unsupported dtype {dtype}")


def _build(x, C, length, layout, device, dtype):
    base_off, pad = layout
    if base_off < 0 or pad < 0 or C < 1 or length < 1:
        raise ValueError("layout_lib: negative offset / padding or empty payload")
    stride = length + pad
    base = GUARD + base_off
    total = base + (C - 1) * stride + length + GUARD
    img = _guard_image(total, dtype)
    pay = np.zeros(total, dtype=bool)
    for c in range(C):
        pay[base + c * stride:base + c * stride + length] = True
    if x is None:
        if dtype != np.float64:
            raise TypeError("layout_lib: output placements are float64")
        img[pay] += _OUT_TAG
    elif dtype == np.float64:
        img[pay] = np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.int64)
    else:
        img[pay] = np.ascontiguousarray(x, dtype=np.uint16).reshape(-1).astype(np.int64)
    if dtype == np.float64:
        flat = torch.from_numpy(img.copy().view(np.float64)).to(device)
        itemsize = 8
    else:
        flat = torch.from_numpy(img.astype(np.uint16).view(np.int16)).to(device)
        itemsize = 2
    assert flat.data_ptr() % 16 == 0, "layout_lib: allocation is not 16-byte aligned"
    return Buf(flat, img, C, length, stride, base, itemsize)


def place(x, layout: Layout, device="cpu") -> Buf:
    """`x` ([C][len], or 1-D for one row; float64 or uint16) placed at `layout`."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    dtype = np.uint16 if x.dtype == np.uint16 else np.float64
    return _build(x, x.shape[0], x.shape[1], layout, device, dtype)


def empty(C: int, length: int, layout: Layout, device="cpu") -> Buf:
    """An output placement: the payload too holds index NaNs (of a range of
    their own), so an element the call did not write is still recognisable."""
    return _build(None, C, length, layout, device, np.float64)


def rows(buf: Buf):
    """The [C][len] payload view of the placement (a torch view of `flat`)."""
    return buf.flat.as_strided((buf.C, buf.len), (buf.stride, 1), buf.base)


def image(buf: Buf) -> np.ndarray:
    """int64 image of the whole allocation as it is now."""
    a = buf.flat.cpu().numpy()
    return a.view(np.int64).copy() if buf.itemsize == 8 else a.view(np.uint16).astype(np.int64)


def payload(buf: Buf) -> np.ndarray:
    """The [C][len] payload as a host array (float64 or uint16)."""
    a = buf.flat.cpu().numpy()
    a = a if buf.itemsize == 8 else a.view(np.uint16)
    return np.stack([a[buf.base + c * buf.stride:buf.base + c * buf.stride + buf.len] for c in range(buf.C)])


def where(buf: Buf, i: int) -> str:
    """Flat element index -> a location a person can act on."""
    if i < buf.base:
        return f"front guard, {buf.base - i} element(s) before the base"
    if i >= buf.end:
        return f"back guard, {i - buf.end + 1} element(s) after the last row"
    r, c = divmod(i - buf.base, buf.stride)
    if c >= buf.len:
        return f"padding after row {r}, column {c} ({c - buf.len + 1} past len {buf.len})"
    return f"row {r}, column {c}"


def _first_diff(buf, now, mask, what):
    bad = np.flatnonzero((now != buf.expect) & mask)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {where(buf, i)} changed (flat index {i}: {int(buf.expect[i]):#x} -> "
                             f"{int(now[i]):#x}; {bad.size} element(s) differ)")


def check_guards(buf: Buf, untouched=()):
    """Every guard element -- front, inter-row padding, back -- is bit-unchanged.
    `untouched`: column ranges (lo, hi) of every payload row that must also
    still hold what the placement put there (the part of an output a segment
    call must not write)."""
    now = image(buf)
    mask = ~buf.payload_mask()
    for lo, hi in untouched:
        for c in range(buf.C):
            mask[buf.base + c * buf.stride + lo:buf.base + c * buf.stride + min(hi, buf.len)] = True
    _first_diff(buf, now, mask, "guard")


def check_unchanged(buf: Buf, x=None):
    """The payload of an input is bit-unchanged (against `x` when given, which
    must itself be what was placed), and so is every guard element."""
    now = image(buf)
    if x is not None:
        x = np.asarray(x)
        want = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.int64) if buf.itemsize == 8
                else np.ascontiguousarray(x, dtype=np.uint16).reshape(-1).astype(np.int64))
        assert np.array_equal(buf.expect[buf.payload_mask()], want), "check_unchanged: x is not what was placed"
    _first_diff(buf, now, np.ones(now.size, dtype=bool), "input")
