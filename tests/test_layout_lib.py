"""The layout helper of the device-buffer contract tests, proven on CPU
tensors: the guard check passes on an untouched placement and fails, naming
the place, after each single stray write a kernel could make."""
import numpy as np
import pytest
import torch

import layout_lib as LL

C, N = 3, 10


def _x():
    return np.arange(C * N, dtype=np.float64).reshape(C, N) + 0.5


@pytest.mark.parametrize("lay", [LL.L0, LL.L1, LL.L2(N), LL.L2(N + 1), LL.L3])
def test_geometry_and_clean_pass(lay):
    x = _x()
    b = LL.place(x, lay)
    assert b.stride == N + lay.stride_pad and b.base == LL.GUARD + lay.base_off
    assert b.flat.numel() == 2 * LL.GUARD + lay.base_off + (C - 1) * b.stride + N  # no padding after the last row
    assert b.ptr == b.flat.data_ptr() + 8 * b.base
    assert LL.GUARD >= 16384 and LL.GUARD % 2 == 0
    assert np.array_equal(LL.rows(b).numpy(), x) and np.array_equal(LL.payload(b), x)
    assert LL.rows(b).data_ptr() == b.ptr
    g = b.flat.numpy()[~b.payload_mask()]
    assert np.isnan(g).all() and np.unique(g.view(np.int64)).size == g.size  # every guard slot is its own NaN
    LL.check_guards(b)
    LL.check_unchanged(b, x)
    o = LL.empty(C, N, lay)
    assert np.isnan(o.flat.numpy()).all() and np.unique(LL.image(o)).size == o.flat.numel()
    LL.check_guards(o, untouched=[(0, N)])
    LL.rows(o)[:, 2:5] = 1.0  # a segment call's own range
    LL.check_guards(o, untouched=[(0, 2), (5, N)])
    with pytest.raises(AssertionError, match=r"row 0, column 2"):
        LL.check_guards(o, untouched=[(0, N)])


def test_l2_rows_all_unaligned_l1_alternates():
    for n in (N, N + 1):
        b = LL.place(np.zeros((C, n)), LL.L2(n))
        assert b.stride % 2 == 0 and all((b.ptr + 8 * c * b.stride) % 16 == 8 for c in range(C))
    b = LL.place(np.zeros((C, N)), LL.L1)
    assert [(b.ptr + 8 * c * b.stride) % 16 for c in range(C)] == [0, 8, 0]
    assert LL.place(np.zeros((C, N)), LL.L0).ptr % 16 == 0


@pytest.mark.parametrize("lay", [LL.L1, LL.L3])
def test_stray_writes_are_named(lay):
    def fresh():
        return LL.place(_x(), lay)

    b = fresh()
    b.flat[b.base + 1 * b.stride + N] = 0.0  # one element past row 1's len
    with pytest.raises(AssertionError, match=r"padding after row 1, column 10 \(1 past len 10\)"):
        LL.check_guards(b)

    b = fresh()
    b.flat[b.base - 1] = 0.0  # one element before the base
    with pytest.raises(AssertionError, match=r"front guard, 1 element\(s\) before the base"):
        LL.check_guards(b)

    b = fresh()
    b.flat[b.end] = 0.0  # one element after the last row
    with pytest.raises(AssertionError, match=r"back guard, 1 element\(s\) after the last row"):
        LL.check_guards(b)

    b = fresh()
    b.flat[b.base + N + 1] = b.flat[b.base + N].clone()  # a guard slot copied over its neighbour: still a NaN
    assert torch.isnan(b.flat[b.base + N + 1])
    with pytest.raises(AssertionError, match=r"padding after row 0, column 11 \(2 past len 10\)"):
        LL.check_guards(b)

    b = fresh()
    v = LL.rows(b).view(torch.int64)
    v[2, 7] ^= 1  # one flipped payload bit of an input
    LL.check_guards(b)  # not a guard
    with pytest.raises(AssertionError, match=r"input: row 2, column 7"):
        LL.check_unchanged(b, _x())


def test_uint16_placement():
    codes = (np.arange(2 * 7, dtype=np.uint16) * 37).reshape(2, 7)
    b = LL.place(codes, LL.Layout(3, 5))
    assert b.ptr == b.flat.data_ptr() + 2 * (LL.GUARD + 3)
    assert np.array_equal(LL.payload(b), codes)
    g = LL.image(b)[~b.payload_mask()]
    assert ((g & 0x7C00) == 0x7C00).all() and ((g & 0x3FF) != 0).all()  # every guard is a half-precision NaN
    LL.check_unchanged(b, codes)
    b.flat[b.base + 7] = 0
    with pytest.raises(AssertionError, match=r"padding after row 0, column 7"):
        LL.check_unchanged(b, codes)
