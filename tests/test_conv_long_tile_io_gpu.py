"""Tile I/O of the long-block column kernels (conv_long_kernels.hip), long
plan forced ON: the forward kernel's loads and the inverse kernel's stores
are classified per instruction (16 rows x 16 columns) as inside the signal /
the block's outputs, outside, or straddling an end, and only the last kind
tests per lane (tests/test_long_tile_bounds_model.py checks the classification
itself on the CPU).  Here the ends are put where that can go wrong: on an
instruction boundary, one element either side of it, mid-tile, and in a
signal so short that nearly every instruction is outside.

Every call goes through test_conv_long_gpu._run: the input is padded with NaN
beyond n and the output prefilled with NaN and followed by guard cells, so a
load outside [0, n) poisons the result, a missing store leaves a NaN and a
store outside [0, out_len) trips a guard.

In-block positions (N2 = 4096 columns, an instruction = 16 rows): the first
output of a block is point skip = K - 1, i.e.

    K = 65537   row 16, column 0      an instruction boundary
    K = 65536   row 15, column 4095   the last element of an instruction
    K = 100003  row 24, column 1698   mid-tile
    K = 131072  row 31, column 4095

and the signal begins at the same point of block 0.

Bounds: GAMMA err_scale on exact integer references (sparse integer kernel,
dense integer input: conv_exact) as in test_conv_long_gpu.test_three_hops_exact,
the long-double windows and the model of _check_noise for noise through the
Large Church IR, and the contract's 1e-7 RMS / 1e-9 max abs throughout.
"""
import functools

import numpy as np
import pytest

import conv_exact as E
import conv_long_model as LM
from algodsp import irlib, signals
from test_conv_long_gpu import GUARD, _check_exact, _check_noise, _engine, _run

pytestmark = pytest.mark.gpu

INSTR = 16 * LM.N2  # in-block points from one load / store instruction to the next


def _sparse_kernel(K, seed):
    """<= 64 integer taps, the first and the last of the K among them."""
    hpos, hval = E.sparse_int(K, 8192, seed)
    assert hpos[0] == 0 and hpos[-1] == K - 1
    return hpos, hval


def _exact_case(K, n, out_len, seed):
    hpos, hval = _sparse_kernel(K, seed)
    return LM._unit(E.case_sparse_kernel(n, hpos, hval, K, seed + 2, out_len))


def _stride(out_len, parity):
    stride = out_len + GUARD
    return stride + (stride + parity) % 2


@pytest.mark.parametrize("n", [9, 4096 + 7])
def test_tiny_signal_one_partial_block(gpu, n):
    """Almost every load instruction is outside the signal and one straddles
    its end; C = 3 with ir_index [0, 1, 0], in_stride > n, odd out_stride."""
    ir = irlib.large_church()
    index = [0, 1, 0]
    out_len = n + ir.shape[1] - 1
    x = np.stack([signals.white_noise(n, 0x60 + c) for c in range(3)])
    y = _run(_engine(ir, 3, index), x, out_len, in_pad=13, out_stride=_stride(out_len, 1))
    for c, r in enumerate(index):
        _check_noise(y[c], x[c], ir[r], seams=False)


@pytest.mark.parametrize("K", [65537, 65536, 100003, 131072])
def test_skip_positions_exact(gpu, K):
    """The signal's start and the first stored output at the positions listed
    above; n = 11 instructions and a bit, one partial block."""
    n = 11 * INSTR + 1234
    out_len = n + K - 1
    assert out_len <= LM.hop_long(K)
    case = _exact_case(K, n, out_len, 0x70)
    y = _run(_engine(case.h[None, :], 1), case.x[None, :], out_len, in_pad=3, out_stride=_stride(out_len, K % 2))
    _check_exact(y[0], case)


K_EDGE = 65537  # skip = 16 N2: the block's outputs begin on an instruction boundary


@pytest.mark.parametrize("extra,parity", [(1, 0), (INSTR, 1), (INSTR + 1, 0)])
def test_two_blocks_ends_on_instruction_boundaries(gpu, extra, parity):
    """out_len = hop + 1, hop + 16 N2, hop + 16 N2 + 1 at K = 65537: the second
    block stores one element, exactly one instruction, one instruction and an
    element; n = out_len - K + 1 puts the signal's end at the same point of the
    forward kernel's second block.  Even and odd out_stride, in_stride > n."""
    hop = LM.hop_long(K_EDGE)
    out_len = hop + extra
    n = out_len - K_EDGE + 1
    case = _exact_case(K_EDGE, n, out_len, 0x80)
    y = _run(_engine(case.h[None, :], 1), case.x[None, :], out_len, in_pad=11, out_stride=_stride(out_len, parity))
    _check_exact(y[0], case)


@functools.lru_cache(maxsize=None)
def _three_block_case():
    hop = LM.hop_long(K_EDGE)
    out_len = 2 * hop + 5 * INSTR + 77
    return _exact_case(K_EDGE, out_len - K_EDGE + 1, out_len, 0x90)


def test_same_handle_interior_then_edge(gpu):
    """Three blocks (the middle one has every load inside the signal), then a
    short signal on the same handle (one partial block, nearly every load
    outside): each equals a fresh handle's result bit for bit, and the long
    one the exact reference."""
    case = _three_block_case()
    out_len = case.exact.size
    h = case.h[None, :]
    n2 = 4096 + 7
    x2, out2 = case.x[None, :n2], n2 + K_EDGE - 1
    eng = _engine(h, 1)
    y = _run(eng, case.x[None, :], out_len)
    _check_exact(y[0], case)
    y2 = _run(eng, x2, out2, in_pad=5)
    fresh2 = _run(_engine(h, 1), x2, out2, in_pad=5)
    assert np.array_equal(y2, fresh2)
    again = _run(eng, case.x[None, :], out_len)
    assert np.array_equal(again, y)
    hpos, hval = _sparse_kernel(K_EDGE, 0x90)
    xi2 = np.rint(case.x[:n2] * 2.0 ** 15).astype(np.int64)  # _unit's scaling undone: the integers again
    exact2, partial2 = E.sparse_convolve(hpos, hval, xi2, out2)
    _check_exact(y2[0], LM._unit(E.Case("sparse-kernel", xi2, E.densify(hpos, hval, K_EDGE), exact2, partial2)))
