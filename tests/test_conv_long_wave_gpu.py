"""The long-block plan's wave-local exchanges (conv_long_kernels.hip), long
plan forced ON.

The row kernel deals its butterflies so that wave = k0 and syncs four of its
six exchanges at wave scope.  Three things can go wrong that the existing
cases need not show:
a digit routed to the wrong lane or slice, an exchange that lacks a sync, and
a slice shared between co-resident items.

Digit sweep: x = e_p, h = e_Q1 + 2 e_Q2 (K = 4096), so y = e_(p+Q1) +
2 e_(p+Q2) exactly.  Block 0 starts at -(K - 1): x[p] sits at in-block index
i = p + K - 1 = N2 n1 + n2.  p runs over every single radix-8 digit of n2
(512 a, 64 a, 8 a, a for a = 1 .. 7, at n1 = 1, the least that keeps p >= 0),
every pass digit of n1 of the 512-point column plan (radix 2, 16, 16: 256,
16 a, a for a = 1 .. 15, at n2 = 0), and sums of these.  Bound: GAMMA
err_scale as for the exact cases of test_conv_long_gpu.py, plus the contract.

Race check: five calls on one handle must agree bit for bit (an exchange
without its sync shows as run-to-run difference), and the result passes the
long-double windows and the model of test_conv_long_gpu._check_noise.
"""
import numpy as np
import pytest

import conv_exact as E
import conv_long_model as LM
from algodsp import irlib, signals
from test_conv_long_gpu import _check_exact, _check_noise, _engine, _run

pytestmark = pytest.mark.gpu

K = 4096
Q1, Q2 = 5, K - 1
N2_DIGITS = {f"n2-digit-{w}": [LM.N2 + w * a for a in range(1, 8)] for w in (512, 64, 8, 1)}
N1_DIGITS = {
    "n1-pass0": [LM.N2 * 256],
    "n1-pass1": [LM.N2 * 16 * a for a in range(1, 16)],
    "n1-pass2": [LM.N2 * a for a in range(1, 16)],
}
SUMS = {
    "sums": [
        LM.N2 + 512 * 7 + 64 * 7 + 8 * 7 + 7,            # n2 = 4095: every digit at its top
        LM.N2 + 512 * 1 + 64 * 2 + 8 * 3 + 4,
        LM.N2 * 3 + 512 * 5 + 1,
        LM.N2 * (256 + 16 * 9 + 6) + 64 * 3 + 8 * 6,
        LM.N2 * 510 + 4095,                              # the last column
        LM.N2 * 511,                                     # the largest index one partial block holds
        LM.N2 * (16 * 15 + 15) + 512 * 4 + 64 * 4 + 8 * 4 + 4,
    ]
}
GROUPS = {**N2_DIGITS, **N1_DIGITS, **SUMS}


@pytest.fixture(scope="module")
def pair_engine(gpu):
    h = np.zeros(K)
    h[Q1], h[Q2] = 1.0, 2.0
    return h, _engine(h[None, :], 1)


@pytest.mark.parametrize("group", list(GROUPS))
def test_digit_sweep(pair_engine, group):
    h, eng = pair_engine
    for i in GROUPS[group]:
        p = i - (K - 1)
        assert p >= 0
        n = p + 1
        out_len = n + K - 1
        assert out_len <= LM.hop_long(K), "one partial block"
        x = E.impulse(n, p, 1.0)
        exact = np.zeros(out_len)
        exact[p + Q1], exact[p + Q2] = 1.0, 2.0
        case = E.Case(f"{group} i={i}", x, h, exact)
        y = _run(eng, x[None, :], out_len)
        _check_exact(y[0], case)


def _church_noise(channels, seed):
    ir = irlib.large_church()
    out_len = LM.hop_long(ir.shape[1]) + 4097  # two blocks, the second 4097 samples
    n = out_len - ir.shape[1] + 1
    return ir, np.stack([signals.white_noise(n, seed + c) for c in range(channels)]), out_len


def test_race_five_calls(gpu):
    ir, x, out_len = _church_noise(2, 0x40)
    eng = _engine(ir, 2)
    ys = [_run(eng, x, out_len) for _ in range(5)]
    for k in range(1, 5):
        assert np.array_equal(ys[0], ys[k]), f"call {k} differs from call 0"
    for c in range(2):
        _check_noise(ys[0][c], x[c], ir[c])


def test_many_items(gpu):
    """C = 3 with ir_index [0, 1, 0] over two blocks: six items per row and
    column tile, guard cells and NaN prefill as in _run."""
    ir, x, out_len = _church_noise(3, 0x50)
    index = [0, 1, 0]
    y = _run(_engine(ir, 3, index), x, out_len)
    for c, r in enumerate(index):
        _check_noise(y[c], x[c], ir[r])
