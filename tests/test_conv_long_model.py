"""CPU proof of tests/conv_long_model.py: the numpy restatement of the
long-block plan (same index map, same block seams as conv_long_kernels.hip)
against conv_exact's exact references, at small factorizations where every
seam and length class is cheap and at the kernels' own N = 512 x 4096.  The
same run measures gamma_ref for the long plan: the worst error / err_scale
(conv_exact's scale with M replaced by N), which test_conv_long_gpu.py's
bound is 8 times.  No GPU.
"""
import numpy as np
import pytest

import conv_exact as E
import conv_long_model as LM
import oracle_lib as O

SANE = 4.0  # as test_conv_exact.py: a wrong index or convention gives 10^10


def _ratio(got, exact, scale):
    assert got.shape == exact.shape
    return float(np.max(np.abs(got - exact))) / scale


def _small_cases(n_fft):
    """Exact cases around every length class of a plan of n_fft points."""
    out = []
    for K in (n_fft // 4, n_fft // 4 - 3, 5, 1):
        hop = LM.hop_long(K, n_fft)
        for ol in (hop // 3, hop, 3 * hop - 1, 3 * hop, 3 * hop + 1):
            n = max(1, ol - K + 1)
            ol = min(ol, n + K - 1)
            out.append(E.case_kernel_impulse(n, K, K - 1, 2.0, 100 + ol, ol))
            out.append(E.case_input_impulse(n, E.noise(K, 7 + K), min(n - 1, hop - 1), 0.25, ol))
            if n * K <= E.DENSE_LIMIT:
                c = E.case_dense_int(n, E.dense_int(K, 9, E.DENSE_INT_RANGE), 200 + ol)
                out.append(E.Case(c.family, c.x, c.h, c.exact[:ol], c.partial))
    return out


@pytest.mark.parametrize("n1,n2", [(32, 16), (64, 32), (16, 64)])
def test_small_factorizations(n1, n2):
    worst = 0.0
    for c in _small_cases(n1 * n2):
        got = LM.long_numpy(c.x, c.h, c.exact.size, n1, n2)
        r = _ratio(got, c.exact, LM.scale_of(c, n1 * n2))
        assert r <= SANE, (c.family, c.x.size, c.h.size, r)
        worst = max(worst, r)
    print(f"GAMMA_REF_LONG {n1}x{n2} numpy={worst:.3f} recorded={LM.GAMMA_REF_LONG}")
    assert worst <= LM.GAMMA_REF_LONG


def test_dense_float_against_long_double():
    """Noise x noise against the C oracle's long-double direct sum."""
    n1, n2 = 64, 32
    h = E.noise(500, 3)
    c = E.case_dense_float(3 * LM.hop_long(500, n1 * n2) + 17, h, 4, O.direct_ld)
    r = _ratio(LM.long_numpy(c.x, c.h, None, n1, n2), c.exact, LM.scale_of(c, n1 * n2))
    print(f"GAMMA_REF_LONG dense-float numpy={r:.3f}")
    assert r <= LM.GAMMA_REF_LONG


@pytest.mark.parametrize("name", ["impulse-K=N/4", "sparse-K=100003", "sparse-input-K=131072"])
def test_gamma_ref_full_size(name):
    """The GPU tests' exact cases through the model at N = 512 x 4096."""
    c = LM.exact_cases()[name]
    got = LM.long_numpy(c.x, c.h, c.exact.size)
    r = _ratio(got, c.exact, LM.scale_of(c))
    print(f"GAMMA_REF_LONG {name} numpy={r:.3f} recorded={LM.GAMMA_REF_LONG}")
    assert r <= LM.GAMMA_REF_LONG


def test_scale_reduces_to_one_partition():
    """One block, K <= L: the long scale at N = 2L is conv_exact.err_scale."""
    L, K = 256, 100
    x, h = E.noise(L - K + 1, 1), E.noise(K, 2)
    a = LM.err_scale_long(x, h, 3.0, None, 2 * L)
    b = E.err_scale(x, h, L, 3.0)
    assert abs(a - b) <= 1e-12 * b
