"""The long-block overlap-save plan (csrc/conv_long_kernels.hip) restated in
numpy, its error scale, and the cases shared by the CPU measurement of its
gamma_ref (test_conv_long_model.py) and the GPU tests (test_conv_long_gpu.py).
A helper module, not a test.

The plan: blocks of N = N1 N2 points, hop N - K + 1.  Block j transforms
x[j hop - (K-1) .. j hop - (K-1) + N) (zeros outside the signal) with
n = N2 n1 + n2, k = k1 + N1 k2:

  columns  real N1-point FFT over n1 for every n2, rows k1 = 0 .. N1/2 kept;
  rows     times W_N^(n2 k1), complex N2-point FFT over n2 -> X[k1 + N1 k2];
           times H (same layout, scaled 1/N); unnormalised inverse over k2;
           times conj W_N^(n2 k1);
  columns  complex-to-real unnormalised inverse over k1 (rows above N1/2 are
           the mirror; the imaginary parts of rows 0 and N1/2 are dropped).

The block's outputs are its last hop samples.

Error scale: conv_exact.err_scale with one partition and M replaced by N,

    err_scale = eps (sqrt(log2 N) max_j |w_j|_2 |h|_2 / sqrt(N) + max|exact|),

w_j the N-sample window of block j.
"""
import functools
import math

import numpy as np

import conv_exact as E
from conv_exact import EPS

N1, N2 = 512, 4096  # kLongN1, kLongN2 of conv_long_kernels.hpp
N = N1 * N2
MIN_BLOCKS = 4      # Upols::kLongMinBlocks


def hop_long(K, n_fft=N):
    return n_fft - K + 1


@functools.lru_cache(maxsize=4)
def _twiddle(n1, n2):
    k1 = np.arange(n1 // 2 + 1, dtype=np.int64)[:, None]
    c = np.arange(n2, dtype=np.int64)[None, :]
    a = -2.0 * np.pi * ((k1 * c) % (n1 * n2)).astype(np.float64) / (n1 * n2)
    return np.cos(a) + 1j * np.sin(a)


def _forward(seg, n1, n2):
    t = np.fft.rfft(seg.reshape(n1, n2), axis=0)
    return np.fft.fft(t * _twiddle(n1, n2), axis=1)


def long_spectrum(h, n1=N1, n2=N2):
    """H rows [n1/2 + 1][n2] of the zero-padded kernel, scaled by 1/N."""
    buf = np.zeros(n1 * n2)
    buf[: len(h)] = h
    return _forward(buf, n1, n2) / (n1 * n2)


def long_numpy(x, h, out_len=None, n1=N1, n2=N2, H=None):
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    n_fft, K = n1 * n2, h.size
    assert 4 * K <= n_fft
    hop = hop_long(K, n_fft)
    out_len = x.size + K - 1 if out_len is None else out_len
    H = long_spectrum(h, n1, n2) if H is None else H
    J = -(-out_len // hop)
    out = np.empty(J * hop)
    tw = _twiddle(n1, n2)
    for j in range(J):
        lo = j * hop - (K - 1)
        seg = np.zeros(n_fft)
        a, b = max(lo, 0), min(lo + n_fft, x.size)
        if b > a:
            seg[a - lo: b - lo] = x[a:b]
        v = np.fft.ifft(_forward(seg, n1, n2) * H, axis=1) * n2 * np.conj(tw)
        y = np.fft.irfft(v, n=n1, axis=0) * n1
        out[j * hop: (j + 1) * hop] = y.ravel()[K - 1:]
    return out[:out_len]


def err_scale_long(x, h, peak, out_len=None, n_fft=N):
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    K = h.size
    hop = hop_long(K, n_fft)
    out_len = x.size + K - 1 if out_len is None else out_len
    J = -(-out_len // hop)
    cs = np.concatenate([[0.0], np.cumsum(x * x)])
    worst = 0.0
    for j in range(J):
        lo = j * hop - (K - 1)
        a, b = min(max(lo, 0), x.size), min(max(lo + n_fft, 0), x.size)
        worst = max(worst, cs[b] - cs[a])
    return EPS * (math.sqrt(math.log2(n_fft)) * math.sqrt(worst) * E.norm2(h) / math.sqrt(n_fft) + float(peak))


def scale_of(case, n_fft=N):
    return err_scale_long(case.x, case.h, case.peak, case.exact.size, n_fft)


def seam_positions(K, out_len, n_fft=N):
    """Output indices around every block seam of the long plan."""
    hop = hop_long(K, n_fft)
    out = []
    for j in range(1, -(-out_len // hop)):
        out += [j * hop - 1, j * hop, j * hop + 1]
    return [p for p in out if 0 <= p < out_len]


# ------------------------------------------------------- exact cases, full size
K_QUARTER = N // 4        # the largest kernel the plan takes
K_ODD = 100003            # not a multiple of any UPOLS hop


def _unit(case, bits=15):
    """An integer case with both operands times 2^-bits: as exact (powers of
    two), and at the unit scale the contract's absolute bars are written for."""
    s = 2.0 ** -bits
    return E.Case(case.family, case.x * s, case.h * s, case.exact * (s * s), case.partial)


@functools.lru_cache(maxsize=None)
def exact_cases():
    """name -> conv_exact.Case at the kernels' own N, out_len around 3 hops."""
    out = {}
    # kernel impulse on the last tap of K = N/4: out_len = 3 hop + 1 (4 blocks)
    K = K_QUARTER
    ol = 3 * hop_long(K) + 1
    out["impulse-K=N/4"] = E.case_kernel_impulse(ol - K + 1, K, K - 1, 0.5, 11, ol)
    # sparse integer kernel, taps on both ends: out_len = 3 hop - 1 (3 blocks)
    K = K_ODD
    ol = 3 * hop_long(K) - 1
    hpos, hval = E.sparse_int(K, 8192, 21)
    out["sparse-K=100003"] = _unit(E.case_sparse_kernel(ol - K + 1, hpos, hval, K, 23, ol))
    # sparse integer input with taps at the seams against a dense integer kernel: out_len = 3 hop
    K = 131072
    ol = 3 * hop_long(K)
    n = ol - K + 1
    seams = [p - d for p in seam_positions(K, ol) for d in (0, K - 1) if 0 <= p - d < n]
    xpos = E.boundary_positions(n, hop_long(K), 31, extra=tuple(sorted(set(seams)))[:24])
    xval = np.random.default_rng(32).integers(-E.INT_RANGE, E.INT_RANGE, size=xpos.size).astype(np.int64)
    xval[xval == 0] = 1
    hi = E.dense_int(K, 33)
    exact, partial = E.sparse_convolve(xpos, xval, hi, ol)
    out["sparse-input-K=131072"] = _unit(E.Case("sparse-input", E.densify(xpos, xval, n), hi, exact, partial))
    return out


# worst error / err_scale of long_numpy over exact_cases() and the small
# factorizations, measured by test_conv_long_model.py when it was written
# (numpy 2.x pocketfft); the device is held to GAMMA = 8 GAMMA_REF_LONG
GAMMA_REF_LONG = 1.5  # measured: 1.48 (sparse-K=100003), 1.37, 1.26 at full size; 1.32 at 16 x 64
GAMMA = 8 * GAMMA_REF_LONG
