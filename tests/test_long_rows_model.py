"""k_long_rows' thread mapping (conv_long_kernels.hip), restated on the CPU
from the address patterns of tools/lds_conflicts.py: every exchange is free of
bank conflicts under the model, and the four forward and four inverse passes,
with the butterfly indices the kernel passes to twiddle_root, compute the
4096-point transforms in the orders the kernel's comment states."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import lds_conflicts as L  # noqa: E402

M, T = 4096, 512


def test_exchanges_conflict_free():
    L.check_long_rows_exchange()
    for name, p in L.long_rows_patterns().items():
        assert L.extra_cycles(p, 0, lambda i: i) == 0, name
    plain = L.long_rows_patterns(xor=False)
    assert L.extra_cycles(plain["F pass 2 -> 3"], 0, lambda i: i) > 0  # what the lane ^ slot swizzle is for


def _butterflies(v, jb, ns, fwd):
    sign = -2j if fwd else 2j
    if ns > 1:
        e = (jb & (ns - 1)) * (M // (ns * 8))
        v = v * np.exp(sign * np.pi * e[:, None] * np.arange(8)[None, :] / M)
    return np.fft.fft(v, axis=1) if fwd else np.fft.ifft(v, axis=1) * 8


def _exchange(v, pats):
    lds = np.zeros(M, complex)
    for s in range(8):
        lds[[a for _, a in pats[s][1]]] = v[:, s]
    return np.stack([lds[[a for _, a in pats[8 + s][1]]] for s in range(8)], 1)


def test_mapping_computes_the_transforms():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    h = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    pats = list(L.long_rows_patterns().values())
    tid = np.arange(T)
    lane, wv = tid & 63, tid >> 6
    l0, l1 = lane & 7, lane & 56
    v = np.stack([x[tid + T * s] for s in range(8)], 1)
    v = _butterflies(v, tid, 1, True)
    for pat, jb, ns in [(pats[0], wv, 8), (pats[1], l1 + wv, 64), (pats[2], 64 * l0 + l1 + wv, 512)]:
        v = _butterflies(_exchange(v, pat), jb, ns, True)
    X = np.fft.fft(x)
    k = wv + 8 * (lane >> 3) + 64 * (lane & 7)  # the forward result's order: k0 = wave
    assert np.allclose(v, np.stack([X[k + T * s] for s in range(8)], 1), rtol=0, atol=1e-10)
    v = v * np.stack([h[k + T * s] for s in range(8)], 1)
    v = _butterflies(v, tid, 1, False)
    for pat, jb, ns in [(pats[3], l0, 8), (pats[4], lane, 64), (pats[5], tid, 512)]:
        v = _butterflies(_exchange(v, pat), jb, ns, False)
    y = np.fft.ifft(X * h) * M
    assert np.allclose(v, np.stack([y[tid + T * s] for s in range(8)], 1), rtol=0, atol=1e-8 * np.abs(y).max())
