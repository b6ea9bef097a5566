"""CPU proof of tests/spectral_exact.py: the C oracle (oracle_lib) and numpy's
fp64 FFT run through every exact reference the GPU sweep uses, at k <= 16, so
the references and their index conventions are proved without a GPU.  The
same run measures gamma_ref, the worst error / err_scale of numpy's FFT per
API, which test_spectral_plans_gpu.py's bound is 8 times; and the plan table
restated in spectral_exact is checked against the sweep's parameter lists.
"""
import numpy as np
import pytest

import oracle_lib as O
import spectral_exact as X
import test_spectral_plans_gpu as G
from test_spectral_gpu import _np_correlate_fft

CPU_K = range(0, 17)
ORACLE_ALL_K = 12  # the C oracle on every case up to here, on each split's first two above
# a correct fp64 FFT stays within a few err_scale; a wrong index or convention gives 10^15
SANE = 4.0
# the recorded gamma_ref may not trail what this run measures by more than this
DRIFT = 1.25


def _np_deconvolve(x, h, o):
    N = X.next_pow2(len(x))
    eps = X.resolve_eps(o[0], o[1], o[2], o[3], x)
    Xf, H = np.fft.fft(x, N), np.fft.fft(h, N)
    Y = Xf / H if o[0] == 0 else Xf * np.conj(H) / (np.abs(H) ** 2 + eps)
    olen = len(x) - len(h) + 1
    return np.fft.ifft(Y).real[: olen if olen > 0 else len(x)]


def _np_inverse_filter(h, length, eps):
    N = X.next_pow2(length)
    H = np.fft.fft(np.asarray(h)[:N], N)
    return np.fft.ifft(np.conj(H) / (np.abs(H) ** 2 + eps)).real[:length]


def _check(worst, who, name, got, exact, scale):
    assert got.shape == exact.shape, (who, name)
    r = G._ratio(float(np.max(np.abs(got - exact))) if exact.size else 0.0, scale)
    assert r <= SANE, f"{who} {name}: {r:.3g} err_scale"
    worst[who] = max(worst.get(who, 0.0), r)


def _report(api, worst):
    print(f"GAMMA_REF api={api} numpy={worst.get('numpy', 0):.3f} oracle={worst.get('oracle', 0):.3f} "
          f"recorded={G.GAMMA_REF[api]}")
    assert worst["numpy"] <= DRIFT * G.GAMMA_REF[api], (
        f"numpy's measured ratio {worst['numpy']:.3f} left the recorded gamma_ref {G.GAMMA_REF[api]}")


def test_correlate_references():
    worst = {}
    for k in CPU_K:
        for n, m in X.corr_splits(k):
            for i, (_, name, a, b, exact, scale, _leak) in enumerate(X.corr_cases(k, n, m)):
                tag = f"2^{k} n={n} m={m} {name}"
                _check(worst, "numpy", tag, _np_correlate_fft(a, b), exact, scale)
                if k <= ORACLE_ALL_K or i < 2:
                    _check(worst, "oracle", tag, O.correlate_fft(a, b), exact, scale)
    _report("corr", worst)


def test_correlate_small_exhaustive_reference():
    """np.correlate's lag order is the reference's for every small (n, m)."""
    for n in range(1, 14):
        for m in range(1, 14):
            ai, bi = X.int_signal(n, 7 * n + m), X.int_signal(m, 11 * m + n)
            got = O.correlate_fft(ai.astype(np.float64), bi.astype(np.float64))
            assert np.max(np.abs(got - X.int_correlate(ai, bi))) < 1e-9


def test_sparse_correlate_matches_dense():
    for k, n, m in [(5, 20, 13), (10, 700, 300), (13, 3000, 5000)]:
        (pa, va), (pb, vb) = X.sparse_signal(n, k, 3), X.sparse_signal(m, k, 4)
        idx, val = X.sparse_correlate(pa, va, pb, vb, m)
        dense = X.int_correlate(X.densify(pa, va, n).astype(np.int64), X.densify(pb, vb, m).astype(np.int64))
        assert np.array_equal(X.densify(idx, val, n + m - 1), dense)


def test_deconvolve_references():
    worst = {}
    for k in CPU_K:
        for _, name, x, h, o, exact, scale in X.deconv_cases(k):
            tag = f"2^{k} {name}"
            _check(worst, "numpy", tag, _np_deconvolve(x, h, o), exact, scale)
            _check(worst, "oracle", tag, O.deconvolve(x, h, *o), exact, scale)
    _report("deconv", worst)


def test_inverse_filter_references():
    worst = {}
    for k in CPU_K:
        for _, name, h, length, eps, exact, scale in X.invfilt_cases(k):
            tag = f"2^{k} {name}"
            _check(worst, "numpy", tag, _np_inverse_filter(h, length, eps), exact, scale)
            _check(worst, "oracle", tag, O.inverse_filter(h, length, eps), exact, scale)
    _report("invfilt", worst)


def test_longdouble_dft_is_a_dft():
    """The O(N^2) longdouble DFT against its definition's fixed points: an
    impulse gives the twiddles, the inverse undoes the forward."""
    N = 64
    x = X.noise(N, 1)
    fr, fi = X.ld_dft(x, np.zeros(N), -1)
    br, bi = X.ld_dft(fr, fi, +1)
    assert float(np.max(np.abs(br / N - x))) < 1e-17 and float(np.max(np.abs(bi / N))) < 1e-17
    er, ei = X.ld_dft(X.impulse(N, 3, 1.0), np.zeros(N), -1)
    ang = -2 * np.pi * ((3 * np.arange(N)) % N) / N  # fp64 angles below 2 pi: rounded by up to 2 pi 2^-53 = 7e-16
    assert float(np.max(np.abs(er - np.cos(ang)))) < 2e-15 and float(np.max(np.abs(ei - np.sin(ang)))) < 2e-15


def test_zero_bins_match_oracle():
    """The mathematical first zero bin is what the C oracle reports, at every
    k <= 16 of the GPU sweep, except for the pairs the sweep lists as dropped
    (at most a fifth of the pairs that depend on a computed |H| < 1e-15)."""
    inexact = dropped = 0
    for k in G.ZERO_BIN_KS:
        if k > max(CPU_K):
            continue
        N = 1 << k
        x = X.impulse(N, 0, 1.0)
        for h, want in X.zero_bin_cases(N):
            inexact += h != (1.0, -1.0)
            with pytest.raises(O.OracleError) as e:
                O.deconvolve(x, np.array(h), 0)
            if (k, h) in G.ZERO_BIN_DROPPED:
                dropped += 1
                assert e.value.bad_bin != want, f"2^{k} {h} is listed as dropped but the oracle reports bin {want}"
            else:
                assert e.value.bad_bin == want, (k, h, e.value.bad_bin)
    assert all(h != (1.0, -1.0) for _, h in G.ZERO_BIN_DROPPED)
    assert len(G.ZERO_BIN_DROPPED) * 5 <= 2 * len(G.ZERO_BIN_KS)
    assert dropped * 5 <= inexact


# --------------------------------------------------------------- plan table
def test_plan_table_is_the_documented_one():
    """BigFft::BigFft's rule (copied by hand): naive DFT to 2^3, one pass to
    2^12, then ceil(k / 9) passes of near-equal radix, the larger first."""
    for k in range(X.K_MAX + 1):
        if k <= 3:
            want = ()
        elif k <= 12:
            want = (1 << k,)
        else:
            np_ = (k + 8) // 9
            base, extra = divmod(k, np_)
            want = tuple(1 << (base + (1 if p < extra else 0)) for p in range(np_))
        assert X.PLAN_RADICES[k] == want
        assert int(np.prod(want, dtype=np.int64)) == (1 << k) or not want
    assert [k for k in range(28) if X.corr_fused(k)] == [16, 17, 24]
    assert [k for k in range(28) if X.corr_split(k)] == [24]


def test_gpu_sweep_covers_every_plan():
    """The GPU sweep's parameter lists touch every row of the plan table and
    both outcomes of every path predicate, per API."""
    assert set(G.CORR_KS) == set(range(0, 28))
    assert set(G.DECONV_KS) >= set(range(0, 26)) and set(G.DECONV_BIG_KS) == {26, 27}
    assert set(G.INVFILT_KS) >= set(range(0, 26))
    assert set(G.ZERO_BIN_KS) == set(range(2, 26))
    assert G.HOST_FORM_MAX_K >= 22
    for name, ks, preds in [
        ("corr", G.CORR_KS, [X.unfused, X.corr_fused, X.corr_split, lambda k: X.persistent_passes(k, True) > 0,
                             lambda k: X.mirror_paired(k, False, True)]),
        ("deconv", G.DECONV_KS, [X.unfused, lambda k: X.persistent_passes(k, False) > 0]),
        ("invfilt", G.INVFILT_KS, [X.unfused, lambda k: X.persistent_passes(k, False) > 0,
                                   lambda k: X.mirror_paired(k, False, False)]),
        ("zero bin", G.ZERO_BIN_KS, [X.unfused, lambda k: X.persistent_passes(k, False) > 0]),
    ]:
        rows = {X.PLAN_RADICES[k] for k in ks}
        limit = 27 if name == "corr" else 25
        assert rows >= {X.PLAN_RADICES[k] for k in range(2 if name == "zero bin" else 0, limit + 1)}, name
        for i, pred in enumerate(preds):
            assert {bool(pred(k)) for k in ks} == {True, False}, (name, i)
    # every persistent-pass count and the splits' store alignments are reached
    assert {X.persistent_passes(k, True) for k in G.CORR_KS} == {X.persistent_passes(k, True) for k in range(28)}
    for k in G.CORR_KS:
        sp = X.corr_splits(k)
        packed = [X.corr_packs(1 << k, n, m) for n, m in sp]
        assert any(packed) == (5 <= k <= 24), k  # the packed plans (fused and split among them) are run
        assert k < 18 or not all(packed), k  # and so is the two-transform path of unequal lengths
        assert all(X.next_pow2(n + m - 1) == 1 << k for n, m in sp)
        if k >= 3:
            assert any(n + m - 1 == 1 << k for n, m in sp) and any(n + m - 1 == (1 << k) // 2 + 1 for n, m in sp)
            assert any(m == 1 for _, m in sp) and any(n == 1 for n, _ in sp) and any(m > n > 1 for n, m in sp)
            assert {(m - 1) & 1 for _, m in sp} == {0, 1} and {n & 1 for n, _ in sp} == {0, 1}
