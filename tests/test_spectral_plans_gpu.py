"""Every launch plan of the spectral FFT (csrc/bigfft.hip) against exact
references: CorrelateFFT at N = 2^0 .. 2^27, Deconvolve (three methods) and
InverseFilter at 2^0 .. 2^25, the naive method's zero-bin report at
2^2 .. 2^25.  The references (tests/spectral_exact.py) are shifts, integer
sums, closed forms and, up to N = 1024, a longdouble DFT: none is an FFT, and
tests/test_spectral_exact.py proves them against the C oracle and numpy on
the CPU.

Bound.  For every case  max |gpu - exact| <= GAMMA * err_scale,  GAMMA =
8 gamma_ref, with err_scale as spectral_exact defines it and gamma_ref the
worst error / err_scale of numpy's fp64 FFT over the same cases at k <= 16
(test_spectral_exact.py measures it and fails when it leaves the figure
below).  The factor 8 is for what the device legitimately does differently:
radix-512 LDS transforms, mirror extraction, the half-length inverse.  A
wrong or low-precision twiddle costs orders of magnitude.  The older bar,
1e-10 max|want|, is about 10^5 err_scale.

    API             gamma_ref (numpy)   C oracle   GAMMA    MI355X worst
    CorrelateFFT    1.51                1.57       12.08    5.57 (two transforms)
    Deconvolve      1.21                1.10        9.68    4.81
    InverseFilter   1.05                0.66        8.40    3.23

(CPU figures at k <= 16, the MI355X over every k of the sweep; RECORDED
below has the device's figure per plan.)

The packed correlation.  Where CorrelateFFT takes one transform of a + i b
(spectral_exact.corr_packs: 2^5 <= N < 2^25 and max(n, m) <= 2^17
sqrt(min(n, m))) the bound gains the cross-talk term that
spectral_exact.leak_term derives, LEAK eps (|a'|^2 + |b'|^2) 2^(ea+eb) with
LEAK = 8, and is capped at the older bar.  The measured leak coefficient is
0.3 .. 1.53 (RECORDED), the worst error 0.38 of the bound.  Before
SpectralRun::packs existed every size packed, and this sweep measured, for a
noise signal against an impulse or a single tap, 88 err_scale at 2^12,
6.0e3 at 2^20, 4.2e5 at 2^25 (8.9e-10 absolute on unit-variance lags, past
the 1e-10 bar) and 3.9e6 at 2^27 (6.2e-9); with two transforms the same
cases measure 2 .. 3.4.

Host-form Deconvolve at 2^26 and 2^27 runs one naive unit-kernel case each
(1.3 s at 2^27).
"""
import ctypes as C
import re

import numpy as np
import pytest

import spectral_exact as X

pytestmark = pytest.mark.gpu

GAMMA_REF = {"corr": 1.51, "deconv": 1.21, "invfilt": 1.05}
GAMMA = {api: 8.0 * g for api, g in GAMMA_REF.items()}

CORR_KS = list(range(0, 28))
DECONV_KS = list(range(0, 26))
DECONV_BIG_KS = [26, 27]
INVFILT_KS = list(range(0, 26))
ZERO_BIN_KS = list(range(2, 26))
HOST_FORM_MAX_K = 22  # CorrelateFFT: host form too, bit for bit, up to here; device arrays and checks above
SMALL_EXHAUSTIVE_MAX = 40  # every (n, m) with n + m - 1 <= this

# (k, kernel) pairs of the zero-bin report left out because the C oracle
# itself does not report the mathematical bin there (its computed |H| stays
# above 1e-15); test_spectral_exact.py keeps this list honest at k <= 16.
ZERO_BIN_DROPPED = []

# The device's measured figures per plan (MI355X, one run of this file; the
# tests print those of every run): k -> (CorrelateFFT worst error / err_scale
# over the two-transform cases, CorrelateFFT worst leak coefficient over the
# packed cases, Deconvolve, InverseFilter worst error / err_scale).  0.00 in
# the first two columns: no case of that kind at that k.
RECORDED = {
    0: (0.00, 0.00, 0.39, 0.48), 1: (0.16, 0.00, 0.44, 0.00), 2: (0.45, 0.00, 0.58, 0.18),
    3: (0.87, 0.00, 0.68, 0.66), 4: (0.58, 0.00, 0.87, 0.71), 5: (0.00, 0.40, 0.76, 0.38),
    6: (0.00, 0.59, 0.99, 0.46), 7: (0.00, 0.70, 1.12, 0.86), 8: (0.00, 0.74, 1.55, 1.28),
    9: (0.00, 0.66, 1.37, 0.94), 10: (0.00, 0.87, 1.62, 1.75), 11: (0.00, 0.88, 1.67, 1.24),
    12: (0.00, 0.96, 2.10, 1.83), 13: (0.00, 1.53, 1.92, 3.07), 14: (0.00, 0.85, 1.74, 1.69),
    15: (0.00, 1.11, 1.89, 2.01), 16: (0.00, 1.12, 2.30, 1.58), 17: (0.00, 1.12, 2.38, 2.10),
    18: (3.30, 0.85, 2.23, 1.78), 19: (3.10, 0.28, 2.66, 3.23), 20: (2.99, 0.32, 2.10, 1.47),
    21: (3.05, 0.54, 2.28, 2.46), 22: (3.30, 0.55, 2.49, 2.85), 23: (3.48, 0.51, 3.70, 2.88),
    24: (3.94, 0.32, 4.81, 2.66), 25: (5.57, 0.00, 3.70, 3.19), 26: (4.34, 0.00, 2.93, None),
    27: (5.05, 0.00, 3.19, None),
}


def _ratio(err, scale):
    if err != err:
        return float("inf")
    if scale > 0:
        return err / scale
    return 0.0 if err == 0 else float("inf")


class _Worst:
    """Worst error / err_scale of a test's cases; for the packed correlation
    (leak > 0, spectral_exact.corr_bound) the worst error / bound and the
    worst measured leak coefficient, error / (eps (|a'|^2 + |b'|^2) 2^(ea+eb))."""

    def __init__(self, api, k):
        self.api, self.k, self.worst, self.name, self.bad = api, k, 0.0, "", []
        self.packed_frac = self.rho = 0.0

    def add(self, name, err, scale, leak=0.0, peak=0.0):
        r = _ratio(err, scale)
        bound = X.corr_bound(GAMMA[self.api], scale, leak, peak)
        if leak > 0:
            self.packed_frac = max(self.packed_frac, _ratio(err, bound))
            self.rho = max(self.rho, _ratio(err, leak / X.LEAK))
        elif r >= self.worst:
            self.worst, self.name = r, name
        if not err <= bound:
            self.bad.append(f"{name}: err {err:.3e} = {r:.1f} err_scale, bound {bound:.3e}")

    def finish(self):
        print(f"SPECTRAL_RATIO api={self.api} k={self.k} plan={X.plan_kind(self.k)!r} worst={self.worst:.3f} "
              f"case={self.name!r} gamma={GAMMA[self.api]:.2f} packed_err_over_bound={self.packed_frac:.3f} "
              f"packed_leak_coeff={self.rho:.3f}")
        assert not self.bad, f"{self.api} at 2^{self.k} ({X.plan_kind(self.k)}): " + "; ".join(self.bad[:8])


# ------------------------------------------------------------- CorrelateFFT
def _dev_call(da, db, off):
    """ad_correlate_fft_device into a NaN-filled output that starts `off`
    doubles into its allocation (both alignments of the 16-byte stores)."""
    import torch

    from algodsp._lib import check, lib

    n, m = da.numel(), db.numel()
    buf = torch.full((n + m - 1 + off,), float("nan"), dtype=torch.float64, device="cuda")
    out = buf[off:]
    st = torch.cuda.current_stream()
    check(lib().ad_correlate_fft_device(C.c_void_p(da.data_ptr()), n, C.c_void_p(db.data_ptr()), m,
                                        C.c_void_p(out.data_ptr()), 0, C.c_void_p(st.cuda_stream)))
    st.synchronize()
    if off:
        assert bool(torch.isnan(buf[0])), "wrote ahead of the output"
    return out


def _to_dev(x, off):
    """x on the device, starting `off` doubles into its allocation."""
    import torch

    buf = torch.empty((len(x) + off,), dtype=torch.float64, device="cuda")
    buf[off:] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return buf[off:]


def _host_cases(k, w):
    from algodsp import conv

    i = 0
    for n, m in X.corr_splits(k):
        for _, name, a, b, exact, scale, leak in X.corr_cases(k, n, m):
            off = i & 1
            i += 1
            got = _dev_call(_to_dev(a, off), _to_dev(b, (i >> 1) & 1), off).cpu().numpy()
            assert np.array_equal(got, conv.CorrelateFFT(a, b)), f"device form != host form: n={n} m={m} {name}"
            w.add(f"n={n} m={m} {name}", float(np.max(np.abs(got - exact))), scale, leak, X.peak_of(exact))


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _region_err(out, start, vals):
    """max |out - want| where want is `vals` at [start, start + len) and 0 elsewhere."""
    e = _amax(out[start: start + vals.numel()] - vals)
    for part in (out[:start], out[start + vals.numel():]):
        v = _amax(part)
        e = v if (v != v or v > e) else e
    return e


def _device_cases(k, w):
    """The cases of spectral_exact.corr_cases built from device tensors."""
    import torch

    N = 1 << k
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + k)
    A0 = torch.randn(N + 1, dtype=torch.float64, device="cuda", generator=g)
    B0 = torch.randn(N + 1, dtype=torch.float64, device="cuda", generator=g)
    i = 0

    def imp(length, p, c, off):
        v = torch.zeros(length + off, dtype=torch.float64, device="cuda")[off:]
        v[p] = c
        return v

    for n, m in X.corr_splits(k):
        packs = X.corr_packs(N, n, m)

        def run(name, a, b, start, vals, dense):
            nonlocal i
            off = i & 1
            i += 1
            out = _dev_call(a, b, off)
            nd, pd = float(torch.linalg.vector_norm(dense)), _amax(dense)
            leak = X.leak_term(nd, pd, 1.0, 1.0) if packs else 0.0
            w.add(f"n={n} m={m} {name}", _region_err(out, start, vals), X.err_scale(N, nd, 1.0, pd), leak, pd)

        a0, b0 = A0[(n & 1): (n & 1) + n], B0[(m & 1): (m & 1) + m]
        for p in X.impulse_positions(m):
            run(f"shift_b p={p}", a0, imp(m, p, 1.0, p & 1), m - 1 - p, a0, a0)
        for p in X.impulse_positions(n):
            run(f"shift_a p={p}", imp(n, p, 1.0, p & 1), b0, p, b0.flip(0), b0)
        (sa, sb), (sa2, sb2) = X.SCALE_PAIRS
        run(f"shift_b scales {sa:g},{sb:g}", sa * a0, imp(m, m // 3, sb, 0), m - 1 - m // 3, a0, a0)
        run(f"shift_a scales {sb2:g},{sa2:g}", imp(n, n // 3, sb2, 1), sa2 * b0, n // 3, b0.flip(0), b0)
        # the integer correlation: dense from the host where n m allows, else sparse
        if n * m <= X.DENSE_LIMIT:
            ai, bi = X.int_signal(n, 31 * k + n), X.int_signal(m, 37 * k + m)
            exact = X.int_correlate(ai, bi).astype(np.float64)
            out = _dev_call(_to_dev(ai, 1), _to_dev(bi, 0), 0)
            err = _amax(out - torch.from_numpy(exact).cuda())
            leak = X.leak_term(X.norm2(ai), X.peak_of(ai), X.norm2(bi), X.peak_of(bi)) if packs else 0.0
            w.add(f"n={n} m={m} int dense", err, X.err_scale(N, X.norm2(ai), X.norm2(bi), X.peak_of(exact)), leak,
                  X.peak_of(exact))
        else:
            (pa, va), (pb, vb) = X.sparse_signal(n, k, 41 * k + n), X.sparse_signal(m, k, 43 * k + m)
            idx, val = X.sparse_correlate(pa, va, pb, vb, m)
            a = torch.zeros(n, dtype=torch.float64, device="cuda")
            a[torch.from_numpy(pa).cuda()] = torch.from_numpy(va.astype(np.float64)).cuda()
            b = torch.zeros(m, dtype=torch.float64, device="cuda")
            b[torch.from_numpy(pb).cuda()] = torch.from_numpy(vb.astype(np.float64)).cuda()
            out = _dev_call(a, b, 1)
            out[torch.from_numpy(idx).cuda()] -= torch.from_numpy(val.astype(np.float64)).cuda()
            leak = X.leak_term(X.norm2(va), X.peak_of(va), X.norm2(vb), X.peak_of(vb)) if packs else 0.0
            w.add(f"n={n} m={m} int sparse", _amax(out), X.err_scale(N, X.norm2(va), X.norm2(vb), X.peak_of(val)),
                  leak, X.peak_of(val))
        del a0, b0


@pytest.mark.parametrize("k", CORR_KS)
def test_correlate_plan(gpu, k):
    """Every (n, m) split of spectral_exact.corr_splits at N = 2^k: the shift
    property with a noise operand in both directions, at unit scales, 2^+-40
    and 2^+-600, and the integer correlation.  The device form throughout; up
    to 2^22 the host form too, equal bit for bit."""
    w = _Worst("corr", k)
    if k <= HOST_FORM_MAX_K:
        _host_cases(k, w)
    else:
        _device_cases(k, w)
    w.finish()


def test_correlate_small_exhaustive(gpu):
    """Every (n, m) with n + m - 1 <= 40, integer-valued, against np.correlate
    on int64: k = 0 .. 5 on the unfused path, and the fused path's first sizes
    (N = 32, 64) at every padding; host and device forms."""
    from algodsp import conv

    bad, worst = [], 0.0
    for n in range(1, SMALL_EXHAUSTIVE_MAX + 1):
        for m in range(1, SMALL_EXHAUSTIVE_MAX + 2 - n):
            ai, bi = X.int_signal(n, 7 * n + m), X.int_signal(m, 11 * m + n)
            exact = X.int_correlate(ai, bi).astype(np.float64)
            a, b = ai.astype(np.float64), bi.astype(np.float64)
            N = X.next_pow2(n + m - 1)
            scale = X.err_scale(N, X.norm2(a), X.norm2(b), X.peak_of(exact))
            host = conv.CorrelateFFT(a, b)
            dev = _dev_call(_to_dev(a, n & 1), _to_dev(b, m & 1), (n + m) & 1).cpu().numpy()
            if not np.array_equal(host, dev):
                bad.append(f"n={n} m={m}: device form != host form")
            err = float(np.max(np.abs(host - exact)))
            leak = X.leak_term(X.norm2(a), X.peak_of(a), X.norm2(b), X.peak_of(b)) if X.corr_packs(N, n, m) else 0.0
            r = _ratio(err, scale)
            worst = max(worst, r)
            if not err <= X.corr_bound(GAMMA["corr"], scale, leak, X.peak_of(exact)):
                bad.append(f"n={n} m={m}: {r:.1f} err_scale")
    print(f"SPECTRAL_RATIO api=corr k=small-exhaustive worst={worst:.3f} gamma={GAMMA['corr']:.2f}")
    assert not bad, "; ".join(bad[:10])


# --------------------------------------------------------------- Deconvolve
def _opts(o):
    from algodsp import conv

    return conv.DeconvOptions(int(o[0]), float(o[1]), float(o[2]), float(o[3]))


@pytest.mark.parametrize("k", DECONV_KS)
def test_deconvolve_plan(gpu, k):
    """n = N = 2^k, all three methods: the unit kernels c e_p, the integer
    round trip (naive), and up to 2^10 a dense kernel against the longdouble
    DFT (regularised, Wiener)."""
    from algodsp import conv

    w = _Worst("deconv", k)
    for _, name, x, h, o, exact, scale in X.deconv_cases(k):
        got = conv.Deconvolve(x, h, _opts(o))
        assert got.shape == exact.shape, name
        w.add(name, float(np.max(np.abs(got - exact))), scale)
    w.finish()


@pytest.mark.parametrize("k", DECONV_BIG_KS)
def test_deconvolve_plan_big(gpu, k):
    """2^26 and 2^27: one naive unit-kernel case each (zeros and a few writes)."""
    from algodsp import conv

    N = 1 << k
    pos, val = X.sparse_signal(N, k, 50 + k)
    x = X.densify(pos, val, N)
    p, c = 1, 0.125
    got = conv.Deconvolve(x, X.impulse(p + 1, p, c), _opts((0, 0.0, 0.0, 0.0)))
    exact = X.deconv_unit(x, p, c, 0.0)
    w = _Worst("deconv", k)
    w.add(f"unit naive p={p} c={c}", float(np.max(np.abs(got - exact))),
          X.err_scale(N, X.norm2(val), 1.0 / c, X.peak_of(exact)))
    w.finish()


@pytest.mark.parametrize("k", ZERO_BIN_KS)
def test_deconvolve_zero_bin(gpu, k):
    """The naive method's first-zero-bin report at N = 2^k: [1, -1] at bin 0,
    [1, 1] at N/2, [1, 0, 1] at N/4 (the first of N/4 and 3N/4, one mirror
    pair of the fused inverse).  The bins are the mathematics' own."""
    from algodsp import conv

    N = 1 << k
    x = np.zeros(N)
    x[0] = 1.0
    for h, want in X.zero_bin_cases(N):
        if (k, h) in ZERO_BIN_DROPPED:
            continue
        with pytest.raises(conv.ErrDivisionByZero) as e:
            conv.Deconvolve(x, np.array(h), _opts((0, 0.0, 0.0, 0.0)))
        got = int(re.search(r"bin (\d+)", str(e.value)).group(1))
        assert got == want, f"kernel {list(h)} at 2^{k}: bin {got}, expected {want}"


# ------------------------------------------------------------ InverseFilter
@pytest.mark.parametrize("k", INVFILT_KS)
def test_inverse_filter_plan(gpu, k):
    """N = 2^k: the impulse closed form, length < N (with the peak cut off and
    kept), the kernel longer than N, and up to 2^10 a dense kernel against the
    longdouble DFT."""
    from algodsp import conv

    w = _Worst("invfilt", k)
    for _, name, h, length, eps, exact, scale in X.invfilt_cases(k):
        got = conv.InverseFilter(h, length, eps)
        assert got.shape == exact.shape, name
        w.add(name, float(np.max(np.abs(got - exact))), scale)
    w.finish()
