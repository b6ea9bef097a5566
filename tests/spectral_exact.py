"""Exact references for the spectral row (CorrelateFFT, Deconvolve,
InverseFilter) and the error scale their results are judged on.

A helper module, not a test.  None of the references is an FFT: each is exact
by construction (a shift, an integer sum in int64, a closed form) or, for the
dense regularised inverses where no closed form exists, an O(N^2) DFT in
np.longdouble (N <= 1024).  tests/test_spectral_exact.py proves them and the
index conventions against the C oracle and numpy on the CPU;
tests/test_spectral_plans_gpu.py runs the device FFT's plans against them.

Conventions (correlate.go:111-172, deconvolve.go:72-394):
  CorrelateFFT(a, b)[j] = sum_i a[i + j - (m-1)] b[i],  j = 0 .. n+m-2,
      transform size N = nextPow2(n + m - 1);
  Deconvolve(x, h): N = nextPow2(n), circular division at N, the first
      n - m + 1 samples (n when that is not positive);
  InverseFilter(h, length, eps): N = nextPow2(length), the kernel cut to N,
      IDFT(conj H / (|H|^2 + eps)), the first `length` samples.

Error scale.  A max-abs error is divided by

    err_scale = eps * (sqrt(log2 N) * |a|_2 |b|_2 / sqrt(N) + max|exact|)

The first term is the rounding noise of an fp64 FFT correlation: every
output is a sum over N bins, each carrying relative rounding of order
eps sqrt(log2 N) on a product of size |a|_2 |b|_2 / N per bin, summed
randomly and scaled by 1/N in the inverse.  It does not shrink or grow with N
for inputs of fixed density, so a ratio of order 1 means "as good as a
correct fp64 FFT" at 2^5 and at 2^27 alike (eps log2 N |a| |b| would shrink
200-fold over that range).  log2 N is taken as at least 1 (N = 1, 2).

The second term is the rounding of the result itself: an output of value v
cannot be expected closer than a few eps |v|, because the inverse
transform's last butterflies add two partial sums of size |v| / 2, each
rounded to eps |v| / 2.  For two dense operands the two terms are of one
size (|a| |b| / sqrt(N) ~ sigma^2 sqrt(N) ~ the largest lag).  Where an
operand set is sparse (n = 1 or m = 1, an impulse against a one-sample
signal, the sparse integer signals above 10^7 products, the impulse kernels
of InverseFilter) |a|_2 |b|_2 / sqrt(N) falls below one unit in the last
place of the largest output, by sqrt(N / log2 N), 2000-fold at 2^27: numpy's
own ratio on the first term alone grows from 1.5 at 2^4 to 52 at 2^15 on
exactly those cases, and stays below 1.6 at every k <= 16 with both terms.
"""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)  # 2^-52

# ---------------------------------------------------------------------------
# The device FFT's launch plans, restated.  COPIED BY HAND from
# algo-dsp_amd/csrc/bigfft.hip (BigFft::BigFft, go_pass, corr_split,
# spectral_half) and capi_spectral.cpp (SpectralRun::fused): a change there
# must be repeated here, and test_spectral_exact.py then shows which plans
# the GPU sweep no longer reaches.
# ---------------------------------------------------------------------------
PLAN_RADICES = {
    0: (), 1: (), 2: (), 3: (),  # k_dft_small
    4: (16,), 5: (32,), 6: (64,), 7: (128,), 8: (256,), 9: (512,), 10: (1024,), 11: (2048,), 12: (4096,),
    13: (128, 64), 14: (128, 128), 15: (256, 128), 16: (256, 256), 17: (512, 256), 18: (512, 512),
    19: (128, 64, 64), 20: (128, 128, 64), 21: (128, 128, 128), 22: (256, 128, 128), 23: (256, 256, 128),
    24: (256, 256, 256), 25: (512, 256, 256), 26: (512, 512, 256), 27: (512, 512, 512),
}
K_MAX = 27
PF_F, PF_G = 16, 512  # AD_FFT_PF_F, AD_FFT_PF_G
SPLIT0_F, ABSMAX_MAX_GROUPS = 16, 8192  # AD_SPLIT0_F, kAbsmaxMaxGroups


def plan_kind(k):
    r = PLAN_RADICES[k]
    return "dft_small" if not r else f"{len(r)}-pass " + "x".join(map(str, r))


def unfused(k):
    """capi_spectral.cpp SpectralRun::fused(): N < 32 stages zero-padded copies
    and runs forward, k_spec_op and inverse separately."""
    return (1 << k) < 32


def corr_packs(N, n, m):
    """capi_spectral.cpp SpectralRun::packs (and fused()): CorrelateFFT takes
    one transform of a + i b below 2^25 while max(n, m) <= 2^17 sqrt(min(n, m));
    otherwise two transforms, as Deconvolve."""
    return 32 <= N < (1 << 25) and max(n, m) ** 2 <= (1 << 34) * min(n, m)


def corr_fused(k):
    """spectral_half: forward-last / inverse-first kernel (packed CorrelateFFT only)."""
    if unfused(k) or k >= 25:
        return False
    f, h = PLAN_RADICES[k], PLAN_RADICES[k - 1]
    return len(f) >= 2 and len(h) >= 2 and f[-1] == 256 and h[0] == 256 and (1 << k) // 256 >= 16


def corr_split(k):
    """BigFft::corr_split: k_corr_split0 + the PACKIN second pass."""
    if not corr_fused(k):
        return False
    N, f = 1 << k, PLAN_RADICES[k]
    return f == (256, 256, 256) and N // 256 // SPLIT0_F <= ABSMAX_MAX_GROUPS and N // 256 // PF_F >= 2 * PF_G


def _pf_ok(N, Ns):
    return (N // 256) % PF_F == 0 and (Ns == 1 or Ns >= PF_F) and N // 256 // PF_F >= 2 * PF_G


def persistent_passes(k, correlate):
    """Number of k_fft_pass_pf launches (go_pass: radix 256, complex in and
    out, not the half inverse's first pass) in a call at 2^k; `correlate`
    counts the PACKIN launch and leaves out what the fused kernel replaces."""
    if unfused(k):
        return 0
    N, f, h = 1 << k, PLAN_RADICES[k], PLAN_RADICES[k - 1]
    fused = correlate and corr_fused(k)
    cnt, Ns = 0, 1
    for p, R in enumerate(f):
        last = p == len(f) - 1
        if p > 0 and R == 256 and not (fused and last) and (_pf_ok(N, Ns) or (correlate and corr_split(k) and p == 1)):
            cnt += 1
        Ns *= R
    Ns = 1
    for p, R in enumerate(h):
        if 0 < p < len(h) - 1 and R == 256 and _pf_ok(N // 2, Ns):
            cnt += 1
        Ns *= R
    return cnt


def mirror_paired(k, two_input, correlate):
    """go_pass: the half inverse's first pass takes mirror-paired tiles when
    the spectrum is packed (one transform of a + i b, or one input), the pass
    is not the last, and the fused kernel does not replace it."""
    if unfused(k) or two_input or (correlate and k >= 25):  # CorrelateFFT from 2^25: two transforms
        return False
    return len(PLAN_RADICES[k - 1]) >= 2 and not (correlate and corr_fused(k))


def next_pow2(x):
    return 1 << max(0, (int(x) - 1).bit_length())


def log2n(N):
    return max(1.0, float(np.log2(N)))


def err_scale(N, norm_a, norm_b, peak):
    """See the module docstring.  norm_a, norm_b: the operands' 2-norms (or a
    norm and a gain, times the condition factor for the inverses); peak:
    max |exact result|."""
    return EPS * (np.sqrt(log2n(N)) * float(norm_a) * float(norm_b) / np.sqrt(float(N)) + float(peak))


# The packed transform's cross-talk (capi_spectral.cpp SpectralRun::packs).
# With a' = a 2^-ea, b' = b 2^-eb (ea, eb the exponents of max|a|, max|b|)
# in one transform, a fraction rho of each signal reaches the other, and a
# lag is off by up to rho (|a'|_2^2 + |b'|_2^2) 2^(ea+eb), coherently.  rho is
# the asymmetry between a computed twiddle and its mirror's conjugate: each
# twiddle of the LDS transforms is a product of two rounded table entries
# (1/2 ulp each) raised by a register recurrence to at most the 15th power
# (radix 16), 7.5 in the mean, which multiplies the phase error: 7.5 * (1/2 +
# 1/2) ulp ~ 8 eps for one twiddle, and rho is a mean over many.  The packed
# cases are therefore held to GAMMA err_scale + LEAK eps (|a'|^2 + |b'|^2)
# 2^(ea+eb), and never to more than the suite's older bar, 1e-10 max(1, max|exact|).
LEAK = 8.0
OLD_BAR = 1e-10


def leak_term(norm_a, max_a, norm_b, max_b):
    if not (max_a > 0 and max_b > 0):
        return 0.0
    ea, eb = math.frexp(max_a)[1], math.frexp(max_b)[1]
    na, nb = math.ldexp(norm_a, -ea), math.ldexp(norm_b, -eb)
    return LEAK * EPS * math.ldexp(na * na + nb * nb, ea + eb)


def corr_bound(gamma, scale, leak, peak):
    """The largest |error| a correlation case may show: gamma err_scale, plus
    the packed transform's leak (0 when it is not taken), capped at the older bar."""
    return min(gamma * scale + leak, OLD_BAR * max(1.0, peak)) if leak > 0 else gamma * scale


def norm2(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.dot(x, x)))


# ---------------------------------------------------------------- correlation
def impulse(length, p, c):
    v = np.zeros(length)
    v[p] = c
    return v


def shift_b(a, m, p, c):
    """CorrelateFFT(a, c e_p) with e_p of length m: c a, moved to m-1-p."""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros(a.size + m - 1)
    out[m - 1 - p: m - 1 - p + a.size] = c * a
    return out


def shift_a(n, p, c, b):
    """CorrelateFFT(c e_p, b) with e_p of length n: c b reversed, moved to p."""
    b = np.asarray(b, dtype=np.float64)
    out = np.zeros(n + b.size - 1)
    out[p: p + b.size] = c * b[::-1]
    return out


def peak_of(x):
    x = np.asarray(x)
    return float(np.max(np.abs(x))) if x.size else 0.0


def impulse_positions(length):
    return sorted({0, min(1, length - 1), length // 3, length - 1})


DENSE_LIMIT = 10_000_000  # n * m up to which np.correlate on int64 is affordable


def int_signal(length, seed):
    v = np.random.default_rng(seed).integers(-15, 16, size=length)
    if not v.any():
        v[0] = 7
    return v


def int_correlate(a, b):
    """Exact: np.correlate on int64 (|lag| <= 225 min(n, m) < 2^53)."""
    return np.correlate(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), "full")


def sparse_positions(length, k, seed, count=64):
    """At most `count` positions below `length` that hit every digit of plan
    k's index split: 0, 1, R0-1, R0, R0 R1, N/2-1, N/2, the last sample, and
    random ones for the rest."""
    N, r = 1 << k, PLAN_RADICES[k]
    want = [0, 1, N // 2 - 1, N // 2, length - 1, length - 2]
    if r:
        want += [r[0] - 1, r[0], N // r[0], N // r[0] - 1]
        if len(r) > 1:
            want += [r[0] * r[1], r[0] * r[1] + 1, N // (r[0] * r[1])]
    pos = {p for p in want if 0 <= p < length}
    rng = np.random.default_rng(seed)
    while len(pos) < min(count, length):
        pos.add(int(rng.integers(0, length)))
    return np.array(sorted(pos), dtype=np.int64)


def sparse_signal(length, k, seed, count=64):
    """(positions, integer values in [-15, 15] \\ {0})."""
    pos = sparse_positions(length, k, seed, count)
    rng = np.random.default_rng(seed + 1)
    val = rng.integers(1, 16, size=pos.size) * rng.choice([-1, 1], size=pos.size)
    return pos, val.astype(np.int64)


def sparse_correlate(pa, va, pb, vb, m):
    """Exact correlation of two sparse integer signals from their index/value
    lists: (output positions, int64 values), every other lag zero."""
    idx = (pa[:, None] - pb[None, :] + (m - 1)).ravel()
    val = (va[:, None] * vb[None, :]).ravel()
    u, inv = np.unique(idx, return_inverse=True)
    s = np.zeros(u.size, dtype=np.int64)
    np.add.at(s, inv, val)
    return u, s


def densify(pos, val, length):
    x = np.zeros(length)
    x[pos] = val
    return x


# ------------------------------------------------------------------ inverses
REG_DEFAULT_EPS = 1e-6


def go_variance(x):
    """deconvolve.go:326-349: two passes, sequential sums."""
    n = len(x)
    if n == 0:
        return 0.0
    mean = 0.0
    for v in x.tolist():
        mean += v
    mean /= float(n)
    s = 0.0
    for v in x.tolist():
        d = v - mean
        s += d * d
    return s / float(n)


def resolve_eps(method, eps=0.0, noise_var=0.0, signal_var=0.0, signal=None):
    """The regularisation ad_deconvolve resolves (deconvolve.go:180-262); 0 for
    the naive method."""
    if method == 0:
        return 0.0
    if method == 1:
        return eps if eps > 0 else REG_DEFAULT_EPS
    sv = signal_var if signal_var > 0 else go_variance(np.asarray(signal, dtype=np.float64))
    nv = noise_var if noise_var > 0 else sv * 0.01
    nsr = nv / sv
    return nsr if nsr > 0 else 1e-6


def unit_gain(c, eps):
    """The gain on x of a division by h = c e_p: 1/c naive, c / (c^2 + eps)."""
    return 1.0 / c if eps == 0.0 else c / (c * c + eps)


def deconv_unit(x, p, c, eps):
    """Deconvolve(x, c e_p) with m = p + 1: out[t] = x[t + p] gain."""
    x = np.asarray(x, dtype=np.float64)
    olen = x.size - p
    return x[p: p + olen] * unit_gain(c, eps)


# short integer kernels without a spectral zero and the closed-form bounds of
# |H(w)| over all w (so over every DFT grid):
#   [3, 1]:     |H|^2 = 10 + 6 cos w              in [4, 16]
#   [4, -1, 1]: |H|^2 = 16 cos^2 w - 10 cos w + 10, minimum 8.4375 at
#               cos w = 5/16, maximum 36 at cos w = -1
ROUND_TRIP_KERNELS = {
    (3, 1): (2.0, 4.0),
    (4, -1, 1): (float(np.sqrt(8.4375)), 6.0),
}


def round_trip_cond(h):
    lo, hi = ROUND_TRIP_KERNELS[tuple(h)]
    return hi / lo


def circular_convolve_int(x, h):
    """Exact circular convolution at len(x), int64."""
    x = np.asarray(x, dtype=np.int64)
    y = np.zeros_like(x)
    for i, c in enumerate(h):
        y += int(c) * np.roll(x, i)
    return y


def inverse_filter_impulse(N, p, c, eps, length):
    """InverseFilter(c e_p, length, eps), p < N = nextPow2(length):
    c / (c^2 + eps) at (N - p) mod N."""
    out = np.zeros(N)
    out[(N - p) % N] = c / (c * c + eps)
    return out[:length]


# the naive method's zero-bin kernels: (kernel, the first bin with H = 0)
def zero_bin_cases(N):
    cases = [((1.0, -1.0), 0), ((1.0, 1.0), N // 2)]
    if N >= 4:
        cases.append(((1.0, 0.0, 1.0), N // 4))
    return cases


# --------------------------------------------- O(N^2) DFT in np.longdouble
LD = np.longdouble
LD_MAX_N = 1024


def _ld_twiddles(N, sign):
    two_pi = 8 * np.arctan(LD(1))
    ang = two_pi * np.arange(N, dtype=LD) / LD(N)
    return np.cos(ang), sign * np.sin(ang)


def ld_dft(xr, xi, sign):
    """DFT (sign = -1) or unscaled inverse (sign = +1) of xr + i xi in
    np.longdouble, O(N^2), in row chunks; returns (re, im)."""
    N = len(xr)
    assert N <= LD_MAX_N
    xr, xi = np.asarray(xr, dtype=LD), np.asarray(xi, dtype=LD)
    wr, wi = _ld_twiddles(N, sign)
    n = np.arange(N, dtype=np.int64)
    outr, outi = np.empty(N, dtype=LD), np.empty(N, dtype=LD)
    for k0 in range(0, N, 128):
        kk = np.arange(k0, min(N, k0 + 128), dtype=np.int64)
        idx = (kk[:, None] * n[None, :]) % N
        cr, ci = wr[idx], wi[idx]
        outr[kk] = cr @ xr - ci @ xi
        outi[kk] = cr @ xi + ci @ xr
    return outr, outi


def _pad(x, N):
    v = np.zeros(N, dtype=LD)
    x = np.asarray(x, dtype=np.float64)[:N]
    v[: x.size] = x
    return v


def ld_deconvolve(x, h, eps):
    """Regularised / Wiener Deconvolve in longdouble: (out, |H| as float64)."""
    n, m = len(x), len(h)
    N = next_pow2(n)
    z = np.zeros(N, dtype=LD)
    xr, xi = ld_dft(_pad(x, N), z, -1)
    hr, hi = ld_dft(_pad(h, N), z, -1)
    d = hr * hr + hi * hi + LD(eps)
    yr, yi = (xr * hr + xi * hi) / d, (xi * hr - xr * hi) / d  # X conj(H) / d
    outr, _ = ld_dft(yr, yi, +1)
    olen = n - m + 1 if n - m + 1 > 0 else n
    return (outr / LD(N))[:olen].astype(np.float64), np.sqrt((hr * hr + hi * hi).astype(np.float64))


def ld_inverse_filter(h, length, eps):
    N = next_pow2(length)
    hr, hi = ld_dft(_pad(h, N), np.zeros(N, dtype=LD), -1)
    d = hr * hr + hi * hi + LD(eps)
    outr, _ = ld_dft(hr / d, -hi / d, +1)
    return (outr / LD(N))[:length].astype(np.float64), np.sqrt((hr * hr + hi * hi).astype(np.float64))


def reg_factors(absH, eps):
    """(largest gain |H| / (|H|^2 + eps), condition factor) of a regularised
    division: the factor is max|H| over the smallest effective divisor,
    max(min|H|, sqrt(eps)), the amplification of a relative rounding eps_m in
    H's large bins when it lands on the small ones."""
    absH = np.asarray(absH, dtype=np.float64)
    gain = float(np.max(absH / (absH * absH + eps)))
    cond = float(np.max(absH) / max(float(np.min(absH)), float(np.sqrt(eps))))
    return gain, max(1.0, cond)


def dense_kernel(m, seed):
    """A dense kernel for the longdouble reference: noise with a dominant tap
    (|H| stays clear of zero for short m, reaches small values for long m)."""
    h = np.random.default_rng(seed).standard_normal(m)
    h[0] += 2.0
    return h


# ---------------------------------------------------------------------------
# The sweep's cases, shared by the CPU proof of the references (C oracle and
# numpy, k <= 16) and the GPU sweep, so that what the GPU is held to is what
# the CPU run proved.  Host (numpy) arrays: the GPU sweep builds the same
# cases from device tensors above 2^22.
# ---------------------------------------------------------------------------
def noise(length, seed):
    return np.random.default_rng(seed).standard_normal(length)


def corr_splits(k):
    """(n, m) with nextPow2(n + m - 1) = 2^k: no padding, maximal padding,
    m = 1, n = 1, m > n, and both parities of m - 1 and of n."""
    N = 1 << k
    if k == 0:
        return [(1, 1)]
    m1, m2, h = N // 3 + 1, N // 3 + 2, N // 2 + 2
    cand = [(N - m1 + 1, m1), (N - m2 + 1, m2),  # n + m - 1 = N, m - 1 of both parities
            (h - max(1, h // 3), max(1, h // 3)),  # n + m - 1 = N/2 + 1
            (N, 1), (N - 1, 1), (1, N), (1, N - 1),  # m = 1, n = 1
            (max(1, N // 4), (2 * N) // 3 + 1), (max(1, N // 4) + 1, (2 * N) // 3)]  # m > n
    out = []
    for n, m in cand:
        if n >= 1 and m >= 1 and next_pow2(n + m - 1) == N and (n, m) not in out:
            out.append((n, m))
    return out


SCALE_PAIRS = ((2.0**40, 2.0**-40), (2.0**600, 2.0**-600))  # the second takes the clamped two-factor path


def corr_cases(k, n, m):
    """Yields (kind, name, a, b, exact, scale, leak) for one (n, m) split;
    leak is leak_term where the packed transform is taken, else 0."""
    N = 1 << k
    packs = corr_packs(N, n, m)

    def lk(na_, ma_, nb_, mb_):
        return leak_term(na_, ma_, nb_, mb_) if packs else 0.0

    a0, b0 = noise(n, 1000 * k + n), noise(m, 2000 * k + m)
    na, nb, pa_, pb_ = norm2(a0), norm2(b0), peak_of(a0), peak_of(b0)
    for p in impulse_positions(m):
        yield "corr", f"shift_b p={p}", a0, impulse(m, p, 1.0), shift_b(a0, m, p, 1.0), err_scale(N, na, 1.0, pa_), lk(na, pa_, 1.0, 1.0)
    for p in impulse_positions(n):
        yield "corr", f"shift_a p={p}", impulse(n, p, 1.0), b0, shift_a(n, p, 1.0, b0), err_scale(N, nb, 1.0, pb_), lk(1.0, 1.0, nb, pb_)
    for i, (sa, sb) in enumerate(SCALE_PAIRS):
        if i == 0:
            yield ("corr", f"shift_b scales {sa:g},{sb:g}", sa * a0, impulse(m, m // 3, sb),
                   shift_b(a0, m, m // 3, 1.0), err_scale(N, na, 1.0, pa_), lk(na, pa_, 1.0, 1.0))
        else:
            yield ("corr", f"shift_a scales {sb:g},{sa:g}", impulse(n, n // 3, sb), sa * b0,
                   shift_a(n, n // 3, 1.0, b0), err_scale(N, nb, 1.0, pb_), lk(1.0, 1.0, nb, pb_))
    if n * m <= DENSE_LIMIT:
        ai, bi = int_signal(n, 31 * k + n), int_signal(m, 37 * k + m)
        exact = int_correlate(ai, bi).astype(np.float64)
        yield ("corr", "int dense", ai.astype(np.float64), bi.astype(np.float64), exact,
               err_scale(N, norm2(ai), norm2(bi), peak_of(exact)),
               lk(norm2(ai), peak_of(ai), norm2(bi), peak_of(bi)))
    else:
        (pa, va), (pb, vb) = sparse_signal(n, k, 41 * k + n), sparse_signal(m, k, 43 * k + m)
        idx, val = sparse_correlate(pa, va, pb, vb, m)
        exact = densify(idx, val, n + m - 1)
        yield ("corr", "int sparse", densify(pa, va, n), densify(pb, vb, m), exact,
               err_scale(N, norm2(va), norm2(vb), float(np.max(np.abs(val)))),
               lk(norm2(va), peak_of(va), norm2(vb), peak_of(vb)))


DENSE_K = 22  # noise-filled host arrays up to here; zeros and a few writes above
LD_K = 10  # the longdouble DFT reference up to N = 1024
WIENER_DEFAULT_K = 12  # Wiener with its default variances (sequential sums restated in Python) for 1 <= k <= this
# (n = 1 has variance 0 and the reference's noise-to-signal ratio is 0/0: given variances there)


def _signal(k, seed, integer=False):
    """(x, sparse?) of length N = 2^k: dense noise / integers up to DENSE_K,
    a sparse integer signal above."""
    N = 1 << k
    if k <= DENSE_K:
        return (int_signal(N, seed).astype(np.float64) if integer else noise(N, seed)), False
    pos, val = sparse_signal(N, k, seed)
    return densify(pos, val, N), True


def deconv_cases(k):
    """Yields (kind, name, x, h, (method, eps, noise_var, signal_var), exact,
    scale); n = N = 2^k."""
    N = 1 << k
    x, sparse = _signal(k, 50 + k)
    nx = norm2(x)
    ps = sorted({0, min(1, N - 1), N // 2, N - 1})
    for method in (0, 1, 2):
        for i, p in enumerate(ps):
            for c in ((1.0, 0.125) if k <= DENSE_K else ((1.0, 0.125)[i % 2],)):
                if method == 1:
                    o = (1, 0.0 if c == 1.0 else 1e-3, 0.0, 0.0)
                elif method == 2:
                    o = (2, 0.0, 0.0, 0.0) if 1 <= k <= WIENER_DEFAULT_K else (2, 0.0, 2.0**-7, 1.0)
                else:
                    o = (0, 0.0, 0.0, 0.0)
                eps = resolve_eps(o[0], o[1], o[2], o[3], x)
                exact = deconv_unit(x, p, c, eps)
                peak = peak_of(exact)
                yield ("deconv", f"unit method={method} p={p} c={c:g}", x,
                       impulse(p + 1, p, c), o, exact, err_scale(N, nx, unit_gain(c, eps), peak))
    xi, sparse = _signal(k, 60 + k, integer=True)
    for h in ROUND_TRIP_KERNELS:
        if len(h) > N:
            continue
        y = circular_convolve_int(xi.astype(np.int64), h).astype(np.float64)
        exact = xi[: N - len(h) + 1]
        peak = peak_of(exact)
        yield ("deconv", f"round trip h={list(h)}", y,
               np.array(h, dtype=np.float64), (0, 0.0, 0.0, 0.0), exact,
               err_scale(N, norm2(xi), round_trip_cond(h), peak))
    if k <= LD_K:
        h = dense_kernel(min(N, N // 4 + 1), 70 + k)
        for o in ((1, 1e-3, 0.0, 0.0), (2, 0.0, 0.0, 0.0) if k >= 1 else (2, 0.0, 2.0**-7, 1.0)):
            eps = resolve_eps(o[0], o[1], o[2], o[3], x)
            exact, absH = ld_deconvolve(x, h, eps)
            gain, cond = reg_factors(absH, eps)
            yield ("deconv", f"dense kernel method={o[0]}", x, h, o, exact, err_scale(N, nx, gain * cond, peak_of(exact)))


def invfilt_cases(k):
    """Yields (kind, name, h, length, eps, exact, scale); N = 2^k."""
    N = 1 << k
    eps = 1e-3
    ps = sorted({0, min(1, N - 1), N // 2, N - 1})
    for i, p in enumerate(ps):
        c = (1.0, 0.125)[i % 2]
        peak = c / (c * c + eps)
        yield ("invfilt", f"impulse p={p} c={c:g}", impulse(p + 1, p, c), N, eps,
               inverse_filter_impulse(N, p, c, eps, N), err_scale(N, peak, 1.0, peak))
    if k >= 2:
        L = N - 1  # length < N, same transform
        peak = 1.0 / (1.0 + eps)
        for p in (1, N // 2):  # the peak at N - 1 is cut (all zeros), the one at N/2 stays
            yield ("invfilt", f"impulse p={p} length=N-1", impulse(p + 1, p, 1.0), L, eps,
                   inverse_filter_impulse(N, p, 1.0, eps, L), err_scale(N, peak, 1.0, peak))
    # the kernel longer than N: what lies past index N must not matter (deconvolve.go:367)
    p = min(1, N - 1)
    h = np.concatenate([impulse(N, p, 0.125), 1e6 * noise(7, 80 + k)])
    peak = 0.125 / (0.125 * 0.125 + eps)
    yield ("invfilt", "kernel longer than N", h, N, eps, inverse_filter_impulse(N, p, 0.125, eps, N),
           err_scale(N, peak, 1.0, peak))
    if k <= LD_K:
        h = dense_kernel(N // 2 + 1, 90 + k)
        exact, absH = ld_inverse_filter(h, N, eps)
        _, cond = reg_factors(absH, eps)
        yield "invfilt", "dense kernel", h, N, eps, exact, err_scale(N, norm2(exact), cond, peak_of(exact))
