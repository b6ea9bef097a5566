"""Exact references for the FFT convolution engine (Upols: csrc/upols_engine.cpp,
conv_kernels.hip, fft_kernels.hip, fft_device.hpp) and the error scale its
results are judged on.

A helper module, not a test.  None of the references is an FFT:

  kernel impulse   h = c e_p, c a power of two, any input: y = c x moved by p, exact;
  input impulse    x = c e_q, any kernel: y = c h moved by q, exact;
  sparse integer   at most 64 non-zero integer taps (values uniform in
                   [-2^15, 2^15)) against a dense integer operand of the same
                   range, in either role: the int64 sum of <= 64 shifted scaled
                   copies, O(64 n); every partial sum is below 64 2^30 = 2^36,
                   so it is exact in int64 and in float64;
  dense integer    np.convolve on int64, |values| < 2^10, n K <= DENSE_LIMIT;
  dense float      oracle_lib.direct_ld, the O(n K) sum in long double, n K <=
                   LD_LIMIT.  The one reference that is NOT exact: each term
                   and each addition rounds to 2^-64 relative, so its error is
                   at most about 2^-64 sum_k |h_k x_{t-k}|, 2^-11 of the 2^-53
                   relative roundings the device is judged on.

tests/test_conv_exact.py proves them against each other and the C oracle on
the CPU and measures gamma_ref; tests/test_conv_plans_gpu.py runs every plan
of the device engine against them.

Error scale.  A case at hop L transforms at M = 2L.  Block j transforms the
input window w_j = x[(j-1)L .. (j+1)L) (zeros before the start and past the
end), the kernel is cut into partitions h_p of L taps (the last zero padded),
and output block j is the last L samples of the inverse transform of
sum_p W_{j-p} H_p.  A max-abs error is divided by

    err_scale = eps (sqrt(log2 M) sqrt(max_j sum_p |w_{j-p}|_2^2 |h_p|_2^2) / sqrt(M) + max|exact|)

The first term is spectral_exact.err_scale's, summed over the partitions that
meet in one output block: each product W_{j-p} H_p carries the rounding noise
of an fp64 FFT correlation of w_{j-p} with h_p, eps sqrt(log2 M) |w|_2 |h|_2 /
sqrt(M), and the P noises are independent, so their squares add.  For one
partition it is spectral_exact.err_scale(M, |w|, |h|, peak).  The second term
is the rounding of the result itself.  upols_numpy below restates the
algorithm with numpy's fp64 rfft / irfft: its worst error / err_scale over the
sweep's cases is gamma_ref (per hop), and the device is held to 8 gamma_ref.

Composite handles: a stereo mix side is judged on the sum of its channels'
scales; a partitioned handle on the sum over its stages of the scale of that
stage's taps at that stage's partition size (the layout StageInfo reports);
a float32 handle on the fp64 bound plus half a float32 ulp of |exact| (the
ABI: computed in fp64, rounded once to float32).
"""
import math

import numpy as np

import spectral_exact as X
from spectral_exact import EPS, DENSE_LIMIT, impulse, norm2, peak_of  # noqa: F401  (shared vocabulary)

LD_LIMIT = 300_000_000  # n * K up to which oracle_lib.direct_ld is affordable
HOPS = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
INT_RANGE = 1 << 15  # sparse / dense integer operands: uniform in [-2^15, 2^15)
DENSE_INT_RANGE = 1 << 10  # dense x dense through np.convolve
F32_INT_RANGE = 1 << 7  # float32 handles: 64 taps * 2^14 < 2^24, every output an exact float32
MAX_TAPS = 64

# ---------------------------------------------------------------------------
# The engine's plan choices, restated.  COPIED BY HAND from
# algo-dsp_amd/csrc/upols_engine.cpp (pick_pc, Q_, mid_in_k3), capi_conv.cpp
# (batch_hop, setup_stream_engine, gate_setup, ad_conv_multi_stream_create)
# and nupols_engine.cpp (the stage layout): a change there must be repeated
# here, and test_conv_exact.py then shows which plans the GPU sweep no longer
# reaches.
# ---------------------------------------------------------------------------


def n_partitions(K, L):
    return -(-K // L)


def pick_pc(P):
    pc = 1
    while pc < P and pc < 16:
        pc *= 2
    return pc


def ring_rows(P, chunk_blocks):
    """Upols::Q_: rows of the frequency-domain delay line."""
    return chunk_blocks + P + 2 * pick_pc(P) + 1


def mid_in_k3(L, P):
    return L >= 2048 and P <= 256


def batch_hop(K):
    return min(X.next_pow2(max(K, 256)), 8192)


def _largest_pow2_divisor(B, cap):
    d = B & -B
    return min(d, cap)


def stream_hop(B, K, multi=False):
    """(hop, carried partial block?) of a streaming handle with blocks of B."""
    hop = _largest_pow2_divisor(B, 8192)
    partial = False
    if hop < 256 and hop != B and (multi or B >= 64):
        hop = min(8192, max(64 if multi else 1, X.next_pow2(B), X.next_pow2((K + 63) // 64)))
        partial = B % hop != 0
    return hop, partial


def stream_gated(B, K):
    """gate_setup: the pre-enqueued K1 / K2 / K3 chain of calls made back to back."""
    hop, partial = stream_hop(B, K)
    return not partial and hop >= 2048 and B == hop


def device_stages(K, lo, hi):
    """NupolsDev's own layout [(partition size, first tap, taps)]: two
    partitions per size while the size doubles, the rest at 2^hi."""
    out, T, p, pmax = [], 0, 1 << lo, 1 << hi
    while T < K:
        nparts = 2 if p < pmax else -(-(K - T) // p)
        out.append((p, T, min(nparts * p, K - T)))
        T += nparts * p
        if p < pmax:
            p *= 2
    return out


def stage_fused(p, taps):
    """k_pc_small: the stateless two-partition stage."""
    return p <= 1024 and taps <= 2 * p


def reference_stages(stage_info):
    """[(partition size, first tap, taps capacity)] from the (partition size,
    count) pairs that StageInfo / oracle_lib.Partitioned.stage_info report."""
    out, T = [], 0
    for p, cnt in stage_info:
        out.append((int(p), T, int(p) * int(cnt)))
        T += int(p) * int(cnt)
    return out


# ------------------------------------------------------------ the error scale
def block_energy(x, L, blocks):
    """|x[jL .. (j+1)L)|_2^2 for j < blocks (zeros past the end)."""
    x = np.asarray(x, dtype=np.float64)
    buf = np.zeros(blocks * L)
    m = min(x.size, buf.size)
    buf[:m] = x[:m]
    return np.sum(buf.reshape(blocks, L) ** 2, axis=1)


def noise_norm(x, h, L, out_len=None):
    """sqrt(max_j sum_p |w_{j-p}|^2 |h_p|^2) over the blocks of out_len outputs."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    out_len = x.size + h.size - 1 if out_len is None else out_len
    J = max(1, -(-out_len // L))
    e = block_energy(x, L, J)
    W = e + np.concatenate([[0.0], e[:-1]])  # |w_j|^2 = |x block j-1|^2 + |x block j|^2
    Hn = block_energy(h, L, n_partitions(h.size, L))
    return float(np.sqrt(np.max(np.convolve(W, Hn)[:J])))


def err_scale(x, h, L, peak, out_len=None):
    """See the module docstring; peak = max |exact|."""
    M = 2 * L
    return EPS * (math.sqrt(math.log2(M)) * noise_norm(x, h, L, out_len) / math.sqrt(M) + float(peak))


def staged_scale(x, h, stages, stage_peaks, out_len):
    """A partitioned handle: the sum over stages (partition size, first tap,
    capacity) of err_scale of that stage's taps, stage_peaks[s] = max |that
    stage's exact contribution|."""
    h = np.asarray(h, dtype=np.float64)
    s = 0.0
    for (p, T, cap), pk in zip(stages, stage_peaks):
        taps = h[T: T + cap]
        if taps.size:
            s += err_scale(x, taps, p, pk, out_len)
    return s


def half_ulp32(v):
    """Half a float32 unit in the last place of |v| (elementwise)."""
    return 0.5 * np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# --------------------------------------------------- the algorithm, in numpy
def partition_spectra(h, L):
    """rfft at 2L of every partition of h: [P][L + 1] complex128."""
    h = np.asarray(h, dtype=np.float64)
    P = n_partitions(h.size, L)
    buf = np.zeros((P, 2 * L))
    hp = np.zeros(P * L)
    hp[: h.size] = h
    buf[:, :L] = hp.reshape(P, L)
    return np.fft.rfft(buf, axis=1)


def upols_numpy(x, h, L, out_len=None, H=None):
    """The engine's algorithm with numpy's fp64 FFT: rfft of the 2L windows,
    the spectral sum over partitions, irfft, the last L samples of each block.
    The CPU yardstick, not a reference.  H: partition spectra to use instead
    of partition_spectra(h, L) (the perturbation tests)."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    out_len = x.size + h.size - 1 if out_len is None else out_len
    J = max(1, -(-out_len // L))
    H = partition_spectra(h, L) if H is None else H
    P = H.shape[0]
    xp = np.zeros((J + 1) * L)
    m = min(x.size, J * L)
    xp[L: L + m] = x[:m]
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * L)[::L][:J]
    Xf = np.fft.rfft(win, axis=1)
    Y = np.zeros_like(Xf)
    for p in range(min(P, J)):
        Y[p:] += Xf[: J - p] * H[p]
    y = np.fft.irfft(Y, n=2 * L, axis=1)[:, L:]
    return y.ravel()[:out_len]


# ------------------------------------------------------------------ operands
def noise(length, seed):
    return np.random.default_rng(seed).standard_normal(length)


def dense_int(length, seed, rng_=INT_RANGE):
    v = np.random.default_rng(seed).integers(-rng_, rng_, size=length).astype(np.int64)
    if not v.any():
        v[0] = 7
    return v


def boundary_positions(length, L, seed, count=MAX_TAPS, extra=()):
    """At most `count` positions below `length`: 0, length - 1, every block
    boundary b L of the hop with both neighbours (b L - 1, b L, b L + 1),
    `extra`, and random ones for the rest.  When 3 (blocks - 1) + 2 exceeds
    `count` (P = 256, 257) the boundaries kept are the first two, the last
    two, those around the MAC's groups of 16 (15, 16, 17, 32) and a random
    draw of the others."""
    nb = n_partitions(length, L)
    bs = list(range(1, nb))
    room = (count - 2 - len(extra)) // 3
    rng = np.random.default_rng(seed)
    if len(bs) > room:
        keep = [b for b in (1, 2, 15, 16, 17, 32, nb - 2, nb - 1) if 1 <= b < nb]
        keep = list(dict.fromkeys(keep))[:room]
        rest = [b for b in bs if b not in keep]
        rng.shuffle(rest)
        bs = keep + rest[: room - len(keep)]
    want = [0, length - 1] + list(extra)
    for b in bs:
        want += [b * L - 1, b * L, b * L + 1]
    pos = {int(p) for p in want if 0 <= p < length}
    while len(pos) < min(count, length):
        pos.add(int(rng.integers(0, length)))
    return np.array(sorted(pos), dtype=np.int64)


def sparse_int(length, L, seed, rng_=INT_RANGE, extra=()):
    """(positions, non-zero integer values uniform in [-rng_, rng_))."""
    pos = boundary_positions(length, L, seed, extra=extra)
    val = np.random.default_rng(seed + 1).integers(-rng_, rng_, size=pos.size).astype(np.int64)
    val[val == 0] = 1
    return pos, val


def densify(pos, val, length):
    v = np.zeros(length)
    v[pos] = val
    return v


# ---------------------------------------------------------------- references
def shift(v, p, c, out_len):
    """c v moved to p, cut or zero padded to out_len: the convolution of v
    with c e_p (c a power of two: exact)."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(max(out_len, p + v.size))
    out[p: p + v.size] = c * v
    return out[:out_len]


def sparse_convolve(pos, val, dense, out_len=None):
    """Exact convolution of the sparse integer signal (pos, val) with the dense
    integer signal `dense`: (int64 result cut to out_len, the largest |partial
    sum| met on the way)."""
    dense = np.asarray(dense, dtype=np.int64)
    full = int(pos[-1]) + dense.size if len(pos) else dense.size
    acc = np.zeros(full, dtype=np.int64)
    worst = 0
    for p, v in zip(pos.tolist(), val.tolist()):
        seg = acc[p: p + dense.size]
        seg += v * dense
        worst = max(worst, int(np.max(np.abs(seg))))
    out_len = full if out_len is None else out_len
    out = np.zeros(out_len, dtype=np.int64)
    m = min(out_len, full)
    out[:m] = acc[:m]
    return out, worst


def int_convolve(a, b):
    """Exact: np.convolve on int64 (|values| < 2^10: |sum| < 2^20 min(n, K))."""
    return np.convolve(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))


class Case:
    """One channel's worth of work: input x, kernel h (float64 arrays), the
    exact result over out_len samples, and the integer cases' largest partial
    sum (0 otherwise)."""

    def __init__(self, family, x, h, exact, partial=0):
        self.family, self.partial = family, partial
        self.x, self.h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
        self.exact = np.asarray(exact, dtype=np.float64)
        self.peak = peak_of(self.exact)

    def scale(self, L):
        return err_scale(self.x, self.h, L, self.peak, self.exact.size)


def case_kernel_impulse(n, K, p, c, seed, out_len=None):
    x = noise(n, seed)
    out_len = n + K - 1 if out_len is None else out_len
    return Case("kernel-impulse", x, impulse(K, p, c), shift(x, p, c, out_len))


def case_input_impulse(n, h, q, c, out_len=None):
    out_len = n + len(h) - 1 if out_len is None else out_len
    return Case("input-impulse", impulse(n, q, c), h, shift(h, q, c, out_len))


def case_sparse_kernel(n, hpos, hval, K, seed, out_len=None, rng_=INT_RANGE):
    """Sparse integer kernel (given) x dense integer input."""
    xi = dense_int(n, seed, rng_)
    exact, partial = sparse_convolve(hpos, hval, xi, n + K - 1 if out_len is None else out_len)
    return Case("sparse-kernel", xi, densify(hpos, hval, K), exact, partial)


def case_sparse_input(n, L, hi_, seed, out_len=None):
    """Dense integer kernel (given) x sparse integer input."""
    xpos, xval = sparse_int(n, L, seed)
    exact, partial = sparse_convolve(xpos, xval, hi_, n + len(hi_) - 1 if out_len is None else out_len)
    return Case("sparse-input", densify(xpos, xval, n), hi_, exact, partial)


def case_dense_int(n, h_small, seed):
    xi = dense_int(n, seed, DENSE_INT_RANGE)
    exact = int_convolve(xi, h_small)
    return Case("dense-int", xi, h_small, exact, int(np.max(np.abs(exact))))


def case_dense_float(n, h, seed, direct_ld):
    x = noise(n, seed)
    return Case("dense-float", x, h, direct_ld(x, h))


# ---------------------------------------------------------------------------
# The sweep's cases, shared by the CPU measurement of gamma_ref (upols_numpy
# and the C oracle) and the GPU sweep, so that what the GPU is held to is what
# the CPU run measured.
# ---------------------------------------------------------------------------
MULTI_P = (1, 2, 3, 5, 9, 17)
MULTI_IR_INDEX = (1, 0, 1)
MULTI_CHUNK = 2
DENSE_FLOAT_MAX_P, DENSE_FLOAT_MAX_HOP = 5, 1024


def multi_variants(L):
    """(name, P, K, n) of entry a: the five PC instances and 17 (a tail after
    a full group of 16), P = 1 with and without zero padding, and P = 3 with
    more blocks than the delay line has rows."""
    out = [("P1 K=L-3", 1, L - 3, 6 * L + 17), ("P1 K=L", 1, L, 6 * L + 17), ("P2 K=L+1", 2, L + 1, 6 * L + 17)]
    out += [(f"P{P}", P, (P - 1) * L + 5, 6 * L + 17) for P in MULTI_P[2:]]
    out.append(("P3 ring wrap", 3, 2 * L + 5, 16 * L + 17))
    return out


def multi_engines(L, P, K, n, direct_ld=None):
    """Entry a at one (hop, K, n): two engines of C = 3 channels over two
    kernels each, ir_index = [1, 0, 1]; returns [(tag, kernels [2][K], [Case
    per channel])].  Engine "float": kernel 0 an impulse, kernel 1 dense
    noise; channels: input impulse, kernel impulse (noise input), and a second
    input impulse or, at P <= 5 and hop <= 1024 with direct_ld given, dense
    noise against the long-double sum.  Engine "int": kernel 0 sparse
    integer, kernel 1 dense integer; channels: sparse integer input, dense
    integer input against the sparse kernel, and dense x dense (np.convolve,
    |values| < 2^10, where n K allows) or a second sparse input."""
    seed = 100003 * int(math.log2(L)) + 101 * P + K % 97
    assert n_partitions(K, L) == P
    p, c = K - 1, 0.125
    k1 = noise(K, seed + 1)
    ch0 = case_input_impulse(n, k1, L + 3 if n > L + 3 else 0, 32.0)
    ch1 = case_kernel_impulse(n, K, p, c, seed + 2)
    if direct_ld is not None and P <= DENSE_FLOAT_MAX_P and L <= DENSE_FLOAT_MAX_HOP and n * K <= LD_LIMIT:
        ch2 = case_dense_float(n, k1, seed + 3, direct_ld)
    else:
        ch2 = case_input_impulse(n, k1, n - 1, 0.5)
    engines = [("float", np.stack([ch1.h, k1]), [ch0, ch1, ch2])]

    hpos, hval = sparse_int(K, L, seed + 10)
    small = n * K <= DENSE_LIMIT
    kd = dense_int(K, seed + 11, DENSE_INT_RANGE if small else INT_RANGE)
    i0 = case_sparse_input(n, L, kd, seed + 12)
    i1 = case_sparse_kernel(n, hpos, hval, K, seed + 13)
    i2 = case_dense_int(n, kd, seed + 14) if small else case_sparse_input(n, L, kd, seed + 15)
    engines.append(("int", np.stack([i1.h, kd.astype(np.float64)]), [i0, i1, i2]))
    return engines


BIG_P = ((2048, 256), (2048, 257), (4096, 257), (8192, 257))  # entry b: (hop, P)


def big_p_case(L, P):
    """Entry b: K = (P - 1) L + 5, n = 4 L + 17, one channel, a sparse integer
    kernel against a dense integer input."""
    K, n = (P - 1) * L + 5, 4 * L + 17
    hpos, hval = sparse_int(K, L, 7000 + L + P)
    return K, n, case_sparse_kernel(n, hpos, hval, K, 7100 + L + P)


MIX_CASES = [(L, P, par) for L in (2048, 4096, 8192) for P in (3, 17) for par in (0, 1)] + [(1024, 3, 0)]


def mix_engine(L, P):
    """Entry c: C = 3 over a sparse integer kernel (0) and a dense integer
    kernel (1), ir_index [1, 0, 1]; integer cases only, so the exact mix is an
    exact integer sum (three channels of < 2^36: below 2^38)."""
    K, n = (P - 1) * L + 5, 6 * L + 17
    seed = 9000 + L + P
    hpos, hval = sparse_int(K, L, seed)
    kd = dense_int(K, seed + 1)
    chans = [case_sparse_input(n, L, kd, seed + 2), case_sparse_kernel(n, hpos, hval, K, seed + 3),
             case_sparse_input(n, L, kd, seed + 4)]
    return K, n, np.stack([chans[1].h, kd.astype(np.float64)]), chans


def mix_sides(chans, L, parity):
    """[(exact, scale)] of the L and R rows: global channel parity + c goes to
    side (parity + c) % 2; a side without channels is all zeros, scale 0."""
    out = []
    for side in range(2):
        mine = [c for i, c in enumerate(chans) if (parity + i) % 2 == side]
        exact = np.zeros(chans[0].exact.size)
        for c in mine:
            exact = exact + c.exact
        out.append((exact, sum(c.scale(L) for c in mine)))
    return out


PART_LO = (6, 7, 10, 13)
PART_HI = 13


def part_kernel_len(lo, hi=PART_HI):
    """Just past the start of the device's order-`hi` stage, 2^(hi+1) -
    2^(lo+1) (device_stages).  It is also the shortest kernel for which the
    layout StageInfo reports has a stage of that order (it starts at 2^hi -
    2^lo there); test_conv_exact.py checks both."""
    return (1 << (hi + 1)) - (1 << (lo + 1)) + 5


def part_call_lengths(lo, cycles=2):
    lat = 1 << lo
    return [lat + 3, 1, 2 * lat, 5 * lat + 7, 20011] * cycles


def part_kernel(lo, stage_info, rng_=INT_RANGE, hi=PART_HI):
    """Entry d's kernel: sparse integer, taps in every stage and on every
    stage boundary of the device's layout (stage starts and the boundary
    between a stage's two partitions, each with both neighbours) and on the
    starts of the layout StageInfo reports."""
    K = part_kernel_len(lo, hi)
    marks = []
    for p, T, taps in device_stages(K, lo, hi):
        marks += [T - 1, T, T + 1, T + p - 1, T + p, T + p + 1, T + min(taps, p) // 2]
    marks += [T for _, T, _ in reference_stages(stage_info)]
    marks = [m for m in dict.fromkeys(marks) if 0 <= m < K][: MAX_TAPS - 2]
    pos = np.array(sorted(set(marks) | {0, K - 1}), dtype=np.int64)
    rng = np.random.default_rng(500 + lo)
    have = set(pos.tolist())
    while len(have) < min(MAX_TAPS, K):
        have.add(int(rng.integers(0, K)))
    pos = np.array(sorted(have), dtype=np.int64)
    val = rng.integers(-rng_, rng_, size=pos.size).astype(np.int64)
    val[val == 0] = 1
    return K, pos, val


def part_case(lo, stage_info, seed, rng_=INT_RANGE, cycles=2):
    """(K, call lengths, Case, scale): dense integer input, exact = the linear
    convolution delayed by 2^lo, the scale summed over StageInfo's stages."""
    K, pos, val = part_kernel(lo, stage_info, rng_)
    sizes = part_call_lengths(lo, cycles)
    n, lat = sum(sizes), 1 << lo
    xi = dense_int(n, seed, rng_)
    full, partial = sparse_convolve(pos, val, xi, n)
    exact = np.concatenate([np.zeros(lat, dtype=np.int64), full])[:n]
    case = Case("partitioned", xi, densify(pos, val, K), exact, partial)
    stages = reference_stages(stage_info)
    peaks = []
    for p, T, cap in stages:
        sel = (pos >= T) & (pos < T + cap)
        peaks.append(float(np.max(np.abs(sparse_convolve(pos[sel] - T, val[sel], xi, n)[0]))) if sel.any() else 0.0)
    return K, sizes, case, staged_scale(case.x, case.h, stages, peaks, n)


STREAM_BLOCKS = 12


def stream_cases(B, K, L, rng_=INT_RANGE):
    """Entry e, one handle each: kernel impulse, dense noise kernel with an
    input impulse, sparse integer kernel with a dense integer input; n =
    12 blocks of B, the output cut to n."""
    n = STREAM_BLOCKS * B
    seed = 3000 + B + K % 89
    hpos, hval = sparse_int(K, L, seed, rng_)
    return [case_kernel_impulse(n, K, K - 1, 0.25, seed + 2, n),
            case_input_impulse(n, noise(K, seed + 3), min(n - 1, B + 3), 2.0, n),
            case_sparse_kernel(n, hpos, hval, K, seed + 4, n, rng_)]


STREAM_CARRIED = (480, 131072)  # (B, K): hop 2048, the carried partial block


def carried_case():
    B, K = STREAM_CARRIED
    L, partial = stream_hop(B, K)
    n = STREAM_BLOCKS * B
    hpos, hval = sparse_int(K, L, 4800)
    return L, partial, case_sparse_kernel(n, hpos, hval, K, 4801, n)


MULTI_STREAM_B = (256, 1000)


def multi_stream_engine(B):
    """C = 3 over two integer kernels, ir_index [1, 0, 1], K = 3 hop + 5."""
    L = stream_hop(B, 3 * X.next_pow2(B) + 5, multi=True)[0]
    K, n = 3 * L + 5, STREAM_BLOCKS * B
    seed = 5000 + B
    hpos, hval = sparse_int(K, L, seed)
    kd = dense_int(K, seed + 1)
    chans = [case_sparse_input(n, L, kd, seed + 2, n), case_sparse_kernel(n, hpos, hval, K, seed + 3, n),
             case_input_impulse(n, kd.astype(np.float64), B + 1, 4.0, n)]
    return L, K, n, np.stack([chans[1].h, kd.astype(np.float64)]), chans


BATCH_K = (200, 1000, 3 * 8192 + 5)  # batch_hop: 256 (its smallest), 1024, 8192


def batch_cases(K):
    L = batch_hop(K)
    n = 5 * L
    seed = 6000 + K % 83
    hpos, hval = sparse_int(K, L, seed)
    return L, [case_sparse_kernel(n, hpos, hval, K, seed + 1), case_input_impulse(n, noise(K, seed + 2), L + 1, 0.5),
               case_kernel_impulse(n, K, K - 1, 2.0, seed + 3)]


# ---------------------------------------------------------------------------
# Perturbation cases (test_conv_exact.py: the bound has teeth).  Unit-variance
# data, two partitions: a kernel impulse against noise, and an input impulse
# against a kernel whose second partition is a weak tail (|h_1|_2 = 2^-8), as
# a reverb's is: rounding that partition's spectrum through complex64 moves the
# result by ~2^-24 |h_1| -- far inside the older 1e-9 bar.
# ---------------------------------------------------------------------------
def teeth_cases(L):
    K, n = 2 * L, 3 * L + 17
    tail = noise(L, 77 + L)
    h = np.concatenate([impulse(L, 0, 1.0), tail * (2.0**-8 / norm2(tail))])
    return [case_kernel_impulse(n, K, L + 1, 1.0, 78 + L), case_input_impulse(n, h, L + 3, 1.0)]
