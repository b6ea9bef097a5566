"""Every plan of the FFT convolution engine (Upols: csrc/upols_engine.cpp,
conv_kernels.hip, fft_kernels.hip, fft_device.hpp) against exact references,
through every entry point that runs on it:

  a  multi      MultiChannelConvolver.process_device, serial schedule: hops
                64 .. 8192 x P in {1, 2, 3, 5, 9, 17} (the five PC instances
                of the MAC and a tail after a full group of 16), K = L - 3, L,
                L + 1, (P - 1) L + 5, chunks of 2 blocks, the ring wrap;
  b  big-P      P = 256 (the last mid_in_k3 = 1 value) at hop 2048 and P = 257
                (mid_in_k3 = 0 at a split size) at hops 2048, 4096, 8192;
  c  mix        process_device_mix (the fused-mix K3) at hops 2048 .. 8192, both
                parities, P in {3, 17}; the scratch + k_mixdown fallback at 1024;
  d  part       NewPartitionedConvolution(h, lo, 13), lo in {6, 7, 10, 13}, and
                PartitionedConvolutionMulti (lo = 7, C = 2): the accumulate K3
                and the fused two-partition stage;
  e  stream     NewStreamingOverlapSave / Add, B = hop for every hop (the gated
                chain from 2048), B = 480 on a 131072-tap kernel (the carried
                partial block at hop 2048), MultiChannelStreamingConvolver at
                B = 256 and 1000;
  f  batch      NewOverlapSave(h, 0) / NewOverlapAdd(h, 0) at batch_hop = 256
                (the smallest it picks), 1024 and 8192;
  g  float32    NewStreamingOverlapSave32 (B = 4096), NewPartitionedConvolution32
                (7, 13): integer cases whose exact outputs are float32 numbers.

The references (tests/conv_exact.py) are shifts, int64 sums of <= 64 shifted
copies, np.convolve on int64 and, at P <= 5 and hop <= 1024, the C oracle's
long-double direct sum (2^-64 relative, the one reference that is not exact):
none is an FFT, and tests/test_conv_exact.py proves them on the CPU.

Bound.  For every case  max |gpu - exact| <= GAMMA * err_scale,  GAMMA =
8 gamma_ref, err_scale as conv_exact defines it and gamma_ref the worst error /
err_scale of the same algorithm on numpy's fp64 FFT over the same cases, per
hop ("part": the partitioned handles), measured and pinned by
test_conv_exact.py.  The factor 8 is for what the device legitimately does
differently: radix-16 register passes with powered twiddles, the split real
transform, the MAC's run order.  A float32 handle's bound gains half a
float32 ulp of |exact|; where the fp64 bound is below that half ulp the result
must EQUAL the exact value.  The older bars (1e-7 RMS, 1e-9 max on
unit-variance data) are 10^5 .. 10^6 err_scale.

    hop     gamma_ref (numpy)   C oracle   GAMMA    MI355X worst (entry)
    64      1.12                1.14        8.96    2.67 (multi, P = 9)
    128     1.25                1.36       10.00    2.55 (multi, P = 3)
    256     1.44                1.22       11.52    2.31 (multi, P = 1)
    512     1.31                1.25       10.48    2.90 (multi, P = 1)
    1024    1.27                1.36       10.16    2.83 (multi-stream, B = 1000)
    2048    1.11                1.46        8.88    2.81 (multi, P = 1)
    4096    1.21                1.42        9.68    3.34 (multi, P = 1)
    8192    1.31                1.46       10.48    4.04 (mix, P = 17)
    part    1.18                1.26        9.44    2.50 (lo = 13: one stage)

The device is 1.6 .. 3.1 times numpy at every hop, no plan, partition count or
entry point apart from the others: the sweep found nothing to fix.

Every test prints CONV_RATIO lines with the figures of its run; RECORDED has
those of one MI355X run per (entry point, hop, P).
"""
import numpy as np
import pytest

import conv_exact as E
import oracle_lib as O
from test_conv_exact import GAMMA_REF

pytestmark = pytest.mark.gpu

GAMMA = {k: 8.0 * g for k, g in GAMMA_REF.items()}

# The device's worst error / err_scale (MI355X, one run of this file; the
# tests print those of every run).  "multi": hop -> the figures in the order
# of conv_exact.multi_variants (P = 1 at K = L - 3 and K = L, 2, 3, 5, 9, 17,
# P = 3 with the ring wrap); "big-P" and "mix": (hop, P) (both parities give
# one figure); the partitioned entries: lo; the others: hop (overlap-save and
# overlap-add give one figure: the same engine).
RECORDED = {
    "multi": {
        64: (2.33, 2.32, 1.64, 1.71, 1.98, 2.67, 2.03, 2.13),
        128: (1.90, 2.24, 1.81, 2.55, 2.06, 2.09, 2.06, 2.55),
        256: (2.31, 2.01, 2.06, 1.81, 1.71, 2.17, 1.84, 1.96),
        512: (2.39, 2.90, 1.73, 1.88, 1.93, 2.20, 2.03, 1.89),
        1024: (2.33, 2.40, 2.52, 2.12, 2.16, 2.10, 2.65, 2.14),
        2048: (2.81, 2.48, 2.03, 2.05, 2.44, 2.29, 2.27, 2.23),
        4096: (3.34, 3.09, 2.56, 2.50, 2.50, 2.62, 2.64, 2.83),
        8192: (3.38, 3.46, 2.68, 2.48, 2.52, 2.88, 2.99, 2.72),
    },
    "big-P": {(2048, 256): 1.87, (2048, 257): 1.57, (4096, 257): 2.88, (8192, 257): 2.39},
    "mix": {(2048, 3): 2.46, (2048, 17): 2.40, (4096, 3): 2.49, (4096, 17): 2.73, (8192, 3): 3.74, (8192, 17): 4.04,
            (1024, 3): 1.86},
    "part": {6: 0.77, 7: 0.70, 10: 1.17, 13: 2.50},
    "part-multi": {7: 0.72},
    "stream": {64: 1.85, 128: 2.03, 256: 1.80, 512: 1.80, 1024: 2.10, 2048: 1.95, 4096: 2.67, 8192: 2.68},
    "stream-carried": {2048: 1.86},
    "multi-stream": {256: 2.04, 1024: 2.83},
    "batch": {256: 1.79, 1024: 2.22, 8192: 2.28},
    "stream32": {4096: 0.00},  # after the half float32 ulp: every output equals the exact value
    "part32": {7: 0.01},
}


def _ratio(err, scale):
    if err != err:
        return float("inf")
    if scale > 0:
        return err / scale
    return 0.0 if err == 0 else float("inf")


class _Worst:
    """Worst error / err_scale of one (entry point, hop, P); finish() prints
    the CONV_RATIO line and asserts every case's bound."""

    def __init__(self, entry, hop, P, gamma=None):
        self.entry, self.hop, self.P = entry, hop, P
        self.gamma = GAMMA[hop] if gamma is None else gamma
        self.worst, self.name, self.bad, self.count = 0.0, "", [], 0

    def add(self, name, got, exact, scale, slack=None):
        """slack: per-sample addition to the bound (float32: half an ulp of |exact|)."""
        assert got.shape == exact.shape, (name, got.shape, exact.shape)
        d = np.abs(got.astype(np.float64) - exact)
        if slack is not None:
            d = np.where(np.isnan(d), np.inf, np.maximum(d - slack, 0.0))
        err = float(np.max(d)) if d.size else 0.0
        if np.isnan(d).any():
            err = float("nan")
        r = _ratio(err, scale)
        self.count += 1
        if r >= self.worst:
            self.worst, self.name = r, name
        if not err <= self.gamma * scale:
            self.bad.append(f"{name}: err {err:.3e} = {r:.1f} err_scale (bound {self.gamma:.2f})")

    def finish(self, note=""):
        print(f"CONV_RATIO entry={self.entry} hop={self.hop} P={self.P} case={self.name!r} worst={self.worst:.3f} "
              f"gamma={self.gamma:.2f} cases={self.count}{note}")
        assert self.count > 0
        assert not self.bad, f"{self.entry} hop {self.hop} P {self.P}: " + "; ".join(self.bad[:8])


def _guarded(rows, length):
    """NaN-filled device rows with one extra element before and after each:
    (buffer, pointer to row 0's first element, row stride)."""
    import torch

    buf = torch.full((rows, length + 2), float("nan"), dtype=torch.float64, device="cuda")
    return buf, buf.data_ptr() + 8, length + 2


def _unguard(buf, what):
    a = buf.cpu().numpy()
    assert np.isnan(a[:, 0]).all(), f"{what}: wrote ahead of a row"
    assert np.isnan(a[:, -1]).all(), f"{what}: wrote past a row"
    return a[:, 1:-1]


def _to_dev(rows):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.float64)).cuda()


def _multi_call(eng, chans, out_len, mix=None):
    """process_device (or process_device_mix with first parity `mix`) of one
    engine on the cases' inputs; returns the guarded output rows."""
    import torch

    dx = _to_dev([c.x for c in chans])
    n = dx.shape[1]
    buf, ptr, stride = _guarded(len(chans) if mix is None else 2, out_len)
    torch.cuda.synchronize()
    if mix is None:
        eng.process_device(dx.data_ptr(), n, n, ptr, stride, out_len)
    else:
        eng.process_device_mix(dx.data_ptr(), n, n, ptr, stride, out_len, mix, 0, out_len)
    torch.cuda.synchronize()
    return _unguard(buf, "process_device")


# --------------------------------------------------- a. process_device, serial
MULTI_PARAMS = [(L, i) for L in E.HOPS for i in range(len(E.multi_variants(64)))]


@pytest.mark.parametrize("hop,variant", MULTI_PARAMS)
def test_multi_plan(gpu, hop, variant):
    """Two engines of C = 3 (ir_index [1, 0, 1], chunks of 2 blocks) per (hop,
    K): input impulse / kernel impulse / second impulse or dense noise against
    the long-double sum; sparse integer input / sparse integer kernel / dense
    integers or a second sparse input (conv_exact.multi_engines)."""
    from algodsp import conv

    name, P, K, n = E.multi_variants(hop)[variant]
    w = _Worst("multi", hop, P)
    for tag, kernels, chans in E.multi_engines(hop, P, K, n, O.direct_ld):
        eng = conv.MultiChannelConvolver(kernels, hop=hop, channels=3, ir_index=list(E.MULTI_IR_INDEX),
                                         chunk_blocks=E.MULTI_CHUNK)
        assert eng.schedule()[0] == conv.MultiChannelConvolver.SCHED_SERIAL
        y = _multi_call(eng, chans, n + K - 1)
        for i, c in enumerate(chans):
            w.add(f"{name} {tag} ch{i} {c.family}", y[i], c.exact, c.scale(hop))
    w.finish(f" variant={name!r}")


# ------------------------------------------------------ b. P = 256 and 257
@pytest.mark.parametrize("hop,P", E.BIG_P)
def test_big_partition_count(gpu, hop, P):
    """K = (P - 1) L + 5, one channel, n = 4 L + 17: a sparse integer kernel
    (the dense host array is mostly zeros) against a dense integer input."""
    from algodsp import conv

    K, n, c = E.big_p_case(hop, P)
    eng = conv.MultiChannelConvolver(c.h.reshape(1, -1), hop=hop, channels=1, chunk_blocks=E.MULTI_CHUNK)
    y = _multi_call(eng, [c], n + K - 1)
    w = _Worst("big-P", hop, P)
    w.add(f"mid_in_k3={int(E.mid_in_k3(hop, P))} {c.family}", y[0], c.exact, c.scale(hop))
    w.finish()


# ------------------------------------------------------------ c. fused mix
@pytest.mark.parametrize("hop,P,parity", E.MIX_CASES)
def test_mix_plan(gpu, hop, P, parity):
    """process_device_mix, C = 3, integer cases: the exact mix is an exact
    integer sum; a side's scale is the sum of its channels' scales.  Hop 1024
    takes the smaller-hop fallback (convolve into scratch, then k_mixdown)."""
    from algodsp import conv

    K, n, kernels, chans = E.mix_engine(hop, P)
    eng = conv.MultiChannelConvolver(kernels, hop=hop, channels=3, ir_index=list(E.MULTI_IR_INDEX),
                                     chunk_blocks=E.MULTI_CHUNK)
    m = _multi_call(eng, chans, n + K - 1, mix=parity)
    w = _Worst("mix", hop, P)
    for side, (exact, scale) in enumerate(E.mix_sides(chans, hop, parity)):
        assert scale > 0  # C = 3: both sides have a channel
        w.add(f"parity={parity} side={side}", m[side], exact, scale)
    w.finish(f" parity={parity}")


# ----------------------------------------------------- d. partitioned handles
def _stage_info(g):
    return [g.StageInfo(i) for i in range(g.StageCount())]


@pytest.mark.parametrize("lo", E.PART_LO)
def test_partitioned_plan(gpu, lo):
    """NewPartitionedConvolution(h, lo, 13): a sparse integer kernel with taps
    in every stage and on every stage boundary, K just past the start of the
    order-13 stage, host calls of [lat + 3, 1, 2 lat, 5 lat + 7, 20011] twice;
    exact = the linear convolution delayed by 2^lo."""
    from algodsp import conv

    K = E.part_kernel_len(lo)
    probe = O.Partitioned(np.ones(K), lo, E.PART_HI)
    info = [probe.stage_info(i) for i in range(probe.stage_count())]
    K, sizes, case, scale = E.part_case(lo, info, 40 + lo)
    g = conv.NewPartitionedConvolution(case.h, lo, E.PART_HI)
    assert _stage_info(g) == info and g.Latency() == 1 << lo
    pos, got = 0, []
    for m in sizes:
        out = np.full(m + 2, np.nan)
        g.ProcessBlock(case.x[pos: pos + m], out[1:-1])
        assert np.isnan(out[0]) and np.isnan(out[-1])
        got.append(out[1:-1])
        pos += m
    w = _Worst("part", f"2^{lo}..2^13", len(E.device_stages(K, lo, E.PART_HI)), GAMMA["part"])
    w.add(f"lo={lo} host calls", np.concatenate(got), case.exact, scale)
    w.finish()


def test_partitioned_multi_plan(gpu):
    """PartitionedConvolutionMulti (lo = 7, C = 2), device calls of the same
    lengths; each channel has its own dense integer input."""
    import torch

    from algodsp import conv

    lo, C_ = 7, 2
    K = E.part_kernel_len(lo)
    probe = O.Partitioned(np.ones(K), lo, E.PART_HI)
    info = [probe.stage_info(i) for i in range(probe.stage_count())]
    runs = [E.part_case(lo, info, 60 + c) for c in range(C_)]
    sizes, n = runs[0][1], runs[0][2].x.size
    assert np.array_equal(runs[0][2].h, runs[1][2].h)
    g = conv.PartitionedConvolutionMulti(runs[0][2].h, lo, E.PART_HI, C_)
    dx = _to_dev([r[2].x for r in runs])
    buf, ptr, stride = _guarded(C_, n)
    s = torch.cuda.current_stream()
    pos = 0
    for m in sizes:
        g.process_device(dx.data_ptr() + 8 * pos, n, ptr + 8 * pos, stride, m, s.cuda_stream)
        pos += m
    s.synchronize()
    y = _unguard(buf, "pc_multi")
    w = _Worst("part-multi", f"2^{lo}..2^13", len(E.device_stages(K, lo, E.PART_HI)), GAMMA["part"])
    for c, (_, _, case, scale) in enumerate(runs):
        w.add(f"ch{c}", y[c], case.exact, scale)
    w.finish()


# ------------------------------------------------------------- e. streaming
def _stream_run(g, case, B):
    n = case.x.size
    blocks = [np.ascontiguousarray(case.x[i: i + B]) for i in range(0, n, B)]
    outs = [np.full(B + 2, np.nan) for _ in blocks]
    for blk, out in zip(blocks, outs):  # back to back: hops >= 2048 take the gated chain
        g.ProcessBlockTo(out[1:-1], blk)
    for out in outs:
        assert np.isnan(out[0]) and np.isnan(out[-1])
    return np.concatenate([o[1:-1] for o in outs])


@pytest.mark.parametrize("ola", [False, True])
@pytest.mark.parametrize("hop", E.HOPS)
def test_stream_plan(gpu, hop, ola):
    """B = hop, K = 3 hop + 5, twelve blocks back to back, one handle per
    family: kernel impulse, input impulse on a noise kernel, sparse integer
    kernel on dense integers."""
    from algodsp import conv

    K = 3 * hop + 5
    assert E.stream_hop(hop, K) == (hop, False)
    ctor = conv.NewStreamingOverlapAdd if ola else conv.NewStreamingOverlapSave
    w = _Worst("stream-ola" if ola else "stream-ols", hop, 4)
    hits = 0
    for c in E.stream_cases(hop, K, hop):
        g = ctor(c.h, hop)
        w.add(c.family, _stream_run(g, c, hop), c.exact, c.scale(hop))
        hits += g.LowLatencyStats()[0]
        del g
    w.finish(f" gated={int(E.stream_gated(hop, K))} chain_hits={hits}")


@pytest.mark.parametrize("ola", [False, True])
def test_stream_carried_block(gpu, ola):
    """B = 480 on a 131072-tap sparse integer kernel: hop 2048, the partial
    block carried between calls."""
    from algodsp import conv

    B, K = E.STREAM_CARRIED
    L, partial, c = E.carried_case()
    assert (L, partial) == (2048, True)
    g = (conv.NewStreamingOverlapAdd if ola else conv.NewStreamingOverlapSave)(c.h, B)
    w = _Worst("stream-carried-ola" if ola else "stream-carried-ols", L, E.n_partitions(K, L))
    w.add(f"B={B} {c.family}", _stream_run(g, c, B), c.exact, c.scale(L))
    w.finish()


@pytest.mark.parametrize("B", E.MULTI_STREAM_B)
def test_multi_stream_plan(gpu, B):
    """MultiChannelStreamingConvolver, C = 3 over two integer kernels, twelve
    device blocks; B = 1000 carries the partial block at hop 1024."""
    import torch

    from algodsp import conv

    L, K, n, kernels, chans = E.multi_stream_engine(B)
    s = conv.MultiChannelStreamingConvolver(kernels, B, 3, ir_index=list(E.MULTI_IR_INDEX))
    dx = _to_dev([c.x for c in chans])
    buf, ptr, stride = _guarded(3, n)
    st = torch.cuda.current_stream()
    for i in range(E.STREAM_BLOCKS):
        s.process_block_device(dx.data_ptr() + 8 * i * B, n, ptr + 8 * i * B, stride, st.cuda_stream)
    st.synchronize()
    y = _unguard(buf, "multi-stream")
    w = _Worst("multi-stream", L, 4)
    for i, c in enumerate(chans):
        w.add(f"B={B} ch{i} {c.family}", y[i], c.exact, c.scale(L))
    w.finish(f" B={B}")


# ----------------------------------------------------------------- f. batch
@pytest.mark.parametrize("ola", [False, True])
@pytest.mark.parametrize("K", E.BATCH_K)
def test_batch_plan(gpu, K, ola):
    """NewOverlapSave(h, 0) / NewOverlapAdd(h, 0), n = 5 hops, at kernel
    lengths for which batch_hop picks 256 (its smallest), 1024 and 8192."""
    from algodsp import conv

    L, cases = E.batch_cases(K)
    w = _Worst("batch-ola" if ola else "batch-ols", L, E.n_partitions(K, L))
    for c in cases:
        g = (conv.NewOverlapAdd if ola else conv.NewOverlapSave)(c.h, 0)
        out = np.full(c.exact.size + 2, np.nan)
        g.ProcessTo(out[1:-1], c.x)
        assert np.isnan(out[0]) and np.isnan(out[-1])
        w.add(f"K={K} {c.family}", out[1:-1], c.exact, c.scale(L))
    w.finish(f" K={K}")


# --------------------------------------------------------------- g. float32
def _check32(w, name, got, exact, scale):
    """fp64 bound + half a float32 ulp of |exact|; and equality wherever the
    fp64 bound is below that half ulp, which must be so at every non-zero
    (integer) output."""
    assert got.dtype == np.float32
    bound = w.gamma * scale
    half = E.half_ulp32(exact)
    nz = exact != 0
    assert nz.any() and np.all(np.abs(exact) < 2**24) and np.array_equal(exact, np.round(exact))
    assert bound < float(np.min(half[nz])), (bound, float(np.min(half[nz])))  # the precondition of equality
    assert np.array_equal(got[nz].astype(np.float64), exact[nz]), (
        f"{name}: {int(np.sum(got[nz] != exact[nz]))} outputs differ from the exact float32 value")
    w.add(name, got, exact, scale, slack=half)


def test_float32_stream(gpu):
    """NewStreamingOverlapSave32, B = 4096, K = 3 B + 5: integers below 2^7, at
    most 64 taps, so every exact output is an integer below 2^24."""
    from algodsp import conv

    B = 4096
    c = E.stream_cases(B, 3 * B + 5, B, E.F32_INT_RANGE)[2]
    g = conv.NewStreamingOverlapSave32(c.h.astype(np.float32), B)
    x32 = c.x.astype(np.float32)
    outs = []
    for i in range(0, x32.size, B):
        out = np.full(B + 2, np.nan, dtype=np.float32)
        g.ProcessBlockTo(out[1:-1], x32[i: i + B])
        assert np.isnan(out[0]) and np.isnan(out[-1])
        outs.append(out[1:-1])
    w = _Worst("stream32", B, 4)
    _check32(w, c.family, np.concatenate(outs), c.exact, c.scale(B))
    w.finish()


def test_float32_partitioned(gpu):
    """NewPartitionedConvolution32(h, 7, 13) on the integer case of entry d
    with values below 2^7."""
    from algodsp import conv

    lo = 7
    K = E.part_kernel_len(lo)
    probe = O.Partitioned(np.ones(K), lo, E.PART_HI)
    info = [probe.stage_info(i) for i in range(probe.stage_count())]
    K, sizes, case, scale = E.part_case(lo, info, 47, E.F32_INT_RANGE)
    g = conv.NewPartitionedConvolution32(case.h.astype(np.float32), lo, E.PART_HI)
    x32 = case.x.astype(np.float32)
    pos, got = 0, []
    for m in sizes:
        out = np.full(m + 2, np.nan, dtype=np.float32)
        g.ProcessBlock(x32[pos: pos + m], out[1:-1])
        assert np.isnan(out[0]) and np.isnan(out[-1])
        got.append(out[1:-1])
        pos += m
    w = _Worst("part32", f"2^{lo}..2^13", len(E.device_stages(K, lo, E.PART_HI)), GAMMA["part"])
    _check32(w, "lo=7 host calls", np.concatenate(got), case.exact, scale)
    w.finish()
