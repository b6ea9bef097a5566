"""GPU parity of dsp/conv through the HIP C ABI against the CPU oracle.

Tolerances (BASELINE.json north_star): direct convolution is compared
bit-exactly (same operation order, no FMA); FFT paths must be within
1e-7 RMS of the oracle (we also assert a much tighter max-abs bound).
"""
import json
import math
import pathlib

import numpy as np
import pytest

import oracle_lib as O
from algodsp import conv, irlib, signals

pytestmark = pytest.mark.gpu

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "reference_kats.json").read_text())
FFT_RMS_TOL = 1e-7  # north_star: <= 1e-7 RMS for FFT convolution


def rms(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    return float(np.sqrt(np.mean((a - b) ** 2))) if a.size else 0.0


# ------------------------------------------------------------------ Direct
@pytest.mark.parametrize("case", KATS["direct"], ids=lambda c: c["source"])
def test_direct_kat(gpu, case):
    np.testing.assert_allclose(conv.Direct(case["a"], case["b"]), case["expected"], atol=case["tol"], rtol=0)


@pytest.mark.parametrize("n,m", [(1, 1), (7, 3), (100, 15), (100, 16), (48000, 256), (300, 1000), (5, 64),
                                 (3000, 2500), (5000, 1025), (1025, 4097), (70000, 3)])
def test_direct_bit_exact(gpu, n, m):
    a = signals.white_noise(n, 100 + n)
    b = signals.white_noise(m, 200 + m)
    got = conv.Direct(a, b)
    want = O.direct(a, b)
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))


def test_direct_non_finite(gpu):
    """inf / NaN inputs: the LDS kernel's zero-tap shortcut must not turn an
    untaken inf * 0 into NaN (chunks holding one take the bounds-checked loop)."""
    a = signals.white_noise(3000, 7)
    b = signals.white_noise(300, 8)
    a[5], a[1500], a[2999] = np.inf, -np.inf, np.nan
    b[17] = np.inf
    got, want = conv.Direct(a, b), O.direct(a, b)
    assert np.array_equal(got, want, equal_nan=True)


def test_direct_device(gpu):
    import torch

    n, m = 1 << 16, 256
    a, b = signals.white_noise(n, 3), signals.make_test_kernel(m)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dd = torch.empty(n + m - 1, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    conv.direct_device(da.data_ptr(), n, db.data_ptr(), m, dd.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert np.array_equal(dd.cpu().numpy(), O.direct(a, b))
    with pytest.raises(conv.ErrEmptyKernel):
        conv.direct_device(da.data_ptr(), n, db.data_ptr(), 0, dd.data_ptr())


def test_direct_circular(gpu):
    c = KATS["direct_circular"][0]
    np.testing.assert_allclose(conv.DirectCircular(c["a"], c["b"]), c["expected"], atol=1e-10)
    a, b = signals.white_noise(257, 1), signals.white_noise(257, 2)
    assert np.array_equal(conv.DirectCircular(a, b), O.direct_circular(a, b))
    with pytest.raises(conv.ErrLengthMismatch):
        conv.DirectCircular([1, 2, 3], [1, 2])


@pytest.mark.parametrize("m", [5, 64, 65, 300, 5000])
@pytest.mark.parametrize("mode", [conv.ModeFull, conv.ModeSame, conv.ModeValid])
def test_convolve_mode(gpu, m, mode):
    a = signals.make_test_signal(3000)
    b = signals.make_test_kernel(m)
    got = conv.ConvolveMode(a, b, mode)
    want = O.convolve_mode(a, b, mode)
    assert got.shape == want.shape
    if m <= 64:
        assert np.array_equal(got, want)
    else:
        assert rms(got, want) < FFT_RMS_TOL and np.max(np.abs(got - want)) < 1e-9


def test_convolve_commutative_swap(gpu):
    a, b = signals.white_noise(50, 1), signals.white_noise(400, 2)
    np.testing.assert_allclose(conv.Convolve(a, b), conv.Convolve(b, a), atol=1e-10)


# --------------------------------------------------------------- streaming
def test_streaming_ols_impulse_kat(gpu):
    c = KATS["streaming_ols_impulse"]
    s = conv.NewStreamingOverlapSave(c["kernel"], c["block_size"])
    np.testing.assert_allclose(s.ProcessBlock(c["blocks"][0]), c["expected_first"], atol=c["tol"])
    assert s.BlockSize() == 4 and s.KernelLen() == 3 and s.FFTSize() == 8


@pytest.mark.parametrize("ola", [False, True])
@pytest.mark.parametrize("K,B,nb", [(4, 8, 4), (3, 4, 3), (5, 3, 4), (100, 64, 5), (1000, 4096, 3), (16384, 4096, 6),
                                    (2048, 256, 12), (4097, 512, 10), (300, 1000, 3), (20000, 16384, 3)])
def test_streaming_matches_oracle(gpu, ola, K, B, nb):
    h = signals.make_test_kernel(K) if K > 1 else np.ones(1)
    x = signals.white_noise(B * nb, K + B)
    ctor = conv.NewStreamingOverlapAdd if ola else conv.NewStreamingOverlapSave
    g = ctor(h, B)
    o = O.Streaming(h, B, ola=ola)
    assert g.FFTSize() == o.fft_size()
    got, want = [], []
    for i in range(nb):
        blk = x[i * B:(i + 1) * B]
        out = np.empty(B)
        g.ProcessBlockTo(out, blk)
        got.append(out)
        want.append(o.process_block(blk))
    got, want = np.concatenate(got), np.concatenate(want)
    assert rms(got, want) < FFT_RMS_TOL
    assert np.max(np.abs(got - want)) < 1e-9 * max(1.0, math.sqrt(K) / 8)


@pytest.mark.parametrize("ola", [False, True])
@pytest.mark.parametrize("K", [16384, 131072])
@pytest.mark.parametrize("B", [480, 960, 1000, 4800, 12000])
def test_streaming_non_pow2_blocks(gpu, ola, K, B):
    """Blocks with no power-of-two divisor >= 256 (10 ms audio blocks at 48 kHz
    and friends): the engine runs at hop max(nextPow2(B), nextPow2(K/64))
    (<= 8192) and carries the
    unfinished block, re-transforming it with more samples on the next call.
    Zero latency, so the concatenated output is the linear convolution
    (streaming_overlap_save.go:100-164): checked against the oracle's batch
    OverlapSave.Process over enough calls to cross several hop boundaries, then
    a Reset and the first calls again."""
    h = irlib.large_church()[0, :K].copy() if K == 131072 else signals.make_test_kernel(K)
    L = min(8192, max(1 << (B - 1).bit_length(), 1 << (-(-K // 64) - 1).bit_length()))
    nb = max(4, (3 * L) // B + 2)
    x = signals.white_noise(B * nb, K + B)
    g = (conv.NewStreamingOverlapAdd if ola else conv.NewStreamingOverlapSave)(h, B)
    assert g.FFTSize() == 1 << (B + K - 2).bit_length()
    got = []
    for i in range(nb):
        out = np.empty(B)
        g.ProcessBlockTo(out, x[i * B:(i + 1) * B])
        got.append(out)
    got = np.concatenate(got)
    want = O.OverlapSave(h, 0).process(x)[:got.size]
    assert rms(got, want) < FFT_RMS_TOL
    assert np.max(np.abs(got - want)) < 1e-9
    g.Reset()
    again = np.concatenate([g.ProcessBlock(x[i * B:(i + 1) * B]) for i in range(2)])
    np.testing.assert_array_equal(again, got[:2 * B])


def test_streaming_preenqueued_chain_paths(gpu):
    """Blocks of one hop >= 2048 run as pre-enqueued K1 -> K2 -> K3 chains whose
    K1 waits in the GPU for the host's go word (StreamGate, conv_kernels.hpp).
    Every path of that protocol against the oracle: back-to-back calls (the
    chain takes the block), a pause longer than K1's 20 ms wait (the chain
    gives up; the call cancels the chain behind it and runs the block with
    ordinary launches), Reset with a chain pending, two handles interleaved,
    and destroy with a chain pending."""
    import time

    K, B = 16384, 4096
    h = signals.make_test_kernel(K)
    x = signals.white_noise(B * 10, 11)
    g = conv.NewStreamingOverlapSave(h, B)
    g2 = conv.NewStreamingOverlapAdd(h[::-1].copy(), B)
    o = O.Streaming(h, B)
    o2 = O.Streaming(h[::-1].copy(), B, ola=True)
    for i in range(10):
        if i in (3, 7):
            time.sleep(0.05)  # K1 of the pending chain times out
        blk = x[i * B:(i + 1) * B]
        got, want = g.ProcessBlock(blk), o.process_block(blk)
        assert rms(got, want) < FFT_RMS_TOL and np.max(np.abs(got - want)) < 1e-9, i
        got2, want2 = g2.ProcessBlock(blk), o2.process_block(blk)
        assert rms(got2, want2) < FFT_RMS_TOL, i
    g.Reset()
    o = O.Streaming(h, B)
    for i in range(3):
        blk = x[i * B:(i + 1) * B]
        assert rms(g.ProcessBlock(blk), o.process_block(blk)) < FFT_RMS_TOL, i
    del g, g2  # destroy with a chain pending (its K1 released at once)


def test_streaming_non_pow2_vs_streaming_oracle(gpu):
    """B = 1000 on a 16384-tap kernel against the oracle's StreamingOverlapSave
    restatement block by block (fftSize nextPow2(B + K - 1) = 32768)."""
    K, B, nb = 16384, 1000, 12
    h = signals.make_test_kernel(K)
    x = signals.white_noise(B * nb, 77)
    g = conv.NewStreamingOverlapSave(h, B)
    o = O.Streaming(h, B)
    for i in range(nb):
        blk = x[i * B:(i + 1) * B]
        got, want = g.ProcessBlock(blk), o.process_block(blk)
        assert rms(got, want) < FFT_RMS_TOL and np.max(np.abs(got - want)) < 1e-9, i


def test_streaming_reset_and_errors(gpu):
    h = signals.make_test_kernel(257)
    s = conv.NewStreamingOverlapSave(h, 256)
    x = signals.white_noise(512, 3)
    first = s.ProcessBlock(x[:256])
    s.ProcessBlock(x[256:])
    s.Reset()
    np.testing.assert_allclose(s.ProcessBlock(x[:256]), first, atol=1e-13)
    with pytest.raises(conv.ErrLengthMismatch):
        s.ProcessBlock(x[:100])
    with pytest.raises(conv.ErrLengthMismatch):
        s.ProcessBlockTo(np.empty(100), x[:256])


def test_streaming_in_place(gpu):
    h = signals.make_test_kernel(64)
    s = conv.NewStreamingOverlapSave(h, 128)
    o = O.Streaming(h, 128)
    x = signals.white_noise(128, 4)
    buf = x.copy()
    s.ProcessBlockTo(buf, buf)  # aliasing allowed
    assert rms(buf, o.process_block(x)) < 1e-12


# ------------------------------------------------------------------- batch
@pytest.mark.parametrize("K,n", [(1, 10), (3, 10), (64, 1000), (257, 4096), (4096, 4096), (5000, 20000),
                                 (16384, 50000), (131072, 70000)])
def test_batch_ols_ola(gpu, K, n):
    h = signals.make_test_kernel(K) if K > 1 else np.ones(1)
    x = signals.white_noise(n, K)
    ols = conv.NewOverlapSave(h, 0)
    ola = conv.NewOverlapAdd(h, 0)
    o_ols = O.OverlapSave(h, 0)
    o_ola = O.OverlapAdd(h, 0)
    assert ols.FFTSize() == o_ols.fft_size() and ols.StepSize() == o_ols.step_size()
    assert ola.FFTSize() == o_ola.fft_size() and ola.BlockSize() == o_ola.block_size()
    want = o_ols.process(x)
    got = ols.Process(x)
    assert rms(got, want) < FFT_RMS_TOL and np.max(np.abs(got - want)) < 1e-8
    got2 = ola.Process(x)
    assert rms(got2, o_ola.process(x)) < FFT_RMS_TOL
    # ProcessTo + reuse of the same handle
    out = np.empty(n + K - 1)
    ols.ProcessTo(out, x)
    assert np.array_equal(out, got)
    with pytest.raises(conv.ErrLengthMismatch):
        ols.ProcessTo(np.empty(n + K), x)
    with pytest.raises(conv.ErrEmptyInput):
        ols.Process(np.empty(0))


# -------------------------------------------------------------- partitioned
@pytest.mark.parametrize("K,lo,hi", [(64, 4, 10), (256, 5, 12), (1024, 6, 13), (8192, 6, 13), (3, 2, 5), (1, 4, 12),
                                     (95432, 7, 13), (5000, 13, 13), (700, 3, 6)])
def test_partitioned_matches_oracle(gpu, K, lo, hi):
    h = signals.make_impulse_kernel(K)
    lat = 1 << lo
    n = max(4 * lat, min(3 * K, 60000))
    x = signals.white_noise(n, K + lo)
    g = conv.NewPartitionedConvolution(h, lo, hi)
    o = O.Partitioned(h, lo, hi)
    assert g.Latency() == o.latency() == lat
    assert g.StageCount() == o.stage_count()
    assert [g.StageInfo(i) for i in range(g.StageCount())] == [o.stage_info(i) for i in range(o.stage_count())]
    # the last size exceeds a stage launch's batch (Nupols::kBatchSamples = 8192)
    sizes = [lat + 3, 1, 2 * lat, lat - 1 if lat > 1 else 1, 5 * lat + 7, 20011]
    pos, step, got, want = 0, 0, [], []
    while pos < n:
        m = min(sizes[step % len(sizes)], n - pos)
        blk = x[pos:pos + m]
        out = np.empty(m)
        g.ProcessBlock(blk, out)
        got.append(out)
        want.append(o.process_block(blk))
        pos += m
        step += 1
    got, want = np.concatenate(got), np.concatenate(want)
    assert rms(got, want) < FFT_RMS_TOL
    assert np.max(np.abs(got - want)) < 1e-9
    with pytest.raises(conv.ErrStageIndexOutOfRange):
        g.StageInfo(g.StageCount())
    with pytest.raises(conv.ErrLengthMismatch):
        g.ProcessBlock(x[:10], np.empty(9))


@pytest.mark.parametrize("lo,n", [(7, 128), (7, 64), (8, 256), (6, 200)])
def test_partitioned_pre_enqueued_calls(gpu, lo, n):
    """Runs of equal host calls (n <= 256) go through the pre-enqueued emit
    (k_pc_emit_gated: the next call's emit waits in the stream for a go
    word); a call of another length, a ConvolutionReverb wet/dry change and
    Reset cancel it and roll the bookkeeping back.  Every output against the
    oracle (partitioned.go:348-396, convolution.go:60-85)."""
    h = irlib.large_church()[0, :30000].copy()
    g = conv.NewPartitionedConvolution(h, lo, 13)
    o = O.Partitioned(h, lo, 13)
    x = signals.white_noise(200_000, 77 + lo)
    plan = [n] * 40 + [n - 1] + [n] * 30 + ["reset"] + [n] * 25 + [3 * n] + [n] * 10
    pos, got, want = 0, [], []
    for m in plan:
        if m == "reset":
            g.Reset()
            o = O.Partitioned(h, lo, 13)
            continue
        blk = x[pos:pos + m]
        out = np.empty(m)
        g.ProcessBlock(blk, out)
        got.append(out)
        want.append(o.process_block(blk))
        pos += m
    got, want = np.concatenate(got), np.concatenate(want)
    assert rms(got, want) < FFT_RMS_TOL
    assert np.max(np.abs(got - want)) < 1e-9


def test_partitioned_gate_after_pause(gpu):
    """a caller that pauses longer than the pre-enqueued emit's
    timeout (4 call intervals, at least 1 ms) between two equal calls gets the
    timed-out emit rolled back and an ordinary call, with correct outputs;
    after three timeouts in a row pre-enqueueing stops, and it resumes once
    calls come back to back again."""
    import time

    h = irlib.large_church()[0, :30000].copy()
    g = conv.NewPartitionedConvolution(h, 7, 13)
    o = O.Partitioned(h, 7, 13)
    x = signals.white_noise(200_000, 91)
    plan = [128] * 20 + ["sleep"] + [128] * 3 + ["sleep", 128, "sleep", 128, "sleep", 128, "sleep"] + [128] * 40
    pos, got, want = 0, [], []
    for m in plan:
        if m == "sleep":
            time.sleep(0.03)  # > 20 ms, the longest timeout
            continue
        blk = x[pos:pos + m]
        out = np.empty(m)
        g.ProcessBlock(blk, out)
        got.append(out)
        want.append(o.process_block(blk))
        pos += m
    got, want = np.concatenate(got), np.concatenate(want)
    assert rms(got, want) < FFT_RMS_TOL
    assert np.max(np.abs(got - want)) < 1e-9
    hits, timeouts = g.LowLatencyStats()
    assert timeouts >= 1, (hits, timeouts)
    assert hits >= 30, (hits, timeouts)  # resumed after the pauses


def test_partitioned_two_handles_alternating(gpu):
    """two low-latency handles called alternately.  Only one
    pre-enqueued emit may wait at a time (the process-wide slot), and a call
    aborts the other handle's armed emit before it enqueues anything
    (gate_preempt), so neither handle's call queues behind the other's waiting
    emit whichever hardware queues their streams share (streams created
    earlier in the process, torch's included, shift that mapping): no call
    takes as long as a timeout, and both outputs match the oracle."""
    import time

    h = irlib.large_church()[0, :30000].copy()
    gs = [conv.NewPartitionedConvolution(h, 7, 13) for _ in range(2)]
    os_ = [O.Partitioned(h, 7, 13) for _ in range(2)]
    xs = [signals.white_noise(64 * 128, 95 + i) for i in range(2)]
    got = [[], []]
    lat = []
    for b in range(64):
        for i in range(2):
            blk = xs[i][b * 128:(b + 1) * 128]
            out = np.empty(128)
            t0 = time.perf_counter()
            gs[i].ProcessBlock(blk, out)
            lat.append(time.perf_counter() - t0)
            got[i].append(out)
    for i in range(2):
        a = np.concatenate(got[i])
        w = np.concatenate([os_[i].process_block(xs[i][b * 128:(b + 1) * 128]) for b in range(64)])
        assert rms(a, w) < FFT_RMS_TOL
        assert np.max(np.abs(a - w)) < 1e-9
    lat = np.sort(np.array(lat[8:]))
    # no call waits out another handle's 20-ms emit timeout
    assert lat[-1] < 0.010 and lat[int(0.95 * lat.size)] < 0.002, lat[-10:]


def test_partitioned_dirac(gpu):
    c = KATS["partitioned_dirac"]
    x = signals.white_noise(c["signal_len"], 3)
    g = conv.NewPartitionedConvolution(c["kernel"], c["min_order"], c["max_order"])
    lat = 1 << c["min_order"]
    xin = np.concatenate([x, np.zeros(lat)])
    out = np.empty(xin.size)
    g.ProcessBlock(xin, out)
    np.testing.assert_allclose(out[lat:], x, atol=c["tol"])
    g.Reset()
    out2 = np.empty(xin.size)
    g.ProcessBlock(xin, out2)
    np.testing.assert_allclose(out2, out, atol=1e-14)


# ---------------------------------------------------- multi-channel engine
def _multi_run(kernels, x, hop=4096, chunk=0, ir_index=None, out_len=None):
    import torch

    C_, n = x.shape
    K = kernels.shape[1]
    out_len = out_len or n + K - 1
    eng = conv.MultiChannelConvolver(kernels, hop=hop, channels=C_, ir_index=ir_index, chunk_blocks=chunk)
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros((C_, out_len), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.process_device(dx.data_ptr(), n, n, dy.data_ptr(), out_len, out_len)
    torch.cuda.synchronize()
    return dy.cpu().numpy(), eng


def test_multi_stereo_large_church_vs_oracle(gpu):
    """Config 3 shape (stereo x 131072-tap Large Church) at an oracle-sized length."""
    ir = irlib.large_church()
    n = 1 << 16
    x = np.stack([signals.white_noise(n, 0x5EED + c) for c in range(2)])
    y, _ = _multi_run(ir, x, chunk=7)
    for c in range(2):
        want = O.OverlapSave(ir[c], 0).process(x[c])
        assert rms(y[c], want) < FFT_RMS_TOL
        assert np.max(np.abs(y[c] - want)) < 1e-9


@pytest.mark.parametrize("hop", [64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_multi_hops_and_ir_map(gpu, hop):
    K = 3000
    irs = np.stack([signals.make_test_kernel(K), signals.white_noise(K, 7), signals.make_impulse_kernel(K)])
    C_ = 5
    n = 20000
    x = np.stack([signals.white_noise(n, c) for c in range(C_)])
    ir_index = [2, 0, 1, 1, 0]
    y, _ = _multi_run(irs, x, hop=hop, chunk=3, ir_index=ir_index)
    for c in range(C_):
        want = O.direct_ld(x[c], irs[ir_index[c]])
        assert rms(y[c], want) < 1e-10


def test_multi_full_size_spot_check(gpu):
    """Full config-3 length (2 x 2^24): size-independent check of random output
    samples against exact dot products (y[t] = sum_k h[k] x[t-k])."""
    ir = irlib.large_church()
    n = 1 << 24
    x = np.stack([signals.white_noise(n, 0x5EED + c) for c in range(2)])
    y, _ = _multi_run(ir, x, out_len=n)
    rng = np.random.default_rng(1)
    K = ir.shape[1]
    for c in range(2):
        ts = np.concatenate([[0, 1, K - 2, K - 1, K, n - 1], rng.integers(0, n, 40)])
        hr = ir[c][::-1]
        for t in ts:
            lo = max(0, t - K + 1)
            seg = x[c][lo:t + 1]
            ref = float(np.dot(hr[K - seg.size:], seg))
            assert abs(y[c][t] - ref) < 1e-9, (c, t, y[c][t], ref)


def test_mixdown(gpu):
    import torch

    x = torch.from_numpy(np.stack([signals.white_noise(1000, c) for c in range(6)])).cuda()
    mix = torch.zeros((2, 1000), dtype=torch.float64, device="cuda")
    conv.mixdown_device(x.data_ptr(), 6, 1000, 1000, mix.data_ptr())
    torch.cuda.synchronize()
    xn = x.cpu().numpy()
    np.testing.assert_allclose(mix.cpu().numpy()[0], xn[0] + xn[2] + xn[4], atol=1e-15)
    np.testing.assert_allclose(mix.cpu().numpy()[1], xn[1] + xn[3] + xn[5], atol=1e-15)
    # explicit mix stride + segment offset + odd first global channel
    mix2 = torch.zeros((2, 1500), dtype=torch.float64, device="cuda")
    conv.mixdown_device(x.data_ptr() + 8 * 300, 5, 1000, 600, mix2.data_ptr() + 8 * 300, mix_stride=1500,
                        first_parity=1)
    torch.cuda.synchronize()
    m2 = mix2.cpu().numpy()
    np.testing.assert_allclose(m2[1, 300:900], (xn[0] + xn[2] + xn[4])[300:900], atol=1e-15)
    np.testing.assert_allclose(m2[0, 300:900], (xn[1] + xn[3])[300:900], atol=1e-15)
    assert not m2[:, :300].any() and not m2[:, 900:].any()


# ------------------------------------------- the exact instance bench.py times
def _exact_window(x, h, t0, w):
    """y[t0 .. t0+w) of the full linear convolution by direct float64 dot
    products (np.convolve 'valid' over the window's input span)."""
    K = h.size
    lo = t0 - K + 1
    seg = x[max(lo, 0):t0 + w]
    if lo < 0:
        seg = np.concatenate([np.zeros(-lo), seg])
    if seg.size < w + K - 1:
        seg = np.concatenate([seg, np.zeros(w + K - 1 - seg.size)])
    return np.convolve(seg, h, mode="valid")


# test_bench_instance_vs_oracle and the config-4 shard test live in
# test_configs_gpu.py (test_config3_bench_instance, test_config4_shard).


@pytest.mark.parametrize("hop,nseg", [(1024, 3), (8192, 4)])
def test_multi_segments_equal_one_call(gpu, hop, nseg):
    """ad_conv_multi_process_device_segment: consecutive output segments of one
    signal reproduce the single-call result bit for bit (the delay line carries
    over), and out-of-order segments are rejected."""
    import torch

    ir = irlib.large_church()[:, :40000]
    n = 100_000
    x = np.stack([signals.white_noise(n, 0x5EED + c) for c in range(2)])
    want, _ = _multi_run(ir, x, hop=hop, chunk=5)
    out_len = n + ir.shape[1] - 1
    eng = conv.MultiChannelConvolver(ir, hop=hop, channels=2, chunk_blocks=5)
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros((2, out_len), dtype=torch.float64, device="cuda")
    blocks = -(-out_len // hop)
    cuts = [min(out_len, hop * (blocks * i // nseg)) for i in range(nseg + 1)]
    for _ in range(2):  # a second pass restarts at out_begin = 0
        for b, e in zip(cuts[:-1], cuts[1:]):
            eng.process_device_segment(dx.data_ptr(), n, n, dy.data_ptr(), out_len, out_len, b, e)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dy.cpu().numpy(), want)
    eng.process_device_segment(dx.data_ptr(), n, n, dy.data_ptr(), out_len, out_len, 0, cuts[1])
    with pytest.raises(Exception):
        eng.process_device_segment(dx.data_ptr(), n, n, dy.data_ptr(), out_len, out_len, cuts[2], cuts[3])
    with pytest.raises(Exception):
        eng.process_device_segment(dx.data_ptr(), n, n, dy.data_ptr(), out_len, out_len, 1, cuts[1])


@pytest.mark.parametrize("hop,C,parity,nseg", [(8192, 8, 0, 1), (8192, 3, 1, 1), (4096, 1, 0, 1), (2048, 5, 1, 3),
                                                (1024, 4, 0, 2)])
def test_multi_mix_fused(gpu, hop, C, parity, nseg):
    """ad_conv_multi_process_device_mix (the stereo mixdown fused into K3,
    VERDICT r3): the mix of C channels (IR[c mod 2], first global parity
    `parity`) against per-channel outputs + k_mixdown (to rounding: each block
    enters the sum as (acc + A) - W B, and the fused kernel's transforms run
    at 16 values per thread where K3's run at 8) and against the oracle's per-channel OverlapSave sums (<= 1e-7
    RMS per channel summed); segments, a short out_len, odd channel counts
    (a side with no channel is all zeros), hop 1024 (the scratch + k_mixdown
    path) and the per-channel outputs untouched."""
    import torch

    ir = irlib.large_church()[:, :30000]
    K = ir.shape[1]
    n = 70_000
    x = np.stack([signals.white_noise(n, 0x3A11 + c) for c in range(C)])
    out_len = n + K - 1 - (777 if nseg == 1 else 0)
    eng = conv.MultiChannelConvolver(ir, hop=hop, channels=C, ir_index=[c % 2 for c in range(C)], chunk_blocks=7)
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros((C, out_len), dtype=torch.float64, device="cuda")
    ref = torch.full((2, out_len), np.nan, dtype=torch.float64, device="cuda")
    eng.process_device(dx.data_ptr(), n, n, dy.data_ptr(), out_len, out_len)
    conv.mixdown_device(dy.data_ptr(), C, out_len, out_len, ref.data_ptr(), first_parity=parity)
    mix = torch.full((2, out_len + 5), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dy.fill_(7.0)
    blocks = -(-out_len // hop)
    cuts = [min(out_len, hop * (blocks * i // nseg)) for i in range(nseg + 1)]
    for b, e in zip(cuts[:-1], cuts[1:]):
        eng.process_device_mix(dx.data_ptr(), n, n, mix.data_ptr(), out_len + 5, out_len, parity, b, e)
    torch.cuda.synchronize()
    m, r = mix.cpu().numpy()[:, :out_len], ref.cpu().numpy()
    assert np.isnan(mix.cpu().numpy()[:, out_len:]).all()
    assert (dy.cpu().numpy() == 7.0).all()
    for side in range(2):
        chans = [c for c in range(C) if (parity + c) % 2 == side]
        if not chans:
            assert not m[side].any()
            continue
        scale = max(1.0, float(np.max(np.abs(r[side]))))
        assert np.max(np.abs(m[side] - r[side])) <= 1e-13 * scale, float(np.max(np.abs(m[side] - r[side])))
        want = np.zeros(out_len)
        for c in chans:
            want += O.OverlapSave(ir[c % 2], 0).process(x[c])[:out_len]
        assert rms(m[side], want) < FFT_RMS_TOL * len(chans)


def test_comm_mixdown_reduce_world1(gpu):
    """ad_comm_* / ad_mixdown_reduce (the C-ABI RCCL mixdown) at
    world size 1: the reduce to root 0 leaves k_mixdown's partial mix, both for
    a contiguous [2][len] mix (one reduce) and a strided segment (two grouped
    reduces), and a stereo group reduces its output rows in place."""
    import torch

    from algodsp import shard

    comm = shard.Comm(0, 1, 0)
    x = torch.from_numpy(np.stack([signals.white_noise(3000, c) for c in range(8)])).cuda()
    xn = x.cpu().numpy()
    mix = torch.full((2, 3000), np.nan, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    comm.mixdown_reduce(x.data_ptr(), 8, 3000, 3000, mix.data_ptr(), 3000, 0, 0, s.cuda_stream)
    s.synchronize()
    m = mix.cpu().numpy()
    np.testing.assert_allclose(m[0], xn[0::2].sum(0), atol=1e-14)
    np.testing.assert_allclose(m[1], xn[1::2].sum(0), atol=1e-14)
    seg = torch.zeros((2, 3000), dtype=torch.float64, device="cuda")
    comm.mixdown_reduce(x.data_ptr() + 8 * 1000, 3, 3000, 500, seg.data_ptr() + 8 * 1000, 3000, 1, 0, s.cuda_stream)
    s.synchronize()
    sg = seg.cpu().numpy()
    np.testing.assert_allclose(sg[1, 1000:1500], (xn[0] + xn[2])[1000:1500], atol=1e-14)
    np.testing.assert_allclose(sg[0, 1000:1500], xn[1][1000:1500], atol=1e-14)
    assert not sg[:, :1000].any() and not sg[:, 1500:].any()
    st = x[:2].clone()
    comm.mixdown_reduce(0, 0, 3000, 3000, st.data_ptr(), 3000, 0, 0, s.cuda_stream)
    s.synchronize()
    np.testing.assert_array_equal(st.cpu().numpy(), xn[:2])
    with pytest.raises(conv.ADError):
        comm.mixdown_reduce(x.data_ptr(), 8, 3000, 3000, mix.data_ptr(), 3000, 0, 1, s.cuda_stream)  # root >= world
    comm.close()


# ------------------------------------------------- host-buffer multichannel
def test_process_host_multi_chunked(gpu):
    """ad_conv_ols_process_multi (host buffers, chunked PCIe pipeline): several
    16 MiB chunks per call, bit-identical to the device-resident call and
    within the FFT tolerance of the oracle's OverlapSave.Process."""
    ir = irlib.large_church()
    K = ir.shape[1]
    n = 2_500_000  # > 2 chunks of 2^20 samples per channel at 2 channels
    x = np.stack([signals.white_noise(n, 0x5EED + c) for c in range(2)])
    eng = conv.MultiChannelConvolver(ir, hop=8192, channels=2)
    got = eng.process_host(x)
    assert got.shape == (2, n + K - 1)
    dev, _ = _multi_run(ir, x, hop=8192)
    np.testing.assert_array_equal(got, dev)
    want = O.OverlapSave(ir[1], 0).process(x[1])
    assert rms(got[1], want) < FFT_RMS_TOL and np.max(np.abs(got[1] - want)) < 1e-9
    reg_ms, xfer_ms, unreg_ms = eng.host_io_profile()
    assert reg_ms > 0 and xfer_ms > 0 and unreg_ms >= 0  # 2 x 2.6 M samples > 64 MiB: registered
    # every host I/O form gives the same bits (ad_conv_set_host_io)
    for mode, workers in [(conv.MultiChannelConvolver.HOST_IO_STAGE, 1), (conv.MultiChannelConvolver.HOST_IO_STAGE, 8),
                          (conv.MultiChannelConvolver.HOST_IO_REGISTER, 0)]:
        eng.set_host_io(mode, workers)
        np.testing.assert_array_equal(eng.process_host(x), dev)
        r, t, _ = eng.host_io_profile()
        assert (r > 0) == (mode == conv.MultiChannelConvolver.HOST_IO_REGISTER) and t > 0
    eng.set_host_io(conv.MultiChannelConvolver.HOST_IO_AUTO)
    with pytest.raises(conv.ErrInvalidArgument):
        eng.set_host_io(7)
    # second call on the same handle, shorter signal (one chunk)
    got2 = eng.process_host(x[:, :50_000])
    np.testing.assert_allclose(got2[0], O.OverlapSave(ir[0], 0).process(x[0, :50_000]), atol=1e-9)
    with pytest.raises(conv.ErrLengthMismatch):
        eng.process_host(x[:1, :1000])


def test_batch_process_many_chunks(gpu):
    """OverlapSave.Process on a host buffer longer than several pipeline chunks
    (C = 1: 2^21 samples per chunk) against the oracle."""
    h = irlib.large_church()[0, :16384]
    n = 5_000_000
    x = signals.white_noise(n, 11)
    got = conv.NewOverlapSave(h, 0).Process(x)
    want = O.OverlapSave(h, 0).process(x)
    assert rms(got, want) < FFT_RMS_TOL and np.max(np.abs(got - want)) < 1e-9


@pytest.mark.parametrize("K,B", [(16384, 4096), (3000, 512), (131072, 8192)])
def test_multi_stream_vs_oracle(gpu, K, B):
    """ad_conv_multi_stream_*: 5 channels x n_ir kernels, block by block, host
    and device calls interleaved, Reset; each channel against the oracle's
    StreamingOverlapSave (streaming_overlap_save.go:100-164)."""
    import torch

    irs = np.stack([signals.make_test_kernel(K), irlib.large_church()[1, :K]])
    ir_index = [1, 0, 0, 1, 1]
    C_, nb = 5, 5
    x = np.stack([signals.white_noise(B * nb, 70 + c) for c in range(C_)])
    s = conv.MultiChannelStreamingConvolver(irs, B, C_, ir_index=ir_index)
    assert s.BlockSize() == B and s.FFTSize() == O.Streaming(irs[0], B).fft_size()
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros_like(dx)
    for rep in range(2):
        got = np.empty_like(x)
        for i in range(nb):
            if i % 2:
                st = torch.cuda.current_stream()
                s.process_block_device(dx.data_ptr() + 8 * i * B, B * nb, dy.data_ptr() + 8 * i * B, B * nb,
                                       st.cuda_stream)
                st.synchronize()
                got[:, i * B:(i + 1) * B] = dy.cpu().numpy()[:, i * B:(i + 1) * B]
            else:
                got[:, i * B:(i + 1) * B] = s.ProcessBlock(x[:, i * B:(i + 1) * B])
        for c in range(C_):
            o = O.Streaming(irs[ir_index[c]], B)
            want = np.concatenate([o.process_block(x[c, i * B:(i + 1) * B]) for i in range(nb)])
            assert rms(got[c], want) < FFT_RMS_TOL and np.max(np.abs(got[c] - want)) < 1e-9
        s.Reset()
    with pytest.raises(conv.ErrLengthMismatch):
        s.ProcessBlock(x[:, :B - 1])
    with pytest.raises(conv.ErrLengthMismatch):
        s.ProcessBlock(x[:4, :B])


@pytest.mark.parametrize("C_,K,B", [(64, 131072, 480), (64, 131072, 960), (8, 131072, 1000), (64, 131072, 4800),
                                    (5, 16384, 100), (3, 3000, 33), (4, 20000, 12000)])
def test_multi_stream_any_block_size(gpu, C_, K, B):
    """ad_conv_multi_stream_* takes any block size, as the
    reference's NewStreamingOverlapSave does (streaming_overlap_save.go:45-58):
    blocks that are not a whole number of hops carry the unfinished block
    between calls at hop = nextPow2(B) (>= K/64), so none runs below hop 256
    on a long IR.  64 channels x the 131072-tap Large Church IR[c mod 2] at
    B = 480 / 960 / 4800 (config 4's real-time form at 48 kHz block sizes),
    odd sizes and B > hop; host and device calls interleaved, then Reset;
    every channel against the oracle's StreamingOverlapSave."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    irs = irlib.large_church()[:, :K]
    ir_index = [c % 2 for c in range(C_)]
    nb = 5
    x = np.stack([signals.white_noise(B * nb, 170 + c) for c in range(C_)])
    s = conv.MultiChannelStreamingConvolver(irs, B, C_, ir_index=ir_index)
    assert s.BlockSize() == B and s.FFTSize() == O.Streaming(irs[0], B).fft_size()
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros_like(dx)

    def want_of(c):
        o = O.Streaming(irs[ir_index[c]], B)
        return np.concatenate([o.process_block(x[c, i * B:(i + 1) * B]) for i in range(nb)])

    chans = list(range(C_)) if C_ <= 8 else [0, 1, 2, 31, 62, 63]
    with ThreadPoolExecutor(8) as ex:
        want = dict(zip(chans, ex.map(want_of, chans)))
    for rep in range(2):
        got = np.empty_like(x)
        for i in range(nb):
            if i % 2:
                st = torch.cuda.current_stream()
                s.process_block_device(dx.data_ptr() + 8 * i * B, B * nb, dy.data_ptr() + 8 * i * B, B * nb,
                                       st.cuda_stream)
                st.synchronize()
                got[:, i * B:(i + 1) * B] = dy.cpu().numpy()[:, i * B:(i + 1) * B]
            else:
                got[:, i * B:(i + 1) * B] = s.ProcessBlock(np.ascontiguousarray(x[:, i * B:(i + 1) * B]))
        for c in chans:
            assert rms(got[c], want[c]) < FFT_RMS_TOL and np.max(np.abs(got[c] - want[c])) < 1e-9, (rep, c)
        s.Reset()


@pytest.mark.parametrize("K,B", [(131072, 4096), (16384, 8192), (3000, 1024), (40000, 2048)])
def test_stream_blocks_bit_identical_to_offline(gpu, K, B):
    """A streaming call (one output block per channel: K2's single-row form,
    k_fdl_mac_row, all partitions in one launch) gives bit for bit what the
    offline engine at the same hop gives (the run-based K2, one launch per
    chunk of 16 partitions with a Z read-modify-write when P > 16): the same
    products in the same order.  P = 32, 2, 3 and 20."""
    irs = irlib.large_church()[:, :K]
    ir_index = [0, 1, 0]
    C_, nb = 3, 6
    n = nb * B
    x = np.stack([signals.white_noise(n, 90 + c) for c in range(C_)])
    s = conv.MultiChannelStreamingConvolver(irs, B, C_, ir_index=ir_index)
    got = np.concatenate([s.ProcessBlock(x[:, i * B:(i + 1) * B]) for i in range(nb)], axis=1)
    want, _ = _multi_run(irs, x, hop=B, ir_index=ir_index)
    assert np.array_equal(got, want[:, :n])


@pytest.mark.parametrize("K,lo,hi", [(95432, 7, 13), (1000, 6, 13), (20000, 10, 11), (5000, 13, 13)])
def test_partitioned_multi_vs_oracle(gpu, K, lo, hi):
    """ad_conv_pc_multi_* (many-channel, device-resident partitioned engine):
    3 channels sharing one IR, device calls of varying length (shorter and
    longer than every stage, > one accumulator span), each channel against the
    oracle's PartitionedConvolution; Reset restarts the stream; the reverb form
    mixes dry/wet in place."""
    import torch

    h = signals.make_impulse_kernel(K) if K < 90000 else irlib.large_church(pad_to=None)[0]
    C_ = 3
    lat = 1 << lo
    sizes = [lat, 1, 3 * lat + 5, 20011, 7, 40000, lat]
    n = sum(sizes)
    x = np.stack([signals.white_noise(n, 300 + c) for c in range(C_)])
    g = conv.PartitionedConvolutionMulti(h, lo, hi, C_)
    assert g.Latency() == lat and g.StageCount() == O.Partitioned(h, lo, hi).stage_count()
    dx = torch.from_numpy(x).cuda()
    dy = torch.full_like(dx, np.nan)
    s = torch.cuda.current_stream()
    for rep in range(2):
        pos = 0
        for m in sizes:
            g.process_device(dx.data_ptr() + 8 * pos, n, dy.data_ptr() + 8 * pos, n, m, s.cuda_stream)
            pos += m
        s.synchronize()
        y = dy.cpu().numpy()
        for c in range(C_):
            o = O.Partitioned(h, lo, hi)
            want = np.concatenate([o.process_block(x[c, a:a + m]) for a, m in
                                   zip(np.cumsum([0] + sizes[:-1]), sizes)])
            assert rms(y[c], want) < FFT_RMS_TOL
            assert np.max(np.abs(y[c] - want)) < 1e-9
        g.Reset()
    # reverb form: in place, dry/wet
    r = conv.NewConvolutionReverbMulti(h, lo, C_)
    r.SetWetDry(0.3, 0.8)
    blk = x[:, :5000].copy()
    r.ProcessInPlace(blk)
    for c in range(C_):
        o = O.Partitioned(h, lo, 13)
        want = 0.8 * x[c, :5000] + 0.3 * o.process_block(x[c, :5000])
        assert np.max(np.abs(blk[c] - want)) < 1e-9


# ------------------------------------------------------------ float32 handles
F32_TOL = 1e-4  # the reference's float32 tolerance (streaming_test.go:175-234)


@pytest.mark.parametrize("ola", [False, True])
@pytest.mark.parametrize("K,B,nb", [(5, 16, 8), (3, 8, 2), (16384, 4096, 4), (1000, 512, 6)])
def test_streaming32_vs_oracle(gpu, ola, K, B, nb):
    """NewStreamingOverlapSave32 / NewStreamingOverlapAdd32: float32 blocks in
    and out against the float32 (complex64) oracle at the reference's 1e-4,
    and against the float64 oracle rounded to float32 (one rounding)."""
    h = signals.make_test_kernel(K).astype(np.float32)
    x = signals.white_noise(B * nb, K + 3).astype(np.float32)
    ctor = conv.NewStreamingOverlapAdd32 if ola else conv.NewStreamingOverlapSave32
    g = ctor(h, B)
    o32 = O.Streaming32(h, B, ola=ola)
    o64 = O.Streaming(h.astype(np.float64), B, ola=ola)
    assert g.FFTSize() == o32.fft_size() and g.BlockSize() == B
    for i in range(nb):
        blk = x[i * B:(i + 1) * B]
        got = g.ProcessBlock(blk)
        assert got.dtype == np.float32
        scale = max(1.0, float(np.max(np.abs(got))))
        assert np.max(np.abs(got.astype(np.float64) - o32.process_block(blk))) <= F32_TOL * scale
        w64 = o64.process_block(blk.astype(np.float64))
        assert np.max(np.abs(got - w64.astype(np.float32))) <= 4 * np.finfo(np.float32).eps * scale
    with pytest.raises(conv.ErrLengthMismatch):
        g.ProcessBlock(x[:B - 1])


@pytest.mark.parametrize("K,lo,hi", [(1000, 6, 9), (95432, 7, 13), (3, 2, 5)])
def test_partitioned32_vs_oracle(gpu, K, lo, hi):
    """NewPartitionedConvolution32 against the float32 oracle (1e-4) and the
    float64 oracle, calls of varying length; latency and stage layout."""
    h = (signals.make_impulse_kernel(K) if K < 90000 else irlib.large_church(pad_to=None)[1]).astype(np.float32)
    lat = 1 << lo
    g = conv.NewPartitionedConvolution32(h, lo, hi)
    o32 = O.Partitioned32(h, lo, hi)
    o64 = O.Partitioned(h.astype(np.float64), lo, hi)
    assert g.Latency() == lat and g.StageCount() == o64.stage_count()
    x = signals.white_noise(20000, 9).astype(np.float32)
    pos = 0
    for m in [lat, 3, 5 * lat + 1, 4000, 1, 20000]:
        m = min(m, x.size - pos)
        if m <= 0:
            break
        blk = x[pos:pos + m]
        out = np.empty(m, dtype=np.float32)
        g.ProcessBlock(blk, out)
        w32 = o32.process_block(blk)
        w64 = o64.process_block(blk.astype(np.float64))
        scale = max(1.0, float(np.max(np.abs(w64))) if m else 1.0)
        assert np.max(np.abs(out.astype(np.float64) - w32)) <= F32_TOL * scale
        assert np.max(np.abs(out - w64.astype(np.float32))) <= 4 * np.finfo(np.float32).eps * scale
        pos += m
