"""The long-block overlap-save plan on the GPU (conv_long_kernels.hip), forced
ON on the bench's own instantiation (hop 8192, whole-signal device call).

Bound: max |got - exact| <= GAMMA err_scale with GAMMA = 8 gamma_ref of the
numpy model (conv_long_model.py, measured by test_conv_long_model.py).  Where
no conv_exact reference exists (noise through the Large Church IR) the
reference is dot-product windows computed in long double (64-bit mantissa:
their own rounding is 2^-11 of the float64 roundings judged here) at t = 0,
K - 64, every block seam +- 32, n - 40 and out_len - 64, held to the same
GAMMA err_scale.  The whole output is also compared with the numpy model at
GAMMA err_scale: an extra check of the samples between the windows against a
restatement of the same algorithm, not a reference.  Every case also passes
the contract's 1e-7 RMS and 1e-9 max abs.
"""
import numpy as np
import pytest

import conv_exact as E
import conv_long_model as LM
from algodsp import conv, irlib, signals
from test_conv_gpu import rms

pytestmark = pytest.mark.gpu

GUARD = 5  # cells after each output row that no kernel may touch


def _run(eng, x, out_len, in_pad=0, out_stride=None):
    """process_device into a NaN-prefilled buffer with guard cells: every
    output written, no guard touched.  x: [C][n]."""
    import torch

    C_, n = x.shape
    out_stride = out_len + GUARD if out_stride is None else out_stride
    assert out_stride >= out_len + 1
    xin = np.full((C_, n + in_pad), np.nan)
    xin[:, :n] = x
    dx = torch.from_numpy(xin).cuda()
    dy = torch.full((C_ * out_stride + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.process_device(dx.data_ptr(), n + in_pad, n, dy.data_ptr(), out_stride, out_len)
    torch.cuda.synchronize()
    flat = dy.cpu().numpy()
    rows = flat[: C_ * out_stride].reshape(C_, out_stride)
    assert not np.isnan(rows[:, :out_len]).any(), "an output was not written"
    assert np.isnan(rows[:, out_len:]).all() and np.isnan(flat[C_ * out_stride:]).all(), "a guard cell was touched"
    return rows[:, :out_len].copy()


def _engine(ir, channels, ir_index=None, mode=conv.MultiChannelConvolver.LONG_ON):
    eng = conv.MultiChannelConvolver(ir, hop=8192, channels=channels, ir_index=ir_index)
    eng.set_long_blocks(mode)
    assert eng.long_blocks() == mode
    return eng


def _contract(got, want):
    assert rms(got, want) < 1e-7
    assert np.max(np.abs(got - want)) < 1e-9


def _check_exact(got, case):
    scale = LM.scale_of(case)
    err = float(np.max(np.abs(got - case.exact)))
    print(f"{case.family}: err {err:.3e} = {err / scale:.3f} err_scale (bound {LM.GAMMA})")
    assert err <= LM.GAMMA * scale
    _contract(got, case.exact)


def _window_ld(x, h, t0, w):
    """y[t0 .. t0+w) of the full linear convolution: dot products accumulated
    in long double, rounded once to float64."""
    assert np.finfo(np.longdouble).nmant >= 63, "long double is not wider than float64 here"
    K = h.size
    lo = t0 - K + 1
    seg = np.zeros(w + K - 1, dtype=np.longdouble)
    a, b = max(lo, 0), min(t0 + w, x.size)
    if b > a:
        seg[a - lo: b - lo] = x[a:b]
    return np.convolve(seg, h.astype(np.longdouble), mode="valid").astype(np.float64)


def _check_noise(got, x, h, seams=True):
    """Noise through a dense float kernel: long-double windows at the ends and
    seams (the reference), the model over the whole output (an extra check)."""
    K, n, out_len = h.size, x.size, got.size
    model = LM.long_numpy(x, h, out_len)
    scale = LM.err_scale_long(x, h, E.peak_of(model), out_len)
    hop = LM.hop_long(K)
    t0s = [0, K - 64, n - 40, out_len - 64]
    if seams:
        t0s += [j * hop - 32 for j in range(1, -(-out_len // hop))]
    worst = 0.0
    for t0 in t0s:
        t0 = min(max(t0, 0), out_len - 64)
        ref = _window_ld(x, h, t0, 64)
        werr = float(np.max(np.abs(got[t0:t0 + 64] - ref)))
        worst = max(worst, werr)
        assert werr <= LM.GAMMA * scale, (t0, werr / scale)
        assert werr < 1e-9
    err = float(np.max(np.abs(got - model)))
    print(f"noise: windows {worst:.3e} = {worst / scale:.3f} err_scale, vs model {err:.3e} = {err / scale:.3f} "
          f"err_scale (bound {LM.GAMMA})")
    assert err <= LM.GAMMA * scale
    _contract(got, model)


def _church():
    return irlib.large_church()


def test_single_partial_block(gpu):
    """n shorter than one block; C = 3 with ir_index [0, 1, 0], in_stride > n,
    odd out_stride."""
    ir = _church()
    n = 70001
    out_len = n + ir.shape[1] - 1
    x = np.stack([signals.white_noise(n, 0x10 + c) for c in range(3)])
    eng = _engine(ir, 3, [0, 1, 0])
    y = _run(eng, x, out_len, in_pad=13, out_stride=out_len + GUARD + (out_len + GUARD + 1) % 2)
    for c, r in enumerate([0, 1, 0]):
        _check_noise(y[c], x[c], ir[r], seams=False)
    assert eng.schedule() == (0, 0)


@pytest.mark.parametrize("name,parity", [("sparse-K=100003", 0), ("sparse-input-K=131072", 1), ("impulse-K=N/4", 0)])
def test_three_hops_exact(gpu, name, parity):
    """out_len = 3 hop - 1, 3 hop, 3 hop + 1 (the last a fourth block of one
    sample) on exact references; K off every UPOLS hop and K = N/4; even and
    odd out_stride."""
    case = LM.exact_cases()[name]
    out_len = case.exact.size
    stride = out_len + GUARD
    stride += (stride + parity) % 2
    eng = _engine(case.h[None, :], 1)
    y = _run(eng, case.x[None, :], out_len, out_stride=stride)
    _check_exact(y[0], case)


def test_stereo_church_seams_and_second_signal(gpu):
    """Stereo noise through the Large Church IR over three blocks (windows at
    every seam), then a shorter signal on the same handle, then a segmented
    call on the same handle, which equals a fresh handle's bit for bit."""
    import torch

    ir = _church()
    K = ir.shape[1]
    hop = LM.hop_long(K)
    out_len = 2 * hop + 4097
    n = out_len - K + 1
    x = np.stack([signals.white_noise(n, 0x20 + c) for c in range(2)])
    eng = _engine(ir, 2)
    y = _run(eng, x, out_len)
    _check_noise(y[0], x[0], ir[0])
    _check_noise(y[1], x[1], ir[1], seams=False)
    n2 = 50000
    y2 = _run(eng, x[:, :n2], n2 + K - 1, in_pad=3)
    _check_noise(y2[1], x[1, :n2], ir[1], seams=False)
    # the long calls left the partitioned engine's state as a fresh handle's
    n3 = 3 * 8192 + 11
    ol3 = n3 + K - 1
    outs = []
    for e in (eng, conv.MultiChannelConvolver(ir, hop=8192, channels=2)):
        dx = torch.from_numpy(x[:, :n3].copy()).cuda()
        dy = torch.zeros((2, ol3), dtype=torch.float64, device="cuda")
        cut = 5 * 8192
        e.process_device_segment(dx.data_ptr(), n3, n3, dy.data_ptr(), ol3, ol3, 0, cut)
        e.process_device_segment(dx.data_ptr(), n3, n3, dy.data_ptr(), ol3, ol3, cut, ol3)
        torch.cuda.synchronize()
        outs.append(dy.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


def test_auto_selection(gpu):
    """AUTO = OFF bit for bit below kLongMinBlocks hops, = ON from there on;
    the reported schedule stays serial."""
    ir = _church()[:1]
    K = ir.shape[1]
    thr = LM.MIN_BLOCKS * LM.hop_long(K)
    M = conv.MultiChannelConvolver
    for out_len, same, other in [(thr - 1, M.LONG_OFF, M.LONG_ON), (thr, M.LONG_ON, M.LONG_OFF)]:
        n = out_len - K + 1
        x = signals.white_noise(n, 0x30)[None, :]
        got = {}
        for mode in (M.LONG_AUTO, M.LONG_OFF, M.LONG_ON):
            eng = _engine(ir, 1, mode=mode)
            got[mode] = _run(eng, x, out_len)
            assert eng.schedule() == (0, 0)
        assert np.array_equal(got[M.LONG_AUTO], got[same])
        assert not np.array_equal(got[M.LONG_AUTO], got[other])
        _contract(got[M.LONG_ON], got[M.LONG_OFF])
