"""The device-buffer layout contract of include/algodsp.h ("Device buffers"):
every *_device entry point at base alignments and row strides the rest of the
suite never uses, on buffers whose every non-payload element is a guard
(layout_lib).  Each case computes the result at the reference placement (every
row 16-byte aligned, LA), anchors it once to the oracle at the bar the existing
test of that entry point uses, then repeats the same handle configuration at
the other placements and asserts: the result has the same bits, no guard
element changed (padding between rows, before the base, after the last row),
and the input kept its bits.  Shapes are the smallest that reach each kernel
path; nothing here can write outside memory the test owns unless a kernel
overruns a row by more than 16384 elements.
"""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import layout_lib as LL
import oracle_lib as O
from algodsp import conv, design, effectchain as E, irlib, processors as P, signals
from algodsp._lib import check, lib
from test_conv_gpu import FFT_RMS_TOL, rms
from test_dsp_gpu import RMS_TOL
from test_fxgraph import BRANCHED, FS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def sync():
    import torch

    torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    """Bit equality (np.array_equal on the int64 images: NaNs and signed zeros count)."""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def pairs(n_in, n_out):
    """(input, output) placements beside the reference (LA, LA): aligned in /
    unaligned out, unaligned in / aligned out, both unaligned, alternating
    rows, wide padding; and plain contiguous where that is not LA itself."""
    ps = [(LL.LA(n_in), LL.L2(n_out)), (LL.L2(n_in), LL.LA(n_out)), (LL.L2(n_in), LL.L2(n_out)), (LL.L1, LL.L1),
          (LL.L3, LL.L3)]
    if LL.LA(n_in) != LL.L0 or LL.LA(n_out) != LL.L0:
        ps.append((LL.L0, LL.L0))
    return ps


# --------------------------------------------------------------- the many-channel engine
IR_INDEX = [1, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def _shape(hop, n, K=None, C_=3):
    """White-noise signal, two IRs and the long-double direct convolution of
    every channel (computed once per shape, shared, never modified)."""
    K = K or 2 * hop + hop // 2 + 1  # three partitions
    if K == 1:
        # two-bit taps: h*x is exact in the oracle's long double, so its
        # product rounds once to float64, as the float64 product does
        irs = np.array([[0.75], [-1.5]])
    else:
        irs = np.stack([signals.white_noise(K, 0x1B0 + i) for i in range(2)])
    x = np.stack([signals.white_noise(n, 0xA000 + c) for c in range(C_)])
    with ThreadPoolExecutor(8) as ex:
        want = np.stack(list(ex.map(lambda c: O.direct_ld(x[c], irs[IR_INDEX[c]]), range(C_))))
    for a in (irs, x, want):
        a.setflags(write=False)
    return irs, x, want


def _anchor(y, want, K):
    """test_multi_hops_and_ir_map: RMS < 1e-10 against direct_ld (its K = 3000);
    the larger K: test_multi_stereo_large_church_vs_oracle's FFT_RMS_TOL and
    max-abs < 1e-9."""
    for c in range(y.shape[0]):
        w = want[c, :y.shape[1]]
        if K <= 3000:
            assert rms(y[c], w) < 1e-10, (c, rms(y[c], w))
        else:
            assert rms(y[c], w) < FFT_RMS_TOL and np.max(np.abs(y[c] - w)) < 1e-9, (c, rms(y[c], w))


def _run_multi(eng, x, out_len, lin, lout):
    n = x.shape[1]
    i, o = LL.place(x, lin, DEV), LL.empty(x.shape[0], out_len, lout, DEV)
    sync()
    eng.process_device(i.ptr, i.stride, n, o.ptr, o.stride, out_len)
    sync()
    LL.check_unchanged(i, x)
    LL.check_guards(o)
    return LL.payload(o)


SERIAL, PIPELINED = conv.MultiChannelConvolver.SCHED_SERIAL, conv.MultiChannelConvolver.SCHED_PIPELINED


@pytest.mark.parametrize("odd", [77, 78])
@pytest.mark.parametrize("hop,sched,chunk", [(64, None, 0), (1024, None, 0), (1024, None, 2), (2048, SERIAL, 0),
                                             (2048, SERIAL, 2), (2048, PIPELINED, 0), (2048, PIPELINED, 2),
                                             (8192, None, 0)])
def test_multi_process_device(gpu, hop, sched, chunk, odd):
    """ad_conv_multi_process_device: plain (hop 64, 1024) and split (2048, 8192)
    K1 / K3, last block partial, odd and even n (the stride parity of a
    contiguous buffer), out_len full, cut at n, hop + 1, hop and 1.  chunk 2:
    the six output blocks run as three chunks (serial: max_chunk_blocks;
    pipelined: the schedule's chunk, so the ring-reuse waits run too)."""
    n = 3 * hop + odd
    irs, x, want = _shape(hop, n)
    K = irs.shape[1]
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=3, ir_index=IR_INDEX[:3],
                                     chunk_blocks=0 if sched == PIPELINED else chunk)
    if sched is not None:
        eng.set_schedule(sched, chunk if sched == PIPELINED else 0)
    for out_len in (n + K - 1, n, hop + 1, hop, 1):
        ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
        _anchor(ref, want, K)
        for lin, lout in pairs(n, out_len):
            got = _run_multi(eng, x, out_len, lin, lout)
            assert same(got, ref), (out_len, lin, lout)


def test_multi_process_device_nontemporal_k3(gpu):
    """The non-temporal K3 (k3_nt: channels x blocks of one launch >= 1024).
    Hop 2048, 64 channels, 17 blocks + 5 samples, K = 5121: the output has
    ceil((n + K - 1) / hop) = 20 blocks; under SCHED_SERIAL the engine cuts a
    call into ceil(J / jc_max) balanced chunks and jc_max (max_chunk_blocks 0 =
    auto) is at least 64, so the 20 blocks are one chunk and its K3 launch has
    64 x 20 = 1280 items.  The engine's launch profile confirms one K3 launch."""
    hop, C_ = 2048, 64
    n, K = 17 * hop + 5, 2 * hop + hop // 2 + 1
    out_len = n + K - 1
    irs = np.stack([signals.white_noise(K, 0x1B0 + i) for i in range(2)])
    x = np.stack([signals.white_noise(n, 0xB000 + c) for c in range(C_)])
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=C_)
    eng.set_schedule(eng.SCHED_SERIAL)
    eng.profile_enable(True)
    ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
    launches = eng.profile_read()["k_irfft_store"][1]
    eng.profile_enable(False)
    assert launches == 1 and C_ * -(-out_len // hop) >= 1024, launches
    with ThreadPoolExecutor(16) as ex:
        want = np.stack(list(ex.map(lambda c: O.direct_ld(x[c], irs[c % 2]), range(C_))))
    _anchor(ref, want, K)
    assert same(_run_multi(eng, x, out_len, LL.L3, LL.L3), ref)
    # the fused mix's non-temporal form (the same 1280 items), at
    # test_multi_mix_fused's bar against the summed long-double convolutions
    mixes = []
    for lin, lmix in [(LL.LA(n), LL.LA(out_len)), (LL.L3, LL.L3)]:
        i, m = LL.place(x, lin, DEV), LL.empty(2, out_len, lmix, DEV)
        sync()
        eng.process_device_mix(i.ptr, i.stride, n, m.ptr, m.stride, out_len)
        sync()
        LL.check_unchanged(i, x)
        LL.check_guards(m)
        mixes.append(LL.payload(m))
    for side in range(2):
        assert rms(mixes[0][side], np.sum(want[side::2], axis=0)) < FFT_RMS_TOL * (C_ // 2)
    assert same(mixes[1], mixes[0])


SMALL = [("1", "1"), ("1", "h"), ("h", "1"), ("h", "h-1"), ("h", "h"), ("h+1", "h+1"), ("3", "2*h+1")]


@pytest.mark.parametrize("hop", [64, 2048])
@pytest.mark.parametrize("Ks,ns", SMALL)
def test_multi_small_lengths(gpu, hop, Ks, ns):
    """in_len < hop, in_len == 1, K == 1 through the device call, full output.
    K = 1 is a scaling: bit-exact against direct_ld (taps chosen so the
    oracle's product rounds once, see _shape)."""
    K, n = eval(Ks, {"h": hop}), eval(ns, {"h": hop})
    irs, x, want = _shape(hop, n, K)
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=3, ir_index=IR_INDEX[:3])
    out_len = n + K - 1
    ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
    for c in range(3):  # print before asserting: the figures of a failure
        print(f"hop {hop} K {K} n {n} ch {c}: rms {rms(ref[c], want[c]):.3e} max {np.max(np.abs(ref[c] - want[c])):.3e}")
    if K == 1:
        assert same(ref, want)
    else:
        _anchor(ref, want, K)
    assert same(_run_multi(eng, x, out_len, LL.L3, LL.L3), ref)


@pytest.mark.parametrize("hop", [64, 2048])
def test_multi_single_tap_forms(gpu, hop):
    """A one-tap handle is a gain in every form: the segment calls, the mix
    (against ad_conv_mixdown_device over the per-channel outputs) and the host
    call give the bits of the one device call, which are direct_ld's."""
    n = 2 * hop + 5
    irs, x, want = _shape(hop, n, 1)
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=3, ir_index=IR_INDEX[:3])
    ref = _run_multi(eng, x, n, LL.LA(n), LL.LA(n))
    assert same(ref, want)
    assert same(_run_multi(eng, x, hop + 1, LL.L3, LL.L2(hop + 1)), want[:, :hop + 1])
    assert same(eng.process_host(x), want)
    i, o, m = LL.place(x, LL.L3, DEV), LL.empty(3, n, LL.L3, DEV), LL.empty(2, n, LL.L1, DEV)
    r, mr = LL.place(ref, LL.L0, DEV), LL.empty(2, n, LL.L0, DEV)
    sync()
    for b, e in [(0, hop), (hop, n)]:
        eng.process_device_segment(i.ptr, i.stride, n, o.ptr, o.stride, n, b, e)
        sync()
        LL.check_guards(o, untouched=[(e, n)])
    for b, e in [(0, 2 * hop), (2 * hop, n)]:
        eng.process_device_mix(i.ptr, i.stride, n, m.ptr, m.stride, n, 1, b, e)
        sync()
        LL.check_guards(m, untouched=[(e, n)])
    conv.mixdown_device(r.ptr, 3, r.stride, n, mr.ptr, mix_stride=mr.stride, first_parity=1)
    sync()
    LL.check_unchanged(i, x)
    assert same(LL.payload(o), want)
    assert same(LL.payload(m), LL.payload(mr))


@pytest.mark.parametrize("hop", [1024, 2048])
def test_multi_segments(gpu, hop):
    """ad_conv_multi_process_device_segment: three segments; each leaves
    everything outside [out_begin, out_end) as it was, and together they are
    the one-call result of the reference placement, bit for bit."""
    n = 3 * hop + 77
    irs, x, want = _shape(hop, n)
    K = irs.shape[1]
    out_len = n + K - 1
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=3, ir_index=IR_INDEX[:3])
    ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
    _anchor(ref, want, K)
    cuts = [0, 2 * hop, 4 * hop, out_len]
    for lin, lout in [(LL.LA(n), LL.LA(out_len))] + pairs(n, out_len):
        i, o = LL.place(x, lin, DEV), LL.empty(3, out_len, lout, DEV)
        for b, e in zip(cuts[:-1], cuts[1:]):
            before = bits(LL.payload(o))
            sync()
            eng.process_device_segment(i.ptr, i.stride, n, o.ptr, o.stride, out_len, b, e)
            sync()
            LL.check_guards(o, untouched=[(e, out_len)])  # the part no segment has written yet
            assert np.array_equal(bits(LL.payload(o))[:, :b], before[:, :b]), (lin, lout, b)
        LL.check_unchanged(i, x)
        assert same(LL.payload(o), ref), (lin, lout)


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("C_", [1, 3, 4])
@pytest.mark.parametrize("hop", [1024, 2048])
def test_multi_mix(gpu, hop, C_, parity):
    """ad_conv_multi_process_device_mix: hop 1024 (per-channel outputs into the
    handle's scratch, then k_mixdown) and hop 2048 (the mix fused into K3);
    d_mix at every placement with mix_stride > out_len, the input placement
    varied independently; a short out_len; two segments."""
    n = 3 * hop + 77
    irs, x4, want4 = _shape(hop, n, None, 4)
    x, want = np.ascontiguousarray(x4[:C_]), want4[:C_]
    K = irs.shape[1]
    full = n + K - 1
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=C_, ir_index=IR_INDEX[:C_])

    def run(out_len, lin, lmix, cuts=None):
        i, m = LL.place(x, lin, DEV), LL.empty(2, out_len, lmix, DEV)
        for b, e in zip((cuts or [0, out_len])[:-1], (cuts or [0, out_len])[1:]):
            before = bits(LL.payload(m))
            sync()
            eng.process_device_mix(i.ptr, i.stride, n, m.ptr, m.stride, out_len, parity, b, e)
            sync()
            LL.check_guards(m, untouched=[(e, out_len)])
            assert np.array_equal(bits(LL.payload(m))[:, :b], before[:, :b]), (lin, lmix, b)
        LL.check_unchanged(i, x)
        return LL.payload(m)

    def anchor(y):  # test_multi_mix_fused's bar, against the summed long-double convolutions
        for side in range(2):
            chans = [c for c in range(C_) if (parity + c) % 2 == side]
            if not chans:
                assert not y[side].any()  # a side with no channel is written as zeros
                continue
            assert rms(y[side], np.sum(want[chans], axis=0)[:y.shape[1]]) < FFT_RMS_TOL * len(chans)

    ref = run(full, LL.LA(n), LL.LA(full))
    anchor(ref)
    for lin, lmix in pairs(n, full):
        if lmix.stride_pad == 0:
            continue  # mix_stride > out_len in every variant
        assert same(run(full, lin, lmix), ref), (lin, lmix)
    short = hop + 1
    ref_s = run(short, LL.LA(n), LL.LA(short))
    anchor(ref_s)
    for lin, lmix in [(LL.L3, LL.L3), (LL.L2(n), LL.L1)]:
        assert same(run(short, lin, lmix), ref_s), (lin, lmix)
    for lin, lmix in [(LL.L3, LL.L3), (LL.LA(n), LL.L2(full))]:
        assert same(run(full, lin, lmix, [0, 3 * hop, full]), ref), (lin, lmix)


def test_multi_stride_validation(gpu):
    """With more than one channel a stride shorter than the row is
    AD_ERR_LENGTH_MISMATCH and a null pointer AD_ERR_INVALID_ARGUMENT, in the
    plain, segment and mix forms, before any device work: the guarded output
    keeps every bit.  A single channel has no stride to check."""
    hop, n = 64, 200
    irs, x, want = _shape(hop, n)
    K = irs.shape[1]
    out_len = n + K - 1
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=3, ir_index=IR_INDEX[:3])
    i, o, m = LL.place(x, LL.L1, DEV), LL.empty(3, out_len, LL.L1, DEV), LL.empty(2, out_len, LL.L1, DEV)
    forms = [
        lambda ip, istr, op, ostr: eng.process_device(ip, istr, n, op, ostr, out_len),
        lambda ip, istr, op, ostr: eng.process_device_segment(ip, istr, n, op, ostr, out_len, 0, hop),
    ]
    sync()
    for f in forms:
        for args, err in [((i.ptr, n - 1, o.ptr, o.stride), conv.ErrLengthMismatch),
                          ((i.ptr, i.stride, o.ptr, out_len - 1), conv.ErrLengthMismatch),
                          ((0, i.stride, o.ptr, o.stride), conv.ErrInvalidArgument),
                          ((i.ptr, i.stride, 0, o.stride), conv.ErrInvalidArgument)]:
            with pytest.raises(err) as ei:
                f(*args)
            assert type(ei.value) is err
    for args, err in [((i.ptr, n - 1, n, m.ptr, m.stride, out_len), conv.ErrLengthMismatch),
                      ((i.ptr, i.stride, n, m.ptr, out_len - 1, out_len), conv.ErrLengthMismatch),
                      ((0, i.stride, n, m.ptr, m.stride, out_len), conv.ErrInvalidArgument),
                      ((i.ptr, i.stride, n, 0, m.stride, out_len), conv.ErrInvalidArgument)]:
        with pytest.raises(err) as ei:
            eng.process_device_mix(*args)
        assert type(ei.value) is err
    sync()
    LL.check_unchanged(i, x)
    LL.check_guards(o, untouched=[(0, out_len)])
    LL.check_guards(m, untouched=[(0, out_len)])
    # the calls still work after the refusals, and one channel ignores its strides
    eng.process_device(i.ptr, i.stride, n, o.ptr, o.stride, out_len)
    sync()
    LL.check_guards(o)
    _anchor(LL.payload(o), want, K)
    one = conv.MultiChannelConvolver(irs[1:2], hop=hop, channels=1)
    i1, o1 = LL.place(x[:1], LL.L3, DEV), LL.empty(1, out_len, LL.L3, DEV)
    sync()
    one.process_device(i1.ptr, 0, n, o1.ptr, 0, out_len)
    sync()
    LL.check_guards(o1)
    LL.check_unchanged(i1, x[:1])
    _anchor(LL.payload(o1), want[:1], K)


# --------------------------------------------------------------- streaming blocks
@pytest.mark.parametrize("B", [64, 2048, 100, 3000])
def test_multi_stream_block_device(gpu, B):
    """ad_conv_multi_stream_process_block_device, five blocks: whole hops on
    the plain (64) and split (2048) families, the carry path at hop 128
    (B = 100) and with B larger than its hop (3000), each block's input and
    output placed on its own.  Against the same blocks through the host
    ProcessBlock (bit for bit), itself against the oracle at
    test_multi_stream_any_block_size's bar.  The header does not allow
    d_out == d_in for this call, so no aliased run."""
    K, C_, nb = 3000, 3, 5
    irs = np.stack([signals.white_noise(K, 0x2B0 + i) for i in range(2)])
    x = np.stack([signals.white_noise(B * nb, 0xC000 + c) for c in range(C_)])
    blocks = [np.ascontiguousarray(x[:, k * B:(k + 1) * B]) for k in range(nb)]
    host = conv.MultiChannelStreamingConvolver(irs, B, C_, ir_index=IR_INDEX[:3])
    ref = [host.ProcessBlock(b) for b in blocks]
    for c in range(C_):
        o = O.Streaming(irs[IR_INDEX[c]], B)
        w = np.concatenate([o.process_block(b[c]) for b in blocks])
        g = np.concatenate([r[c] for r in ref])
        assert rms(g, w) < FFT_RMS_TOL and np.max(np.abs(g - w)) < 1e-9
    for lin, lout in [(LL.LA(B), LL.LA(B))] + pairs(B, B):
        s = conv.MultiChannelStreamingConvolver(irs, B, C_, ir_index=IR_INDEX[:3])
        for k, b in enumerate(blocks):
            i, o = LL.place(b, lin, DEV), LL.empty(C_, B, lout, DEV)
            sync()
            s.process_block_device(i.ptr, i.stride, o.ptr, o.stride)
            sync()
            LL.check_unchanged(i, b)
            LL.check_guards(o)
            assert same(LL.payload(o), ref[k]), (lin, lout, k)


# --------------------------------------------------------------- partitioned / reverb form
PC_SIZES = [64, 1, 197, 7, 1000]


def _pc_calls(C_=3):
    K = 1000
    h = signals.make_impulse_kernel(K)
    x = np.stack([signals.white_noise(sum(PC_SIZES), 0xD000 + c) for c in range(C_)])
    cuts = np.cumsum([0] + PC_SIZES)
    return h, x, [np.ascontiguousarray(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def test_pc_multi_process_device(gpu):
    """ad_conv_pc_multi_process_device: K = 1000, orders (6, 9), calls of 64,
    1, 197, 7 and 1000 samples, every call's buffers placed on their own;
    against the contiguous run, itself against O.Partitioned at
    test_partitioned_multi_vs_oracle's bar."""
    h, x, calls = _pc_calls()
    ref = None
    for lin, lout in [(LL.L0, LL.L0)] + [p for m in (64, 197) for p in pairs(m, m)]:
        g = conv.PartitionedConvolutionMulti(h, 6, 9, 3)
        got = []
        for blk in calls:
            m = blk.shape[1]
            i, o = LL.place(blk, lin, DEV), LL.empty(3, m, lout, DEV)
            sync()
            g.process_device(i.ptr, i.stride, o.ptr, o.stride, m)
            sync()
            LL.check_unchanged(i, blk)
            LL.check_guards(o)
            got.append(LL.payload(o))
        got = np.concatenate(got, axis=1)
        if ref is None:
            ref = got
            for c in range(3):
                o_ = O.Partitioned(h, 6, 9)
                w = np.concatenate([o_.process_block(b[c]) for b in calls])
                assert rms(ref[c], w) < FFT_RMS_TOL and np.max(np.abs(ref[c] - w)) < 1e-9
        else:
            assert same(got, ref), (lin, lout)


def test_reverb_multi_process_device(gpu):
    """ad_conv_reverb_multi_process_device: the same calls in place with
    wet / dry = 0.3 / 0.8; against the contiguous run, itself against
    O.Partitioned(h, 6, 13) at the bar of test_partitioned_multi_vs_oracle's
    reverb-form check (max-abs < 1e-9)."""
    h, x, calls = _pc_calls()
    ref = None
    for lay in [LL.L0, LL.L1, LL.L2(64), LL.L2(197), LL.L3]:
        r = conv.NewConvolutionReverbMulti(h, 6, 3)
        r.SetWetDry(0.3, 0.8)
        got = []
        for blk in calls:
            m = blk.shape[1]
            b = LL.place(blk, lay, DEV)
            sync()
            r.process_inplace_device(b.ptr, b.stride, m)
            sync()
            LL.check_guards(b)
            got.append(LL.payload(b))
        got = np.concatenate(got, axis=1)
        if ref is None:
            ref = got
            for c in range(3):
                o_ = O.Partitioned(h, 6, 13)
                w = 0.8 * x[c] + 0.3 * np.concatenate([o_.process_block(b[c]) for b in calls])
                assert np.max(np.abs(ref[c] - w)) < 1e-9
        else:
            assert same(got, ref), lay


# --------------------------------------------------------------- effect chain
FXE = P.EffectChain
COMP = {"auto_makeup": 0, "makeup_db": 0.0}
VERB = (0.3, 0.8, 0.8, 0.3, 0.02)
CHAINS = {  # (eq, compressor, freeverb)
    "config5": (True, True, True),
    "eq": (True, False, False),
    "comp": (False, True, False),
    "verb": (False, False, True),  # under TIME_PARALLEL: k_fxtp_verb in place on the caller's buffer
    "eq+verb": (True, False, True),
}
ENGINES = {"fused": FXE.ENGINE_FUSED, "nosplit": FXE.ENGINE_STAGED_NOSPLIT, "staged": FXE.ENGINE_STAGED,
           "tp": FXE.ENGINE_TIME_PARALLEL, "auto": FXE.ENGINE_AUTO}


def _fx(C_, chain):
    eq, comp, verb = CHAINS[chain]
    return FXE(C_, design.config5_eq(FS) if eq else (), COMP if comp else None, VERB if verb else None, FS)


def _engine_expected(engine, chain):
    """capi_dsp.cpp fx_run: what ad_fx_chain_last_engine reports for a request."""
    eq, comp, _ = CHAINS[chain]
    if engine == FXE.ENGINE_FUSED:
        return FXE.ENGINE_FUSED
    if engine == FXE.ENGINE_TIME_PARALLEL or (engine == FXE.ENGINE_AUTO and comp):
        return FXE.ENGINE_TIME_PARALLEL
    if engine == FXE.ENGINE_STAGED_NOSPLIT:
        return FXE.ENGINE_STAGED_NOSPLIT
    return FXE.ENGINE_STAGED if eq else FXE.ENGINE_STAGED_NOSPLIT  # a split / per-section / lanes EQ stage


@functools.lru_cache(maxsize=None)
def _fx_oracle(chain, C_, n, seed, chans):
    eq, comp, verb = CHAINS[chain]
    x = np.stack([0.5 * signals.white_noise(n, seed + c) for c in range(C_)])
    want = {}
    for c in chans:
        v = x[c].copy()
        if eq:
            for co, g in design.config5_eq(FS):
                v, _ = O.biquad_chain_block(np.ravel(co), np.zeros(2 * len(co)), g, v)
        if comp:
            v = O.Compressor(FS, **COMP).process_in_place(v)
        if verb:
            fv = O.Freeverb()
            fv.set(*VERB)
            v = fv.process_in_place(v)
        want[c] = v
    x.setflags(write=False)
    return x, want


def _fx_case(engine, chain, C_, n, calls, chunk, lays):
    x, want = _fx_oracle(chain, C_, n, 0xE000, (0, C_ - 1))
    expected = _engine_expected(engine, chain)
    fx = _fx(C_, chain)
    fx.SetEngine(engine, chunk)
    host = x.copy()
    for lo, hi in calls:
        b = np.ascontiguousarray(host[:, lo:hi])
        fx.Process(b)
        host[:, lo:hi] = b
    assert fx.LastEngine()[0] == expected
    fx.close()
    exact = expected != FXE.ENGINE_TIME_PARALLEL and not CHAINS[chain][1]
    for c, w in want.items():  # biquad / Freeverb bit-exact; a compressor or the time-parallel engine: RMS_TOL
        assert same(host[c], w) if exact else rms(host[c], w) <= RMS_TOL, (c, rms(host[c], w))
    for lay in lays:
        fx = _fx(C_, chain)
        fx.SetEngine(engine, chunk)
        b = LL.place(x, lay, DEV)
        for lo, hi in calls:
            before = bits(LL.payload(b))
            sync()
            fx.process_device(b.ptr + 8 * lo, b.stride, hi - lo)
            sync()
            LL.check_guards(b)
            now = bits(LL.payload(b))
            assert np.array_equal(now[:, :lo], before[:, :lo]) and np.array_equal(now[:, hi:], bits(x)[:, hi:]), (lay, lo)
        assert fx.LastEngine()[0] == expected
        fx.close()
        assert same(LL.payload(b), host), (lay,)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_fx_chain_process_device(gpu, engine, chain):
    """ad_fx_chain_process_device in place at every placement: 70 channels (a
    ragged channel group), 3000 samples in calls of 700, 1 and 2299 at a
    256-sample chunk, against the same calls through the host Process (the
    same engine and chunking: bit for bit), each call leaving the rest of the
    row alone."""
    n = 3000
    _fx_case(ENGINES[engine], chain, 70, n, [(0, 700), (700, 701), (701, n)], 256,
             [LL.LA(n)] + LL.variants(n))


def test_fx_chain_process_device_default_chunk(gpu):
    """The time-parallel engine at its default chunk, one call just over one
    49152-sample chunk (config 5, 3 channels, wide padding)."""
    _fx_case(FXE.ENGINE_TIME_PARALLEL, "config5", 3, 50000, [(0, 50000)], 0, [LL.L3])


@pytest.mark.parametrize("n", [1, 777])
def test_fx_graph_process_device(gpu, n):
    """ad_fx_graph_process_device: test_branched_graph's graph, two calls, in
    place at L0, L1 and L3, against the host Process bit for bit, itself
    against the oracle graph at test_branched_graph's bar."""
    C_ = 3
    xs = [np.stack([0.5 * signals.white_noise(n, 1000 * k + c) for c in range(C_)]) for k in range(2)]
    ch = E.Chain(FS, C_, designer=design.RBJDesigner())
    ch.LoadGraph(BRANCHED)
    oracles = [O.FxGraph(ch.spec, FS) for _ in range(C_)]
    host = []
    for x in xs:
        y = x.copy()
        assert ch.Process(y)
        for c in range(C_):
            w = oracles[c].process(x[c])
            assert rms(y[c], w) < RMS_TOL and np.max(np.abs(y[c] - w)) < 1e-10
        host.append(y)
    ch.close()
    for lay in (LL.L0, LL.L1, LL.L3):
        ch = E.Chain(FS, C_, designer=design.RBJDesigner())
        ch.LoadGraph(BRANCHED)
        for x, y in zip(xs, host):
            b = LL.place(x, lay, DEV)
            sync()
            assert ch.process_device(b.ptr, b.stride, n)
            sync()
            LL.check_guards(b)
            assert same(LL.payload(b), y), lay
        ch.close()


# --------------------------------------------------------------- FIR
@pytest.mark.parametrize("taps", [7, 300])
def test_fir_process_device(gpu, taps):
    """ad_fir_process_device: 4 channels, two calls of n = 1501 (and of 1500,
    aligned to aligned: the vector form), source and destination placed
    independently, and in place at L3; against the host ProcessBlock bit for
    bit, itself against the oracle (bit-exact under 32 taps, else RMS_TOL:
    test_fir_vs_oracle)."""
    h = signals.make_test_kernel(taps)
    C_ = 4
    for n in (1501, 1500):
        x = np.stack([signals.white_noise(2 * n, 0xF000 + c) for c in range(C_)])
        calls = [np.ascontiguousarray(x[:, :n]), np.ascontiguousarray(x[:, n:])]
        f = P.Filter(h, channels=C_)
        host = []
        for blk in calls:
            y = blk.copy()
            f.ProcessBlock(y)
            host.append(y)
        f.close()
        for c in range(C_):
            w = O.Fir(h).process_block(x[c])
            g = np.concatenate([y[c] for y in host])
            assert same(g, w) if taps < 32 else rms(g, w) <= RMS_TOL
        for lsrc, ldst in [(LL.LA(n), LL.LA(n))] + pairs(n, n) + [(LL.L3, None)]:
            f = P.Filter(h, channels=C_)
            for blk, y in zip(calls, host):
                s = LL.place(blk, lsrc, DEV)
                d = s if ldst is None else LL.empty(C_, n, ldst, DEV)  # None: in place
                sync()
                f.process_device(s.ptr, s.stride, d.ptr, d.stride, n)
                sync()
                if ldst is not None:
                    LL.check_unchanged(s, blk)
                LL.check_guards(d)
                assert same(LL.payload(d), y), (n, lsrc, ldst)
            f.close()


# --------------------------------------------------------------- one-shot calls
SHIFTS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]  # each array at +0 / +8 bytes


@pytest.mark.parametrize("n,m", [(100, 15), (5, 64), (1, 1)])
def test_direct_device(gpu, n, m):
    """ad_conv_direct_device: a, b and dst each shifted by 8 bytes
    independently; against the host Direct bit for bit (itself bit-exact
    against the oracle, as test_config1_direct holds it)."""
    a, b = signals.white_noise(n, 11 + n), signals.white_noise(m, 13 + m)
    host = conv.Direct(a, b)
    assert same(host, O.direct(a, b))
    for sa, sb, sd in SHIFTS:
        da, db = LL.place(a, LL.Layout(sa, 0), DEV), LL.place(b, LL.Layout(sb, 0), DEV)
        dd = LL.empty(1, n + m - 1, LL.Layout(sd, 0), DEV)
        sync()
        conv.direct_device(da.ptr, n, db.ptr, m, dd.ptr)
        sync()
        LL.check_unchanged(da, a)
        LL.check_unchanged(db, b)
        LL.check_guards(dd)
        assert same(LL.payload(dd)[0], host), (sa, sb, sd)


@pytest.mark.parametrize("n,m", [(33, 31), (1000, 37), (40000, 25000)])
def test_correlate_fft_device(gpu, n, m):
    """ad_correlate_fft_device (one- and two-pass plans): a, b and out each
    shifted by 8 bytes; against the host CorrelateFFT bit for bit, as
    test_correlate_fft_device_matches_host compares the aligned call."""
    a, b = signals.white_noise(n, 5 + n), signals.white_noise(m, 9 + m)
    host = conv.CorrelateFFT(a, b)
    for sa, sb, sd in SHIFTS:
        da, db = LL.place(a, LL.Layout(sa, 0), DEV), LL.place(b, LL.Layout(sb, 0), DEV)
        dd = LL.empty(1, n + m - 1, LL.Layout(sd, 0), DEV)
        sync()
        check(lib().ad_correlate_fft_device(C.c_void_p(da.ptr), n, C.c_void_p(db.ptr), m, C.c_void_p(dd.ptr), 0,
                                            C.c_void_p(0)))
        sync()
        LL.check_unchanged(da, a)
        LL.check_unchanged(db, b)
        LL.check_guards(dd)
        assert same(LL.payload(dd)[0], host), (sa, sb, sd)


@pytest.mark.parametrize("channels,frames", [(1, 7), (2, 1031), (3, 5000)])
def test_decode_f16_device(gpu, channels, frames):
    """ad_decode_f16_device: the uint16 input shifted by 0, 2 and 6 bytes, the
    output by 0 and 8; against the host ad_decode_f16 bit for bit (NaN codes
    included), itself against the oracle per code."""
    rng = np.random.default_rng(channels * 7919 + frames)
    codes = rng.integers(0, 65536, frames * channels).astype(np.uint16)
    host = irlib.decode_f16_gpu(codes, channels)
    want = np.array([O.decode_f16(int(v)) for v in codes], dtype=np.float64).reshape(frames, channels).T
    assert np.array_equal(host, want, equal_nan=True)
    for si in (0, 1, 3):
        for so in (0, 1):
            i = LL.place(codes, LL.Layout(si, 0), DEV)
            o = LL.empty(1, channels * frames, LL.Layout(so, 0), DEV)
            sync()
            check(lib().ad_decode_f16_device(C.c_void_p(i.ptr), frames, channels, C.c_void_p(o.ptr), C.c_void_p(0)))
            sync()
            LL.check_unchanged(i, codes)
            LL.check_guards(o)
            assert same(LL.payload(o)[0].reshape(channels, frames), host), (si, so)


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("channels", [1, 5])
def test_mixdown_device(gpu, channels, parity):
    """ad_conv_mixdown_device: misaligned d_chan and d_mix, mix_stride > len;
    against the aligned call bit for bit, itself against the sums in
    increasing channel order at test_mixdown's bar (atol 1e-15)."""
    n = 1001
    x = np.stack([signals.white_noise(n, 0x777 + c) for c in range(channels)])
    ref = None
    for lch, lmix in [(LL.LA(n), LL.LA(n)), (LL.L2(n), LL.L2(n)), (LL.L3, LL.L1), (LL.L1, LL.L3), (LL.L0, LL.L2(n))]:
        i, m = LL.place(x, lch, DEV), LL.empty(2, n, lmix, DEV)
        sync()
        conv.mixdown_device(i.ptr, channels, i.stride, n, m.ptr, mix_stride=m.stride, first_parity=parity)
        sync()
        LL.check_unchanged(i, x)
        LL.check_guards(m)
        got = LL.payload(m)
        if ref is None:
            ref = got
            for side in range(2):
                w = np.zeros(n)
                for c in range(channels):
                    if (parity + c) % 2 == side:
                        w = w + x[c]
                np.testing.assert_allclose(ref[side], w, atol=1e-15, rtol=0)
        else:
            assert same(got, ref), (lch, lmix)
