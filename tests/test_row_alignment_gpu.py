"""Per-row alignment of K1's loads and K3's stores (fft_kernels.hip).

A row of a [C][stride] buffer starts on a 16-byte boundary or 8 bytes past one,
and the kernels decide that per item: aligned rows take the 16-byte path,
rows 8 bytes off take the same 16-byte accesses shifted by one double (the
neighbour lane's value by an in-wave exchange, the wave's two edge values as
singles), partial last blocks the scalar path.  The placements that matter are
the ones callers use: a contiguous [C][n + K - 1] output has an odd stride, so
its rows alternate (L0 with an odd length), and an offset base puts every row
off (L2).

Every case follows test_device_layout_gpu: the result at the reference
placement LA (every row aligned) is anchored once to O.direct_ld at that
file's bars, every other placement must give the same bits, no guard or
padding element may change, and the input keeps its bits.  Shapes are the
smallest that reach each path; hop 8192 gives the split kernels' workgroups
eight waves, so wave-edge singles meet a neighbouring wave's slots.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import layout_lib as LL
import oracle_lib as O
from algodsp import conv, signals
from test_conv_gpu import FFT_RMS_TOL, rms
from test_device_layout_gpu import DEV, IR_INDEX, _anchor, _run_multi, _shape, bits, same, sync

pytestmark = pytest.mark.gpu

SERIAL = conv.MultiChannelConvolver.SCHED_SERIAL


def _engine(irs, hop, C_=3):
    return conv.MultiChannelConvolver(irs, hop=hop, channels=C_, ir_index=IR_INDEX[:C_])


def _out_layouts(out_len):
    """Output placements beside LA: rows alternating (L0 when out_len is odd,
    L1 when it is even), every row off (L2), an off base with an odd or even
    wide stride (L3)."""
    return [LL.L0, LL.L1, LL.L2(out_len), LL.L3]


@pytest.mark.parametrize("odd", [77, 78])
@pytest.mark.parametrize("hop", [64, 1024, 2048, 4096, 8192])
def test_k3_rows(gpu, hop, odd):
    """K3's stores, the input aligned: the plain forms (hop 64: four lanes per
    transform, 1024: one wave) and the split kernels (2048, 4096, 8192: two,
    four and eight waves per workgroup), 3 channels with IR_INDEX mixed,
    K = 2 hop + hop/2 + 1, out_len full (odd for even n), n, hop + 1, hop, 1."""
    n = 3 * hop + odd
    irs, x, want = _shape(hop, n)
    K = irs.shape[1]
    eng = _engine(irs, hop)
    for out_len in (n + K - 1, n, hop + 1, hop, 1):
        ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
        _anchor(ref, want, K)
        for lout in _out_layouts(out_len):
            assert same(_run_multi(eng, x, out_len, LL.LA(n), lout), ref), (out_len, lout)


@pytest.mark.parametrize("odd", [77, 78])
@pytest.mark.parametrize("hop", [64, 1024, 2048, 4096, 8192])
def test_k1_rows(gpu, hop, odd):
    """K1's loads against an aligned output: the input contiguous (L0; rows
    alternate when n is odd), alternating the other way (L1), every row off
    (L2), an off base with wide padding (L3).  Three whole blocks take the
    shifted 16-byte loads, the partial fourth the scalar path."""
    n = 3 * hop + odd
    irs, x, want = _shape(hop, n)
    K = irs.shape[1]
    out_len = n + K - 1
    eng = _engine(irs, hop)
    ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
    _anchor(ref, want, K)
    for lin in (LL.L0, LL.L1, LL.L2(n), LL.L3):
        assert same(_run_multi(eng, x, out_len, lin, LL.LA(out_len)), ref), lin


def test_nontemporal_rows(gpu):
    """The non-temporal K3 (launches of >= 1024 items) on off rows: hop 2048,
    64 channels, 17 blocks + 5 samples, K = 5121, so 64 x 20 = 1280 items in
    one launch (confirmed by the engine's launch profile).  The output
    contiguous (out_len odd: rows alternate) and with every row off; then the
    fused mix's non-temporal form with its [2][out_len] rows placed the same
    ways."""
    hop, C_ = 2048, 64
    n, K = 17 * hop + 5, 2 * hop + hop // 2 + 1
    out_len = n + K - 1
    assert out_len % 2 == 1
    irs = np.stack([signals.white_noise(K, 0x1B0 + i) for i in range(2)])
    x = np.stack([signals.white_noise(n, 0xB000 + c) for c in range(C_)])
    eng = conv.MultiChannelConvolver(irs, hop=hop, channels=C_)
    eng.set_schedule(SERIAL)
    eng.profile_enable(True)
    ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
    launches = eng.profile_read()["k_irfft_store"][1]
    eng.profile_enable(False)
    assert launches == 1 and C_ * -(-out_len // hop) >= 1024, launches
    with ThreadPoolExecutor(16) as ex:
        want = np.stack(list(ex.map(lambda c: O.direct_ld(x[c], irs[c % 2]), range(C_))))
    _anchor(ref, want, K)
    for lout in (LL.L0, LL.L2(out_len)):
        eng.profile_enable(True)
        got = _run_multi(eng, x, out_len, LL.LA(n), lout)
        launches = eng.profile_read()["k_irfft_store"][1]
        eng.profile_enable(False)
        assert launches == 1, launches
        assert same(got, ref), lout
    mixes = []
    for lmix in (LL.LA(out_len), LL.L0, LL.L2(out_len)):
        i, m = LL.place(x, LL.LA(n), DEV), LL.empty(2, out_len, lmix, DEV)
        sync()
        eng.process_device_mix(i.ptr, i.stride, n, m.ptr, m.stride, out_len)
        sync()
        LL.check_unchanged(i, x)
        LL.check_guards(m)
        mixes.append(LL.payload(m))
    for side in range(2):  # test_multi_mix_fused's bar, against the summed long-double convolutions
        assert rms(mixes[0][side], np.sum(want[side::2], axis=0)) < FFT_RMS_TOL * (C_ // 2)
    assert same(mixes[1], mixes[0]) and same(mixes[2], mixes[0])


@pytest.mark.parametrize("parity", [0, 1])
def test_fused_mix_rows(gpu, parity):
    """ad_conv_multi_process_device_mix with the mix fused into K3: hop 2048,
    4 channels, both first_parity values, the two mix rows contiguous (L0: the
    second row off when out_len is odd), alternating (L1) and both off (L2);
    the full output (a partial last block) and a whole number of blocks."""
    hop, C_ = 2048, 4
    n = 3 * hop + 77
    irs, x, want = _shape(hop, n, None, 4)
    K = irs.shape[1]
    eng = _engine(irs, hop, C_)

    def run(out_len, lmix):
        i, m = LL.place(x, LL.LA(n), DEV), LL.empty(2, out_len, lmix, DEV)
        sync()
        eng.process_device_mix(i.ptr, i.stride, n, m.ptr, m.stride, out_len, parity)
        sync()
        LL.check_unchanged(i, x)
        LL.check_guards(m)
        return LL.payload(m)

    for out_len in (n + K - 1, 5 * hop, hop + 1):
        ref = run(out_len, LL.LA(out_len))
        for side in range(2):
            chans = [c for c in range(C_) if (parity + c) % 2 == side]
            assert rms(ref[side], np.sum(want[chans], axis=0)[:out_len]) < FFT_RMS_TOL * len(chans)
        for lmix in (LL.L0, LL.L1, LL.L2(out_len)):
            assert same(run(out_len, lmix), ref), (out_len, lmix)


@pytest.mark.parametrize("hop", [1024, 2048])
def test_segment_rows(gpu, hop):
    """ad_conv_multi_process_device_segment cut at hop multiples, the output
    contiguous (odd out_len: rows alternate) and with every row off: each
    segment leaves the rest of the rows alone, and together they are the
    one-call result of the reference placement."""
    n = 3 * hop + 77
    irs, x, want = _shape(hop, n)
    K = irs.shape[1]
    out_len = n + K - 1
    eng = _engine(irs, hop)
    ref = _run_multi(eng, x, out_len, LL.LA(n), LL.LA(out_len))
    _anchor(ref, want, K)
    cuts = [0, hop, 4 * hop, out_len]
    for lout in (LL.L0, LL.L2(out_len)):
        i, o = LL.place(x, LL.LA(n), DEV), LL.empty(3, out_len, lout, DEV)
        for b, e in zip(cuts[:-1], cuts[1:]):
            before = bits(LL.payload(o))
            sync()
            eng.process_device_segment(i.ptr, i.stride, n, o.ptr, o.stride, out_len, b, e)
            sync()
            LL.check_guards(o, untouched=[(e, out_len)])
            assert np.array_equal(bits(LL.payload(o))[:, :b], before[:, :b]), (lout, b)
        LL.check_unchanged(i, x)
        assert same(LL.payload(o), ref), lout


def test_accumulate_stage(gpu):
    """K3 with accumulate set: the partitioned convolver's stage of 2048-sample
    partitions (orders 6..11, K = 5000: five fused stages, then one UPOLS
    engine that adds into the shared accumulator through the split K3).  The
    accumulator is the handle's own buffer, whose rows the engine keeps 16-byte
    aligned, so what a caller can vary is where its own rows lie: the calls'
    buffers with every row off against the aligned run, bit for bit, and that
    against O.Partitioned at test_partitioned_multi_vs_oracle's bar."""
    K, C_, sizes = 5000, 3, [2048, 1, 2500, 77]
    h = signals.white_noise(K, 0x2C0)  # the 2048 stage's taps, 3968 on, weigh as much as the rest
    x = np.stack([signals.white_noise(sum(sizes), 0xD100 + c) for c in range(C_)])
    cuts = np.cumsum([0] + sizes)
    calls = [np.ascontiguousarray(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]

    def run(lay):
        g = conv.PartitionedConvolutionMulti(h, 6, 11, C_)
        got = []
        for blk in calls:
            m = blk.shape[1]
            i, o = LL.place(blk, lay(m), DEV), LL.empty(C_, m, lay(m), DEV)
            sync()
            g.process_device(i.ptr, i.stride, o.ptr, o.stride, m)
            sync()
            LL.check_unchanged(i, blk)
            LL.check_guards(o)
            got.append(LL.payload(o))
        return np.concatenate(got, axis=1)

    ref = run(LL.LA)
    for c in range(C_):
        o_ = O.Partitioned(h, 6, 11)
        w = np.concatenate([o_.process_block(b[c]) for b in calls])
        assert rms(ref[c], w) < FFT_RMS_TOL and np.max(np.abs(ref[c] - w)) < 1e-9, (c, rms(ref[c], w))
    assert same(run(LL.L2), ref)
