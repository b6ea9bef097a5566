"""The GPU crossover (MultiBandCrossover) and multiband compressor
(MultibandCompressor) against the restatement in tests/multiband_ref.py.

The crossover is compared on float64 bits -- every band, every channel, the
state after every call -- in the pipelined form and in the one-stage-per-launch
form.  The compressors behind it are held to the project's compressor bars
(1e-12 relative RMS, 1e-10 max abs, no sample excluded) per band, and the sum
to the bars the triangle inequality gives.

Shapes: N = 1501 in calls of [700, 1, 800] (the walk's tiles of 8 samples end
inside calls, one call is a single sample), channels 1, 3 and 65 (one past a
wave), distinct noise per channel at amplitude 2, 48 kHz; the last row's tail
decays into denormals.
"""
import functools
import math

import numpy as np
import pytest
import torch

import layout_lib as LL
import multiband_ref as R
from algodsp import _lib, effectchain as E, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10
METRICS_RTOL = 1e-11  # the compressor's metrics bar on the time-parallel engine (test_dynamics_space_gpu.py)
FS = 48000.0
N, CUTS = 1501, (700, 1, 800)
CHANNELS = [1, 3, 65]
NAN, INF = float("nan"), float("inf")
F8 = (60.0, 150.0, 400.0, 1000.0, 2500.0, 6000.0, 12000.0)

CONFIGS = {
    "2 bands LR2": ((1000.0,), 2),  # inverted HP, first-order sections
    "2 bands LR4": ((1000.0,), 4),
    "3 bands LR6": ((200.0, 2000.0), 6),
    "3 bands LR8": ((200.0, 2000.0), 8),
    "8 bands LR4": (F8, 4),
    "8 bands LR24": (F8, 24),  # 7 waves, 12 sections per side
    "edge LR24": ((20.0, 23999.0), 24),  # the outer bands near 1e-13 and in the denormal range
}
COMP_CONFIGS = [k for k in CONFIGS if k != "edge LR24"]


@functools.lru_cache(maxsize=None)
def noise(channels, n=N, seed=0xB4D, amplitude=2.0):
    x = np.stack([signals.white_noise(n, seed + c) for c in range(channels)]) * amplitude
    t = np.arange(1000, n)
    x[-1, 1000:] = 1e-300 * 10.0 ** (-(t - 1000) / 20.0)  # down through the denormals to zero
    x.setflags(write=False)
    return x


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(got, want, what=""):
    """Bit patterns, the sign of zero included; a NaN by position only."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(-1) & ~gn.reshape(-1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at flat index {i}: "
                             f"got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def rms(a):
    return math.sqrt(float(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


def within_bars(got, want, what=""):
    err = np.asarray(got) - np.asarray(want)
    rel = rms(err) / max(rms(want), 1e-300)
    worst = float(np.max(np.abs(err)))
    print(f"{what}: relative rms {rel:.3e}, max abs {worst:.3e}")
    assert rel <= RMS_BAR and worst <= ABS_BAR, (what, rel, worst)


def edges(cuts):
    pos = 0
    for m in cuts:
        yield pos, pos + m
        pos += m


# ---- crossover --------------------------------------------------------------
def xover_ref(freqs, order, x, cuts):
    """Per call: bands [bands][C][m] and states [C][stages][2][S][2]."""
    refs = [R.MultiBand(freqs, order, FS) for _ in range(x.shape[0])]
    out = []
    for a, b in edges(cuts):
        bands = np.stack([r.ProcessBlock(x[c, a:b]) for c, r in enumerate(refs)], axis=1)
        out.append((bands, np.stack([r.get_state() for r in refs])))
    return out


@functools.lru_cache(maxsize=None)
def xover_ref_cached(name, channels):
    freqs, order = CONFIGS[name]
    return xover_ref(freqs, order, noise(channels), CUTS)


def xover_run(h, x, cuts, want, what):
    got = []
    for (a, b), (bands, states) in zip(edges(cuts), want):
        y = h.ProcessBlock(x[:, a:b].copy())
        same_bits(y, bands, f"{what}: bands of call [{a}, {b})")
        same_bits(np.stack([h.get_state(c) for c in range(x.shape[0])]), states, f"{what}: state after {b}")
        got.append(y)
    return got


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_crossover_is_bit_exact(gpu, name, channels):
    freqs, order = CONFIGS[name]
    x = noise(channels)
    want = xover_ref_cached(name, channels)
    assert all(np.isfinite(b).all() for b, _ in want)
    runs = []
    for pipelined in (True, False):
        h = P.MultiBandCrossover(freqs, order, FS, channels)
        h.set_pipelined(pipelined)
        waves, tile, lds = h.kernel_info()
        assert (waves, tile) == (len(freqs) if pipelined else 1, 8)
        assert lds == (3 * waves + 1) * 64 * 9 * 8 <= 160 * 1024  # sized by the launch's waves
        same_bits(h.sections(), R.MultiBand(freqs, order, FS).sections(), f"{name}: sections")
        runs.append(xover_run(h, x, CUTS, want, f"{name}, {channels} ch, pipelined={pipelined}"))
    for a, b in zip(*runs):
        same_bits(a, b, f"{name}: the two forms")


@pytest.mark.parametrize("name", ["2 bands LR2", "3 bands LR6", "8 bands LR24"])
def test_crossover_non_finite_input(gpu, name):
    freqs, order = CONFIGS[name]
    x = noise(3).copy()
    x[0, 720], x[0, 1200] = INF, NAN
    x[0, 5], x[0, 6] = -0.0, 1e-320
    want = xover_ref(freqs, order, x, CUTS)
    clean = xover_ref_cached(name, 3)
    for pipelined in (True, False):
        h = P.MultiBandCrossover(freqs, order, FS, 3)
        h.set_pipelined(pipelined)
        got = xover_run(h, x, CUTS, want, f"{name} non-finite, pipelined={pipelined}")
        for g, (cb, _) in zip(got, clean):
            same_bits(g[:, 1:], cb[:, 1:], f"{name}: the other channels")
        assert np.isnan(got[2][:, 0]).any() and np.isfinite(got[2][:, 1:]).all()


def test_crossover_signed_zeros(gpu):
    """First-order sections run the whole recurrence: an input of -0.0 comes out as the restatement's zeros."""
    z = np.zeros((1, 64))
    z[0, ::2] = -0.0
    for name in ("2 bands LR2", "3 bands LR6"):
        freqs, order = CONFIGS[name]
        xover_run(P.MultiBandCrossover(freqs, order, FS, 1), z, [64], xover_ref(freqs, order, z, [64]), name)


@pytest.mark.parametrize("name", ["2 bands LR2", "8 bands LR24"])
def test_crossover_checkpoint_and_reset(gpu, name):
    freqs, order = CONFIGS[name]
    x = noise(3)
    want = xover_ref_cached(name, 3)
    h = P.MultiBandCrossover(freqs, order, FS, 3)
    xover_run(h, x, CUTS[:1], want[:1], f"{name}: call 1")
    resumed = P.MultiBandCrossover(freqs, order, FS, 3)
    for c in range(3):
        resumed.set_state(c, h.get_state(c))
    for (a, b), (bands, states) in list(zip(edges(CUTS), want))[1:]:
        same_bits(resumed.ProcessBlock(x[:, a:b].copy()), bands, f"{name}: resumed call [{a}, {b})")
        same_bits(np.stack([resumed.get_state(c) for c in range(3)]), states, f"{name}: resumed state after {b}")
    resumed.Reset()  # MultiBand.Reset: equal to a fresh handle
    same_bits(resumed.get_state(1), np.zeros_like(want[0][1][1]), f"{name}: state after Reset")
    xover_run(resumed, x, CUTS, want, f"{name}: after Reset")
    with pytest.raises(_lib.ErrInvalidArgument):
        h.get_state(3)
    with pytest.raises(ValueError):
        h.set_state(0, np.zeros(3))


@pytest.mark.parametrize("pipelined", [True, False])
def test_crossover_process_device_layouts(gpu, pipelined):
    """Strides greater than n and rows 8 bytes off 16-byte alignment give the restatement's bits and touch nothing
    around the rows; the input is not written."""
    name, C_ = "3 bands LR6", 3
    freqs, order = CONFIGS[name]
    x = noise(C_)
    nb = len(freqs) + 1
    want = np.concatenate([b for b, _ in xover_ref_cached(name, C_)], axis=2)
    for layout in [LL.LA(N)] + LL.variants(N):
        h = P.MultiBandCrossover(freqs, order, FS, C_)
        h.set_pipelined(pipelined)
        src = LL.place(x, layout, DEV)
        dst = LL.empty(nb * C_, N, layout, DEV)  # band b of channel c is row b * C + c
        torch.cuda.synchronize()
        h.process_device(src.ptr, src.stride, dst.ptr, dst.stride, C_ * dst.stride, 700)
        h.process_device(src.ptr + 8 * 700, src.stride, dst.ptr + 8 * 700, dst.stride, C_ * dst.stride, 801)
        torch.cuda.synchronize()
        LL.check_guards(dst)
        LL.check_unchanged(src, x)
        same_bits(LL.payload(dst).reshape(nb, C_, N), want, f"{layout}")
    h = P.MultiBandCrossover(freqs, order, FS, C_)
    src, dst = LL.place(x, LL.L1, DEV), LL.empty(nb * C_, N, LL.L1, DEV)
    torch.cuda.synchronize()
    for args in ((src.ptr, N - 1, dst.ptr, dst.stride, C_ * dst.stride, N), (src.ptr, src.stride, dst.ptr, N - 1, C_ * dst.stride, N),
                 (src.ptr, src.stride, dst.ptr, dst.stride, (C_ - 1) * dst.stride + N - 1, N), (0, src.stride, dst.ptr, dst.stride, C_ * dst.stride, N),
                 (src.ptr, src.stride, 0, dst.stride, C_ * dst.stride, N), (src.ptr, src.stride, dst.ptr, dst.stride, C_ * dst.stride, -1)):
        with pytest.raises(_lib.ErrInvalidArgument):
            h.process_device(*args)
    h.process_device(src.ptr, src.stride, dst.ptr, dst.stride, C_ * dst.stride, 0)
    torch.cuda.synchronize()
    LL.check_unchanged(src, x)
    LL.check_guards(dst, untouched=[(0, N)])


def test_crossover_create_rejects(gpu):
    for freqs, order in (((), 4), ((5000.0, 500.0), 4), ((1000.0,), 3), ((24000.0,), 4), ((1000.0,), 26), (F8 + (20000.0,), 4)):
        with pytest.raises(_lib.ErrInvalidArgument):
            P.MultiBandCrossover(freqs, order, FS, 1)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.MultiBandCrossover((1000.0,), 4, FS, 0)


# ---- multiband compressor ---------------------------------------------------
def setup_defaults(mc):
    return mc


def setup_table(mc):
    """Another threshold / ratio / knee / attack / release per band; band 0 with manual makeup and side-chain cuts,
    band 1 on the RMS detector, the top band in the feedback topology."""
    nb = mc.NumBands()
    for b in range(nb):
        mc.SetBandThreshold(b, -30.0 + 3.0 * b)
        mc.SetBandRatio(b, 2.0 + b)
        mc.SetBandKnee(b, (0.0, 3.0, 6.0, 12.0)[b % 4])
        mc.SetBandAttack(b, (0.1, 1.0, 5.0, 20.0)[b % 4])
        mc.SetBandRelease(b, (20.0, 50.0, 100.0, 300.0)[b % 4])
    mc.SetBandMakeupGain(0, 3.0)
    mc.SetBandSidechainLowCut(0, 200.0)
    mc.SetBandSidechainHighCut(0, 6000.0)
    mc.SetBandDetectorMode(1, 1)
    mc.SetBandRMSWindow(1, 10.0)
    mc.SetBandTopology(nb - 1, 1)
    return mc


def setup_all_bands(mc):
    mc.SetAllBandsThreshold(-24.0)
    mc.SetAllBandsRatio(6.0)
    mc.SetAllBandsKnee(4.0)
    mc.SetAllBandsAttack(2.0)
    mc.SetAllBandsRelease(80.0)
    mc.SetAllBandsDetectorMode(1)
    mc.SetAllBandsRMSWindow(5.0)
    mc.SetAllBandsTopology(0)
    mc.SetAllBandsFeedbackRatioScale(False)
    return mc


def change_before_call_3(mc):
    mc.SetBandThreshold(0, -35.0)
    mc.SetBandRatio(mc.NumBands() - 1, 8.0)
    mc.SetBandConfig(1, {"KneeDB": 0.0, "AttackMs": 0.5, "Ratio": 0, "MakeupGainDB": 1.5})
    return mc


SETUPS = {"defaults": (setup_defaults, None), "band table": (setup_table, None), "all bands": (setup_all_bands, None),
          "changed before call 3": (setup_table, change_before_call_3)}


def multi_ref(name, channels, setup, change):
    freqs, order = CONFIGS[name]
    x = noise(channels)
    refs = [setup(R.MultibandCompressor(freqs, order, FS)) for _ in range(channels)]
    out = []
    for i, (a, b) in enumerate(edges(CUTS)):
        if i == 2 and change:
            for r in refs:
                change(r)
        bands = np.stack([r.ProcessInPlaceMulti(x[c, a:b]) for c, r in enumerate(refs)], axis=1)
        out.append((bands, [r.GetMetrics() for r in refs]))
    return refs, out


@functools.lru_cache(maxsize=None)
def multi_ref_cached(name, channels, setup_name):
    return multi_ref(name, channels, *SETUPS[setup_name])


def channels_for(name, setup_name):
    """One past a wave once per kernel shape; elsewhere the settings change constants only."""
    return 65 if setup_name == "band table" and name in ("2 bands LR2", "8 bands LR24") else 3


@pytest.mark.parametrize("setup_name", list(SETUPS))
@pytest.mark.parametrize("name", COMP_CONFIGS)
def test_multiband_per_band(gpu, name, setup_name):
    per_band_case(name, setup_name, channels_for(name, setup_name))


@pytest.mark.parametrize("name,setup_name,channels", [
    ("3 bands LR6", "band table", 1), ("8 bands LR24", "defaults", 1), ("2 bands LR4", "changed before call 3", 1),
    ("3 bands LR8", "changed before call 3", 65), ("8 bands LR4", "all bands", 65), ("3 bands LR6", "defaults", 65)])
def test_multiband_per_band_channel_counts(gpu, name, setup_name, channels):
    """One channel and one past a wave, at settings and networks the case above runs at 3 channels."""
    per_band_case(name, setup_name, channels)


def per_band_case(name, setup_name, channels):
    freqs, order = CONFIGS[name]
    setup, change = SETUPS[setup_name]
    x = noise(channels)
    refs, want = multi_ref_cached(name, channels, setup_name)
    h = setup(P.MultibandCompressor(freqs, order, FS, channels))
    for i, ((a, b), (bands, metrics)) in enumerate(zip(edges(CUTS), want)):
        if i == 2 and change:
            change(h)
        blk = x[:, a:b].copy()
        got = h.ProcessInPlaceMulti(blk)
        same_bits(blk, x[:, a:b], "the input is not written")
        for k in range(len(freqs) + 1):
            within_bars(got[k], bands[k], f"{name} / {setup_name}: band {k} of call [{a}, {b})")
        for c in sorted({0, channels - 1}):
            np.testing.assert_allclose(np.array(h.GetMetrics(c)), np.array(metrics[c]), rtol=METRICS_RTOL, atol=0,
                                       err_msg=f"{name} / {setup_name}: metrics of channel {c} after {b}")
    ref_cfg = refs[0].Band(0)
    view = h.Band(0)
    assert all(getattr(view, k) == v for k, v in ref_cfg.items()), (ref_cfg, view)
    same_bits(np.stack([h.xover_state(c) for c in range(channels)]),
              xover_ref_cached(name, channels)[-1][1], f"{name}: crossover state")


@pytest.mark.parametrize("name,channels", [(k, 3) for k in COMP_CONFIGS] + [
    ("2 bands LR2", 1), ("8 bands LR4", 1), ("3 bands LR6", 65), ("8 bands LR24", 65)])
def test_multiband_sum(gpu, name, channels):
    """ProcessInPlace is the band-order sum of ProcessInPlaceMulti on bits, and within the triangle-inequality
    bars of the restatement end to end."""
    freqs, order = CONFIGS[name]
    nb = len(freqs) + 1
    x = noise(channels)
    _, want = multi_ref_cached(name, channels, "band table")
    a_, b_ = setup_table(P.MultibandCompressor(freqs, order, FS, channels)), \
        setup_table(P.MultibandCompressor(freqs, order, FS, channels))
    for (a, b), (bands, _) in zip(edges(CUTS), want):
        y = x[:, a:b].copy()
        a_.ProcessInPlace(y)
        per_band = b_.ProcessInPlaceMulti(x[:, a:b].copy())
        acc = per_band[0].copy()
        for k in range(1, nb):
            acc += per_band[k]
        same_bits(y, acc, f"{name}: sum of call [{a}, {b})")
        ref = bands[0].copy()
        for k in range(1, nb):
            ref += bands[k]
        err = y - ref
        bar = RMS_BAR * sum(rms(bands[k]) for k in range(nb))
        print(f"{name} call [{a}, {b}): rms error {rms(err):.3e} (bar {bar:.3e}), max abs {np.max(np.abs(err)):.3e}")
        assert float(np.max(np.abs(err))) <= nb * ABS_BAR and rms(err) <= bar
    z = np.zeros((channels, 64))
    z[:, ::2] = -0.0
    y = z.copy()
    P.MultibandCompressor((1000.0,), 4, FS, channels).ProcessInPlace(y)
    want0 = np.stack([R.MultibandCompressor((1000.0,), 4, FS).ProcessInPlace(z[c]) for c in range(channels)])
    same_bits(y, want0, "zeros in, the restatement's zeros out")


def test_multiband_process_device_layouts(gpu):
    name, C_ = "3 bands LR6", 3
    freqs, order = CONFIGS[name]
    x, nb = noise(C_), 3

    def run(layout):
        h = setup_table(P.MultibandCompressor(freqs, order, FS, C_))
        buf = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        h.process_device(buf.ptr, buf.stride, 700)
        h.process_device(buf.ptr + 8 * 700, buf.stride, 801)
        torch.cuda.synchronize()
        LL.check_guards(buf)
        m = setup_table(P.MultibandCompressor(freqs, order, FS, C_))
        src, dst = LL.place(x, layout, DEV), LL.empty(nb * C_, N, layout, DEV)
        torch.cuda.synchronize()
        m.process_multi_device(src.ptr, src.stride, dst.ptr, dst.stride, C_ * dst.stride, N)
        torch.cuda.synchronize()
        LL.check_guards(dst)
        LL.check_unchanged(src, x)
        return LL.payload(buf), LL.payload(dst).reshape(nb, C_, N)

    want = run(LL.LA(N))
    for layout in LL.variants(N):
        got = run(layout)
        same_bits(got[0], want[0], f"in place, {layout}")
        same_bits(got[1], want[1], f"per band, {layout}")
    h = P.MultibandCompressor(freqs, order, FS, C_)
    buf = LL.place(x, LL.L1, DEV)
    torch.cuda.synchronize()
    for args in ((buf.ptr, N - 1, N), (0, buf.stride, N), (buf.ptr, buf.stride, -1)):
        with pytest.raises(_lib.ErrInvalidArgument):
            h.process_device(*args)
    h.process_device(buf.ptr, buf.stride, 0)
    torch.cuda.synchronize()
    LL.check_unchanged(buf, x)


def test_multiband_metrics_and_reset_metrics(gpu):
    name, channels = "3 bands LR8", 3
    freqs, order = CONFIGS[name]
    x = noise(channels)
    _, want = multi_ref_cached(name, channels, "band table")
    xo = xover_ref_cached(name, channels)
    h, twin = (setup_table(P.MultibandCompressor(freqs, order, FS, channels)) for _ in range(2))
    (a, b), (a1, b1), (a2, b2) = edges(CUTS)
    for m in (h, twin):
        m.ProcessInPlaceMulti(x[:, a:b].copy())
        m.ProcessInPlaceMulti(x[:, a1:b1].copy())
    for c in range(channels):
        np.testing.assert_allclose(np.array(h.GetMetrics(c)), np.array(want[1][1][c]), rtol=METRICS_RTOL, atol=0)
    h.ResetMetrics()  # :547-551: CompressorMetrics{GainReduction: 1.0}
    for c in range(channels):
        assert h.GetMetrics(c) == [(0.0, 0.0, 1.0)] * 3
        assert twin.GetMetrics(c) != [(0.0, 0.0, 1.0)] * 3
    got, other = (m.ProcessInPlaceMulti(x[:, a2:b2].copy()) for m in (h, twin))
    same_bits(got, other, "the audio state is not touched by ResetMetrics")
    for c in range(channels):
        for k, (ip, op, gr) in enumerate(h.GetMetrics(c)):  # the peaks since the reset, exactly
            assert ip == float(np.max(np.abs(xo[2][0][k, c]))) and op == float(np.max(np.abs(got[k, c])))
            assert 0.0 < gr <= 1.0
    h.Reset()  # :528-534
    fresh = setup_table(P.MultibandCompressor(freqs, order, FS, channels))
    same_bits(h.ProcessInPlaceMulti(x[:, a:b].copy()), fresh.ProcessInPlaceMulti(x[:, a:b].copy()), "after Reset")
    assert h.GetMetrics(1) == fresh.GetMetrics(1)


@pytest.mark.parametrize("name,channels", [("2 bands LR2", 3), ("8 bands LR24", 3), ("3 bands LR6", 1),
                                           ("8 bands LR4", 65)])
def test_multiband_chunking(gpu, name, channels):
    """A call cut into passes of 256 samples carries every state: the crossover on bits, the compressors within
    their bars of the uncut call."""
    freqs, order = CONFIGS[name]
    nb = len(freqs) + 1
    x = noise(channels)
    xo = np.concatenate([b for b, _ in xover_ref_cached(name, channels)], axis=2)
    for chunk in (256, 0):  # ratio 1, no makeup: each band leaves its compressor as it came from the crossover
        h = P.MultibandCompressor(freqs, order, FS, channels)
        for k in range(nb):
            h.SetBandRatio(k, 1.0)
            h.SetBandMakeupGain(k, 0.0)
        h.SetChunk(chunk)
        same_bits(h.ProcessInPlaceMulti(x.copy()), xo, f"{name}: crossover bands, chunk {chunk}")
        same_bits(np.stack([h.xover_state(c) for c in range(channels)]), xover_ref_cached(name, channels)[-1][1],
                  f"{name}: crossover state, chunk {chunk}")
    cut, whole = (setup_table(P.MultibandCompressor(freqs, order, FS, channels)) for _ in range(2))
    cut.SetChunk(256)
    got, want = cut.ProcessInPlaceMulti(x.copy()), whole.ProcessInPlaceMulti(x.copy())
    for k in range(nb):
        within_bars(got[k], want[k], f"{name}: band {k}, 256-sample passes against one pass")
    y, y2 = x.copy(), x.copy()
    cut.Reset(), whole.Reset()
    cut.ProcessInPlace(y), whole.ProcessInPlace(y2)
    assert float(np.max(np.abs(y - y2))) <= nb * ABS_BAR
    with pytest.raises(_lib.ErrInvalidArgument):
        cut.SetChunk(-1)


def test_multiband_setter_semantics(gpu):
    freqs, order = CONFIGS["3 bands LR6"]
    x = noise(3)
    h, twin = (setup_table(P.MultibandCompressor(freqs, order, FS, 3)) for _ in range(2))
    before = [{n: getattr(h.Band(b), n) for n, _ in _lib.CompressorConfig._fields_} for b in range(3)]
    for call in (lambda: h.SetBandRatio(0, 0.5), lambda: h.SetBandThreshold(1, NAN), lambda: h.SetBandKnee(2, -1.0),
                 lambda: h.SetBandAttack(0, 0.01), lambda: h.SetBandRelease(0, 0.1), lambda: h.SetBandRMSWindow(1, 0.5),
                 lambda: h.SetBandSidechainLowCut(0, 7000.0), lambda: h.SetBandTopology(0, 2),
                 lambda: h.SetBandConfig(2, {"Ratio": 200.0})):
        with pytest.raises(_lib.ErrInvalidArgument):
            call()
    for call in (lambda: h.SetBandThreshold(-1, -20.0), lambda: h.SetBandRatio(3, 2.0), lambda: h.SetBandConfig(5, {}),
                 lambda: h.Band(3), lambda: h.SetBandMakeupGain(7, 1.0)):
        with pytest.raises(_lib.ErrInvalidArgument):
            call()
    assert before == [{n: getattr(h.Band(b), n) for n, _ in _lib.CompressorConfig._fields_} for b in range(3)]
    same_bits(h.ProcessInPlaceMulti(x.copy()), twin.ProcessInPlaceMulti(x.copy()), "rejected values change nothing")
    # SetBandConfig stops at the first field that is rejected: the ones before it stay (applyBandConfig :563-658)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.SetBandConfig(0, {"ThresholdDB": -12.0, "Ratio": 0.5, "KneeDB": 9.0})
    assert (h.Band(0).Threshold(), h.Band(0).Ratio(), h.Band(0).Knee()) == (-12.0, before[0]["ratio"], before[0]["knee_db"])
    # SetAllBands* stops at the first band that rejects: the bands before it stay changed (:331-437)
    h.SetBandSidechainHighCut(1, 100.0)
    with pytest.raises(_lib.ErrInvalidArgument):
        h._all("SetBandSidechainLowCut", 150.0)
    assert [h.Band(b).SidechainLowCut() for b in range(3)] == [150.0, 0.0, 0.0]
    h.SetBandMakeupGain(1, 2.0)
    assert not h.Band(1).AutoMakeup() and h.Band(1).MakeupGain() == 2.0
    with pytest.raises(AttributeError):
        h.Band(1).ratio = 3.0
    assert (h.NumBands(), h.CrossoverFreqs(), h.CrossoverOrder(), h.SampleRate()) == (3, list(freqs), order, FS)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.MultibandCompressor(freqs, order, FS, 1, configs=[{}, {}])
    with pytest.raises(_lib.ErrInvalidArgument):
        P.MultibandCompressor((10.0,), 4, FS, 1)
    made = P.MultibandCompressor((1000.0,), 4, FS, 1, configs=[{"ThresholdDB": -30.0, "KneeDB": 0.0}, {"Ratio": 0}])
    assert (made.Band(0).Threshold(), made.Band(0).Knee(), made.Band(1).Ratio()) == (-30.0, 0.0, made.Band(0).Ratio())


def test_dyn_multiband_node_is_still_refused(gpu):
    """The scope of this processor: the graph runtime has no dyn-multiband node yet."""
    graph = E._graph_json([{"id": "m", "type": "dyn-multiband"}],
                          [(E.INPUT_NODE_ID, "m"), ("m", E.OUTPUT_NODE_ID)])
    with pytest.raises(E.UnknownEffect):
        E.Chain(FS, 2).LoadGraph(graph)
