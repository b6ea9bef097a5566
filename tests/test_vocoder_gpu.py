"""The GPU vocoder against the restatement in tests/vocoder_ref.py, on float64
bits in every mode: the device computes no transcendental, and the host tables
come from the same C library as the restatement's.

Shapes: the kernel walks chunks of 64 samples, so total lengths 1, 7, 63, 64,
65 and 3 * 64 + 5; channels 1, 2, 3, 65 and 130 (a workgroup is one channel, so
these are grid sizes; 65 and 130 also cross the older one-channel-per-lane
boundaries).  The vocoder is causal and its channels are independent, so one
reference per configuration, 130 channels by 197 samples, serves every shape as
a prefix.  Distinct noise per channel; the three levels are set so that every
term of the mix is live.
"""
import functools

import numpy as np
import pytest
import torch

import vocoder_ref as R
from algodsp import _lib, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 48000.0
TILE = 64
LENGTHS = [1, 7, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
CHANNELS = [1, 2, 3, 65, 130]
LEVELS = dict(inputLevel=0.3, synthLevel=0.2, vocoderLevel=1.5)
GPU_LEVELS = dict(input_level=0.3, synth_level=0.2, vocoder_level=1.5)
NAN, INF = float("nan"), float("inf")


def noise(n, channels, seed):
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(got, want, what=""):
    """Bit patterns, the sign of zero included; a NaN by position only."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(-1) & ~gn.reshape(-1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at flat index {i}: "
                             f"got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def gpu_process(h, m, c, alias="sep", pad=0):
    """One device call on rows of stride n + pad; the padding is filled with a sentinel and checked."""
    ch, n = m.shape
    sentinel = -777.25

    def rows(x):
        t = torch.full((ch, n + pad), sentinel, dtype=torch.float64, device=DEV)
        if x is not None:
            t[:, :n] = torch.from_numpy(np.array(x, dtype=np.float64)).to(DEV)
        return t

    dm, dc = rows(m), rows(c)
    do = {"mod": dm, "car": dc, "sep": rows(None)}[alias]
    h.process(dm[:, :n], dc[:, :n], do[:, :n])
    torch.cuda.synchronize()
    for t in (dm, dc, do):
        assert bool((t[:, n:] == sentinel).all()), "padding written"
    if alias != "mod":
        same_bits(dm[:, :n].cpu().numpy(), m, "the modulator rows are read only")
    if alias != "car":
        same_bits(dc[:, :n].cpu().numpy(), c, "the carrier rows are read only")
    return do[:, :n].cpu().numpy()


def gpu_blocks(h, m, c, cuts, alias="mod"):
    out = np.empty_like(m)
    pos = 0
    for k in cuts:
        out[:, pos:pos + k] = gpu_process(h, m[:, pos:pos + k], c[:, pos:pos + k], alias)
        pos += k
    assert pos == m.shape[1]
    return out


@functools.lru_cache(maxsize=None)
def shared(downsample: bool):
    """Modulator, carrier and the reference output, 130 channels by 197 samples (read only)."""
    n, ch = LENGTHS[-1], CHANNELS[-1]
    m, c = noise(n, ch, 0x70C0), noise(n, ch, 0xCA44)
    want = R.Vocoder(FS, channels=ch, downsample=downsample, **LEVELS).process_many(m, c)
    for a in (m, c, want):
        a.setflags(write=False)
    return m, c, want


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(gpu, channels, n, downsample):
    m, c, want = shared(downsample)
    h = P.Vocoder(FS, channels, downsample=downsample, **GPU_LEVELS)
    got = gpu_process(h, m[:channels, :n], c[:channels, :n])
    same_bits(got, want[:channels, :n], f"{channels} ch, n {n}, downsampling {downsample}")


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("channels", [3, 65])
def test_uneven_blocks_equal_one_call(gpu, channels, downsample):
    """Blocks of 1, 130, 63 and the rest: no block is a multiple of 128 (downsampleMax at 48 kHz), so the
    counter and every state cross call boundaries at odd phases."""
    n = 1 + 130 + 63 + 107
    m, c = noise(n, channels, 0xB10C), noise(n, channels, 0xB20C)
    want = R.Vocoder(FS, channels=channels, downsample=downsample, **LEVELS).process_many(m, c)
    one = gpu_process(P.Vocoder(FS, channels, downsample=downsample, **GPU_LEVELS), m, c)
    same_bits(one, want, "one call")
    h = P.Vocoder(FS, channels, downsample=downsample, **GPU_LEVELS)
    same_bits(gpu_blocks(h, m, c, [1, 130, 63, 107]), want, "uneven blocks")
    if downsample:
        assert h.get_state(0)[1] == n % 128


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("alias", ["sep", "mod", "car"])
def test_aliasing_and_stride(gpu, alias, downsample):
    m, c, want = shared(downsample)
    ch, n = 3, LENGTHS[-1]
    h = P.Vocoder(FS, ch, downsample=downsample, **GPU_LEVELS)
    same_bits(gpu_process(h, m[:ch, :n], c[:ch, :n], alias, pad=11), want[:ch, :n], f"out is {alias}, stride n + 11")


def test_same_rows_for_both_inputs(gpu):
    """The graph's node without a side parent: modulator, carrier and out are one buffer."""
    n, ch = 150, 3
    x = noise(n, ch, 0x5A3E)
    want = R.Vocoder(FS, channels=ch, **LEVELS).process_many(x, x)
    h = P.Vocoder(FS, ch, **GPU_LEVELS)
    d = torch.from_numpy(x).to(DEV)
    assert h.process(d, d) is d
    torch.cuda.synchronize()
    same_bits(d.cpu().numpy(), want, "one buffer")


def test_overlapping_out_is_refused(gpu):
    h = P.Vocoder(FS, 2)
    d = torch.zeros((2, 64), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process(d[:, :32], d[:, 32:], d[:, 8:40])
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process(d[:, :32], d[:, :16])


CONFIGS = [(fs, layout, q) for fs in (48000.0, 44100.0, 8000.0) for layout in (R.THIRD_OCTAVE, R.BARK)
           for q in (None, 2.5)] + [(100.0, R.THIRD_OCTAVE, None)]
BANDS = {(48000.0, 0): 32, (48000.0, 1): 24, (44100.0, 0): 31, (44100.0, 1): 24, (8000.0, 0): 24, (8000.0, 1): 16,
         (100.0, 0): 5}


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("fs,layout,q", CONFIGS)
def test_layouts_rates_and_q(gpu, fs, layout, q, downsample):
    n, ch = 150, 3
    m, c = noise(n, ch, 0x1A70), noise(n, ch, 0x2A70)
    kw = {} if q is None else {"synthQ": q}
    gkw = {} if q is None else {"synth_q": q}
    ref = R.Vocoder(fs, channels=ch, layout=layout, downsample=downsample, attackMs=0.2, releaseMs=7.0, **LEVELS, **kw)
    h = P.Vocoder(fs, ch, layout=layout, downsample=downsample, attack_ms=0.2, release_ms=7.0, **GPU_LEVELS, **gkw)
    assert h.NumBands() == ref.NumBands() == BANDS[(fs, layout)]
    assert h.DownsampleFactors() == ref.DownsampleFactors()
    d = h.derived()
    same_bits(d["analysis"], ref.analysisCoeffs, "analysis sections")
    same_bits(d["synthesis"], ref.synthesisCoeffs, "synthesis sections")
    if downsample:
        same_bits(d["decimated"], ref.downsampleAnalysisCoeffs, "decimated sections")
        same_bits(d["antialias"], ref.downsampleGroupAACoeffs, "anti-alias sections")
        same_bits(d["ds_attack"], ref.downsampleAttackCoeffs, "decimated attack")
        same_bits(d["ds_release"], ref.downsampleReleaseCoeffs, "decimated release")
    same_bits(gpu_blocks(h, m, c, [70, 80]), ref.process_many(m, c), f"fs {fs}, layout {layout}, Q {q}")


def test_setters_between_blocks(gpu):
    """SetDownsampling toggled (on, on again, off), SetSampleRate, the times, the levels and Reset between
    blocks: each keeps and clears exactly what the restatement's does."""
    ch, blk = 3, 90
    steps = [("SetDownsampling", True), ("SetDownsampling", True), ("SetAttack", 3.0), ("SetDownsampling", False),
             ("SetRelease", 40.0), ("SetSampleRate", 44100.0), ("SetDownsampling", True), ("SetSampleRate", 8000.0),
             ("SetInputLevel", 1.0), ("SetSynthLevel", 0.0), ("SetVocoderLevel", 10.0), ("Reset", None),
             ("SetDownsampling", False)]
    n = blk * (len(steps) + 1)
    m, c = noise(n, ch, 0x5E77), noise(n, ch, 0x5E99)
    ref = R.Vocoder(FS, channels=ch, layout=R.BARK, **LEVELS)
    h = P.Vocoder(FS, ch, layout=P.Vocoder.BARK, **GPU_LEVELS)
    for i in range(len(steps) + 1):
        s = slice(i * blk, (i + 1) * blk)
        got = gpu_process(h, m[:, s], c[:, s], "mod")
        same_bits(got, ref.process_many(m[:, s], c[:, s]), f"block {i}, after {steps[:i][-1:]}")
        assert h.NumBands() == ref.NumBands() and h.DownsampleFactors() == ref.DownsampleFactors()
        if i < len(steps):
            name, v = steps[i]
            for o in (ref, h):
                getattr(o, name)(*([] if v is None else [v]))


SPECIALS = [INF, -INF, NAN, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1e-310, 1e308, -1e308]


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("where", ["modulator", "carrier"])
def test_nonfinite_channel_stays_in_its_channel(gpu, where, downsample):
    """Channel 1 carries +-inf, NaN, +-0 and denormals; it agrees on NaN positions and on bits elsewhere, and
    its neighbours, which share its wave's product tiles with nobody and its launch with it, are bit-exact."""
    m, c, want = shared(downsample)
    ch, n = 3, LENGTHS[-1]
    m, c = m[:ch, :n].copy(), c[:ch, :n].copy()
    row = m if where == "modulator" else c
    row[1, 20:20 + len(SPECIALS)] = SPECIALS
    row[1, 100:104] = [0.0, -0.0, 5e-324, NAN]
    ref = R.Vocoder(FS, channels=ch, downsample=downsample, **LEVELS).process_many(m, c)
    got = gpu_process(P.Vocoder(FS, ch, downsample=downsample, **GPU_LEVELS), m, c)
    same_bits(got, ref, f"specials in the {where}")
    same_bits(got[[0, 2]], want[[0, 2], :n], "the neighbours")
    assert np.isnan(got[1]).any()


def test_channel_order(gpu):
    """Distinct data per channel: every output row matches its own channel's reference and no other's."""
    m, c, want = shared(False)
    ch, n = 65, 130
    got = gpu_process(P.Vocoder(FS, ch, **GPU_LEVELS), m[:ch, :n], c[:ch, :n])
    for a in range(ch):
        same = [b for b in range(ch) if np.array_equal(bits(got[a]), bits(want[b, :n]))]
        assert same == [a], (a, same)


def test_host_rows(gpu):
    m, c, want = shared(True)
    h = P.Vocoder(FS, 2, downsample=True, **GPU_LEVELS)
    same_bits(h.ProcessBlock(m[:2, :100].copy(), c[:2, :100].copy()), want[:2, :100], "ProcessBlock")
    with pytest.raises(TypeError):
        h.ProcessInPlace(np.zeros((2, 8)))


def test_refused_values_change_nothing(gpu):
    h = P.Vocoder(FS, 2, layout=P.Vocoder.BARK, downsample=True)
    fields = lambda: tuple(getattr(h.config(), k) for k, _ in _lib.VocoderConfig._fields_)  # noqa: E731
    before = fields()
    for name, v in [("SetAttack", 0.005), ("SetAttack", 100.5), ("SetAttack", NAN), ("SetRelease", 0.001),
                    ("SetRelease", 1000.5), ("SetRelease", INF), ("SetInputLevel", -0.1), ("SetInputLevel", 10.5),
                    ("SetSynthLevel", NAN), ("SetVocoderLevel", 11.0), ("SetSampleRate", 0.0), ("SetSampleRate", -1.0),
                    ("SetSampleRate", NAN), ("SetSampleRate", INF), ("SetSampleRate", 100.0)]:
        with pytest.raises(_lib.ErrInvalidArgument):
            getattr(h, name)(v)
        assert fields() == before and h.NumBands() == 24, (name, v)
    for kw in (dict(layout=2), dict(synth_q=0.05), dict(synth_q=20.5), dict(attack_ms=0.0), dict(release_ms=2000.0),
               dict(input_level=-1.0), dict(synth_level=11.0), dict(vocoder_level=NAN)):
        with pytest.raises(_lib.ErrInvalidArgument):
            P.Vocoder(FS, 1, **kw)
    with pytest.raises(_lib.ErrInvalidArgument) as e:
        P.Vocoder(100.0, 1, layout=P.Vocoder.BARK)
    assert "no usable Bark bands" in str(e.value)
    # the getters
    h = P.Vocoder(44100.0, 1, synth_q=3.0, attack_ms=1.5, release_ms=9.0, **GPU_LEVELS)
    assert (h.SampleRate(), h.Layout(), h.SynthesisQ(), h.Attack(), h.Release()) == (44100.0, 0, 3.0, 1.5, 9.0)
    assert (h.InputLevel(), h.SynthLevel(), h.VocoderLevel(), h.Downsampling()) == (0.3, 0.2, 1.5, False)
    assert h.DownsampleFactors() is None and h.NumBands() == 31
    h.SetDownsampling(True)
    f = h.DownsampleFactors()
    assert h.Downsampling() and len(f) == 31 and f[0] == 128 and f[-1] == 1


def test_kernel_info(gpu):
    lanes, tile, lds = P.Vocoder(FS, 1).kernel_info()
    assert (lanes, tile) == (64, TILE)
    assert lds == (2 * TILE + 2 * 32 * (TILE + 1)) * 8 == 34304
