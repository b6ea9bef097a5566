"""algodsp.pitch.PitchShifter on the GPU against tests/pitchtime_ref.py.

The search's argmax is discontinuous: one ulp in a score can select another
candidate, and from there the block differs by whole samples.  So every
comparison is on the bit patterns of every sample of every channel; there is no
tolerance anywhere in this file.

Most cases run at fs = 8000 with the smallest parameters the setters take
(sequence 20 ms = 160 samples, overlap 4 ms = 32, search 2 ms = 16), where a
reference run is milliseconds; the cases that need a size say which.
"""
import math

import numpy as np
import pytest
import torch

import pitchtime_ref as R
from algodsp import _lib, pitch

pytestmark = pytest.mark.gpu

SMALL = dict(sequence_ms=20.0, overlap_ms=4.0, search_ms=2.0)
RATIOS = [0.25, 0.5, math.pow(2, -5 / 12.0), 1 - 1e-9, 1 + 2e-9, math.pow(2, 7 / 12.0), 4.0]
PAD = 7.25  # what the rows hold past n


def noise(channels, n, seed):
    return 0.5 * np.random.default_rng(seed).standard_normal((channels, n))


def reference(fs, ratio, x, sequence_ms=82.0, overlap_ms=10.0, search_ms=28.0):
    """Every row of x through its own reference instance."""
    r = R.PitchShifter(fs)
    r.SetSequence(sequence_ms), r.SetOverlap(overlap_ms), r.SetSearch(search_ms), r.SetPitchRatio(ratio)
    return np.stack([r.Process(row) for row in x]) if x.shape[1] else x.copy()


def same(got, want, nan=False):
    """Equal on bits; with `nan`, NaN where the reference has NaN and equal on bits elsewhere."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    if nan:
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            return False
        got, want = np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want)
    return np.array_equal(got.view(np.uint64), want.view(np.uint64))


def on_device(ps, x, stride=None, stream=None):
    """process_device on rows of `stride` doubles; the padding must come back untouched."""
    channels, n = x.shape
    stride = n if stride is None else stride
    buf = torch.full((channels, stride), PAD, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.from_numpy(x)
    torch.cuda.synchronize()
    if stream is None:
        ps.process_device(buf.data_ptr(), stride, n)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            ps.process_device(buf.data_ptr(), stride, n, stream.cuda_stream)
        stream.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[:, n:] == PAD), "the padding between rows was written"
    return out[:, :n]


def small(ratio, channels, fs=8000.0):
    return pitch.PitchShifter(fs, channels, pitch_ratio=ratio, **SMALL)


@pytest.mark.parametrize("ratio", RATIOS)
def test_ratios_and_lengths(gpu, ratio):
    """n below, at and above one sequence, and n = 0, 1, 2, 7: the zero-padded reads and both short
    branches of the resample (targetLen == 1, n == 1)."""
    ps = small(ratio, 3)
    for n in (0, 1, 2, 7, 159, 160, 161, 4096):
        x = noise(3, n, 100 + n)
        want = reference(8000.0, ratio, x, **SMALL)
        got = x.copy()
        ps.ProcessInPlace(got)
        assert same(got, want), f"host call, n = {n}"
        if n:
            assert same(on_device(ps, x, stride=n + 5), want), f"device call, n = {n}"
    if abs(ratio - 1) <= 1e-9:
        assert same(want, x)  # the identity leaves every bit


@pytest.fixture(scope="module")
def many():
    x = noise(130, 2048, 7)
    return x, reference(8000.0, RATIOS[5], x, **SMALL)


@pytest.mark.parametrize("channels", [65, 130])
def test_many_channels_strided_rows_and_streams(gpu, many, channels):
    x, want = many[0][:channels], many[1][:channels]
    ps = small(RATIOS[5], channels)
    assert same(on_device(ps, x, stride=2048 + 24), want)
    assert same(on_device(ps, x, stride=2048 + 3, stream=torch.cuda.Stream()), want)  # rows 8 bytes off alignment
    assert same(ps.Process(x), want)


def test_identity_keeps_nan_payloads_and_signed_zeros(gpu):
    x = noise(2, 300, 3)
    x[0, 5], x[0, 6], x[1, 0] = -0.0, np.float64(np.nan), np.inf
    x[1, 7:9] = np.array([0x7FF8000000000123, 0xFFF0000000000000], dtype=np.uint64).view(np.float64)
    ps = small(1 + 1e-10, 2)
    bits = x.view(np.uint64).copy()
    assert np.array_equal(ps.Process(x).view(np.uint64), bits)
    assert np.array_equal(on_device(ps, x, stride=301).view(np.uint64), bits)


def test_selection_edges(gpu):
    n = 2048
    t = np.arange(n)
    x = np.zeros((6, n))
    # 0: silence, every score is 0 / sqrt(1e-24): the lowest candidate wins
    x[1] = np.where((t // 2) % 2 == 0, 1.0, -1.0)  # period 4 divides the range: exact ties, the lowest wins
    x[2] = np.where((t // 4) % 2 == 0, 1.0, -1.0)  # period 8
    x[3] = noise(1, n, 11)[0]
    x[3, 700] = np.inf  # scores of the frames that see it are NaN: nothing wins, predicted stays
    x[4] = noise(1, n, 12)[0]
    x[4, 900] = np.nan
    x[5] = noise(1, n, 13)[0]
    x[5, 1024:] *= 1e-310  # a denormal tail: the energies stay at 1e-12
    for ratio in (0.5, RATIOS[5], 4.0):
        want = reference(8000.0, ratio, x, **SMALL)
        ps = small(ratio, 6)
        assert same(ps.Process(x), want, nan=True), f"ratio {ratio}"
        assert same(on_device(ps, x), want, nan=True), f"ratio {ratio}, device"


@pytest.mark.parametrize("name,fs,params,n,channels,ratio", [
    # the largest LDS window the setters allow at 48 kHz: 5760 / 2880 / 1920, three refills of the term window
    ("maxima", 48000.0, dict(sequence_ms=120.0, overlap_ms=60.0, search_ms=40.0), 16384, 2, RATIOS[5]),
    # 10753 candidates of 1920 terms: eleven candidate tiles, two refills
    ("tiled", 192000.0, dict(sequence_ms=82.0, overlap_ms=10.0, search_ms=28.0), 32768, 1, 2.0),
    ("defaults", 48000.0, dict(sequence_ms=82.0, overlap_ms=10.0, search_ms=28.0), 16384, 2, math.pow(2, 1 / 12.0)),
])
def test_large_frames(gpu, name, fs, params, n, channels, ratio):
    x = noise(channels, n, 21)
    want = reference(fs, ratio, x, **params)
    ps = pitch.PitchShifter(fs, channels, pitch_ratio=ratio, **params)
    assert same(ps.Process(x), want)


def test_channel_groups(gpu):
    """A call whose stretched rows pass the scratch bound runs in channel groups: 65 channels of 2^20 samples at
    ratio 4 are 65 rows of 33.6 MB against 2 GiB, so 63 channels and then 2.  Two distinct signals alternate
    over the channels, so both groups hold both.  The one case here that needs a size: a second of reference."""
    n, params = 1 << 20, dict(sequence_ms=120.0, overlap_ms=4.0, search_ms=2.0)
    two = noise(2, n, 31)
    want = reference(8000.0, 4.0, two, **params)
    x = np.ascontiguousarray(two[np.arange(65) % 2])
    ps = pitch.PitchShifter(8000.0, 65, pitch_ratio=4.0, **params)
    got = on_device(ps, x)
    for c in range(65):
        assert same(got[c], want[c % 2]), f"channel {c}"


def test_position_row_is_cached_per_length(gpu):
    ps = small(RATIOS[2], 2)
    xa, xb = noise(2, 1500, 41), noise(2, 900, 42)
    xc = noise(2, 1500, 43)
    for x in (xa, xb, xc, xa):  # 1500, 900, then 1500 again
        assert same(ps.Process(x), reference(8000.0, RATIOS[2], x, **SMALL))
    ps.SetPitchRatio(0.5)  # another targetLen for the same n
    assert same(ps.Process(xa), reference(8000.0, 0.5, xa, **SMALL))


def test_setter_error_leaves_the_outputs(gpu):
    ps = small(RATIOS[5], 2)
    x = noise(2, 1000, 51)
    before = ps.Process(x)
    for call, value in ((ps.SetOverlap, 30.0), (ps.SetPitchRatio, 5.0), (ps.SetSequence, 10.0), (ps.SetSearch, 1.0),
                        (ps.SetSampleRate, float("nan")), (ps.SetPitchSemitones, 30.0), (ps.SetOverlap, float("nan"))):
        with pytest.raises(_lib.ErrInvalidArgument):
            call(value)
    assert (ps.PitchRatio(), ps.Sequence(), ps.Overlap(), ps.Search(), ps.SampleRate()) == \
        (RATIOS[5], 20.0, 4.0, 2.0, 8000.0)
    assert same(ps.Process(x), before)
    ps.SetPitchSemitones(-5)
    ps.SetSequence(30.0)
    assert ps.PitchRatio() == RATIOS[2] and abs(ps.PitchSemitones() + 5) < 1e-12
    assert same(ps.Process(x), reference(8000.0, RATIOS[2], x, sequence_ms=30.0, overlap_ms=4.0, search_ms=2.0))
    ps.Reset()
    assert same(ps.Process(x), reference(8000.0, RATIOS[2], x, sequence_ms=30.0, overlap_ms=4.0, search_ms=2.0))


def test_in_place_and_copy_agree(gpu):
    ps = small(RATIOS[5], 3)
    x = noise(3, 3000, 61)
    out = ps.Process(x)
    assert out is not x and same(x, noise(3, 3000, 61))  # Process leaves its input
    buf = x.copy()
    assert ps.ProcessInPlace(buf) is buf and same(buf, out)
    one = pitch.PitchShifter(8000.0, 1, pitch_ratio=RATIOS[5], **SMALL)
    row = x[0].copy()  # a 1-d block on a one-channel processor
    one.ProcessInPlace(row)
    assert same(row, out[0])
