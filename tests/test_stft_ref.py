"""The restatement in tests/stft_ref.py held to the reference's own properties,
and the bars and decision margins of every case tests/test_stft_gpu.py runs
(tests/stft_cases.py).  No GPU.
"""
import math

import numpy as np
import pytest

import stft_cases as K
import stft_ref as R

FS = K.FS


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- the window and the tables ------------------------------------------------
def test_hann_periodic():
    w = R.window_periodic(R.TYPE_HANN, 64)
    assert w[0] == 0.0 and w[32] == 1.0
    want = [0.5 + -0.5 * math.cos(1.0 * (2 * math.pi * (i / 64))) for i in range(64)]
    np.testing.assert_allclose(w, want, rtol=0, atol=2e-16)
    assert np.all(R.window_periodic(R.TYPE_RECTANGULAR, 8) == 1.0)
    with pytest.raises(ValueError):
        R.window_periodic(7, 8)


def test_window_matches_the_python_layer():
    from algodsp import processors as P

    for t in range(4):
        np.testing.assert_array_equal(bits(R.window_periodic(t, 256)), bits(P.spectral_window(t, 256)))
    with pytest.raises(ValueError):
        P.spectral_window(6, 64)


# ---- reconstruction and the edge cases ----------------------------------------
@pytest.mark.parametrize("frame,hop,n", [(64, 16, 165), (64, 24, 123), (64, 63, 318), (64, 1, 200)])
def test_unfrozen_reconstructs(frame, hop, n):
    """Polar -> rectangular -> inverse gives the input back to 1e-13 max abs wherever norm > 1e-12.

    At N = 64 only.  Sample 1 is covered by frame 0 alone, so its sum is x w[1]^2 with the round trip's
    error of about eps sqrt(log2 N) rms(frame) w[1] ~ 1e-16 w[1], and the division by norm = w[1]^2 leaves
    1e-16 / w[1].  w[1] ~ (pi / N)^2 is 2.4e-3 at N = 64 and 6e-4 at N = 128: from N = 128 on no float64
    transform meets 1e-13 at that sample, so larger frames are held on the overlap-add sums below."""
    x = K.noise(n, 1)[0]
    r = K.make_freeze(frame, hop)
    y = r.Process(x)
    ok = r.last_norm[:n] > R.NORM_FLOOR
    assert ok.sum() >= n - 2
    assert float(np.max(np.abs(y[ok] - x[ok]))) <= 1e-13


@pytest.mark.parametrize("frame,hop,n", [(256, 96, 549), (1024, 1023, 2085), (4096, 1024, 8229)])
def test_unfrozen_reconstructs_on_the_sums(frame, hop, n):
    """The same bound on (y - x) * norm, the measure of every device comparison, at the larger frames."""
    x = K.noise(n, 1)[0]
    r = K.make_freeze(frame, hop)
    y = r.Process(x)
    norm = r.last_norm[:n]
    ok = norm > R.NORM_FLOOR
    assert ok.sum() >= n - 2
    assert float(np.max(np.abs((y[ok] - x[ok]) * norm[ok]))) <= 1e-13


def test_sample_zero_stays_undivided():
    x = K.noise(300, 1)[0]
    r = K.make_freeze(64, 16)
    y = r.Process(x)
    assert r.last_norm[0] == 0.0  # w[0] = 0 with the periodic Hann
    assert y[0] == r.last_sum[0] * 1.0 and abs(y[0]) < 1e-15  # the undivided sum, not the input


def test_mix_zero_returns_the_inputs_bits():
    x = K.noise(500, 1)[0]
    for frozen in (False, True):
        y = K.make_freeze(256, 64, mix=0.0, frozen=frozen).Process(x)
        np.testing.assert_array_equal(bits(y), bits(x))


@pytest.mark.parametrize("ratio", [1.1, 1.5, 1.2])
def test_silence_gives_exact_zeros(ratio):
    z = np.zeros(700)
    y = K.make_pitch(ratio, 256, 64 if ratio != 1.2 else 2).Process(z)  # 1.5: the no-peak branch; 1.2 at hop 2: no resampling
    assert y.shape == z.shape and np.all(y == 0.0)
    for frozen in (False, True):
        assert np.all(K.make_freeze(256, 64, frozen=frozen).Process(z) == 0.0)


def test_freeze_state_rules():
    x = K.noise(900, 1)[0]
    r = K.make_freeze(256, 64, frozen=True)
    r.Process(x[:300])
    held = r.heldMagnitude.copy()
    r.Process(x[300:600])
    np.testing.assert_array_equal(held, r.heldMagnitude)  # later calls keep the capture
    r.SetFrozen(True)  # no change: nothing cleared
    assert r.hasFrozenFrame
    r.Unfreeze()
    assert not r.hasFrozenFrame
    r.Freeze()
    r.Process(x[600:])
    assert not np.array_equal(held, r.heldMagnitude)
    r.Reset()
    assert not r.hasFrozenFrame and np.all(r.phaseAcc == 0)
    r.SetHopSize(200)
    r.SetFrameSize(128)  # hop >= frame: pulled down to frame / 4
    assert r.hopSize == 32 and not r.hasFrozenFrame and len(r.heldMagnitude) == 65
    for bad in (lambda: r.SetFrameSize(100), lambda: r.SetFrameSize(32), lambda: r.SetHopSize(128),
                lambda: r.SetHopSize(0), lambda: r.SetMix(1.5), lambda: r.SetMix(float("nan")),
                lambda: r.SetPhaseMode(2), lambda: r.SetSampleRate(0)):
        with pytest.raises(ValueError):
            bad()
    assert (r.frameSize, r.hopSize, r.mix, r.phaseMode) == (128, 32, 1.0, R.PHASE_ADVANCE)


def test_phase_hold_and_advance():
    x = K.noise(700, 1)[0]
    hold = K.make_freeze(256, 64, mode=R.PHASE_HOLD, frozen=True)
    hold.Process(x)
    first = hold.phaseAcc.copy()
    hold.Process(x)
    np.testing.assert_array_equal(first, hold.phaseAcc)
    adv = K.make_freeze(256, 64, mode=R.PHASE_ADVANCE, frozen=True)
    adv.Process(x)  # 11 frames: the captured one un-advanced, ten steps
    want = first.copy()
    for _ in range(10):
        want = want + adv.omega * 64.0
    np.testing.assert_array_equal(bits(want), bits(adv.phaseAcc))


# ---- peak assignment ----------------------------------------------------------
def test_nearest_peak_assignment_equals_the_forward_walk():
    rng = np.random.default_rng(7)
    half = 128
    sets = [[5], [1], [127], [3, 4], [10, 11, 12], [10, 20], [10, 21], [1, 127], [2, 4, 6, 8]]  # one peak, adjacent, ties
    for _ in range(1000):
        m = int(rng.integers(1, 40))
        sets.append(sorted(rng.choice(np.arange(1, half), size=m, replace=False).tolist()))
    for peaks in sets:
        np.testing.assert_array_equal(R.nearest_peak_vec(peaks, half), R.nearest_peak_walk(peaks, half), err_msg=str(peaks))
    assert R.nearest_peak_vec([10, 20], half)[15] == 10  # a tie goes to the lower peak


# ---- hops and ratios ------------------------------------------------------------
@pytest.mark.parametrize("ratio,hop,bin_shift", [
    (0.25, 64, False),
    (0.85, 218, False),  # 0.85 - 1 is -0.15000000000000002 in float64: past the threshold
    (1.15, 294, True),   # 1.15 - 1 is 0.1499999999999999: the threshold itself takes the bin-shift path
    (1.1500001, 294, False), (2 ** (7 / 12), 384, False), (4.0, 1024, False)])
def test_synthesis_hop_and_effective_ratio(ratio, hop, bin_shift):
    r = R.SpectralPitchShifter(FS)
    r.SetPitchRatio(ratio)
    assert r.synthesisHop == hop  # round(256 * ratio), whichever path
    assert r.use_bin_shifting() == bin_shift
    assert r.SynthesisHop() == (256 if bin_shift else hop)
    assert r.EffectivePitchRatio() == (ratio if bin_shift else hop / 256)


def test_identity_shortcut_and_setters():
    x = K.noise(600, 1)[0]
    r = R.SpectralPitchShifter(FS)
    for ratio in (1.0, 1 + 5e-10, 1 - 1e-9):
        r.SetPitchRatio(ratio)
        np.testing.assert_array_equal(bits(r.Process(x)), bits(x))
    r.SetPitchRatio(1 + 2e-9)
    assert not np.array_equal(r.Process(x), x)
    for bad in (lambda: r.SetPitchRatio(0), lambda: r.SetPitchRatio(0.1), lambda: r.SetPitchRatio(6),
                lambda: r.SetPitchRatio(float("nan")), lambda: r.SetPitchSemitones(float("nan")),
                lambda: r.SetSampleRate(0), lambda: r.SetFrameSize(1000), lambda: r.SetFrameSize(32),
                lambda: r.SetAnalysisHop(0), lambda: r.SetAnalysisHop(1024)):
        with pytest.raises(ValueError):
            bad()
    r.SetPitchSemitones(7)
    assert r.synthesisHop == 384
    r.SetAnalysisHop(600)
    r.SetFrameSize(512)
    assert r.analysisHop == 128 and r.synthesisHop == round(128 * 2 ** (7 / 12))


def test_stateless_between_calls():
    x = K.noise(549, 1)[0]
    for ratio in (1.1, 1.5):
        r = K.make_pitch(ratio, 256, 64)
        np.testing.assert_array_equal(bits(r.Process(x)), bits(r.Process(x)))


def test_same_hop_stretch_skips_the_resampler():
    r = K.make_pitch(1.2, 64, 2)
    assert not r.use_bin_shifting() and r.synthesisHop == r.analysisHop == 2
    r.resample = None  # would raise if called
    assert r.Process(K.noise(201, 1)[0]).shape == (201,)


# ---- the graph runtimes ------------------------------------------------------------------
@pytest.mark.parametrize("n,want", [(0, 256), (255, 256), (256, 256), (300, 256), (384, 256), (385, 512), (1000, 1024),
                                    (3072, 2048), (3073, 4096), (4096, 4096), (5000, 4096)])
def test_sanitize_frame_size(n, want):
    from algodsp import effectchain as E

    assert R.sanitize_spectral_pitch_frame_size(n) == want == E.sanitize_spectral_frame_size(n)


def test_graph_compiler_follows_the_runtimes():
    """effectchain.spectral_freeze_params / spectral_pitch_params against the restated Configure of both runtimes."""
    from algodsp import effectchain as E

    grid = [{}, {"frameSize": 300, "hopRatio": 0.995}, {"frameSize": 5000, "hopRatio": 0.995}, {"frameSize": 100, "hopRatio": 0.001},
            {"frameSize": 2048, "hopRatio": 0.5, "mix": 1.7, "frozen": 0.49}, {"frameSize": 511.5, "mix": -1, "frozen": 0.5},
            {"frameSize": float("nan"), "hopRatio": float("inf"), "semitones": 30}, {"semitones": -30, "hopRatio": 0.3},
            {"semitones": 2}, {"semitones": 7, "frameSize": 700}]
    for num in grid:
        for mode in (None, "hold", "advance", "other"):
            strs = {} if mode is None else {"phaseMode": mode}
            r = R.spectral_freeze_runtime(K.FS, dict(num), strs)
            c = E.spectral_freeze_params(E.Params("n", "spectral-freeze", num=dict(num), str_=strs), K.FS)[0]
            assert (c.frame_size, c.hop_size, c.mix, c.phase_mode, bool(c.frozen), c.window_type, c.sample_rate) == \
                (r.frameSize, r.hopSize, r.mix, r.phaseMode, r.frozen, r.windowType, r.sampleRate), (num, mode)
        r = R.spectral_pitch_runtime(K.FS, dict(num))
        c, _w, taps = E.spectral_pitch_params(E.Params("n", "pitch-spectral", num=dict(num)), K.FS)
        assert (c.frame_size, c.analysis_hop, c.pitch_ratio, c.resample_quality) == \
            (r.frameSize, r.analysisHop, r.pitchRatio, r.resampleQuality), num
        needs = not r.use_bin_shifting() and r.synthesisHop != r.analysisHop
        assert (taps is not None) == needs
        if needs:
            np.testing.assert_array_equal(taps, r.resample_taps())
    assert R.spectral_freeze_runtime(K.FS, {"frameSize": 300, "hopRatio": 0.995}, {}).hopSize == 253
    assert R.spectral_freeze_runtime(K.FS, {"frameSize": 5000, "hopRatio": 0.995}, {}).hopSize == 4055
    assert R.spectral_freeze_runtime(K.FS, {}, {}).frozen  # frozen defaults to 1


# ---- the pinned choice: bins 0 and N/2 --------------------------------------------
def test_pinned_real_bins_tame_the_bin_shift_path():
    """With the imaginary parts of bins 0 and N/2 free, rounding noise there decides atan2's branch and the
    bin-shift output moves by percents; pinned to +0.0 the same perturbation moves it by ~1e-13."""
    x = K.noise(2085, 1)[0]
    clean = K.make_pitch(1.1, 1024, 256).Process(x)
    r = K.make_pitch(1.1, 1024, 256)
    r.spectrum_hook = K.perturb_hook(3)
    pinned = r.Process(x)
    assert K.deviation(pinned, clean, r.last_norm)[0] < 1e-11


# ---- margins and bars of the GPU cases ----------------------------------------------
def _all_bars():
    out = [(("freeze",) + s, K.freeze_bar(*s)) for s in K.FREEZE_SHAPES]
    for mode in (R.PHASE_HOLD, R.PHASE_ADVANCE):
        for mix in (1.0, 0.3):
            out.append((("frozen", mode, mix), K.freeze_bar(256, 64, sum(K.CUTS), 65, mix, mode, True, K.CUTS)))
    out += [(("pitch",) + c, K.pitch_bar(*c)) for c in K.PITCH_CASES]
    return out


def test_decision_margins_of_the_gpu_cases():
    """No GPU comparison needs to leave a sample out: every data-dependent decision the restatement takes on
    the GPU tests' inputs has more room than any transform error could use up."""
    least, where = math.inf, None
    for name, bar in _all_bars():
        m = bar.margins
        print(name, f"peak {m.peak_gap:.2e} wrap {m.wrap_gap:.2e} dc {m.dc_re:.2e} nyquist {m.nyq_re:.2e}")
        if m.least() < least:
            least, where = m.least(), name
        assert m.least() > K.MARGIN_FLOOR, (name, vars(m))
    print("smallest margin", least, where)


def test_bars_of_the_gpu_cases():
    worst = 0.0
    for name, bar in _all_bars():
        print(name, f"bar: relative rms {bar.rms:.3e}, max abs {bar.abs:.3e}")
        assert bar.perturbed_rms <= K.BAD_CASE_RMS, (name, bar.perturbed_rms)  # else the case is badly chosen
        assert bar.rms <= 1e-9, name
        worst = max(worst, bar.rms)
    print("largest bar", worst)
