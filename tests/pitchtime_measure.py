"""The signals and measuring functions of the reference's pitch shifter tests
(dsp/effects/pitch/pitch_shifter_test.go, internal/testutil), restated once
for tests/test_pitchtime_ref.py and tests/test_pitchtime_reference_cases_gpu.py.
The transforms are numpy's.
"""
import math

import numpy as np

from pitchtime_ref import go_round


def sine(freq, fs, amplitude, n):  # testutil.DeterministicSine signals.go:9-18
    step = 2 * math.pi * freq / fs
    return amplitude * np.sin(step * np.arange(n, dtype=np.float64))


def bin_sine(out_freq, ratio, n=32768, fs=48000.0, amplitude=0.8):
    """The quality tests' input (:364-367): a sine that the shift moves onto out_freq."""
    return amplitude * np.sin(2 * math.pi * (out_freq / ratio) * np.arange(n, dtype=np.float64) / fs)


def normalized_autocorrelation(x, lag):  # :662-685
    n = len(x) - lag
    if n <= 0:
        return -1.0
    a, b = x[:n], x[lag:lag + n]
    dot, e0, e1 = float(np.dot(a, b)), float(np.dot(a, a)), float(np.dot(b, b))
    if e0 <= 1e-12 or e1 <= 1e-12:
        return -1.0
    return dot / math.sqrt(e0 * e1)


def estimate_frequency(x, fs, min_hz, max_hz):  # estimateFrequencyAutoCorrelation :266-326
    lag_min = max(int(math.floor(fs / max_hz)), 1)
    lag_max = min(int(math.ceil(fs / min_hz)), len(x) - 2)
    assert lag_max > lag_min
    c = x - np.mean(x)
    scores = [normalized_autocorrelation(c, lag) for lag in range(lag_min, lag_max + 1)]
    best = lag_min + int(np.argmax(scores))
    lag = float(best)
    if lag_min < best < lag_max:
        s0, s1, s2 = scores[best - 1 - lag_min], scores[best - lag_min], scores[best + 1 - lag_min]
        den = s0 - 2 * s1 + s2
        if abs(den) > 1e-12:
            lag += 0.5 * (s0 - s2) / den
    return fs / lag


def snr_db(out, freqs, fs, fft_len):  # measureTimeDomainSNR :615-660, measureTimeDomainTwoToneSNR :565-611
    mid = max(len(out) // 2 - fft_len // 2, 0)
    mag2 = np.abs(np.fft.fft(out[mid:mid + fft_len])) ** 2
    k = np.arange(1, fft_len // 2 + 1)
    sig = np.zeros(k.shape, dtype=bool)
    for f in freqs:
        tb = int(go_round(f * fft_len / fs))
        sig |= (k >= tb - 10) & (k <= tb + 10)
    noise = float(np.sum(mag2[k][~sig]))
    return 100.0 if noise <= 1e-30 else 10 * math.log10(float(np.sum(mag2[k][sig])) / noise)
