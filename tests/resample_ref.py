"""Restatement of resample.Resampler's streaming core (dsp/resample/resample.go)
for the resampler tests: Process (:249-292) and PredictOutputLen (:295-313) as
the literal loops with the skip rule, and a vectorised numpy form of the same
arithmetic for larger shapes.  Both take the prototype as an array, so a
comparison against the GPU never depends on how the prototype was designed.
"""
from __future__ import annotations

import math

import numpy as np


# (up, down, taps per phase) of the GPU parity tests; the CPU tests hold the
# restatement's two forms to each other on the same shapes
SHAPES = [
    (1, 1, 16), (2, 1, 32), (1, 2, 32), (3, 2, 32), (160, 147, 32), (147, 160, 16),
    (1, 6, 16),          # calls that produce no output
    (7, 1, 1),           # no delay line
    (4097, 4096, 16),    # a 524 KiB table: read from global memory, every output its own row
    (5, 3, 64),
]
# beyond those: the other combinations of where the table and the window live
MORE_SHAPES = [
    (160, 147, 64),      # table too large for LDS, lanes still share a phase
    (257, 256, 16),      # table in LDS, up > 256: no shared phase
    (1, 40, 16),         # steep decimation: window read from global memory
    (160, 6007, 64), (257, 10000, 16), (4097, 200000, 16),  # window from global memory, each table path
    (32, 97, 16),        # several tiles per workgroup, window too long to be loaded ahead in registers
]
N_IN = (1500, 4099)


def random_taps(up: int, T: int, seed: int) -> np.ndarray:
    """An asymmetric prototype: a symmetric one hides a reversed tap or phase order."""
    return np.random.default_rng(seed).standard_normal(T * up)


def random_input(channels: int, n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((channels, n))


class Ref:
    """One stream.  phases[p] = taps[p], taps[p+up], ... (resample_design.go:55-66)."""

    def __init__(self, up: int, down: int, taps):
        g = math.gcd(up, down)
        self.up, self.down = up // g, down // g
        self.taps = np.ascontiguousarray(taps, dtype=np.float64)
        self.phases = [self.taps[p::self.up].copy() for p in range(self.up)]
        self.max_phase_len = max(len(p) for p in self.phases)
        self.table = np.zeros((self.up, self.max_phase_len))
        for p, row in enumerate(self.phases):
            self.table[p, :len(row)] = row
        self.reset()

    def reset(self):  # :241-246
        self.phase = 0
        self.input_index = 0
        self.total_in = 0
        self.history = np.zeros(0)

    def predict_output_len(self, input_len: int) -> int:  # :295-313
        if input_len <= 0:
            return 0
        last_avail = self.total_in + input_len - 1
        i = self.input_index
        phase = self.phase
        count = 0
        while i <= last_avail:
            count += 1
            phase += self.down
            i += phase // self.up
            phase %= self.up
        return count

    def _work(self, x):
        work = np.concatenate([self.history, x])
        return work, self.total_in - len(self.history), self.total_in + len(x) - 1

    def _finish(self, work, n):
        self.total_in += n
        keep = min(max(0, self.max_phase_len - 1), len(work))
        self.history = work[len(work) - keep:].copy()

    def process(self, x) -> np.ndarray:
        """The literal loop (:264-283)."""
        x = np.asarray(x, dtype=np.float64)
        if len(x) == 0:
            return np.zeros(0)
        work, base_index, last_avail = self._work(x)
        out = []
        while self.input_index <= last_avail:
            taps = self.phases[self.phase]
            y = np.float64(0.0)
            for k in range(len(taps)):
                idx = self.input_index - k
                if idx < base_index or idx > last_avail:
                    continue
                y = y + taps[k] * work[idx - base_index]
            out.append(y)
            self.phase += self.down
            self.input_index += self.phase // self.up
            self.phase %= self.up
        self._finish(work, len(x))
        return np.array(out, dtype=np.float64)

    def process_vec(self, x) -> np.ndarray:
        """The same sums with every output advanced together: y = y + c[phase, k] * x[idx - k]
        over k, a term outside the available range leaving y as it is."""
        x = np.asarray(x, dtype=np.float64)
        if len(x) == 0:
            return np.zeros(0)
        n_out = self.predict_output_len(len(x))
        work, base_index, last_avail = self._work(x)
        num = self.phase + np.arange(n_out, dtype=np.int64) * self.down
        idx = self.input_index + num // self.up
        ph = num % self.up
        y = np.zeros(n_out)
        for k in range(self.max_phase_len):
            i = idx - k
            ok = (i >= base_index) & (i <= last_avail)
            term = self.table[ph, k] * work[np.where(ok, i - base_index, 0)]
            y = np.where(ok, y + term, y)
        end = self.phase + n_out * self.down
        self.input_index += end // self.up
        self.phase = end % self.up
        self._finish(work, len(x))
        return y


def resample(up: int, down: int, taps, x, chunks=None, vec=True):
    """x [C][n] through one Ref per channel, whole or cut into `chunks`-sample
    calls; returns ([C][n_out], the per-call output lengths)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[1]
    step = n if chunks is None else chunks
    rows, lens = [], []
    for c in range(x.shape[0]):
        r = Ref(up, down, taps)
        parts = []
        for s in range(0, n, step):
            blk = x[c, s:s + step]
            parts.append(r.process_vec(blk) if vec else r.process(blk))
        rows.append(np.concatenate(parts) if parts else np.zeros(0))
        lens = [len(p) for p in parts]
    return np.stack(rows), lens
