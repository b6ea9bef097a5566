#!/usr/bin/env python3
"""Throughput of the spectral freeze and the spectral pitch shifter
(ad_specfreeze_process_device, ad_pitchspec_process_device) on one MI355X,
device-resident and in place: 256 channels x 2^20 samples and 4096 channels x
2^16 samples per call at 48 kHz, frame 1024, hop 256, beside a device copy of
the same buffer and processors.Compressor on the same buffers in the same run.

Cases: the freeze unfrozen (analysis and synthesis fused); the freeze frozen
in Advance mode (no forward transform); the pitch shifter at +1 semitone (bin
shifting) and at +7 semitones (time stretch with resampling).

Per case: ms per call and Gsamples/s (median of the 7 timed windows after
warm-up, with their min and max), the FP64 transform work per second that
implies (2 * 5 N log2 N flops per frame for the two transforms of a frame; the
frozen freeze runs one), and the share of one profiled call's time in each
pass (events around the launches: analysis, walk, synthesis, overlap-add, the
resampling, or the fused frame pass).

The first samples of the first and last channel are checked against the
restated reference before timing.

  python tools/stft_bench.py [--out profiles/stft_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from fdn_bench import ROOT, WINDOWS, row, windows  # noqa: E402  (also sets sys.path)

FS = 48000.0
SHAPES = [(256, 1 << 20), (4096, 1 << 16)]
FRAME, HOP = 1024, 256
CHECK_N = 2085


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stft_bench.json"))
    args = ap.parse_args()

    import torch

    import stft_ref as R
    from algodsp import processors

    assert torch.cuda.is_available(), "stft_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    def freeze(ch, frozen):
        return processors.SpectralFreeze(FS, ch, frame_size=FRAME, hop_size=HOP, frozen=int(frozen))

    def freeze_ref(frozen):
        r = R.SpectralFreeze(FS)
        r.SetFrozen(frozen)
        return r

    def pitch(ch, semitones):
        h = processors.SpectralPitchShifter(FS, ch, frame_size=FRAME, analysis_hop=HOP)
        h.SetPitchSemitones(semitones)
        return h

    def pitch_ref(semitones):
        r = R.SpectralPitchShifter(FS)
        r.SetPitchSemitones(semitones)
        return r

    cases = [("freeze unfrozen", lambda ch: freeze(ch, False), lambda: freeze_ref(False), 2),
             ("freeze frozen advance", lambda ch: freeze(ch, True), lambda: freeze_ref(True), 1),
             ("pitch +1 semitone (bin shift)", lambda ch: pitch(ch, 1), lambda: pitch_ref(1), 2),
             ("pitch +7 semitones (time stretch, resampled)", lambda ch: pitch(ch, 7), lambda: pitch_ref(7), 2)]

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen) * 0.5
        w = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()

        ms, clocks, reps = windows(lambda: w.copy_(x), lambda: None, stream)
        copy = row("device copy", ch, n, ms, clocks, reps)
        copy["copy_gbytes_per_s"] = round(ch * n * 16 / (copy["ms_per_call"]["median"] * 1e-3) / 1e9, 1)
        emit(copy)

        for name, make, ref, transforms in cases:
            h = make(ch)
            w.copy_(x)
            h.process_device(w.data_ptr(), n, CHECK_N, sp)
            torch.cuda.synchronize()
            got = w[:, :CHECK_N].cpu().numpy()
            worst = 0.0
            for c in (0, ch - 1):
                want = ref().Process(xh[c])
                worst = max(worst, float(np.sqrt(np.mean((got[c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))))

            def restart():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart, stream)
            restart()
            h.profile(True)
            h.process_device(w.data_ptr(), n, n, sp)
            passes = h.profile(False, read=True)
            total = sum(passes.values())
            frames = ch * (1 + (n - 1) // HOP)
            flops = transforms * 5 * FRAME * math.log2(FRAME) * frames
            d = row(name, ch, n, ms, clocks, reps, rel_rms_vs_reference_first_samples=worst, frame=FRAME, hop=HOP,
                    transforms_per_frame=transforms)
            d["fft_gflops_per_s"] = round(flops / (d["ms_per_call"]["median"] * 1e-3) / 1e9, 1)
            d["profiled_call_ms"] = {k: round(v, 3) for k, v in passes.items() if v > 0}
            d["pass_share"] = {k: round(v / total, 3) for k, v in passes.items() if v > 0}
            emit(d)
            h.close()

        f = processors.Compressor(FS, ch)

        def restart_y():
            f.Reset()
            w.copy_(x)

        ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_y, stream)
        emit(row("compressor defaults", ch, n, ms, clocks, reps, yardstick=True))
        f.close()
        del x, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/stft_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS, windows=WINDOWS,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
