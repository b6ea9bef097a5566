#!/usr/bin/env python3
"""Throughput of the vocoder and the lookahead limiter
(ad_vocoder_process_device, ad_lookahead_process_device) on one MI355X,
device-resident: 256 channels x 2^20 samples and 4096 channels x 2^16 samples
per call at 48 kHz, beside a device copy of the same buffer and three
yardsticks on the same buffers in the same run: the phaser at 1 stage,
processors.Compressor and the de-esser in wideband mode.

Cases: the vocoder in the ThirdOctave (32 bands) and Bark (24 bands) layouts,
downsampling off and on, out in place on the modulator; the limiter at 3 ms
with the program as its own detector.

The vocoder's walk is one wave per channel, a band per lane: a sample costs the
channel 64 sections (32 analysis, 32 synthesis), walked by 64 lanes at once,
where the de-esser's wideband walk costs a channel one section per filter
order and an envelope, walked by one lane, 64 channels to a wave.  Per case: ms
per call and Gsamples/s (median of the 7 timed windows after warm-up, with
their min and max), the shader clock while a window ran, `cycles_per_sample`:
the median time of a call in shader clocks over the n samples of a row, and for
the vocoder `cycles_per_sample_resident`: the same over the rounds in which the
workgroups are resident (4 workgroups of 34,304 B LDS per compute unit, 256
compute units), which is what a sample of the walk costs a wave.  The last
column is the ratio of cycles_per_sample to the de-esser wideband row's of the
same shape.

The first samples of the first and last channel are checked against the
restated reference before timing (the vocoder on bits).

  python tools/vocoder_bench.py [--out profiles/vocoder_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from fdn_bench import ROOT, WINDOWS, row, windows  # noqa: E402  (also sets sys.path)

FS = 48000.0
SHAPES = [(256, 1 << 20), (4096, 1 << 16)]
CHECK_N = 300
COMPUTE_UNITS, WORKGROUPS_PER_CU = 256, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vocoder_bench.json"))
    args = ap.parse_args()

    import torch

    import dynfx_ref
    import lookahead_ref
    import vocoder_ref
    from algodsp import processors

    assert torch.cuda.is_available(), "vocoder_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    def cycles(d, n):
        if d["sclk_mhz"]:
            d["cycles_per_sample"] = round(d["ms_per_call"]["median"] * 1e-3 * d["sclk_mhz"] * 1e6 / n, 1)
        else:
            d["cycles_per_sample"] = "clock not read"

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        car = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        pick = [0, ch - 1]
        xh, ch_ = x[pick, :CHECK_N].cpu().numpy(), car[pick, :CHECK_N].cpu().numpy()

        ms, clocks, reps = windows(lambda: w.copy_(x), lambda: None, stream)
        copy = row("device copy", ch, n, ms, clocks, reps)
        copy["copy_gbytes_per_s"] = round(ch * n * 16 / (copy["ms_per_call"]["median"] * 1e-3) / 1e9, 1)
        emit(copy)

        for layout, lname in ((processors.Vocoder.THIRD_OCTAVE, "ThirdOctave"), (processors.Vocoder.BARK, "Bark")):
            for ds in (False, True):
                h = processors.Vocoder(FS, ch, layout=layout, downsample=ds, input_level=0.2, synth_level=0.1)
                w.copy_(x)
                h.process_device(w.data_ptr(), n, car.data_ptr(), n, w.data_ptr(), n, CHECK_N, sp)
                torch.cuda.synchronize()
                ref = vocoder_ref.Vocoder(FS, channels=2, layout=layout, downsample=ds, inputLevel=0.2, synthLevel=0.1)
                want = ref.process_many(xh, ch_)
                same = bool(np.array_equal(w[pick, :CHECK_N].cpu().numpy().view(np.int64), want.view(np.int64)))

                def restart():
                    h.Reset()
                    w.copy_(x)

                ms, clocks, reps = windows(
                    lambda: h.process_device(w.data_ptr(), n, car.data_ptr(), n, w.data_ptr(), n, n, sp), restart, stream)
                d = row(f"vocoder {lname} downsampling {'on' if ds else 'off'}", ch, n, ms, clocks, reps,
                        bands=h.NumBands(), same_bits_as_reference_first_samples=same, kernel_info=list(h.kernel_info()),
                        workgroups=ch)
                cycles(d, n)
                rounds = -(-ch // (COMPUTE_UNITS * WORKGROUPS_PER_CU))
                if d["sclk_mhz"]:
                    d["rounds"] = rounds
                    d["cycles_per_sample_resident"] = round(d["cycles_per_sample"] / rounds, 1)
                emit(d)
                h.close()

        h = processors.LookaheadLimiter(FS, ch, threshold_db=-12.0, lookahead_ms=3.0)
        w.copy_(x)
        h.process_device(w.data_ptr(), n, CHECK_N, sp)
        torch.cuda.synchronize()
        ref = lookahead_ref.LookaheadLimiter(FS, 2)
        ref.SetThreshold(-12.0)
        want = ref.process_many(xh)
        got = w[pick, :CHECK_N].cpu().numpy()
        worst = float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))

        def restart_l():
            h.Reset()
            w.copy_(x)

        ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart_l, stream)
        d = row("lookahead limiter 3 ms", ch, n, ms, clocks, reps, rel_rms_vs_reference_first_samples=worst,
                delay_samples=h.DelaySamples(), workgroups=(ch + 63) // 64)
        cycles(d, n)
        emit(d)
        h.close()

        def deesser():
            f = processors.DeEsser(FS, ch)
            f.SetMode(dynfx_ref.WIDEBAND)
            return f

        for name, make in (("phaser 1 stages", lambda: processors.Phaser(FS, ch, stages=1)),
                           ("compressor defaults", lambda: processors.Compressor(FS, ch)),
                           ("de-esser wideband order 2", deesser)):
            f = make()

            def restart_y():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_y, stream)
            d = row(name, ch, n, ms, clocks, reps, yardstick=True, workgroups=(ch + 63) // 64)
            cycles(d, n)
            emit(d)
            f.close()
        base = [r for r in rows if r["channels"] == ch and r["case"].startswith("de-esser")][0]
        for r in rows:
            if r["channels"] == ch and isinstance(r.get("cycles_per_sample"), float) \
                    and isinstance(base.get("cycles_per_sample"), float):
                r["ratio_to_deesser_wideband"] = round(r["cycles_per_sample"] / base["cycles_per_sample"], 2)
        del x, car, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/vocoder_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS, windows=WINDOWS,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
