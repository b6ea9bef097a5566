#!/usr/bin/env python3
"""Throughput of the transient shaper and the de-esser
(ad_transient_process_device, ad_deesser_process_device) on one MI355X,
device-resident and in place: 256 channels x 2^20 samples and 4096 channels x
2^16 samples per call at 48 kHz, beside a device copy of the same buffer and
two yardsticks on the same buffers in the same run: processors.Compressor and
the phaser at 1 stage.

Cases: the transient shaper at its defaults; the de-esser in split-band mode at
filter order 2 and 4, in wideband mode and in listen mode.  All of them are
serial walks along time, one channel per lane, followed (listen mode excepted)
by a pointwise pass: compare with the phaser, not with the copy.

Per case: ms per call and Gsamples/s (median of the 7 timed windows after
warm-up, with their min and max), the shader clock while a window ran, and
`cycles_per_sample`: the median time of a call in shader clocks over the n
samples every lane walks.  All workgroups of a case are resident at once
(`workgroups` of 64 channels on 256 compute units), so this is what a sample
of the serial walk costs end to end, the pointwise pass and the launches
between the passes of a long call included.  Listen mode has no pointwise
pass: its figure is the walk's alone.

The first samples of the first and last channel are checked against the
restated reference before timing (the de-esser given the device's own curve).

  python tools/dynfx_bench.py [--out profiles/dynfx_bench.json]
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
CHECK_N = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dynfx_bench.json"))
    args = ap.parse_args()

    import torch

    import dynfx_ref as R
    from algodsp import processors

    assert torch.cuda.is_available(), "dynfx_bench needs a GPU"
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
        d["workgroups"] = (d["channels"] + 63) // 64

    def apply(obj, setup):
        for name, v in setup:
            getattr(obj, name)(v)
        return obj

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()

        ms, clocks, reps = windows(lambda: w.copy_(x), lambda: None, stream)
        copy = row("device copy", ch, n, ms, clocks, reps)
        copy["copy_gbytes_per_s"] = round(ch * n * 16 / (copy["ms_per_call"]["median"] * 1e-3) / 1e9, 1)
        emit(copy)

        def case(name, make, ref, **more):
            h = make()
            w.copy_(x)
            h.process_device(w.data_ptr(), n, CHECK_N, sp)
            torch.cuda.synchronize()
            got = w[:, :CHECK_N].cpu().numpy()
            worst = 0.0
            for c in (0, ch - 1):
                r = ref()
                if isinstance(r, R.DeEsser) and not r.listen:
                    r.trace = []
                    r.ProcessInPlace(xh[c].copy())
                    it = iter(h.gain(np.asarray(r.trace)).tolist())
                    r = ref()
                    r.gain_fn = lambda env, it=it: next(it)
                want = r.ProcessInPlace(xh[c].copy())
                worst = max(worst, float(np.sqrt(np.mean((got[c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))))

            def restart():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart, stream)
            d = row(name, ch, n, ms, clocks, reps, rel_rms_vs_reference_first_samples=worst,
                    kernel_info=list(h.kernel_info()), **more)
            cycles(d, n)
            emit(d)
            h.close()

        case("transient shaper defaults", lambda: processors.TransientShaper(FS, ch), lambda: R.TransientShaper(FS))
        deess = [("de-esser split band order 2", [("SetFilterOrder", 2)]),
                 ("de-esser split band order 4", [("SetFilterOrder", 4)]),
                 ("de-esser wideband order 2", [("SetMode", R.WIDEBAND)]),
                 ("de-esser listen order 2", [("SetListen", True)])]
        for name, setup in deess:
            case(name, lambda setup=setup: apply(processors.DeEsser(FS, ch), setup),
                 lambda setup=setup: apply(R.DeEsser(FS), setup), cascades_walked=1)

        # the two-cascade walk: a handle whose cascades count as diverged (one state set apart by the sign of a
        # zero past the order), and no Reset between the windows, which would make them count as equal again
        h = apply(processors.DeEsser(FS, ch), [("SetFilterOrder", 2)])
        e, det, band = h.get_state(0)
        band[3, 1] = -0.0
        h.set_state(0, e, det, band)
        assert h.kernel_info()[3] == 2
        ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), lambda: w.copy_(x), stream)
        assert h.kernel_info()[3] == 2
        d = row("de-esser split band order 2, both cascades walked", ch, n, ms, clocks, reps,
                kernel_info=list(h.kernel_info()), cascades_walked=2)
        cycles(d, n)
        emit(d)
        h.close()

        for name, make in (("compressor defaults", lambda: processors.Compressor(FS, ch)),
                           ("phaser 1 stages", lambda: processors.Phaser(FS, ch, stages=1))):
            f = make()

            def restart_y():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_y, stream)
            d = row(name, ch, n, ms, clocks, reps, yardstick=True)
            cycles(d, n)
            emit(d)
            f.close()
        del x, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/dynfx_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS, windows=WINDOWS,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
