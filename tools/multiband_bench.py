#!/usr/bin/env python3
"""Throughput of the N-way crossover and the multiband compressor
(ad_xover_process_device, ad_multiband_process_device) on one MI355X,
device-resident: 256 channels x 2^20 samples and 4096 channels x 2^16 samples
per call at 48 kHz, for 2, 4 and 8 bands at Linkwitz-Riley orders 4 and 24, in
one run on the same buffers:

  (a) the crossover, all stages in one launch as a pipeline over time tiles;
  (b) the crossover, one stage per launch;
  (c) what the library offered before these processors: one processors.Chain
      pass per LP and per HP cascade on torch copies (the crossover), then one
      processors.Compressor per band and a torch add (the multiband call);
  (d) the whole multiband call, in place;
  (e) two yardsticks: processors.Compressor and the phaser at 1 stage.

All of (a), (b) and (d) are serial walks along time, one channel per lane:
compare with the phaser, not with a copy.  Per case: ms per call and
Gsamples/s of input (median of the 7 timed windows after warm-up, with their
min and max) and the shader clock while a window ran.

The first samples of the first and last channel of (a) and (b) are checked on
bits against the restated reference before timing.

  python tools/multiband_bench.py [--out profiles/multiband_bench.json] [--shapes 256x1048576,4096x65536]
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
FREQS = {2: (1000.0,), 4: (200.0, 1000.0, 5000.0), 8: (60.0, 150.0, 400.0, 1000.0, 2500.0, 6000.0, 12000.0)}
ORDERS = (4, 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multiband_bench.json"))
    ap.add_argument("--shapes", default=",".join(f"{c}x{n}" for c, n in SHAPES))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

    import torch

    import multiband_ref as R
    from algodsp import processors

    assert torch.cuda.is_available(), "multiband_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    for ch, n in shapes:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        bands = torch.empty((8, ch, n), dtype=torch.float64, device=cuda)
        xh = x[:, :CHECK_N].cpu().numpy()

        for order in ORDERS:
            for nb, freqs in FREQS.items():
                tag = dict(bands=nb, order=order)
                want = {c: R.MultiBand(freqs, order, FS).ProcessBlock(xh[c]) for c in (0, ch - 1)}
                for form, pipelined in (("(a) crossover, pipelined", True), ("(b) crossover, one stage per launch", False)):
                    h = processors.MultiBandCrossover(freqs, order, FS, ch)
                    h.set_pipelined(pipelined)
                    h.process_device(x.data_ptr(), n, bands.data_ptr(), n, ch * n, CHECK_N, sp)
                    torch.cuda.synchronize()
                    got = bands[:nb, :, :CHECK_N].cpu().numpy()
                    exact = all(np.array_equal(got[:, c].view(np.int64), want[c].view(np.int64)) for c in want)
                    ms, clocks, reps = windows(
                        lambda: h.process_device(x.data_ptr(), n, bands.data_ptr(), n, ch * n, n, sp), h.Reset, stream)
                    emit(row(form, ch, n, ms, clocks, reps, bit_exact_first_samples=exact,
                             kernel_info=list(h.kernel_info()), **tag))
                    h.close()

                # (c) one Chain pass per cascade on torch copies
                secs = processors.crossover_sections(freqs, order, FS)
                lps = [processors.Chain(secs[i, 0], 1.0, ch) for i in range(nb - 1)]
                hps = [processors.Chain(secs[i, 1], 1.0, ch) for i in range(nb - 1)]
                comps = [processors.Compressor(FS, ch) for _ in range(nb)]

                def split():
                    w.copy_(x)
                    for i in range(nb - 1):
                        bands[i].copy_(w)
                        lps[i].process_device(bands[i].data_ptr(), n, n, sp)
                        hps[i].process_device(w.data_ptr(), n, n, sp)
                    bands[nb - 1].copy_(w)

                def composed():
                    split()
                    for i in range(nb):
                        comps[i].process_device(bands[i].data_ptr(), n, n, sp)
                    torch.sum(bands[:nb], dim=0, out=w)

                def restart_c():
                    for f in lps + hps + comps:
                        f.Reset()

                split()
                torch.cuda.synchronize()
                got = bands[:nb, :, :CHECK_N].cpu().numpy()
                exact = all(np.array_equal(got[:, c].view(np.int64), want[c].view(np.int64)) for c in want)
                ms, clocks, reps = windows(split, restart_c, stream)
                emit(row("(c) crossover composed of Chain passes", ch, n, ms, clocks, reps, baseline=True,
                         bit_exact_first_samples=exact, **tag))
                ms, clocks, reps = windows(composed, restart_c, stream)
                emit(row("(c) multiband composed of Chain and Compressor passes", ch, n, ms, clocks, reps,
                         baseline=True, **tag))
                for f in lps + hps + comps:
                    f.close()

                h = processors.MultibandCompressor(freqs, order, FS, ch)

                def restart_d():
                    h.Reset()
                    w.copy_(x)

                ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart_d, stream)
                emit(row("(d) multiband compressor", ch, n, ms, clocks, reps, **tag))
                h.close()

        for name, make in (("(e) compressor defaults", lambda: processors.Compressor(FS, ch)),
                           ("(e) phaser 1 stages", lambda: processors.Phaser(FS, ch, stages=1))):
            f = make()

            def restart_y():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_y, stream)
            emit(row(name, ch, n, ms, clocks, reps, yardstick=True))
            f.close()
        del x, w, bands
        torch.cuda.empty_cache()

    doc = dict(tool="tools/multiband_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS, windows=WINDOWS,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
