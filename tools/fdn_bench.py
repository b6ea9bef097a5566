#!/usr/bin/env python3
"""Throughput of the FDN reverb (ad_fdn_process_device) on one MI355X,
device-resident and in place: 256 channels x 2^20 samples and 4096 channels x
2^16 samples per call at 48 kHz, with NewFDNReverb's defaults and again with
mod depth 0, beside Freeverb's two engines (the default one and the
time-parallel one) on the same buffers.

Per case: ms per call and Gsamples/s (median of the timed windows, with their
min and max), the shader clock rocm-smi reports while a window runs, and the
serial-chain figures: the damping recurrence is two dependent FP64 operations
per sample and channel, a wave issues an FP64 vector operation over 4 cycles,
so a call cannot take less than n * 2 * 4 cycles; `chain_share` is that bound
over the measured time.  The first samples of the first and last channel are
checked against the restated reference before timing.

  python tools/fdn_bench.py [--out profiles/fdn_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from rows_bench import ROOT  # noqa: E402  (also sets sys.path)

FS = 48000.0
SHAPES = [(256, 1 << 20), (4096, 1 << 16)]
WINDOWS = 7       # timed windows per case
WINDOW_S = 0.3    # a window runs calls for at least this long
WARM_S = 0.5
CHECK_N = 4096
CHAIN_OPS = 2     # dependent FP64 operations per sample of the damping recurrence
FP64_ISSUE = 4    # cycles a wave's FP64 vector operation occupies its SIMD


def sclk_mhz():
    """The shader clock rocm-smi reports right now (MHz), or None."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20)
        card = json.loads(r.stdout)
        card = card.get("card0", next(iter(card.values())))
        for k, v in card.items():
            if "sclk" in k and "(" in str(v):
                return float(str(v).split("(")[1].split("Mhz")[0].split("MHz")[0])
    except Exception:  # noqa: BLE001 - diagnostics only
        pass
    return None


def windows(call, restart, stream):
    """Warm up, then WINDOWS event-timed windows of back-to-back calls;
    restart() runs before each window, outside the timing.  Returns (ms per
    call of every window, the clock read while each window ran)."""
    import torch

    t0 = time.perf_counter()
    calls = 0
    while time.perf_counter() - t0 < WARM_S or calls < 2:
        call()
        torch.cuda.synchronize()
        calls += 1
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    reps = max(2, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6)) + 1)
    ms, clocks = [], []
    for _ in range(WINDOWS):
        restart()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            call()
        e1.record(stream)
        clocks.append(sclk_mhz())
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms, clocks, reps


def row(name, ch, n, ms, clocks, reps, **more):
    rate = sorted(ch * n / 1e6 / m for m in ms)
    seen = [c for c in clocks if c]
    d = dict(case=name, channels=ch, n=n, calls_per_window=reps,
             ms_per_call=dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4)),
             gsamples_per_s=dict(median=round(statistics.median(rate), 3), min=round(rate[0], 3),
                                 max=round(rate[-1], 3)),
             sclk_mhz=statistics.median(seen) if seen else None, **more)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fdn_bench.json"))
    args = ap.parse_args()

    import torch

    import fdn_ref
    from algodsp import processors

    assert torch.cuda.is_available(), "fdn_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    rows = []
    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()
        for name, depth in (("fdn defaults", None), ("fdn mod depth 0", 0.0)):
            h = processors.FDNReverb(FS, ch)
            if depth is not None:
                h.SetModDepth(depth)
            block, sub, lds = h.kernel_info()
            # parity on the first CHECK_N samples, first and last channel
            w.copy_(x)
            h.process_device(w.data_ptr(), n, CHECK_N, sp)
            torch.cuda.synchronize()
            got = w[:, :CHECK_N].cpu().numpy()
            worst = 0.0
            for c in (0, ch - 1):
                r = fdn_ref.FDN(FS, gains=h.derived()[0])
                if depth is not None:
                    r.SetModDepth(depth)
                    r.feedbackGain = [float(g) for g in h.derived()[0]]
                want = r.process(xh[c])
                worst = max(worst, float(np.sqrt(np.mean((got[c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))))

            def restart():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart, stream)
            d = row(name, ch, n, ms, clocks, reps, block=block, sub_block=sub, lds_bytes_per_workgroup=lds,
                    rel_rms_vs_reference_first_samples=worst)
            med_s = statistics.median(ms) / 1e3
            if d["sclk_mhz"]:
                hz = d["sclk_mhz"] * 1e6
                d["cycles_per_sample"] = round(med_s * hz / n, 2)
                d["chain_bound_ms"] = round(n * CHAIN_OPS * FP64_ISSUE / hz * 1e3, 4)
                d["chain_share"] = round(n * CHAIN_OPS * FP64_ISSUE / hz / med_s, 3)
            rows.append(d)
            print(json.dumps(d), flush=True)
            h.close()
        for name, engine in (("freeverb default engine", processors.Reverb.ENGINE_AUTO),
                             ("freeverb time-parallel engine", processors.Reverb.ENGINE_TIME_PARALLEL)):
            f = processors.Reverb(ch)
            f.SetEngine(engine)

            def restart_f():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_f, stream)
            d = row(name, ch, n, ms, clocks, reps, engine_ran=f.LastEngine()[0])
            rows.append(d)
            print(json.dumps(d), flush=True)
            f.close()
        del x, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/fdn_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS, windows=WINDOWS,
               chain_model=dict(dependent_fp64_ops_per_sample=CHAIN_OPS, cycles_per_fp64_issue=FP64_ISSUE), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
