#!/usr/bin/env python3
"""Throughput of the tremolo, the ring modulator and the phaser
(ad_tremolo_process_device, ad_ringmod_process_device, ad_phaser_process_device)
on one MI355X, device-resident and in place: 256 channels x 2^20 samples and
4096 channels x 2^16 samples per call at 48 kHz, beside Freeverb and the
flanger on the same buffers in the same run.

Cases: the tremolo with smoothing 0 (the gain is the target: fully parallel)
and 5 ms (one lane steps the gain's recurrence before the apply kernel), the
ring modulator at 440 Hz, the phaser at 1, 6 and 12 stages.

Per case: ms per call and Gsamples/s (median of the timed windows, with their
min and max) and the shader clock while a window ran.  For the pointwise
effects also the share of the copy bandwidth by algorithmic bytes: 16 B per
sample and channel (the input and the output) over the time, against the best
1:1 copy rate tools/hbm_probe reports in the same run when that probe has been
built (`not measured` otherwise).

The host steps the LFO phase of every call.  That time is given on its own:
`host_ms_per_call` is the wall time of the enqueueing call with the device
idle (the phase steps into the pinned buffer, the upload's and the kernels'
launches), `host_ms_per_call_1024_samples` the same for a call of 1024
samples (the launches alone, near enough).  `device_ms_per_call` is the
event time of one call enqueued behind copies that keep the device busy
meanwhile, so it holds the upload and the kernels and none of the host's
stepping; the share of the copy bandwidth is taken from it.
`host_exceeds_device` says whether the host time is the longer one: the timed
windows enqueue back to back, so there `ms_per_call` measures the host.

The first samples of the first and last channel are checked against the
restated reference before timing.

  python tools/modfx_bench.py [--out profiles/modfx_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from delayfx_bench import hbm_copy_gbps  # noqa: E402
from fdn_bench import ROOT, row, windows  # noqa: E402  (also sets sys.path)

FS = 48000.0
SHAPES = [(256, 1 << 20), (4096, 1 << 16)]
CHECK_N = 2048
HOST_REPS = 9
BLOCKER_COPIES = 24  # copies of the whole buffer enqueued in front of a call whose device time is taken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "modfx_bench.json"))
    args = ap.parse_args()

    import torch

    import modfx_ref as R
    from algodsp import processors

    assert torch.cuda.is_available(), "modfx_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    copy_gbps = hbm_copy_gbps()
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    def host_ms(h, w, n, m):
        """Median wall time of enqueueing a call of m samples, the device idle before each."""
        t = []
        for _ in range(HOST_REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.process_device(w.data_ptr(), n, m, sp)
            t.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        return round(statistics.median(t), 4)

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        w2 = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()

        def device_ms(h):
            """Median event time of a call that is enqueued whole before the device reaches it."""
            t = []
            for _ in range(5):
                torch.cuda.synchronize()
                for _ in range(BLOCKER_COPIES):
                    w2.copy_(x)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                h.process_device(w.data_ptr(), n, n, sp)
                e1.record(stream)
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1))
            return round(statistics.median(t), 4)

        def case(name, make, ref, pointwise, **more):
            h = make()
            w.copy_(x)
            h.process_device(w.data_ptr(), n, CHECK_N, sp)
            torch.cuda.synchronize()
            got = w[:, :CHECK_N].cpu().numpy()
            worst = 0.0
            for c in (0, ch - 1):
                want = ref().process(xh[c])
                worst = max(worst, float(np.sqrt(np.mean((got[c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))))

            def restart():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart, stream)
            d = row(name, ch, n, ms, clocks, reps, rel_rms_vs_reference_first_samples=worst, **more)
            d["host_ms_per_call"] = host_ms(h, w, n, n)
            d["host_ms_per_call_1024_samples"] = host_ms(h, w, n, 1024)
            d["device_ms_per_call"] = device_ms(h)
            d["host_exceeds_device"] = bool(d["host_ms_per_call"] > d["device_ms_per_call"])
            if pointwise:
                gbps = ch * n * 16 / (d["device_ms_per_call"] * 1e-3) / 1e9
                d["algorithmic_bytes_per_sample"] = 16
                d["algorithmic_gbytes_per_s"] = round(gbps, 1)
                d["share_of_copy_bandwidth"] = round(gbps / copy_gbps, 3) if copy_gbps else "not measured"
            emit(d)
            h.close()

        for ms_ in (0.0, 5.0):
            def tref(ms_=ms_):
                return R.Tremolo(FS, smoothing_ms=ms_)
            case(f"tremolo smoothing {ms_:g} ms", lambda: processors.Tremolo(FS, ch, smoothing_ms=ms_), tref,
                 True, smoothing_ms=ms_)
        case("ring modulator 440 Hz", lambda: processors.RingModulator(FS, ch),
             lambda: R.RingModulator(FS), True)
        for stages in (1, 6, 12):
            def pref(stages=stages):
                return R.Phaser(FS, stages=stages)
            case(f"phaser {stages} stages", lambda: processors.Phaser(FS, ch, stages=stages), pref, False,
                 stages=stages, dependent_ops_per_sample=3 * stages + 2)

        for name, make in (("freeverb", lambda: processors.Reverb(ch)), ("flanger defaults", lambda: processors.Flanger(FS, ch))):
            f = make()

            def restart_r():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_r, stream)
            emit(row(name, ch, n, ms, clocks, reps))
            f.close()
        del x, w, w2
        torch.cuda.empty_cache()

    doc = dict(tool="tools/modfx_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS,
               hbm_probe_copy_gbytes_per_s=copy_gbps if copy_gbps else "not measured", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
