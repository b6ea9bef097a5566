#!/usr/bin/env python3
"""Throughput of the distortion and the bit crusher
(ad_distortion_process_device, ad_bitcrusher_process_device) on one MI355X,
device-resident and in place: 256 channels x 2^20 samples and 4096 channels x
2^16 samples per call at 48 kHz, beside a device copy of the same buffer, the
ring modulator and the phaser at 1 stage on the same buffers in the same run.

Cases: one algebraic mode (Waveshaper3), one transcendental mode (Tanh, exact)
and Chebyshev order 16 with weights on the pointwise kernel; Chebyshev order 3
with the DC bypass (one channel per lane, serial along time: compare with the
phaser at 1 stage); the bit crusher at downsample 1 (pointwise), 4 and 256
(span workgroups that stage whole hold periods through LDS).

Per case: ms per call and Gsamples/s (median of the 7 timed windows, with their
min and max) and the shader clock while a window ran.  The handles do no host
work per sample, so the windows of back-to-back calls time the device.  For
every case also the share of the copy bandwidth by algorithmic bytes: 16 B per
sample and channel (the input and the output) over the median time, against
the device copy timed in the same run (`copy_gbytes_per_s`: torch's
device-to-device copy of the same [channels][n] buffer, 8 B read and 8 B written
per sample), and against the best 1:1 copy rate tools/hbm_probe reports when
that probe has been built (`not measured` otherwise).
The ring modulator steps its phase on the host, and at 256 x 2^20 that takes
longer than its kernels, so its windows time the host there.  Its
`device_ms_per_call` is the event time of one call enqueued behind copies that
keep the device busy meanwhile (the upload and the kernels, none of the host's
stepping), as tools/modfx_bench.py takes it.
`slower_than_ringmod_by_more_than_the_spread` compares a pointwise case's
median with the ring modulator's like for like: with its windows' median
where those time the device (`ringmod_windows_time_the_host` false), with its
device time where they time the host.  The spread is the larger of the two
cases' max - min over their windows.  `ms_behind_ringmod_device_time` is given
in both cases.

The first samples of the first and last channel are checked against the
restated reference before timing (the transcendental mode given the device's
own curve).

  python tools/shaper_bench.py [--out profiles/shaper_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from delayfx_bench import hbm_copy_gbps  # noqa: E402
from fdn_bench import ROOT, row, windows  # noqa: E402  (also sets sys.path)

FS = 48000.0
SHAPES = [(256, 1 << 20), (4096, 1 << 16)]
CHECK_N = 2048
BLOCKER_COPIES = 24  # copies of the whole buffer enqueued in front of a call whose device time is taken
W16 = [0.5, -0.25, 0.125, 0.3, -0.2, 0.1, 0.05, -0.05, 0.02, 0.01, -0.01, 0.03, 0.002, -0.004, 0.001, 0.0005]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shaper_bench.json"))
    args = ap.parse_args()

    import torch

    import shaper_ref as R
    from algodsp import processors

    assert torch.cuda.is_available(), "shaper_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    probe_gbps = hbm_copy_gbps()
    rows = []
    M = {name: i for i, name in enumerate(R.MODES)}

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()

        ms, clocks, reps = windows(lambda: w.copy_(x), lambda: None, stream)
        copy = row("device copy", ch, n, ms, clocks, reps)
        copy_gbps = ch * n * 16 / (copy["ms_per_call"]["median"] * 1e-3) / 1e9
        copy["copy_gbytes_per_s"] = round(copy_gbps, 1)
        emit(copy)
        shape_rows = []

        def finish(d):
            gbps = ch * n * 16 / (d["ms_per_call"]["median"] * 1e-3) / 1e9
            d["algorithmic_bytes_per_sample"] = 16
            d["algorithmic_gbytes_per_s"] = round(gbps, 1)
            d["share_of_copy_bandwidth"] = round(gbps / copy_gbps, 3)
            d["share_of_hbm_probe_copy"] = round(gbps / probe_gbps, 3) if probe_gbps else "not measured"
            shape_rows.append(d)

        def case(name, make, ref, **more):
            h = make()
            w.copy_(x)
            h.process_device(w.data_ptr(), n, CHECK_N, sp)
            torch.cuda.synchronize()
            got = w[:, :CHECK_N].cpu().numpy()
            worst = 0.0
            for c in (0, ch - 1):
                r = ref()
                if isinstance(r, R.BitCrusher):
                    r.quantLevels = h.derived()["quant_levels"]
                    want = r.process_many(xh[c:c + 1])[0]
                else:
                    curve = h.curve(r.argument(xh[c:c + 1])) if R.MODES[r.mode] in R.TRANSCENDENTAL and r.approxMode == 0 else None
                    want = r.process_many(xh[c:c + 1], curve)[0]
                worst = max(worst, float(np.sqrt(np.mean((got[c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))))

            def restart():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart, stream)
            d = row(name, ch, n, ms, clocks, reps, rel_rms_vs_reference_first_samples=worst, **more)
            finish(d)
            h.close()

        dist = [("distortion waveshaper3 (algebraic)", dict(mode=M["waveshaper3"], drive=2.0, shape=0.7), "pointwise"),
                ("distortion tanh exact (transcendental)", dict(mode=M["tanh"], drive=2.0), "pointwise"),
                ("distortion chebyshev order 16 with weights", dict(mode=M["chebyshev"], cheb_order=16, cheb_weights=W16), "pointwise"),
                ("distortion chebyshev order 3 DC bypass", dict(mode=M["chebyshev"], cheb_order=3, cheb_dc_bypass=1),
                 "one channel per lane")]
        for name, opts, kernel in dist:
            case(name, lambda opts=opts: processors.Distortion(FS, ch, **opts), lambda opts=opts: R.Distortion(FS, **opts),
                 kernel=kernel)
        for ds in (1, 4, 256):
            case(f"bit crusher downsample {ds}", lambda ds=ds: processors.BitCrusher(FS, ch, downsample=ds),
                 lambda ds=ds: R.BitCrusher(FS, downsample=ds), kernel="pointwise" if ds == 1 else "spans", downsample=ds)

        for name, make in (("ring modulator 440 Hz", lambda: processors.RingModulator(FS, ch)),
                           ("phaser 1 stages", lambda: processors.Phaser(FS, ch, stages=1))):
            f = make()

            def restart_r():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_r, stream)
            d = row(name, ch, n, ms, clocks, reps)
            finish(d)
            if name.startswith("ring"):
                w2 = torch.empty_like(x)
                t = []
                for _ in range(5):
                    torch.cuda.synchronize()
                    for _ in range(BLOCKER_COPIES):
                        w2.copy_(x)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    f.process_device(w.data_ptr(), n, n, sp)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    t.append(e0.elapsed_time(e1))
                del w2
                d["device_ms_per_call"] = round(statistics.median(t), 4)
                d["share_of_copy_bandwidth_device_time"] = round(ch * n * 16 / (d["device_ms_per_call"] * 1e-3) / 1e9 / copy_gbps, 3)
            f.close()

        ring = next(d for d in shape_rows if d["case"].startswith("ring modulator"))
        for d in shape_rows:
            if d is not ring and d.get("kernel") == "pointwise":
                spread = max(d["ms_per_call"]["max"] - d["ms_per_call"]["min"],
                             ring["ms_per_call"]["max"] - ring["ms_per_call"]["min"])
                host_bound = ring["ms_per_call"]["median"] > 1.25 * ring["device_ms_per_call"]
                against = ring["device_ms_per_call"] if host_bound else ring["ms_per_call"]["median"]
                d["ringmod_windows_time_the_host"] = bool(host_bound)
                d["ms_behind_ringmod"] = round(d["ms_per_call"]["median"] - against, 4)
                d["ms_behind_ringmod_device_time"] = round(d["ms_per_call"]["median"] - ring["device_ms_per_call"], 4)
                d["spread_ms"] = round(spread, 4)
                d["slower_than_ringmod_by_more_than_the_spread"] = bool(d["ms_behind_ringmod"] > spread)
            emit(d)
        del x, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/shaper_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS,
               hbm_probe_copy_gbytes_per_s=probe_gbps if probe_gbps else "not measured", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
