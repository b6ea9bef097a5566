#!/usr/bin/env python3
"""Throughput of the feedback delay, delay-simple and the flanger
(ad_delay_process_device, ad_flanger_process_device) on one MI355X,
device-resident and in place: 256 channels x 2^20 samples and 4096 channels x
2^16 samples per call at 48 kHz, beside Freeverb and the FDN reverb on the
same buffers in the same run.

Cases: the delay at 0.25 s (regime 1: one launch per hazard-free block), at
0.001 s (regime 2: one persistent launch) and in the middle of a ramp
(SetTargetTime before every call, so every call uploads a trajectory); the
flanger at its defaults and at the minimum base delay; delay-simple at 20 ms.
`--sweep` adds the delay at a row of delay times with each regime forced, the
data the crossover constant in csrc/capi_delayfx.cpp is chosen from.

Per case: ms per call and Gsamples/s (median of the timed windows, with their
min and max) and the shader clock while a window ran.  For the delay also the
share of the copy bandwidth by algorithmic bytes: 40 B per sample and channel
(the input, the output, two ring reads, one ring write; delay-simple: 32 B)
over the time, against the best 1:1 copy rate tools/hbm_probe reports in the
same run when that probe has been built (`not measured` otherwise).  The first
samples of the first and last channel are checked against the restated
reference before timing.

  python tools/delayfx_bench.py [--sweep] [--out profiles/delayfx_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from fdn_bench import ROOT, row, windows  # noqa: E402  (also sets sys.path)

FS = 48000.0
SHAPES = [(256, 1 << 20), (4096, 1 << 16)]
CHECK_N = 2048
SWEEP_TIMES = [0.001, 0.002, 0.004, 0.008, 0.016, 0.032, 0.064, 0.128]


def hbm_copy_gbps():
    """The best `copy` rate of tools/hbm_probe (GB/s), or None when it is not built."""
    probe = ROOT / "tools" / "hbm_probe"
    if not probe.exists():
        return None
    r = subprocess.run([str(probe)], capture_output=True, text=True, timeout=300)
    rates = [float(m.group(1)) for line in r.stdout.splitlines() if line.lstrip().startswith("copy")
             for m in [re.search(r"([0-9.]+) GB/s", line)] if m]
    return max(rates) if rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "delayfx_bench.json"))
    ap.add_argument("--sweep", action="store_true", help="also sweep the delay time with each regime forced")
    args = ap.parse_args()

    import torch

    import delayfx_ref as R
    from algodsp import _lib, processors

    assert torch.cuda.is_available(), "delayfx_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    copy_gbps = hbm_copy_gbps()
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    def parity(h, ref, x, w, n, xh):
        w.copy_(x)
        h.process_device(w.data_ptr(), n, CHECK_N, sp)
        torch.cuda.synchronize()
        got = w[:, :CHECK_N].cpu().numpy()
        worst = 0.0
        for c in (0, x.shape[0] - 1):
            want = ref().process(xh[c])
            worst = max(worst, float(np.sqrt(np.mean((got[c] - want) ** 2)) / np.sqrt(np.mean(want ** 2))))
        return worst

    def bandwidth(d, ch, n, bytes_per_sample):
        gbps = ch * n * bytes_per_sample / (d["ms_per_call"]["median"] * 1e-3) / 1e9
        d["algorithmic_bytes_per_sample"] = bytes_per_sample
        d["algorithmic_gbytes_per_s"] = round(gbps, 1)
        d["share_of_copy_bandwidth"] = round(gbps / copy_gbps, 3) if copy_gbps else "not measured"

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
        w = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()

        def delay_case(name, time, regime=0, ramp_to=None):
            h = processors.Delay(FS, ch)
            h.SetTime(time)
            h.set_regime(regime)
            k = h.config().smooth_coeff

            def ref():
                r = R.Delay(FS)
                r.smoothCoeff = k
                r.SetTime(time)
                return r

            worst = parity(h, ref, x, w, n, xh)
            targets = [ramp_to, time]

            def restart():
                h.Reset()
                h.SetTime(time)
                w.copy_(x)

            def call():
                if ramp_to is not None:  # every call starts a ramp, so every call carries a trajectory
                    targets.reverse()
                    h.SetTargetTime(targets[0])
                h.process_device(w.data_ptr(), n, n, sp)

            ms, clocks, reps = windows(call, restart, stream)
            block, sub, ran, launches = h.kernel_info()
            d = row(name, ch, n, ms, clocks, reps, delay_seconds=time, block=block, sub_block=sub, regime_ran=ran,
                    launches_per_call=launches, forced_regime=regime, rel_rms_vs_reference_first_samples=worst)
            bandwidth(d, ch, n, 40)
            emit(d)
            h.close()

        delay_case("delay 0.25 s", 0.25)
        delay_case("delay 0.001 s", 0.001)
        delay_case("delay mid-ramp 0.25 s <-> 0.3 s", 0.25, ramp_to=0.3)
        if args.sweep:
            for t in SWEEP_TIMES:
                for regime in (1, 2):
                    delay_case(f"sweep delay {t} s regime {regime}", t, regime)

        for name, options in (("flanger defaults", {}), ("flanger base 0.0001 s", dict(base_delay_seconds=0.0001))):
            h = processors.Flanger(FS, ch, **options)
            worst = parity(h, lambda: R.Flanger(FS, **options), x, w, n, xh)

            def restart_f():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart_f, stream)
            block, sub, group, lds = h.kernel_info()
            emit(row(name, ch, n, ms, clocks, reps, block=block, sub_block=sub, channels_per_workgroup=group,
                     lds_bytes_per_workgroup=lds, rel_rms_vs_reference_first_samples=worst))
            h.close()

        samples = int(round(20.0 * FS / 1000.0))

        def simple_ref():
            s = R.SimpleDelay()
            s.Configure(FS, 20.0)
            return s

        for name, regime in [("delay-simple 20 ms", 0)] + \
                ([(f"sweep delay-simple 20 ms regime {r}", r) for r in (1, 2)] if args.sweep else []):
            h = processors.Delay(channels=ch, config=_lib.DelayConfig(sample_rate=FS, mode=1, delay_samples=samples))
            h.set_regime(regime)
            worst = parity(h, simple_ref, x, w, n, xh)

            def restart_s():
                h.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), restart_s, stream)
            block, sub, ran, launches = h.kernel_info()
            d = row(name, ch, n, ms, clocks, reps, block=block, regime_ran=ran, launches_per_call=launches,
                    forced_regime=regime, rel_rms_vs_reference_first_samples=worst)
            bandwidth(d, ch, n, 32)
            emit(d)
            h.close()

        for name, make in (("freeverb", lambda: processors.Reverb(ch)), ("fdn reverb", lambda: processors.FDNReverb(FS, ch))):
            f = make()

            def restart_r():
                f.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: f.process_device(w.data_ptr(), n, n, sp), restart_r, stream)
            emit(row(name, ch, n, ms, clocks, reps))
            f.close()
        del x, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/delayfx_bench.py", device=torch.cuda.get_device_name(0), sample_rate=FS,
               hbm_probe_copy_gbytes_per_s=copy_gbps if copy_gbps else "not measured", sweep=bool(args.sweep), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
