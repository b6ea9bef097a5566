#!/usr/bin/env python3
"""Throughput of the polyphase resampler (ad_resampler_process_device) on one
MI355X, device-resident: 256 channels x 2^20 input samples per call at
160/147 Balanced, 2/1 Balanced, 1/2 Best and 1/1 with 32 taps, beside
ad_fir_process_device at 32 taps on the same channels and length (the 1/1
resampler does the same arithmetic as that call).

Per case: output Gsamples/s (median of the timed windows, with their min and
max), the HBM bytes/s that rate means under the 8 * (1 + down/up) bytes per
output model (each input read once, each output written once), the LDS bytes
per output of the kernel's layout, and which table / window path ran.  Each
case is first checked bit for bit against the restated reference on its first
samples.

  python tools/resample_bench.py [--out profiles/resample_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__)))
from rows_bench import HBM, ROOT  # noqa: E402  (also sets sys.path)

CHANNELS = 256
N_IN = 1 << 20
WINDOWS = 7      # timed windows per case
REPS = 40        # calls per window
WARM_S = 0.5     # warm-up: calls for at least this long before the first window
CHECK_N = 8192   # samples of the parity check


def windows(call, stream):
    """Warm up until the clocks have settled, then WINDOWS event-timed windows
    of REPS calls each; returns ms per call of every window."""
    import time

    import torch

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(REPS):
            call()
        e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / REPS)
    return out


def spread(ms, per_call):
    """per_call / ms for every window -> (median, min, max)."""
    r = sorted(per_call / m for m in ms)
    return statistics.median(r), r[0], r[-1]


def lds_bytes_per_output(info, up, down, T):
    """LDS traffic of the layout: T window reads per output, T coefficient
    reads per lane shared by its 4 outputs when up <= 256 (else one row per
    output), plus what staging writes, spread over the outputs it serves."""
    tile = info["tile"]
    x_reads = 8.0 * T if info["window_in_lds"] else 0.0
    c_reads = (8.0 * T / (4 if up <= 256 else 1)) if info["table_in_lds"] else 0.0
    win_stage = 8.0 * (((tile - 1) * down + up - 1) // up + T) / tile if info["window_in_lds"] else 0.0
    tab_stage = 8.0 * up * (T | 1) / (info["tiles_per_workgroup"] * tile) if info["table_in_lds"] else 0.0
    return dict(window_reads=x_reads, table_reads=c_reads, staging_writes=round(win_stage + tab_stage, 2),
                total=round(x_reads + c_reads + win_stage + tab_stage, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample_bench.json"))
    ap.add_argument("--channels", type=int, default=CHANNELS)
    ap.add_argument("--n-in", type=int, default=N_IN)
    args = ap.parse_args()

    import torch

    import resample_ref as RR
    from algodsp import processors, resample as R, signals

    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    ch, n = args.channels, args.n_in
    gen = torch.Generator(device=cuda)
    gen.manual_seed(0x5EED)
    x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    xh = x[:, :CHECK_N].cpu().numpy()

    cases = [("160/147 balanced", 160, 147, dict(quality=R.QualityBalanced)),
             ("2/1 balanced", 2, 1, dict(quality=R.QualityBalanced)),
             ("1/2 best", 1, 2, dict(quality=R.QualityBest)),
             ("1/1 T=32", 1, 1, dict(quality=R.QualityBalanced, taps_per_phase=32))]
    rows = []
    for name, up, down, opts in cases:
        r = R.NewRational(up, down, channels=ch, **opts)
        T = r.TapsPerPhase()
        info = r.kernel_info()
        cap = (n * up + down - 1) // down + 8
        y = torch.empty((ch, cap), dtype=torch.float64, device=cuda)
        # parity on the first CHECK_N samples, first and last channel
        k = r.process_device(x.data_ptr(), n, CHECK_N, y.data_ptr(), cap, cap, sp)
        torch.cuda.synchronize()
        got = y[:, :k].cpu().numpy()
        exact = all(np.array_equal(got[c].view(np.int64),
                                   RR.Ref(up, down, r.Prototype()).process_vec(xh[c]).view(np.int64))
                    for c in (0, ch - 1))
        r.Reset()
        produced = []

        def call():
            produced.append(r.process_device(x.data_ptr(), n, n, y.data_ptr(), cap, cap, sp))

        ms = windows(call, stream)
        n_out = statistics.mean(produced)
        med, lo, hi = spread(ms, ch * n_out / 1e6)  # Gsamples/s out
        bytes_per_out = 8.0 * (1.0 + down / up)
        tile = info["tile"]
        rows.append(dict(case=name, up=up, down=down, taps_per_phase=T, channels=ch, n_in=n, n_out=round(n_out, 1),
                         ms_per_call=dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4),
                                          max=round(max(ms), 4)),
                         out_gsamples_per_s=dict(median=round(med, 2), min=round(lo, 2), max=round(hi, 2)),
                         hbm_model_bytes_per_output=round(bytes_per_out, 3),
                         hbm_gbytes_per_s=round(med * bytes_per_out, 1),
                         hbm_share_of_peak=round(med * bytes_per_out / HBM, 3),
                         gflops=round(med * 2 * T, 1),
                         lds_bytes_per_output=lds_bytes_per_output(info, up, down, T),
                         table_path="lds" if info["table_in_lds"] else "global",
                         window_path=("global" if not info["window_in_lds"] else
                                      "lds, next window loaded ahead" if info["window_prefetch"] else "lds"),
                         tiles_per_workgroup=info["tiles_per_workgroup"],
                         tile=tile, lds_bytes_per_workgroup=info["lds_bytes"], bit_exact_first_samples=bool(exact)))
        print(json.dumps(rows[-1]), flush=True)
        r.close()
        del y

    # fir.Filter at 32 taps on the same channels and length
    f = processors.Filter(signals.make_test_kernel(32), channels=ch)
    y = torch.empty((ch, n), dtype=torch.float64, device=cuda)
    ms = windows(lambda: f.process_device(x.data_ptr(), n, y.data_ptr(), n, n, sp), stream)
    med, lo, hi = spread(ms, ch * n / 1e6)
    fir = dict(case="fir 32 taps", channels=ch, n=n,
               ms_per_call=dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4)),
               out_gsamples_per_s=dict(median=round(med, 2), min=round(lo, 2), max=round(hi, 2)),
               hbm_gbytes_per_s=round(med * 16.0, 1))
    print(json.dumps(fir), flush=True)
    f.close()

    doc = dict(tool="tools/resample_bench.py", device=torch.cuda.get_device_name(0), windows=WINDOWS,
               calls_per_window=REPS, hbm_peak_gbytes_per_s=HBM, resampler=rows, fir=fir)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
