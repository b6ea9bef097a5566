#!/usr/bin/env python3
"""Throughput of the time-domain pitch shifter (algodsp.pitch.PitchShifter,
the AD_FXN_PITCHTIME node) on one MI355X, device-resident and in place: 256
channels x 2^20 samples and 4096 channels x 2^16 samples per call at 48 kHz,
at the ratios 2^(1/12), 2^(7/12), 0.5 and 2, with the reference's defaults
(82 / 10 / 28 ms) and the graph node's (40 / 10 / 15 ms), beside
processors.SpectralPitchShifter at +1 and +7 semitones on the same buffers in
the same run.

Per case: ms per call and Gsamples/s (median of the 7 timed windows after
warm-up, with their min and max); the search's multiply-add pairs per second
(frames x candidates x overlap x 2 per channel: the dot and the energy) and
that as a fraction of the FP64 bound blocked_dot.hpp names, 32 pairs per clock
per compute unit, on the whole call and, where the per-pass split could be
taken, on the search kernel's own time.  The split (search, assembly, position
row upload, resample) is one profiled call of a new object
through torch.profiler's kernel records; "unmeasured" where the profiler gave
none.

The first and last channel of a short call are checked on bits against the
restated reference before timing.

  python tools/pitchtime_bench.py [--out profiles/pitchtime_bench.json]
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
RATIOS = [("+1 semitone", math.pow(2, 1 / 12.0)), ("+7 semitones", math.pow(2, 7 / 12.0)), ("octave down", 0.5),
          ("octave up", 2.0)]
PARAMS = [("reference defaults", dict(sequence_ms=82.0, overlap_ms=10.0, search_ms=28.0)),
          ("node defaults", dict(sequence_ms=40.0, overlap_ms=10.0, search_ms=15.0))]
CHECK_N = 20000
PAIRS_PER_CLK_PER_CU = 32
# the profiled region holds one process_device call of a new object and nothing of torch's: its kernels by
# name, and its one host-to-device copy, the position row
PASSES = {"k_pt_search": "search", "k_pt_assemble": "assembly", "k_pt_resample": "resample",
          "Memcpy HtoD": "position row upload"}


def split_of(call):
    """Device milliseconds per pass of one call, from torch.profiler's records; None where it has none."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            for key, name in PASSES.items():
                if key in e.key and us > 0:
                    out[name] = out.get(name, 0.0) + us / 1e3
        return out if "search" in out else None
    except Exception as e:  # noqa: BLE001 - the split is a diagnostic
        print(f"no per-pass split: {e}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pitchtime_bench.json"))
    args = ap.parse_args()

    import torch

    import pitchtime_ref as R
    from algodsp import pitch, processors

    assert torch.cuda.is_available(), "pitchtime_bench needs a GPU"
    cuda = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = []

    def emit(d):
        rows.append(d)
        print(json.dumps(d), flush=True)

    for ch, n in SHAPES:
        gen = torch.Generator(device=cuda)
        gen.manual_seed(0x5EED)
        x = torch.randn((ch, n), dtype=torch.float64, device=cuda, generator=gen) * 0.5
        w = torch.empty_like(x)
        xh = x[:, :CHECK_N].cpu().numpy()

        for pname, params in PARAMS:
            for rname, ratio in RATIOS:
                h = pitch.PitchShifter(FS, ch, pitch_ratio=ratio, **params)
                w.copy_(x)
                h.process_device(w.data_ptr(), n, CHECK_N, sp)
                torch.cuda.synchronize()
                got = w[:, :CHECK_N].cpu().numpy()
                ref = R.PitchShifter(FS)
                ref.SetSequence(params["sequence_ms"]), ref.SetOverlap(params["overlap_ms"])
                ref.SetSearch(params["search_ms"]), ref.SetPitchRatio(ratio)
                exact = all(np.array_equal(got[c].view(np.uint64), ref.Process(xh[c]).view(np.uint64))
                            for c in (0, ch - 1))
                ms, clocks, reps = windows(lambda: h.process_device(w.data_ptr(), n, n, sp), lambda: w.copy_(x), stream)
                seq, ov, search, step = h.frame_lengths()
                target = max(int(pitch.go_round(n * ratio)), 1)
                frames = -(-target // step)
                pairs = ch * frames * (2 * search + 1) * ov * 2
                d = row(f"pitch-time {rname}, {pname}", ch, n, ms, clocks, reps, ratio=ratio, bit_exact_first_samples=exact,
                        sequence_len=seq, overlap_len=ov, search_len=search, frames=frames, search_pairs_per_call=pairs)
                hz = (d["sclk_mhz"] or 2400.0) * 1e6
                bound = PAIRS_PER_CLK_PER_CU * cus * hz
                d["search_gpairs_per_s_whole_call"] = round(pairs / (d["ms_per_call"]["median"] * 1e-3) / 1e9, 1)
                d["fp64_bound_fraction_whole_call"] = round(pairs / (d["ms_per_call"]["median"] * 1e-3) / bound, 4)
                h.close()
                fresh = pitch.PitchShifter(FS, ch, pitch_ratio=ratio, **params)
                w.copy_(x)
                torch.cuda.synchronize()
                passes = split_of(lambda: fresh.process_device(w.data_ptr(), n, n, sp))
                if passes:
                    total = sum(passes.values())
                    d["profiled_call_ms"] = {k: round(v, 3) for k, v in passes.items()}
                    d["pass_share"] = {k: round(v / total, 3) for k, v in passes.items()}
                    d["fp64_bound_fraction_search_kernel"] = round(pairs / (passes["search"] * 1e-3) / bound, 4)
                else:
                    d["pass_share"] = "unmeasured"
                fresh.close()
                emit(d)

        for semitones in (1, 7):
            s = processors.SpectralPitchShifter(FS, ch, frame_size=1024, analysis_hop=256)
            s.SetPitchSemitones(semitones)

            def restart():
                s.Reset()
                w.copy_(x)

            ms, clocks, reps = windows(lambda: s.process_device(w.data_ptr(), n, n, sp), restart, stream)
            emit(row(f"pitch-spectral +{semitones} semitone(s), frame 1024 hop 256", ch, n, ms, clocks, reps, yardstick=True))
            s.close()
        del x, w
        torch.cuda.empty_cache()

    doc = dict(tool="tools/pitchtime_bench.py", device=torch.cuda.get_device_name(0), compute_units=cus, sample_rate=FS,
               windows=WINDOWS, fp64_bound_pairs_per_clk_per_cu=PAIRS_PER_CLK_PER_CU, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
