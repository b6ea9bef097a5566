"""One-channel reference interpreter of an effect graph for every node type the
GPU graph runtime runs (a test helper; the topology suite's expected values).

oracle_lib.FxGraph restates Chain.Process (chain_process.go:11-319): nodes in
topological order, mixParentEdgesInto (zeros / copy / the sum in edge order
times 1/k), split-freq bands read by port (a bypassed split still splits),
_output, pass and bypassed nodes only mix.  Its runtimes are the C oracle's
(biquad, dynamics, Freeverb, partitioned convolution); this class adds the
Python restatements of the other nodes, each built from the node's config dict
in Chain.spec the way its stand-alone GPU test builds it:

    fdn      fdn_ref.FDN + the setters of configureFDNReverb
    delay    delayfx_ref.Delay (SetSampleRate, SetTargetTime, SetFeedback, SetMix: it starts at 0.25 s
             and ramps) or, mode 1, delayfx_ref.SimpleDelay of delay_samples
    flanger  delayfx_ref.Flanger
    phaser, tremolo, ringmod   modfx_ref.Phaser / Tremolo / RingModulator
"""
import numpy as np

import delayfx_ref
import fdn_ref
import modfx_ref
import oracle_lib as O


class FxGraph(O.FxGraph):
    def node_runtime(self, d):
        t = d["type"]
        if t == "fdn":
            c = d["fdn"]
            r = fdn_ref.FDN(c["sample_rate"])
            r.SetWet(c["wet"]), r.SetDry(c["dry"]), r.SetRT60(c["rt60_seconds"]), r.SetDamp(c["damp"])
            r.SetPreDelay(c["pre_delay_seconds"]), r.SetModDepth(c["mod_depth_seconds"]), r.SetModRate(c["mod_rate_hz"])
            return [t, r.process, r.Reset]
        if t == "delay":
            c = d["delay"]
            if c["mode"] == 1:
                r = delayfx_ref.SimpleDelay()
                r.delaySamples, r.buf = c["delay_samples"], [0.0] * (c["delay_samples"] + 1)

                def clear():
                    r.buf, r.write = [0.0] * len(r.buf), 0

                return [t, r.process, clear]
            r = delayfx_ref.Delay(c["sample_rate"])
            r.SetSampleRate(c["sample_rate"]), r.SetTargetTime(c["time_seconds"])
            r.SetFeedback(c["feedback"]), r.SetMix(c["mix"])
            return [t, r.process, r.Reset]
        if t == "flanger":
            c = d["flanger"]
            r = delayfx_ref.Flanger(c["sample_rate"], rate_hz=c["rate_hz"], depth_seconds=c["depth_seconds"],
                                    base_delay_seconds=c["base_delay_seconds"], feedback=c["feedback"], mix=c["mix"])
            return [t, r.process, r.Reset]
        if t == "phaser":
            c = d["phaser"]
            r = modfx_ref.Phaser(c["sample_rate"], rate_hz=c["rate_hz"], min_freq_hz=c["min_freq_hz"],
                                 max_freq_hz=c["max_freq_hz"], stages=c["stages"], feedback=c["feedback"],
                                 mix=c["mix"])
            return [t, r.process, r.Reset]
        if t in ("tremolo", "ringmod"):
            c = {k: v for k, v in d[t].items() if k not in ("sample_rate", "smoothing_coeff")}
            r = modfx_ref.KINDS[t](d[t]["sample_rate"], **c)
            return [t, r.process, r.Reset]
        return super().node_runtime(d)

    def reset(self):
        """ad_fx_graph_reset: every node's own Reset.  The feedback delay's keeps
        the ramp where it is (delay.go:131-137), so a graph with a delay node that
        is still ramping does not repeat its first output after it."""
        for r in self.rt:
            if r[0] == "biquad":
                r[2] = np.zeros_like(r[2])
            elif r[0] == "split":
                r[2], r[4] = np.zeros_like(r[2]), np.zeros_like(r[4])
            elif r[0] in ("comp", "verb", "conv"):
                r[1].reset()
            elif len(r) > 2:
                r[2]()
