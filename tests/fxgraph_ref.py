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
    distortion  shaper_ref.Distortion of the config's fields (the distortion and dist-cheb nodes)
    bitcrusher  shaper_ref.BitCrusher of the config's fields; `.ref` on its process is the instance, for a
                test that hands a fractional depth's quantLevels over from the device (sync_q of
                test_shaper_gpu.py)
    deesser     dynfx_ref.DeEsser through its setters
    transient   dynfx_ref.TransientShaper through its setters
                (both: attack_coeff / release_coeff 0 in the config means derived, as the library reads it; any
                other value is the coefficient itself)

Every runtime is [type, process, Reset]; Reset is the reference's own.
"""
import numpy as np

import delayfx_ref
import dynfx_ref
import fdn_ref
import modfx_ref
import oracle_lib as O
import shaper_ref


def host_spec(json_graph, fs, designer):
    """Chain.spec of a graph without a device handle, for the node types of the newer named graphs
    (tests/fxgraph_topologies.py NEWER): what Chain.LoadGraph records for them, from the same functions of
    algodsp.effectchain.  The GPU suite holds it against Chain.spec itself."""
    from algodsp import effectchain as E

    g = E.parse_graph(json_graph)
    order = [E.INPUT_NODE_ID] + [k for k in g.Order if k != E.INPUT_NODE_ID]
    idx = {k: i for i, k in enumerate(order)}
    spec = []
    for k in order:
        p, t = g.Nodes[k], g.Nodes[k].Type
        split = lambda q: g.Nodes[order[q]].Type == E.NODE_TYPE_SPLIT_FREQ
        sd = {"id": k, "bypassed": bool(p.Bypassed),
              "parents": [(idx[e[0]], 1 if split(idx[e[0]]) and e[2] == 1 else 0) for e in g.Incoming[k]]}
        fields = lambda cfg: {f: getattr(cfg, f) for f, _ in cfg._fields_}
        if k == E.INPUT_NODE_ID:
            sd["type"] = "input"
        elif k == E.OUTPUT_NODE_ID:
            sd["type"] = "output"
        elif t == E.NODE_TYPE_SPLIT_FREQ:
            lp, hp = E.split_freq_sections(p, fs)
            sd.update(type="split", sections=lp, sections2=hp)
        elif t in ("split", "sum"):
            sd["type"] = "pass"
        elif t in E.FILTER_TYPES:
            sd.update(type="biquad", sections=([], 1.0))
            if not p.Bypassed:
                secs, gain = E.filter_chain(p, fs, designer)
                sd["sections"] = (list(secs), gain)
        elif t == "dyn-compressor":
            sd.update(type="comp", comp=fields(E.compressor_config(p, fs)))
        elif t == "phaser":
            sd.update(type="phaser", phaser=fields(E.phaser_params(p, fs)))
        elif t in ("distortion", "dist-cheb"):
            cfg = E.distortion_params(p, fs) if t == "distortion" else E.dist_cheb_params(p, fs)
            sd.update(type="distortion", distortion=E._config_dict(cfg))
        elif t == "bitcrusher":
            sd.update(type="bitcrusher", bitcrusher=E._config_dict(E.bitcrusher_params(p, fs)))
        elif t == "dyn-deesser":
            sd.update(type="deesser", deesser=E._config_dict(E.deesser_params(p, fs)))
        elif t == "dyn-transient":
            sd.update(type="transient", transient=E._config_dict(E.transient_params(p, fs)))
        else:
            raise ValueError(f"host_spec: node type {t!r}")
        spec.append(sd)
    return spec


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
        if t in ("distortion", "bitcrusher"):
            c = dict(d[t])
            kind = shaper_ref.Distortion if t == "distortion" else shaper_ref.BitCrusher
            r = kind(c.pop("sample_rate"), **c)

            def process(block):
                return r.process_many(np.asarray(block, dtype=np.float64)[None, :])[0]

            process.ref = r
            return [t, process, r.Reset]
        if t == "deesser":
            c = d[t]
            r = dynfx_ref.DeEsser(c["sample_rate"])
            r.SetFrequency(c["freq_hz"]), r.SetQ(c["q"]), r.SetThreshold(c["threshold_db"]), r.SetRatio(c["ratio"])
            r.SetKnee(c["knee_db"]), r.SetAttack(c["attack_ms"]), r.SetRelease(c["release_ms"]), r.SetRange(c["range_db"])
            r.SetMode(c["mode"]), r.SetDetector(c["detector"]), r.SetFilterOrder(c["filter_order"])
            r.SetListen(c["listen"] != 0)
        elif t == "transient":
            c = d[t]
            r = dynfx_ref.TransientShaper(c["sample_rate"])
            r.SetAttackAmount(c["attack_amount"]), r.SetSustainAmount(c["sustain_amount"])
            r.SetAttack(c["attack_ms"]), r.SetRelease(c["release_ms"])
        else:
            return super().node_runtime(d)
        if c["attack_coeff"] != 0:
            r.attackCoeff = c["attack_coeff"]
        if c["release_coeff"] != 0:
            r.releaseCoeff = c["release_coeff"]

        def process(block):
            return r.ProcessInPlace(np.array(block, dtype=np.float64))

        process.ref = r
        return [t, process, r.Reset]

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
