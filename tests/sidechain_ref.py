"""One-channel reference interpreter of an effect graph with sidechain inputs
(a test helper): fxgraph_ref.FxGraph plus the two node types that take a second
input, dyn-lookahead and vocoder, built from the restatements
(tests/lookahead_ref.py, tests/vocoder_ref.py) and the node's config dict in
Chain.spec.

The rule is chain_process.go:124-175 and 226-259, applied afresh for every
block: on these two node types the edges with toPortIndex 1 are side parents
(Chain.spec's "side_parents") and the others main parents ("parents").  The
node's buffer is the mix of its main parents; the side buffer is the same mix
over the side parents (a copy for one, the edge-order sum times 1/k for more),
or a copy of the node's own input when there is none; the node runs
ProcessWithSidechain(dst, side): the limiter's detector, the vocoder's carrier
(runtime_misc.go:122-124).  A bypassed node mixes its main parents only.  The
reference itself filters the node's incoming list in place and loses a side
edge listed before a main edge from the second block on; neither the GPU
runtime nor this interpreter does.
"""
import numpy as np

import fxgraph_ref
import lookahead_ref
import oracle_lib as O
import vocoder_ref

SIDE_KINDS = ("lookahead", "vocoder")


class FxGraph(fxgraph_ref.FxGraph):
    def node_runtime(self, d):
        t = d["type"]
        if t == "lookahead":
            c = d[t]
            r = lookahead_ref.LookaheadLimiter(c["sample_rate"])  # lookaheadLimiterRuntime.Configure
            r.SetSampleRate(c["sample_rate"]), r.SetThreshold(c["threshold_db"])
            r.SetRelease(c["release_ms"]), r.SetLookahead(c["lookahead_ms"])

            def process(dst, side):
                return r.process_many(dst[None, :], side[None, :])[0]

            process.ref = r
            return [t, process, r.Reset]
        if t == "vocoder":
            c = d[t]
            r = vocoder_ref.Vocoder(c["sample_rate"])  # vocoderRuntime.Configure
            r.SetSampleRate(c["sample_rate"]), r.SetAttack(c["attack_ms"]), r.SetRelease(c["release_ms"])
            r.SetInputLevel(c["input_level"]), r.SetSynthLevel(c["synth_level"]), r.SetVocoderLevel(c["vocoder_level"])

            def process(dst, side):
                return r.process_many(dst[None, :], side[None, :])[0]

            process.ref = r
            return [t, process, r.Reset]
        return super().node_runtime(d)

    def process(self, block):
        """O.FxGraph.process with the side input of the two sidechain node types."""
        n = len(block)
        buf, low, high = {}, {}, {}

        def src(e):
            j, port = e
            if self.nodes[j]["type"] == "split":
                return high[j] if port == 1 else low[j]
            return buf[j]

        def mix(par):  # mixParentEdgesInto
            if not par:
                return np.zeros(n)
            if len(par) == 1:
                return src(par[0]).copy()
            acc = np.zeros(n)
            for e in par:
                acc = acc + src(e)
            return acc * (1.0 / len(par))

        for i, d in enumerate(self.nodes):
            if i == 0:
                buf[0] = np.array(block, dtype=np.float64)
                continue
            dst = mix(d["parents"])
            buf[i] = dst
            r = self.rt[i]
            if r[0] == "split":
                low[i], r[2] = O.biquad_chain_block(r[1], r[2], 1.0, dst)
                high[i], r[4] = O.biquad_chain_block(r[3], r[4], 1.0, dst)
                continue
            if d["type"] in ("output", "pass") or d["bypassed"]:
                continue
            if r[0] in SIDE_KINDS:  # processSidechainNode
                side = mix(d["side_parents"]) if d["side_parents"] else dst.copy()
                buf[i] = r[1](dst, side)
            elif r[0] == "biquad":
                buf[i], r[2] = O.biquad_chain_block(r[1], r[2], r[3], dst)
            elif r[0] in ("comp", "verb"):
                buf[i] = r[1].process_in_place(dst)
            elif r[0] == "conv":
                rev = r[1].process_block(dst)
                buf[i] = r[3] * dst + r[2] * rev
            elif len(r) > 1:
                buf[i] = r[1](dst)
        return buf[[i for i, d in enumerate(self.nodes) if d["type"] == "output"][0]]
