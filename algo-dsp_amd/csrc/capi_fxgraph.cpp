// Batched effect-chain graph runtime: `channels` copies of one effectchain
// graph (dsp/effectchain) run together on the GPU, one lane per channel.
//
// Reference semantics (chain_process.go:11-319): nodes run in topological
// order; a node's input is the average of its parents' outputs
// (mixParentEdgesInto, :295-318: zeros without parents, a copy for one, the
// sum in edge order times 1/k for k), split-freq nodes write an LR4 low and
// high band (crossover.ProcessBlock, filter/crossover/crossover.go:80-94) that
// their consumers read by port, _output and bypassed nodes only mix, and every
// other node processes its buffer in place.  The output node's buffer is the
// result.
//
// Compilation (ad_fx_graph_create) turns the node list into device ops:
//   * a node whose single parent port feeds nobody else takes over that
//     buffer (no copy; in-place processing as the reference's copy-then-
//     process gives the same values);
//   * consecutive in-place nodes on one buffer fuse into one effect-chain
//     launch when their stages come in the kernel's order: biquad sections
//     (consecutive filter nodes concatenate: per sample, chain after chain),
//     then one compressor/limiter, then one Freeverb.  Per-sample fusion is
//     exact (every stage is causal and sees only its predecessor's output of
//     the same sample), so results are bit-identical with node-by-node runs;
//   * fan-in mixes are one kernel (k_fx_mix) in the reference's summation
//     order; the split-freq low band runs in place on the node's buffer and
//     the high band on a copy;
//   * the reverbs other than Freeverb, the delays and the modulation effects
//     (flanger, phaser, tremolo, ringmod) and the waveshapers (distortion,
//     dist-cheb, bitcrusher), the de-esser, the transient shaper, the spectral
//     freeze and the two pitch shifters are ops of their own on their
//     handles;
//   * the lookahead limiter and the vocoder are ops that rewrite the node's
//     buffer in place and read a second, side buffer (op.srcs): the mix of the
//     node's side parents.  A side consumer counts among a parent's consumers,
//     so the parent's buffer is not handed to a main consumer that would
//     rewrite it, and schedule() orders the side read after its producer and
//     any later writer of that buffer after the read, across lanes;
//   * independent branches run concurrently on up to 8 streams (schedule()).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "ad_common.hpp"
#include "dsp_kernels.hpp"
#include "pitchtime_kernels.hpp"

using namespace adsp;

namespace adsp {
void fx_chain_allow_staged(ad_fx_chain* h, bool on);  // capi_dsp.cpp
}

namespace {

void ck(int rc) {
  if (rc != AD_OK) AD_FAIL(rc, ad_last_error());
}

// An effect handle the graph owns, behind the three calls the graph makes on it.
struct Owned {
  void* h = nullptr;
  int (*process)(void*, double*, int64_t, int64_t, void*) = nullptr;  // in place; null where run() spells the call out
  int (*reset)(void*) = nullptr;
  void (*destroy)(void*) = nullptr;
};

// The record of a handle from its typed ABI functions: ad_X_process_device, ad_X_reset, ad_X_destroy.
template <class H, auto Process, int (*Reset)(H*), void (*Destroy)(H*)>
Owned own(H* h) {
  Owned o;
  o.h = h;
  if constexpr (std::is_invocable_v<decltype(Process), H*, double*, int64_t, int64_t, void*>)
    o.process = [](void* p, double* d, int64_t stride, int64_t n, void* s) {
      return Process(static_cast<H*>(p), d, stride, n, s);
    };
  o.reset = [](void* p) { return Reset(static_cast<H*>(p)); };
  o.destroy = [](void* p) { Destroy(static_cast<H*>(p)); };
  return o;
}

struct FxOp {
  // CHAIN and later kinds process dst in place (schedule() relies on the order)
  enum Kind { ZERO, COPY, MIX, CHAIN, HANDLE, LOOKAHEAD, VOCODER } kind;
  int dst = -1;                  // buffer id (written; CHAIN and later kinds: read and written in place)
  std::vector<int> srcs;         // COPY / MIX: buffers read; LOOKAHEAD / VOCODER: the side buffer, if any (read only)
  int handle = -1;               // CHAIN and later kinds: the handle, an index into ad_fx_graph::owned
  ad_fx_chain* chain = nullptr;  // CHAIN: that handle, typed (schedule() sets its staging)
  // schedule (see schedule()): lane 0 is the caller's stream
  int lane = 0;
  std::vector<int> waits;  // ops on other lanes this op waits for
  bool signal = false;     // another lane waits for this op
};

// Stage group under construction for the fusion pass.
struct Group {
  std::vector<double> sections;  // [nsec][6]
  const ad_fx_node* dyn = nullptr;  // the dynamics node (compressor / limiter / expander / gate)
  const double* verb = nullptr;
  bool open = false;
  int buf = -1;
  int level() const { return verb ? 3 : (dyn ? 2 : (sections.empty() ? 0 : 1)); }
};

}  // namespace

struct ad_fx_graph {
  int device = 0, channels = 0;
  hipStream_t stream = nullptr;
  int nbuf = 1;          // buffer 0 = the caller's block
  int out_buf = 0;
  std::vector<FxOp> ops;
  // Every handle of the graph, chains included, in creation order.  Reset and destroy walk it in that order,
  // not type by type: the handles are independent, and each reset waits for its own handle's last call.
  std::vector<Owned> owned;
  DevBuf<double> pool;   // buffers 1..nbuf-1, [nbuf-1][channels][cap]
  int64_t cap = 0;
  DevBuf<double> work;   // host-call staging
  int lanes_used = 1;
  std::vector<int> lane_tail;        // last op of lanes 1..
  hipStream_t lane[8] = {};          // lanes 1..: internal streams
  hipEvent_t start_ev = nullptr;
  std::vector<hipEvent_t> op_ev;     // per op (signalling ops only)
  ~ad_fx_graph() {
    for (auto& e : op_ev)
      if (e) (void)hipEventDestroy(e);
    if (start_ev) (void)hipEventDestroy(start_ev);
    for (auto& l : lane)
      if (l) {
        (void)hipStreamSynchronize(l);
        (void)lib_stream_destroy(l);
      }
    for (Owned& o : owned) o.destroy(o.h);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)lib_stream_destroy(stream);
    }
  }
};

namespace {

// an op of `kind` on buffer `buf` for the handle created last
FxOp handle_op(const ad_fx_graph* g, FxOp::Kind kind, int buf) {
  FxOp op{kind};
  op.dst = buf;
  op.handle = (int)g->owned.size() - 1;
  return op;
}

// a new chain and its op on buffer `buf` (not yet in g->ops: the caller sets the chain's stages first)
FxOp new_chain(ad_fx_graph* g, int buf) {
  ad_fx_chain* c = nullptr;
  ck(ad_fx_chain_create(g->channels, g->device, &c));
  g->owned.push_back(own<ad_fx_chain, ad_fx_chain_process_device, ad_fx_chain_reset, ad_fx_chain_destroy>(c));
  FxOp op = handle_op(g, FxOp::CHAIN, buf);
  op.chain = c;
  return op;
}

void flush(ad_fx_graph* g, Group& gr) {
  if (!gr.open) return;
  if (gr.level() > 0) {
    const FxOp op = new_chain(g, gr.buf);
    ad_fx_chain* c = op.chain;
    if (!gr.sections.empty()) ck(ad_fx_chain_set_eq(c, gr.sections.data(), (int)(gr.sections.size() / kSecStride), 0));
    if (gr.dyn) {
      if (gr.dyn->dyn_mode == 0)
        ck(ad_fx_chain_set_compressor(c, gr.dyn->comp));
      else
        ck(ad_fx_chain_set_expander(c, gr.dyn->comp, gr.dyn->dyn_mode == 2, gr.dyn->dyn_range_db,
                                    gr.dyn->dyn_hold_ms));
    }
    if (gr.verb) ck(ad_fx_chain_set_freeverb(c, gr.verb[0], gr.verb[1], gr.verb[2], gr.verb[3], gr.verb[4]));
    g->ops.push_back(op);
  }
  gr = Group{};
}

// the configuration of node i when it is there in full: cfg[i] of the size of the node type's structure
template <class Cfg>
const Cfg* node_cfg(const ad_fx_node_cfg* cfg, int i) {
  if (!cfg || !cfg[i].config || cfg[i].bytes != (int64_t)sizeof(Cfg)) return nullptr;
  return static_cast<const Cfg*>(cfg[i].config);
}

// The side parents of node i (the edges with toPortIndex 1 of a dyn-lookahead or vocoder node), or none.
struct Side {
  int n = 0;
  const int* parents = nullptr;
  const int* ports = nullptr;
};
Side side_of(const ad_fx_node* nodes, const ad_fx_node_cfg* cfg, int i) {
  Side s;
  if (nodes[i].type == AD_FXN_LOOKAHEAD) {
    const ad_fx_lookahead_node* c = node_cfg<ad_fx_lookahead_node>(cfg, i);
    if (c) s = Side{c->n_side, c->side_parents, c->side_ports};
  } else if (nodes[i].type == AD_FXN_VOCODER) {
    const ad_fx_vocoder_node* c = node_cfg<ad_fx_vocoder_node>(cfg, i);
    if (c) s = Side{c->n_side, c->side_parents, c->side_ports};
  }
  return s;
}

// ---- the node types that are ops of their own on a handle -----------------------
// Where node i's config lies (null: it is missing): a field of the node or of ext[i], cfg[i] of the size of
// the type's structure, or the `config` of a side node's structure there; the reverb-conv node is its own.
using Source = const void* (*)(const ad_fx_node& d, const ad_fx_node_ext* ext, const ad_fx_node_cfg* cfg, int i);
template <auto Field>
const void* in_node(const ad_fx_node& d, const ad_fx_node_ext*, const ad_fx_node_cfg*, int) {
  return d.*Field;
}
template <auto Field>
const void* in_ext(const ad_fx_node&, const ad_fx_node_ext* ext, const ad_fx_node_cfg*, int i) {
  return ext ? ext[i].*Field : nullptr;
}
template <class Cfg>
const void* in_cfg(const ad_fx_node&, const ad_fx_node_ext*, const ad_fx_node_cfg* cfg, int i) {
  return node_cfg<Cfg>(cfg, i);
}
template <class Node>
const void* in_side_cfg(const ad_fx_node&, const ad_fx_node_ext*, const ad_fx_node_cfg* cfg, int i) {
  const Node* c = node_cfg<Node>(cfg, i);
  return c ? &c->config : nullptr;
}
const void* node_itself(const ad_fx_node& d, const ad_fx_node_ext*, const ad_fx_node_cfg*, int) { return &d; }

template <class Cfg, int (*Validate)(const Cfg*)>
int valid(const void* cfg) {
  return Validate(static_cast<const Cfg*>(cfg));
}

// ad_X_create(cfg, channels, device, out) into g->owned
template <class H, class Cfg, int (*Create)(const Cfg*, int, int, H**), auto Process, int (*Reset)(H*), void (*Destroy)(H*)>
void create(ad_fx_graph* g, const void* cfg) {
  H* h = nullptr;
  ck(Create(static_cast<const Cfg*>(cfg), g->channels, g->device, &h));
  g->owned.push_back(own<H, Process, Reset, Destroy>(h));
}

void create_conv(ad_fx_graph* g, const void* node) {
  const ad_fx_node& d = *static_cast<const ad_fx_node*>(node);
  ad_conv* c = nullptr;
  ck(ad_conv_reverb_multi_create(d.ir, d.ir_len, d.conv_min_order, g->channels, g->device, &c));
  g->owned.push_back(own<ad_conv, ad_conv_reverb_multi_process_device, ad_conv_reset, ad_conv_destroy>(c));
  ck(ad_conv_reverb_set_wet_dry(c, d.conv_wet, d.conv_dry));
}

// One row per node type.  A type the runtime supports has a row here or is one of the structural types
// (input ... freeverb, which compile() handles itself).  `validate` is there for the types whose config is
// checked before anything is created; the others' create refuses a bad config.
struct NodeType {
  int type;
  FxOp::Kind kind;
  Source config;
  int (*validate)(const void* cfg);
  void (*create)(ad_fx_graph* g, const void* cfg);
  const char* missing;  // the error of a node without its config (or, validated, without a valid one of its size)
};
const NodeType kNodeTypes[] = {
    {AD_FXN_CONV_REVERB, FxOp::HANDLE, node_itself, nullptr, create_conv, ""},
    {AD_FXN_FDN_REVERB, FxOp::HANDLE, in_node<&ad_fx_node::fdn>, nullptr,
     create<ad_fdn, ad_fdn_config, ad_fdn_create, ad_fdn_process_device, ad_fdn_reset, ad_fdn_destroy>,
     "fx graph: reverb-fdn node without config"},
    {AD_FXN_DELAY, FxOp::HANDLE, in_node<&ad_fx_node::delay>, nullptr,
     create<ad_delay, ad_delay_config, ad_delay_create, ad_delay_process_device, ad_delay_reset, ad_delay_destroy>,
     "fx graph: delay node without config"},
    {AD_FXN_FLANGER, FxOp::HANDLE, in_node<&ad_fx_node::flanger>, nullptr,
     create<ad_flanger, ad_flanger_config, ad_flanger_create, ad_flanger_process_device, ad_flanger_reset,
            ad_flanger_destroy>,
     "fx graph: flanger node without config"},
    {AD_FXN_PHASER, FxOp::HANDLE, in_ext<&ad_fx_node_ext::phaser>, nullptr,
     create<ad_phaser, ad_phaser_config, ad_phaser_create, ad_phaser_process_device, ad_phaser_reset, ad_phaser_destroy>,
     "fx graph: phaser node without config"},
    {AD_FXN_TREMOLO, FxOp::HANDLE, in_ext<&ad_fx_node_ext::tremolo>, nullptr,
     create<ad_tremolo, ad_tremolo_config, ad_tremolo_create, ad_tremolo_process_device, ad_tremolo_reset,
            ad_tremolo_destroy>,
     "fx graph: tremolo node without config"},
    {AD_FXN_RINGMOD, FxOp::HANDLE, in_ext<&ad_fx_node_ext::ringmod>, nullptr,
     create<ad_ringmod, ad_ringmod_config, ad_ringmod_create, ad_ringmod_process_device, ad_ringmod_reset,
            ad_ringmod_destroy>,
     "fx graph: ringmod node without config"},
    {AD_FXN_DISTORTION, FxOp::HANDLE, in_cfg<ad_distortion_config>, valid<ad_distortion_config, ad_distortion_validate>,
     create<ad_distortion, ad_distortion_config, ad_distortion_create, ad_distortion_process_device,
            ad_distortion_reset, ad_distortion_destroy>,
     "fx graph: distortion node without a valid config of its size"},
    {AD_FXN_BITCRUSHER, FxOp::HANDLE, in_cfg<ad_bitcrusher_config>, valid<ad_bitcrusher_config, ad_bitcrusher_validate>,
     create<ad_bitcrusher, ad_bitcrusher_config, ad_bitcrusher_create, ad_bitcrusher_process_device,
            ad_bitcrusher_reset, ad_bitcrusher_destroy>,
     "fx graph: bitcrusher node without a valid config of its size"},
    {AD_FXN_DEESSER, FxOp::HANDLE, in_cfg<ad_deesser_config>, valid<ad_deesser_config, ad_deesser_validate>,
     create<ad_deesser, ad_deesser_config, ad_deesser_create, ad_deesser_process_device, ad_deesser_reset,
            ad_deesser_destroy>,
     "fx graph: de-esser node without a valid config of its size"},
    {AD_FXN_TRANSIENT, FxOp::HANDLE, in_cfg<ad_transient_config>, valid<ad_transient_config, ad_transient_validate>,
     create<ad_transient, ad_transient_config, ad_transient_create, ad_transient_process_device, ad_transient_reset,
            ad_transient_destroy>,
     "fx graph: transient shaper node without a valid config of its size"},
    {AD_FXN_SPECFREEZE, FxOp::HANDLE, in_cfg<ad_specfreeze_config>, valid<ad_specfreeze_config, ad_specfreeze_validate>,
     create<ad_specfreeze, ad_specfreeze_config, ad_specfreeze_create, ad_specfreeze_process_device,
            ad_specfreeze_reset, ad_specfreeze_destroy>,
     "fx graph: spectral freeze node without a valid config of its size"},
    {AD_FXN_PITCHSPEC, FxOp::HANDLE, in_cfg<ad_pitchspec_config>, valid<ad_pitchspec_config, ad_pitchspec_validate>,
     create<ad_pitchspec, ad_pitchspec_config, ad_pitchspec_create, ad_pitchspec_process_device, ad_pitchspec_reset,
            ad_pitchspec_destroy>,
     "fx graph: spectral pitch shifter node without a valid config of its size"},
    {AD_FXN_LOOKAHEAD, FxOp::LOOKAHEAD, in_side_cfg<ad_fx_lookahead_node>, valid<ad_lookahead_config, ad_lookahead_validate>,
     create<ad_lookahead, ad_lookahead_config, ad_lookahead_create, ad_lookahead_process_device, ad_lookahead_reset,
            ad_lookahead_destroy>,
     "fx graph: lookahead limiter node without a valid config of its size"},
    {AD_FXN_VOCODER, FxOp::VOCODER, in_side_cfg<ad_fx_vocoder_node>, valid<ad_vocoder_config, ad_vocoder_validate>,
     create<ad_vocoder, ad_vocoder_config, ad_vocoder_create, ad_vocoder_process_device, ad_vocoder_reset,
            ad_vocoder_destroy>,
     "fx graph: vocoder node without a valid config of its size"},
    {AD_FXN_PITCHTIME, FxOp::HANDLE, in_cfg<ad_pitchtime_config>, valid<ad_pitchtime_config, pitchtime_validate>,
     create<PitchTime, ad_pitchtime_config, pitchtime_create, pitchtime_process_device, pitchtime_reset,
            pitchtime_destroy>,
     "fx graph: time-domain pitch shifter node without a valid config of its size"},
};
const NodeType* node_type(int type) {
  for (const NodeType& t : kNodeTypes)
    if (t.type == type) return &t;
  return nullptr;
}

void compile(ad_fx_graph* g, const ad_fx_node* nodes, const ad_fx_node_ext* ext, const ad_fx_node_cfg* cfg, int n) {
  if (n < 2 || nodes[0].type != AD_FXN_INPUT) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: node 0 must be the input");
  // consumers of each (node, port)
  std::vector<int> uses((size_t)n * 2, 0);
  int out_node = -1;
  for (int i = 0; i < n; ++i) {
    const ad_fx_node& d = nodes[i];
    const NodeType* t = node_type(d.type);
    if (!t && (d.type < AD_FXN_INPUT || d.type > AD_FXN_FREEVERB))
      AD_FAIL(AD_ERR_UNKNOWN_EFFECT, "fx graph: node type not supported by the GPU runtime");
    if (d.type == AD_FXN_INPUT && i != 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: more than one input node");
    if (d.type == AD_FXN_OUTPUT) {
      if (out_node >= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: more than one output node");
      out_node = i;
    }
    if (d.n_parents < 0 || d.n_parents > AD_FX_MAX_PARENTS || (d.n_parents > 0 && !d.parents))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: bad parent list");
    for (int k = 0; k < d.n_parents; ++k) {
      const int p = d.parents[k];
      const int port = d.parent_ports ? d.parent_ports[k] : 0;
      if (p < 0 || p >= i) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: parents must precede their node (topological order)");
      if (port != 0 && !(port == 1 && nodes[p].type == AD_FXN_SPLIT_FREQ))
        AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: port 1 exists only on split-freq nodes");
      uses[(size_t)p * 2 + port]++;
    }
    if (d.type == AD_FXN_BIQUAD && (d.nsec < 0 || (d.nsec > 0 && !d.sections)))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: filter node without sections");
    if (d.type == AD_FXN_SPLIT_FREQ && (d.nsec <= 0 || !d.sections || d.nsec2 <= 0 || !d.sections2))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: split-freq node needs LP and HP sections");
    if (d.type == AD_FXN_COMPRESSOR && !d.comp) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: compressor without config");
    if (d.type == AD_FXN_CONV_REVERB && !d.bypassed && (!d.ir || d.ir_len <= 0))
      AD_FAIL(AD_ERR_EMPTY_IMPULSE_RESPONSE, "fx graph: reverb-conv node without an impulse response");
    if (t) {
      const void* c = t->config(d, ext, cfg, i);
      if (!c || (t->validate && t->validate(c) != AD_OK)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, t->missing);
    }
    // a side consumer counts: a parent it reads is not rewritten in place by that parent's main consumer
    const Side side = side_of(nodes, cfg, i);
    if (side.n < 0 || side.n > AD_FX_MAX_PARENTS) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: bad side parent list");
    for (int k = 0; k < side.n; ++k) {
      const int p = side.parents[k], port = side.ports[k];
      if (p < 0 || p >= i) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: side parents must precede their node");
      if (port != 0 && !(port == 1 && nodes[p].type == AD_FXN_SPLIT_FREQ))
        AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: port 1 exists only on split-freq nodes");
      uses[(size_t)p * 2 + port]++;
    }
    if (d.type == AD_FXN_COMPRESSOR && (d.dyn_mode < 0 || d.dyn_mode > 2))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: bad dynamics mode");
  }
  if (out_node < 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: no output node");

  std::vector<int> buf_of((size_t)n * 2, -1);  // buffer id of (node, port)
  buf_of[0] = 0;
  Group gr;
  for (int i = 1; i < n; ++i) {
    const ad_fx_node& d = nodes[i];
    // ---- the node's input (mixParentEdgesInto)
    int b;
    const int port0 = d.n_parents ? (d.parent_ports ? d.parent_ports[0] : 0) : 0;
    if (d.n_parents == 1 && uses[(size_t)d.parents[0] * 2 + port0] == 1) {
      b = buf_of[(size_t)d.parents[0] * 2 + port0];  // sole consumer: take the buffer over
    } else {
      b = g->nbuf++;
      FxOp op{d.n_parents == 0 ? FxOp::ZERO : (d.n_parents == 1 ? FxOp::COPY : FxOp::MIX)};
      op.dst = b;
      for (int k = 0; k < d.n_parents; ++k)
        op.srcs.push_back(buf_of[(size_t)d.parents[k] * 2 + (d.parent_ports ? d.parent_ports[k] : 0)]);
      flush(g, gr);
      g->ops.push_back(op);
    }
    if (gr.open && gr.buf != b) flush(g, gr);
    buf_of[(size_t)i * 2] = b;

    // ---- the node itself
    if (d.type == AD_FXN_SPLIT_FREQ) {
      flush(g, gr);
      // high band = HP chain on a copy, low band = LP chain in place
      const int hb = g->nbuf++;
      FxOp cp{FxOp::COPY};
      cp.dst = hb;
      cp.srcs.push_back(b);
      g->ops.push_back(cp);
      const FxOp lo = new_chain(g, b);
      ck(ad_fx_chain_set_eq(lo.chain, d.sections, d.nsec, 0));
      g->ops.push_back(lo);
      const FxOp hi = new_chain(g, hb);
      ck(ad_fx_chain_set_eq(hi.chain, d.sections2, d.nsec2, 0));
      g->ops.push_back(hi);
      buf_of[(size_t)i * 2 + 1] = hb;
      continue;
    }
    if (d.type == AD_FXN_OUTPUT || d.type == AD_FXN_PASS || d.bypassed) continue;
    if (const NodeType* t = node_type(d.type)) {  // an op of its own on a new handle
      flush(g, gr);
      int sb = -1;
      if (t->kind != FxOp::HANDLE) {
        // the side input (processSidechainNode chain_process.go:249-256): one side parent is read where it
        // lies, several mix into a buffer of their own; none means the node's own input, which the limiter
        // takes as "no sidechain" and the vocoder as one pointer for both inputs (a workgroup reads its samples
        // before it stores them)
        const Side side = side_of(nodes, cfg, i);
        if (side.n == 1) {
          sb = buf_of[(size_t)side.parents[0] * 2 + side.ports[0]];
        } else if (side.n > 1) {
          sb = g->nbuf++;
          FxOp mix{FxOp::MIX};
          mix.dst = sb;
          for (int k = 0; k < side.n; ++k) mix.srcs.push_back(buf_of[(size_t)side.parents[k] * 2 + side.ports[k]]);
          g->ops.push_back(mix);
        }
      }
      t->create(g, t->config(d, ext, cfg, i));
      FxOp op = handle_op(g, t->kind, b);
      if (sb >= 0) op.srcs.push_back(sb);
      g->ops.push_back(op);
      continue;
    }
    const int lvl = d.type == AD_FXN_BIQUAD ? 1 : (d.type == AD_FXN_COMPRESSOR ? 2 : 3);
    if (gr.open && (lvl < gr.level() || (lvl == gr.level() && lvl > 1))) flush(g, gr);
    gr.open = true;
    gr.buf = b;
    if (lvl == 1) {
      gr.sections.insert(gr.sections.end(), d.sections, d.sections + (size_t)d.nsec * kSecStride);
    } else if (lvl == 2) {
      gr.dyn = &d;
    } else {
      gr.verb = d.verb;
    }
  }
  flush(g, gr);
  g->out_buf = buf_of[(size_t)out_node * 2];
  if (g->out_buf != 0) {  // copyOutputToBlock (chain_process.go:274-283)
    FxOp op{FxOp::COPY};
    op.dst = 0;
    op.srcs.push_back(g->out_buf);
    g->ops.push_back(op);
  }
}

// Independent branches run concurrently: every chain op is only
// ceil(channels/64) workgroups (one lane per channel, serial in time), so the
// GPU has room for all of them at once.  Dependencies come from the buffers
// each op reads and writes (read-after-write, write-after-read and
// write-after-write); an op continues the lane of a dependency that is the
// lane's last op, otherwise it opens a new lane (at most kLanes), and it
// waits on events of dependencies on other lanes.
constexpr int kLanes = 8;
void schedule(ad_fx_graph* g) {
  const int nb = g->nbuf;
  std::vector<int> last_writer(nb, -1);
  std::vector<std::vector<int>> readers(nb);
  std::vector<int> tail(kLanes, -1);  // last op of each lane
  int used = 1;
  for (int i = 0; i < (int)g->ops.size(); ++i) {
    FxOp& op = g->ops[i];
    std::vector<int> reads = op.srcs;
    if (op.kind >= FxOp::CHAIN) reads.push_back(op.dst);  // the in-place kinds
    std::vector<int> deps;
    for (int b : reads)
      if (last_writer[b] >= 0) deps.push_back(last_writer[b]);
    if (last_writer[op.dst] >= 0) deps.push_back(last_writer[op.dst]);
    for (int r : readers[op.dst]) deps.push_back(r);
    std::sort(deps.begin(), deps.end());
    deps.erase(std::unique(deps.begin(), deps.end()), deps.end());
    deps.erase(std::remove(deps.begin(), deps.end(), i), deps.end());
    int lane = -1;
    for (int d : deps)
      if (tail[g->ops[d].lane] == d) {
        lane = g->ops[d].lane;
        break;
      }
    if (lane < 0) {
      if (deps.empty() && tail[0] < 0) lane = 0;
      else if (used < kLanes) lane = used++;
      else lane = i % kLanes;
    }
    op.lane = lane;
    for (int d : deps)
      if (g->ops[d].lane != lane) {
        op.waits.push_back(d);
        g->ops[d].signal = true;
      }
    tail[lane] = i;
    for (int b : reads) readers[b].push_back(i);
    readers[op.dst].clear();
    last_writer[op.dst] = i;
  }
  // the caller's stream (lane 0) waits for every other lane's last op
  g->lanes_used = used;
  for (FxOp& op : g->ops)
    if (op.kind == FxOp::CHAIN) adsp::fx_chain_allow_staged(op.chain, used == 1);
  for (int l = 1; l < used; ++l)
    if (tail[l] >= 0) {
      g->ops[tail[l]].signal = true;
      g->lane_tail.push_back(tail[l]);
    }
}

double* buf_ptr(ad_fx_graph* g, int b, double* d0) {
  return b == 0 ? d0 : g->pool.p + (size_t)(b - 1) * g->channels * g->cap;
}

void run(ad_fx_graph* g, double* d0, int64_t stride0, int64_t n, hipStream_t s) {
  if (n == 0) return;
  if (g->nbuf > 1 && n > g->cap) {
    AD_HIP(hipStreamSynchronize(s));
    for (int l = 1; l < g->lanes_used; ++l) AD_HIP(hipStreamSynchronize(g->lane[l]));
    g->cap = n;
    g->pool.alloc((size_t)(g->nbuf - 1) * g->channels * g->cap);
  }
  auto st = [&](int b) { return b == 0 ? stride0 : g->cap; };
  auto lane_stream = [&](int l) { return l == 0 ? s : g->lane[l]; };
  if (g->lanes_used > 1) {  // the other lanes start after the caller's prior work
    AD_HIP(hipEventRecord(g->start_ev, s));
    for (int l = 1; l < g->lanes_used; ++l) AD_HIP(hipStreamWaitEvent(g->lane[l], g->start_ev, 0));
  }
  for (size_t i = 0; i < g->ops.size(); ++i) {
    const FxOp& op = g->ops[i];
    hipStream_t ls = lane_stream(op.lane);
    for (int w : op.waits) AD_HIP(hipStreamWaitEvent(ls, g->op_ev[w], 0));
    double* dst = buf_ptr(g, op.dst, d0);
    switch (op.kind) {
      case FxOp::ZERO:
        AD_HIP(hipMemset2DAsync(dst, st(op.dst) * 8, 0, n * 8, g->channels, ls));
        break;
      case FxOp::COPY:
        AD_HIP(hipMemcpy2DAsync(dst, st(op.dst) * 8, buf_ptr(g, op.srcs[0], d0), st(op.srcs[0]) * 8, n * 8,
                                g->channels, hipMemcpyDeviceToDevice, ls));
        break;
      case FxOp::MIX: {
        FxMixArgs m{};
        m.nsrc = (int)op.srcs.size();
        for (int k = 0; k < m.nsrc; ++k) {
          m.src[k] = buf_ptr(g, op.srcs[k], d0);
          m.src_stride[k] = st(op.srcs[k]);
        }
        m.dst = dst;
        m.dst_stride = st(op.dst);
        m.n = n;
        m.channels = g->channels;
        launch_fx_mix(m, ls);
        AD_HIP(hipGetLastError());
        break;
      }
      case FxOp::CHAIN:
      case FxOp::HANDLE: {
        const Owned& o = g->owned[op.handle];
        ck(o.process(o.h, dst, st(op.dst), n, ls));
        break;
      }
      case FxOp::LOOKAHEAD: {
        const bool has = !op.srcs.empty();
        ck(ad_lookahead_process_device(static_cast<ad_lookahead*>(g->owned[op.handle].h), dst, st(op.dst),
                                       has ? buf_ptr(g, op.srcs[0], d0) : nullptr, has ? st(op.srcs[0]) : 0,
                                       has ? n : 0, n, ls));
        break;
      }
      case FxOp::VOCODER: {
        const bool has = !op.srcs.empty();
        ck(ad_vocoder_process_device(static_cast<ad_vocoder*>(g->owned[op.handle].h), dst, st(op.dst),
                                     has ? buf_ptr(g, op.srcs[0], d0) : dst, has ? st(op.srcs[0]) : st(op.dst), dst,
                                     st(op.dst), n, ls));
        break;
      }
    }
    if (op.signal) AD_HIP(hipEventRecord(g->op_ev[i], ls));
  }
  for (int t : g->lane_tail) AD_HIP(hipStreamWaitEvent(s, g->op_ev[t], 0));
}

template <class Fn>
int graph_guard(ad_fx_graph* g, Fn&& fn) {
  return guard([&] {
    if (!g) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null fx graph handle");
    DeviceScope ds(g->device);
    fn();
  });
}

}  // namespace

extern "C" {

int ad_fx_graph_create(const ad_fx_node* nodes, int n_nodes, int channels, int device, ad_fx_graph** out) {
  return ad_fx_graph_create_ext(nodes, nullptr, n_nodes, channels, device, out);
}

int ad_fx_graph_create_ext(const ad_fx_node* nodes, const ad_fx_node_ext* ext, int n_nodes, int channels, int device,
                           ad_fx_graph** out) {
  return ad_fx_graph_create_cfg(nodes, ext, nullptr, n_nodes, channels, device, out);
}

int ad_fx_graph_create_cfg(const ad_fx_node* nodes, const ad_fx_node_ext* ext, const ad_fx_node_cfg* cfg, int n_nodes,
                           int channels, int device, ad_fx_graph** out) {
  if (out) *out = nullptr;
  ad_fx_graph* raw = nullptr;
  const int rc = guard([&] {
    if (!nodes || n_nodes <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fx graph: no nodes");
    if (channels <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "channels must be positive");
    const int dev = pick_device(device);
    DeviceScope ds(dev);
    std::unique_ptr<ad_fx_graph> g(new ad_fx_graph());
    g->device = dev;
    g->channels = channels;
    AD_HIP(lib_stream_create(&g->stream));
    compile(g.get(), nodes, ext, cfg, n_nodes);
    schedule(g.get());
    for (int l = 1; l < g->lanes_used; ++l) AD_HIP(lib_stream_create(&g->lane[l]));
    AD_HIP(hipEventCreateWithFlags(&g->start_ev, hipEventDisableTiming));
    g->op_ev.assign(g->ops.size(), nullptr);
    for (size_t i = 0; i < g->ops.size(); ++i)
      if (g->ops[i].signal) AD_HIP(hipEventCreateWithFlags(&g->op_ev[i], hipEventDisableTiming));
    raw = g.release();
  });
  if (rc == AD_OK && out) *out = raw;
  return rc;
}

int ad_fx_graph_op_count(const ad_fx_graph* g, int* launches, int* buffers, int* lanes) {
  if (!g) return AD_ERR_INVALID_ARGUMENT;
  if (launches) *launches = (int)g->ops.size();
  if (buffers) *buffers = g->nbuf;
  if (lanes) *lanes = g->lanes_used;
  return AD_OK;
}

int ad_fx_graph_process_device(ad_fx_graph* g, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return graph_guard(g, [&] {
    if (n < 0 || stride < n) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
    run(g, d_buf, stride, n, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_fx_graph_process(ad_fx_graph* g, double* buf, int64_t n) {
  return graph_guard(g, [&] {
    if (n < 0 || (n > 0 && !buf)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;  // Chain.Process: an empty block is a no-op (chain_process.go:12-14)
    const size_t bytes = (size_t)g->channels * n * sizeof(double);
    g->work.reserve((size_t)g->channels * n);
    AD_HIP(hipMemcpyAsync(g->work.p, buf, bytes, hipMemcpyHostToDevice, g->stream));
    run(g, g->work.p, n, n, g->stream);
    AD_HIP(hipMemcpyAsync(buf, g->work.p, bytes, hipMemcpyDeviceToHost, g->stream));
    AD_HIP(hipStreamSynchronize(g->stream));
  });
}

int ad_fx_graph_reset(ad_fx_graph* g) {
  return graph_guard(g, [&] {
    for (const Owned& o : g->owned) ck(o.reset(o.h));
  });
}

void ad_fx_graph_destroy(ad_fx_graph* g) {
  if (!g) return;
  const int dev = g->device;
  int cur = -1;
  (void)hipGetDevice(&cur);
  if (cur != dev) (void)hipSetDevice(dev);
  delete g;
  if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
}

}  // extern "C"
