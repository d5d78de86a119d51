// The Nesti-Net graph (models/experts_n_est.py:40-314) as a list of kernel launches per tower, built from the configuration alone
// (graph.cpp).  Host only.
#pragma once
#include <string>
#include <vector>

#include "host.h"

namespace nesti {

struct LayerDesc {
  std::string scope;
  std::string scope2;        // non-empty: a second 1x1 layer on the same input, fused into this launch
  int pool_k = 1;            // avg-pool window applied to scope2's pre-activation (conv4 of an inception)
  bool is_fc = false;
  int k = 1;                 // kernel size (1 for fc)
  int log2S = 0;             // spatial index space the layer runs at
  int s_real = 0;            // 3: the 3^3 Gaussian grid embedded in the 4^3 index space (0: the volume is 2^log2S)
  int cin = 0, cout = 0;     // real channel counts (TF variable shapes); scope2 has the same shape
  std::vector<int> in_pos;   // real input channel -> position inside the padded input slice
  int Cin_p = 0, Cout_p = 0;
  bool bn = true, relu = true;
};

struct BufSpec { int log2S; int C; bool f32; bool aux8 = false; };   // aux8: side buffer of e4m3 planes, 2 bytes per channel (conv8n.hip X8)

struct Op {
  enum Kind { CONV, MAX, MAX3 } kind;   // MAX3: max_pool3d [3,3,3] stride 2 SAME, 3^3 (embedded) -> 2^3
  int in_buf = 0, in_coff = 0, out_buf = 0, out_coff = 0, out_coff2 = 0;
  int in_cstride = 0;          // 0: the input buffer's channel count; else a flattened view (FC on S^3 x C)
  int mp_buf = -1, mp_mode = 0; // fused 2^3 max-pool of the first tile group into this buffer (1: pooled only, 2: both)
  int mp_mode2 = 0;             // 1: the conv4 half writes only its pooled tensor too (host.h: ConvParams::mp_mode2)
  int layer = -1;
  int C = 0, k = 0, log2S = 0;
  bool out_f32 = false;
  // FP8 cross terms (expert towers of NESTI_F16X8 / NESTI_F16X8C models): a block's conv1 (aux_out_buf >= 0) can also write the e4m3
  // planes of its outputs; the block's tap layers (aux_in_buf >= 0, x8_bit = their bit of nesti_model::x8_mask) read them.
  // x8_bits (producer) = the bits of the tap layers that read its planes; aux_layer (consumer) = the producer's layer index
  int aux_out_buf = -1, aux_in_buf = -1, x8_bit = -1, x8_bits = 0, aux_layer = -1;
};

struct Tower {
  std::vector<BufSpec> bufs;   // bufs[0] = MuPS X0 (external)
  std::vector<Op> ops;
  int out_buf = -1;            // f32 [NB, 64]
  int n_out = 0;               // real outputs (E or 3)
  bool side_tail = false;      // the aux8 buffers share ONE block behind everything else (place_tower): the gating net's stage-2 form
};

struct ChanMap { std::vector<int> pos; int C = 0; };   // real channel -> padded position, padded width

struct Graph {
  nesti_config_t cfg;
  int gate_x0_log2S() const { return cfg.grid_n == 3 ? 2 : 3; }   // index space of the MuPS rows of one point
  int mups_cstride = 64;
  bool x8 = false;           // NESTI_F16X8 / NESTI_F16X8C: the expert towers carry side buffers for the FP8 cross terms
  std::vector<LayerDesc> layers;
  Tower gate;
  // NESTI_F16X8C (x8 and a gating net on the 8^3 grid): the gating net once more, same layers and launches, with the side buffers of
  // its three 8^3 blocks (bits 0 .. 5 of Pass::x8_mask = inception1 conv2 / conv3, inception2 ..., inception3 ...) -- the form the
  // recheck's stage 2 runs (model.hip: gate_cascade).  `gate` itself stays free of them: the filter pass and stage 3 never pay for them
  Tower gate2;
  bool has_gate2() const { return !gate2.ops.empty(); }
  std::vector<Tower> experts;
  // -1: the gating net (x8_mask != 0: its stage-2 form), else an expert
  const Tower& tower(int t, int x8_mask = 0) const { return t < 0 ? (x8_mask && has_gate2() ? gate2 : gate) : experts[t]; }
};

// x8: an NESTI_F16X8 / NESTI_F16X8C model (only experts_n_est on the 8^3 grid gets the side buffers)
int build_graph(const nesti_config_t* cfg, Graph* g, bool x8 = false);

}  // namespace nesti
