// Batch-norm folding and the weight packer (pack.cpp): TF tensors -> the byte image of a layer's weights as the MFMA kernels read
// it, plus the padded bias.  Host only -- the caller uploads the image (model.hip: upload); nesti_debug_pack_layer hands the same image to tests.
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "graph.h"

namespace nesti {

struct TensorTable {
  std::map<std::string, const nesti_tensor_t*> by_name;
  const nesti_tensor_t* get(const std::string& n) const {
    auto it = by_name.find(n);
    return it == by_name.end() ? nullptr : it->second;
  }
};
inline TensorTable tensor_table(const nesti_tensor_t* tensors, int n) {
  TensorTable tt;
  for (int i = 0; i < n; ++i) if (tensors[i].name) tt.by_name[tensors[i].name] = &tensors[i];
  return tt;
}

// Expected variables of one layer, in TF naming (utils/tf_util.py:289-302, 332-342, 473-479).
void layer_tensors(const LayerDesc& d, std::vector<std::pair<std::string, std::vector<int64_t>>>* out);

// Which layers run on conv8n_kernel (conv8n.hip): the k^3 taps (k = 3, 5) on the 8^3 volume
bool use_conv8(const LayerDesc& d);
// PackMeta::kind of a layer packed for `dtype`: conv8n_kernel's, conv4n_kernel's, else conv_igemm_kernel's (conv.hip)
int layer_kind(const LayerDesc& d, int dtype);
// PackMeta::n_taps: the k^3 taps that can land inside the volume (the packers keep only those)
int layer_taps(const LayerDesc& d);

// Power-of-two pre-scale of the e4m3 activation planes a block's conv1 writes for the FP8 cross terms (PackMeta::x8_sc)
int x8_activation_exponent(const LayerDesc& d, const TensorTable& tt);

// What a launch needs to know about a packed layer beside its bytes
struct PackMeta {
  int TN = 64, n_tiles = 0, split_tile = 0, n_chunks = 0, n_taps = 0;
  int kind = 0;              // 0: conv_igemm_kernel (conv.hip), 2: conv8n_kernel (conv8n.hip: 4 points x a z half x 64 columns
                             // per workgroup), 3: conv4n_kernel (conv4n.hip: 16 points x 64 voxels x 64 columns)
  bool x3n = false;          // pair modes: K chunks [hi | lo] / [W_hi | W_lo], three MFMAs per fragment set
  float acc_scale = 1.0f;    // 2^-s when the packed weights carry a 2^s scale (NESTI_F16X3)
  int x8_sb = 0;             // X8 / X6 entries (rows [W_hi f16 16 ch | W_hi8 16 ch | W_lo8 16 ch], conv8n.hip X8): W_hi8 = e4m3(W_hi 2^sb),
                             // W_lo8 = e4m3(W_lo 2^(sb + 11))
  int x8_sc = 0;             // producer layers (an 8^3 block's conv1): hi8 = e4m3(v 2^sc), lo8 = e4m3(lo 2^(sc + 11))
  int8_t tap[kMaxTaps][4] = {};
};
// ... and the host image of it: [n_tiles][n_chunks][n_taps][TN rows][row bytes] pre-swizzled weights, n_tiles * TN biases
struct PackedImage : PackMeta {
  std::vector<unsigned char> w;
  std::vector<float> bias;
};

// The form of a launch (plan.cpp: launch_form): the NESTI_DEBUG_FORM_* values of include/nesti_hip.h and, EXPERIMENT
// (nesti_model_set_expert_mix / _gate_mix), a tap layer of a pair-mode tower in plain f16 / bf16 -- it reads the hi
// planes of its pair-layout input, multiplies ONE product and writes its outputs as pairs again
constexpr int kFormMix = NESTI_DEBUG_FORM_X6 + 1;
// ... and the packed weights it runs on: its own, except that X2 multiplies by the pair packing
inline int form_packing(int form) { return form == NESTI_DEBUG_FORM_X2 ? NESTI_DEBUG_FORM_PAIR : form; }

// The packing of a layer for the launches of one form (form_packing), in a model whose main dtype is mdt
int pack_form(const LayerDesc& d, const TensorTable& tt, int form, int mdt, PackedImage* img);

}  // namespace nesti
