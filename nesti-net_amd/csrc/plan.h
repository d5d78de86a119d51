// The planner (plan.cpp): what, from the configuration alone, decides how a model runs -- the form of every launch, where every
// tower buffer lives, the per-mode caps, the forward workspace and every launch's parameters apart from its addresses.  Host only:
// model.hip adds the device pointers and launches; nesti_debug_tower_ops reports the same derivation without a device.
#pragma once
#include <functional>

#include "pack.h"

namespace nesti {

// What the sizing functions read of a model: its graph and the two mode facts
struct Mode { const Graph& g; int dtype; bool cascade; };   // dtype: the main dtype (host.h: main_dtype); cascade: the two-stage gate

// ------------------------------------------------------------------------------------------
// the form of a launch
// ------------------------------------------------------------------------------------------
// One pass of a tower: what, beside the graph and the model's dtype, decides how its launches compute
struct Pass {
  int tower = -1;          // -1: the gating net, else an expert
  bool fast = false;       // NESTI_F16X3C filter pass: the tower runs in plain f16 while the MuPS tensor it reads keeps the model's pair
                           // layout (only the hi plane is read)
  int x8_mask = 0;         // expert towers of NESTI_F16X8 / NESTI_F16X8C models: the tap layers at 8^3 whose bit (Op::x8_bit) is set run
  int x8_fmt = 6;          // their cross terms in FP8 (8) or FP6 (6), on the planes their block's conv1 then also writes
  int mix = 0;             // EXPERIMENT: the tap layers whose mix_bit is set here run single-product (kFormMix)
  bool zero_lo = false;    // EXPERIMENT (gate_mix == 2): every layer writes its outputs rounded to 16 bits (lo plane = 0)
};
// the dtype a pass of a model whose main dtype is mdt computes in (fast: Pass::fast)
inline int pass_dtype(bool fast, int mdt) { return fast ? NESTI_F16 : mdt; }

constexpr int kGateMixBit = 8;   // EXPERIMENT: the bit of Pass::mix the gating net's tap layers share (plan.cpp: mix_bit)

struct LaunchForm {
  int form;        // NESTI_DEBUG_FORM_* or kFormMix
  int family;      // PackMeta::kind of the packing the launch runs on (pools: -1)
  bool producer;   // an 8^3 block's conv1 that also writes the FP8 / FP6 planes of its outputs for the block's tap layers
};
// How the conv launch `op` of a pass computes, for a model whose main dtype is mdt.  THE place that decides it: nesti_model_create
// packs what it names, plan_op hands it to run_op and to nesti_debug_tower_ops.  A function of the configuration alone.
LaunchForm launch_form(const Graph& g, const Op& op, const Pass& ps, int mdt);

// ------------------------------------------------------------------------------------------
// workspace planning
// ------------------------------------------------------------------------------------------
// Workspace placement of a tower's buffers: a buffer lives from the first launch that writes it to the last launch that
// reads it (the tower's output until the end); buffers whose lifetimes do not overlap share memory (first fit), which
// brings the gating tower from 2.5 to 1.6 MB per query in 16-bit and lets one library batch cover a 100k-point cloud.
struct Placement {
  std::vector<size_t> off;   // per buffer (index 0 = the external MuPS tensor: unused)
  std::vector<int> first, last;   // per buffer: the first op that writes it, the last op that reads it (n_ops: the tower's output)
  size_t total = 0;
};
Placement place_tower(const Tower& T, int NB, int dtype);
inline size_t tower_bytes(const Tower& T, int NB, int dtype) { return place_tower(T, NB, dtype).total; }
// recheck stage 2 -- the gating net's 8^3 tap layers in the FP6 cross-term form (model.hip: gate_cascade) -- is planned for: the
// two-stage gate of an NESTI_F16X8C model.  Whether a call runs it is the model's (x8 format 6, nesti_model_set_gate_stage2)
inline bool stage2_planned(const Mode& m) { return m.cascade && m.g.has_gate2(); }

// NESTI_F16X3C: the f16x3 gate re-decides the flagged rows `cap` at a time (its workspace is 3x the filter's per row, and
// only a fraction of a batch is flagged): small batches in one round, large ones in quarters
inline int cascade_cap(int NB) { return NB <= 4096 ? NB : (int)align_up((size_t)(NB + 3) / 4, 256); }
// A routed expert sees about 1 / E of a batch, so its tower is sized for a quarter of a large batch and run in up to four
// rounds over its routing list (rounds beyond the list's length launch empty grids: ~0.2 % of a 100k batch); the workspace of a
// batch is then set by the gating net alone and a whole 100k-point cloud is one library batch in every mode but f16x3 / f32.
constexpr int kExpertRounds = 4;
constexpr int expert_cap(int NB) { return NB <= 8192 ? NB : (int)align_up((size_t)(NB + kExpertRounds - 1) / kExpertRounds, 256); }
// the [E][rounds] round counts at the start of the ecounts block (host.h) end before the conditioning guard's words
static_assert(kExpertRounds * expert_cap(8193) >= 8193 && NESTI_MAX_EXPERTS * kExpertRounds <= kGuardCountOff, "ecounts layout");
// rows of ONE expert the conditioning guard can re-evaluate per pass (a fraction of a per cent of a batch are flagged at all)
inline int guard_cap(int NB) { return expert_cap(NB) < 2048 ? expert_cap(NB) : 2048; }

// channel stride of the MuPS rows the towers read, in elements (pair modes: two planes per 64-channel group)
inline int mups_stride(const Mode& m) { return m.g.mups_cstride * act_planes(m.dtype); }
// bytes of one query's MuPS rows
inline size_t mups_row_bytes(const Mode& m) { return ((size_t)1 << (3 * m.g.gate_x0_log2S())) * mups_stride(m) * dtype_size(m.dtype); }
// columns of a probs output row
inline int probs_cols(const Graph& g) { return g.cfg.arch == NESTI_ARCH_SWITCH ? 1 : g.cfg.n_experts; }

// The forward workspace for a batch capacity NB: byte offsets of its parts; `tower` = the arena every tower pass is placed in
struct WsLayout {
  size_t x0, probs, expert, counts, lists, ecounts, glist, keep, flags, fcounts, tower, total;
};
WsLayout ws_layout(const Mode& m, int NB);

// Recheck stage 2 lives INSIDE the tower arena, whose size it does not change: [the stage-2 gating net of a round of `cap` rows
// (Graph::gate2; the f16x3 gate over the round's residual list reuses its front) | residual list [cap] | stage-2 logits of the
// residual rows [cap, NESTI_MAX_EXPERTS] | stage-2 margin of every flag-list position [NB]], offsets from the arena's start.  cap is
// the recheck's own round where that fits -- batches above 4096, whose arena is set by the filter pass over the whole batch -- and
// the largest smaller round that does otherwise; cap == 0: no round fits (a batch of one row), the call runs without the stage
struct Stage2Plan { int cap = 0, rounds = 0; size_t tower_bytes = 0, residual = 0, logits2 = 0, margin2 = 0, end = 0; };
Stage2Plan stage2_plan(const Mode& m, int NB);

// The fused end-to-end entries put their staging in front of the forward workspace: [points (3^3 grid only) | n_eff | forward]
// 8^3 Gaussian grid: patches_mups_kernel goes from the cloud to the MuPS tensor in one kernel (the patch tensors are never
// written); 3^3 grid: patches_kernel + mups3_kernel through a staging buffer in the workspace.
inline size_t est_points_bytes(const Graph& g, int batch) {
  return g.cfg.grid_n == 8 ? 0 : align_up((size_t)batch * g.cfg.n_scales * g.cfg.points_per_scale * 3 * sizeof(float), 256);
}
inline size_t est_neff_bytes(const Graph& g, int batch) { return align_up((size_t)batch * g.cfg.n_scales * sizeof(int32_t), 256); }
inline size_t est_workspace_bytes(const Mode& m, int batch) {
  return est_points_bytes(m.g, batch) + est_neff_bytes(m.g, batch) + ws_layout(m, batch).total;
}

// ------------------------------------------------------------------------------------------
// one launch of a pass, apart from its addresses
// ------------------------------------------------------------------------------------------
// What run_op launches and nesti_debug_tower_ops reports: derived once, here
struct OpPlan {
  int elem;           // the element type its kernels are instantiated for (a mixed layer is a plain f16 / bf16 kernel inside a
                      // pair-mode tower: the same element type either way)
  int planes;         // planes of the activations the tower writes
  int in_planes;      // ... of the rows this launch reads: the MuPS tensor keeps the model's layout in every pass
  int in_cstride;     // logical channels of an input row (a flattened view for fc1)
  LaunchForm form;    // pools: PLAIN or PAIR, the layout of their values
  int x8_sc_layer;    // conv: the layer whose main packing carries the pre-scale of the FP8 planes this launch reads (a consumer:
                      // its block's conv1) or writes (a producer: itself); -1: neither
};
OpPlan plan_op(const Graph& g, const Tower& T, const Op& op, const Pass& ps, int mdt);

// The parameter block of the conv launch `op` for capacity NB on the packing pk (the one plan.form names); x8_sc =
// PackMeta::x8_sc of plan.x8_sc_layer's main packing.  Every pointer is null and `walk` is 0: the caller's.
ConvParams conv_params(const Graph& g, const Tower& T, const Op& op, const Pass& ps, const OpPlan& plan, const PackMeta& pk, int x8_sc,
                       int NB);
PoolParams pool_params(const Tower& T, const Op& op, const OpPlan& plan, int NB);

// which NESTI_PROF_* conv category a layer's launch is booked under
int conv_category(const LayerDesc& d, const PackMeta& pk);

// nesti_model_macs: multiply-accumulates per query of the conv launches of a tower that fall under `kind` (-1: all);
// main_packing(layer) = the layer's packing in the model's own dtype
void tower_macs(const Graph& g, int tower, int kind, const std::function<const PackMeta&(int)>& main_packing, double* nominal,
                double* useful, double* issued);

constexpr nesti_debug_pass_t kMainPass = {0, 0, 0};   // the two test hooks' pass argument when it is NULL
// the pass arguments of the two test hooks against the graph (cascade: a model with the two-stage gate); `who` prefixes the message
int check_pass(const std::string& who, const Graph& g, bool cascade, int tower, const nesti_debug_pass_t& ps);

}  // namespace nesti
