// The planner: the form of every launch, the placement of every tower buffer, the forward workspace, every launch's parameters
// apart from its addresses, and the C-ABI entries that need nothing else (plan.h).  Host only.
#include "plan.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace nesti {

// ------------------------------------------------------------------------------------------
// the form of a launch
// ------------------------------------------------------------------------------------------
// EXPERIMENT: the bit of Pass::mix that switches a layer of a pair-mode model to kFormMix (-1: none) -- the tap layers on
// conv8n_kernel / conv4n_kernel; the gating net's share one bit, the experts' are "inception<B>Expert_<i>_conv<2|3>" of blocks
// 1, 2 (8^3) and 4 (4^3), two bits per block (conv2, the smaller kernel, first)
static int mix_bit(const LayerDesc& d, int tower, int mdt) {
  if (act_planes(mdt) == 1 || layer_kind(d, mdt) < 2) return -1;
  if (tower < 0) return kGateMixBit;
  const int blk = d.scope.size() > 9 ? d.scope[9] - '0' : 0;
  const int idx = blk == 1 ? 0 : blk == 2 ? 1 : blk == 4 ? 2 : -1;
  return idx < 0 ? -1 : 2 * idx + (d.scope.back() == '3' ? 1 : 0);
}

LaunchForm launch_form(const Graph& g, const Op& op, const Pass& ps, int mdt) {
  const LayerDesc& d = g.layers[op.layer];
  LaunchForm f;
  f.producer = !ps.fast && op.aux_out_buf >= 0 && (ps.x8_mask & op.x8_bits);
  const int mb = !ps.fast && ps.mix ? mix_bit(d, ps.tower, mdt) : -1;
  if (ps.fast) {
    // the filter pass's one-tap layers (1x1x1 conv1|conv4, FC) multiply the plain-f16 activations by the model's own PAIR-packed
    // weights (conv_igemm_kernel's X2 loop: hi * W_hi + hi * W_lo).  Those layers are fill-bound, so the second product costs ~20 %
    // more weight-tile fill and no matrix-pipe time that shows, and it removes the weight-rounding part of their error: the filter's
    // sigma on a logit difference drops from 0.021 to 0.012 (profiles/r05_gate_medium.txt), the threshold with it
    const bool x2 = layer_kind(d, mdt) == 0 && layer_taps(d) == 1;
    f.form = x2 ? NESTI_DEBUG_FORM_X2 : NESTI_DEBUG_FORM_PLAIN;
    f.family = x2 ? 0 : layer_kind(d, NESTI_F16);
  } else if (mb >= 0 && ((ps.mix >> mb) & 1)) {
    f.form = kFormMix;
    f.family = layer_kind(d, kernel_dtype(mdt));
  } else if (op.aux_in_buf >= 0 && op.x8_bit >= 0 && ((ps.x8_mask >> op.x8_bit) & 1)) {
    f.form = ps.x8_fmt == 8 ? NESTI_DEBUG_FORM_X8 : NESTI_DEBUG_FORM_X6;
    f.family = 2;
  } else {
    f.form = act_planes(mdt) > 1 ? NESTI_DEBUG_FORM_PAIR : NESTI_DEBUG_FORM_PLAIN;
    f.family = layer_kind(d, mdt);
  }
  return f;
}

// ------------------------------------------------------------------------------------------
// workspace planning
// ------------------------------------------------------------------------------------------
static size_t buf_bytes(const BufSpec& b, int NB, int dtype) {
  const size_t e = b.aux8 ? 2 : b.f32 ? 4 : dtype_size(dtype) * act_planes(dtype);
  return align_up(((size_t)NB << (3 * b.log2S)) * b.C * e, 256);
}

Placement place_tower(const Tower& T, int NB, int dtype) {
  const int n = (int)T.bufs.size(), n_ops = (int)T.ops.size();
  std::vector<int> first(n, 1 << 30), last(n, -1);
  for (int k = 0; k < n_ops; ++k) {
    const Op& op = T.ops[k];
    for (int b : {op.out_buf, op.mp_buf, op.aux_out_buf})
      if (b >= 1) { first[b] = std::min(first[b], k); last[b] = std::max(last[b], k); }
    for (int b : {op.in_buf, op.aux_in_buf})
      if (b >= 1) last[b] = std::max(last[b], k);
  }
  if (T.out_buf >= 1) last[T.out_buf] = n_ops;
  std::vector<int> order;
  for (int i = 1; i < n; ++i) if (last[i] >= 0) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return first[a] != first[b] ? first[a] < first[b] : a < b; });
  struct Block { size_t off, end; int until; };
  std::vector<Block> placed;   // in address order; the blocks still read (until >= first[i]) never overlap
  Placement P;
  P.off.assign(n, 0);
  P.first = first; P.last = last;
  if (T.side_tail) order.erase(std::remove_if(order.begin(), order.end(), [&](int i) { return T.bufs[i].aux8; }), order.end());
  for (int i : order) {
    // first fit: the lowest gap between the blocks still read that holds the buffer, else right above the highest of them
    const size_t need = buf_bytes(T.bufs[i], NB, dtype);
    size_t at = 0;
    for (const Block& b : placed) {
      if (b.until < first[i]) continue;
      if (b.off >= at + need) break;
      at = b.end;
    }
    P.off[i] = at;
    P.total = std::max(P.total, at + need);
    placed.insert(std::find_if(placed.begin(), placed.end(), [&](const Block& b) { return b.off > at; }), {at, at + need, last[i]});
  }
  if (T.side_tail) {
    // the stage-2 gating net: its side buffers (one per 8^3 block, lifetimes apart) share one block behind everything else, so
    // that the tower is its pair form's bytes plus exactly that block
    const size_t main = P.total;
    for (int i = 1; i < n; ++i)
      if (T.bufs[i].aux8 && last[i] >= 0) { P.off[i] = main; P.total = std::max(P.total, main + buf_bytes(T.bufs[i], NB, dtype)); }
  }
  return P;
}

static size_t max_tower_bytes(const Mode& m, int NB) {
  size_t t = m.cascade ? std::max(tower_bytes(m.g.gate, NB, pass_dtype(true, m.dtype)), tower_bytes(m.g.gate, cascade_cap(NB), m.dtype))
                       : tower_bytes(m.g.gate, NB, m.dtype);
  for (const Tower& e : m.g.experts) t = std::max(t, tower_bytes(e, expert_cap(NB), m.dtype));
  return t;
}

Stage2Plan stage2_plan(const Mode& m, int NB) {
  Stage2Plan S;
  if (!stage2_planned(m)) return S;
  const size_t arena = max_tower_bytes(m, NB);
  const int cap = cascade_cap(NB);
  // the largest round that fits: the recheck's own where the arena has room behind the f16x3 gate of a round (large batches: the
  // filter pass over the whole batch sets the arena), else 7/8 of it (a multiple of 4 rows, one tap-kernel tile), and so on; row
  // by row for small batches
  for (int c = cap; c >= 1; c = c > 64 ? ((c * 7 / 8) & ~3) : c - 1) {
    if ((NB + c - 1) / c > kMaxCascadeRounds) break;
    S.tower_bytes = tower_bytes(m.g.gate2, c, m.dtype);
    S.residual = S.tower_bytes;
    S.logits2 = S.residual + align_up((size_t)c * 4, 256);
    S.margin2 = S.logits2 + align_up((size_t)c * NESTI_MAX_EXPERTS * 4, 256);
    S.end = S.margin2 + align_up((size_t)NB * 4, 256);
    if (S.end <= arena) { S.cap = c; S.rounds = (NB + c - 1) / c; return S; }
  }
  return Stage2Plan();
}

WsLayout ws_layout(const Mode& m, int NB) {
  WsLayout L;
  size_t o = 0;
  L.x0 = o; o += align_up(NB * mups_row_bytes(m), 256);
  L.probs = o; o += align_up((size_t)NB * NESTI_MAX_EXPERTS * 4, 256);
  L.expert = o; o += align_up((size_t)NB * 4, 256);
  L.counts = o; o += 256;
  L.lists = o; o += align_up((size_t)NB * NESTI_MAX_EXPERTS * 4, 256);
  L.ecounts = o; o += kEcountsBytes;  // host.h: [E][rounds] rows of each expert round, the conditioning guard's list lengths and |n| band
  L.glist = o;
  if (m.g.x8) o += align_up((size_t)NESTI_MAX_EXPERTS * guard_cap(NB) * 4, 256);   // the conditioning guard's row lists, one per expert
  L.keep = L.flags = L.fcounts = o;
  if (m.cascade) {   // the f16 gate's logits, the flag list, [flag count | per-round counts]
    L.keep = o; o += align_up((size_t)NB * NESTI_MAX_EXPERTS * 4, 256);
    L.flags = o; o += align_up((size_t)NB * 4, 256);
    L.fcounts = o; o += kFcountsBytes;  // host.h: the two-stage gate's per-call counters
  }
  L.tower = o; o += max_tower_bytes(m, NB);
  L.total = o;
  return L;
}

// ------------------------------------------------------------------------------------------
// one launch of a pass, apart from its addresses
// ------------------------------------------------------------------------------------------
// Which k^3 layers use the Latin-square tile layout (host.h: ConvParams::remap): those where a 32-row tile can
// fall entirely on padding -- 5^3 taps at 8^3 (|d| = 2 clears a y/z pair) and every multi-tap layer at 4^3.  3^3 at
// 8^3 only ever clears single planes, which no 32-row tile shape can balance over four SIMDs.
static int conv_remap(int k, int log2S, int n_taps) {
  if (n_taps <= 1) return 0;
  if (log2S == 1) return 2;              // 2^3: single-voxel tiles of 32 points (conv.hip: remap == 2)
  if (log2S != 2 && log2S != 3) return 0;
  return (log2S == 2 || k >= 4) ? 1 : 0;
}

int conv_category(const LayerDesc& d, const PackMeta& pk) {
  if (pk.kind == 2) return d.k == 5 ? NESTI_PROF_CONV8_K5 : NESTI_PROF_CONV8_K3;
  return pk.n_taps > 1 ? NESTI_PROF_TAPS : NESTI_PROF_ONE_BY_ONE;
}

static bool form_x8(int form) { return form == NESTI_DEBUG_FORM_X8 || form == NESTI_DEBUG_FORM_X6; }

OpPlan plan_op(const Graph& g, const Tower& T, const Op& op, const Pass& ps, int mdt) {
  OpPlan pl;
  const int dt = pass_dtype(ps.fast, mdt);
  pl.elem = kernel_dtype(dt);
  pl.planes = act_planes(dt);
  pl.in_planes = op.in_buf < 1 ? act_planes(mdt) : pl.planes;
  pl.in_cstride = op.in_cstride ? op.in_cstride : T.bufs[op.in_buf].C;
  const bool conv = op.kind == Op::CONV;
  pl.form = conv ? launch_form(g, op, ps, mdt) : LaunchForm{pl.planes > 1 ? NESTI_DEBUG_FORM_PAIR : NESTI_DEBUG_FORM_PLAIN, -1, false};
  pl.x8_sc_layer = !conv ? -1 : form_x8(pl.form.form) ? op.aux_layer : pl.form.producer ? op.layer : -1;
  return pl;
}

ConvParams conv_params(const Graph& g, const Tower& T, const Op& op, const Pass& ps, const OpPlan& plan, const PackMeta& pk, int x8_sc,
                       int NB) {
  const LayerDesc& d = g.layers[op.layer];
  const int form = plan.form.form, planes = plan.planes, in_planes = plan.in_planes;
  const bool x2l = form == NESTI_DEBUG_FORM_X2;
  ConvParams p = {};
  p.in_pair = form == kFormMix ? 1 : 0;
  p.x2 = x2l ? 1 : 0;
  p.npoints = NB;
  // pair modes: strides and the input offset are physical (a 64-aligned logical offset x 3), output column
  // offsets stay logical (host.h: ConvParams::split); an fp32 output buffer is an ordinary one
  p.split = planes > 1 ? (ps.zero_lo ? 2 : 1) : 0;
  p.in_cstride = plan.in_cstride * in_planes; p.in_coff = op.in_coff * in_planes;
  // distance between consecutive K chunks of a PLAIN kernel's input row: 128 B, except in the NESTI_F16X3C filter pass,
  // whose plain-f16 first layer reads the hi plane of each 64-channel group [hi | lo] of the pair-layout MuPS tensor
  p.in_chunk_bytes = kRowBytes * (planes == 1 ? in_planes : 1);
  p.out_cstride = T.bufs[op.out_buf].C * (op.out_f32 ? 1 : planes); p.out_coff = op.out_coff;
  p.n_chunks = pk.n_chunks; p.n_taps = pk.n_taps; p.tap_k = d.k; p.log2S = d.log2S; p.s_real = d.s_real;
  p.relu = d.relu ? 1 : 0; p.out_f32 = op.out_f32 ? 1 : 0; p.acc_scale = pk.acc_scale; p.x3native = (pk.x3n && !x2l) ? 1 : 0;
  const long long rows = (long long)NB << (3 * d.log2S);
  p.m_tiles = pk.kind == 3 ? (NB + 15) / 16 : pk.kind == 2 ? (NB + 3) / 4 : (int)((rows + kTileM - 1) / kTileM);
  p.n_tiles = pk.n_tiles; p.split_tile = pk.split_tile; p.out_coff2 = op.out_coff2; p.pool_k = d.pool_k;
  if (op.mp_buf >= 0) { p.mp_cstride = T.bufs[op.mp_buf].C * planes; p.mp_mode = op.mp_mode; p.mp_mode2 = op.mp_mode2; }
  if (form_x8(form)) {                         // consumer: the FP8 cross-term loop on the planes the block's conv1 wrote
    p.x8 = 1; p.aux8_stride = T.bufs[op.aux_in_buf].C * 2;
    p.x8_scale_a = 127 - (x8_sc + 11); p.x8_scale_b = 127 - pk.x8_sb;
  }
  if (plan.form.producer) {
    p.aux8_stride = T.bufs[op.aux_out_buf].C * 2;
    p.x8_sc = x8_sc; p.x8_sa = p.x8_sc + 11;
  }
  if (p.x8 || plan.form.producer) p.x8_fmt = ps.x8_fmt == 6 ? 6 : 8;
  memcpy(p.tap, pk.tap, sizeof(p.tap));
  p.remap = conv_remap(d.k, d.log2S, pk.n_taps);
  return p;
}

PoolParams pool_params(const Tower& T, const Op& op, const OpPlan& plan, int NB) {
  PoolParams p = {};
  p.npoints = NB;
  p.split = plan.planes > 1 ? 1 : 0;
  p.in_cstride = plan.in_cstride * plan.planes; p.in_coff = op.in_coff;
  p.out_cstride = T.bufs[op.out_buf].C * plan.planes; p.out_coff = op.out_coff;
  p.C = op.C; p.log2S = op.log2S;
  return p;
}

void tower_macs(const Graph& g, int tower, int kind, const std::function<const PackMeta&(int)>& main_packing, double* nominal,
                double* useful, double* issued) {
  double nom = 0, use = 0, iss = 0;
  for (const Op& op : g.tower(tower).ops) {
    if (op.kind != Op::CONV) continue;
    const LayerDesc& d = g.layers[op.layer];
    const PackMeta& pl = main_packing(op.layer);
    if (kind >= 0 && conv_category(d, pl) != kind) continue;
    const int S = d.s_real ? d.s_real : (1 << d.log2S), V = S * S * S;
    long long valid = 0;   // sum over output voxels of the taps that land inside the volume: a kept tap does at S - |offset| per axis
    for (int t = 0; t < pl.n_taps; ++t) valid += (long long)(S - abs(pl.tap[t][0])) * (S - abs(pl.tap[t][1])) * (S - abs(pl.tap[t][2]));
    const int parts = d.scope2.empty() ? 1 : 2;
    nom += (double)parts * V * d.k * d.k * d.k * d.cin * d.cout;
    use += (double)parts * valid * d.cin * d.cout;
    // MFMA tiles the kernels issue: conv8n_kernel (8^3) and the remapped conv_igemm_kernel layout at 4^3 hold one x-line
    // (y, z) per 32-row tile and skip it when y + dy or z + dz leaves the volume; elsewhere every kept tap is issued in full
    // (conv4n_kernel's tile is a single voxel: it issues exactly the taps that land inside the volume)
    double tap_sum = pl.n_taps;
    const int Si = 1 << d.log2S;
    const bool voxel_tiles = pl.kind == 3 || (pl.kind == 0 && !d.s_real && conv_remap(d.k, d.log2S, pl.n_taps) == 2);
    if (pl.n_taps > 1 && (pl.kind >= 1 || voxel_tiles || (d.log2S == 2 && conv_remap(d.k, d.log2S, pl.n_taps)))) {
      tap_sum = 0;
      for (int t = 0; t < pl.n_taps; ++t)
        tap_sum += (double)std::max(0, S - abs(pl.tap[t][0])) * std::max(0, S - abs(pl.tap[t][1])) / ((double)Si * Si) *
                   (voxel_tiles ? (double)std::max(0, S - abs(pl.tap[t][2])) / Si : 1.0);
    }
    iss += (double)(1 << (3 * d.log2S)) * tap_sum * d.Cin_p * d.Cout_p;
  }
  if (nominal) *nominal = nom;
  if (useful) *useful = use;
  if (issued) *issued = iss;
}

int check_pass(const std::string& who, const Graph& g, bool cascade, int tower, const nesti_debug_pass_t& ps) {
  if (tower < -1 || tower >= (int)g.experts.size()) NESTI_FAIL(who + ": tower must be -1 (gate) or an expert index");
  if (tower < 0 && g.cfg.arch != NESTI_ARCH_EXPERTS && g.cfg.arch != NESTI_ARCH_SWITCH) NESTI_FAIL(who + ": this model has no gating net");
  if (ps.fast && !(cascade && tower < 0)) NESTI_FAIL(who + ": the filter pass is the gating net's of NESTI_F16X3C / NESTI_F16X8C models");
  if (tower < 0 && ps.x8_mask) {   // recheck stage 2: the gating net's six 8^3 tap layers in the FP6 form
    if (ps.x8_mask < 0 || ps.x8_mask > 0x3F || ps.fast || !(cascade && g.has_gate2()) || ps.x8_fmt == 8)
      NESTI_FAIL(who + ": the gating net takes an x8_mask of six bits, format 6, in NESTI_F16X8C models, outside the filter pass");
  } else if (ps.x8_mask < 0 || ps.x8_mask > 0xF || (ps.x8_mask && !(g.x8 && tower >= 0))) {
    NESTI_FAIL(who + ": x8_mask has four bits and applies to the expert towers of NESTI_F16X8 / NESTI_F16X8C models");
  }
  if (ps.x8_fmt != 0 && ps.x8_fmt != 6 && ps.x8_fmt != 8) NESTI_FAIL(who + ": x8_fmt is 0 (= 6), 6 or 8");
  return 0;
}

}  // namespace nesti

// ==========================================================================================
// C ABI: the entries that need no device
// ==========================================================================================
using namespace nesti;

extern "C" {

void nesti_default_config(nesti_config_t* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->arch = NESTI_ARCH_EXPERTS;
  cfg->n_scales = 3;                 // --patch_radius 0.01 0.03 0.05 (the published setting; the script default is 0.005 0.01 0.03)
  cfg->points_per_scale = 512;       // --num_point
  cfg->grid_n = 8;                   // --n_gaussians 8
  cfg->variance = 0.0156;            // --gmm_variance
  cfg->n_experts = 7;
  const int lo[7] = {0, 0, 1, 1, 2, 2, 0}, cnt[7] = {1, 1, 1, 1, 1, 1, 3};   // expert_dict  :62
  for (int i = 0; i < 7; ++i) { cfg->expert_scale_lo[i] = lo[i]; cfg->expert_scale_cnt[i] = cnt[i]; }
}

int nesti_gmm_grid(int n, double variance, float* w, float* mu, float* sigma) {
  if (n < 1 || !w || !mu || !sigma) NESTI_FAIL("nesti_gmm_grid: bad arguments");
  // np.mgrid[step-1 : 1-step : n j] per axis, reshape [3,-1].T  => x slowest (utils/utils.py:81-87)
  const double step = 1.0 / n;
  const double a0 = step - 1.0, a1 = 1.0 - step;
  const int G = n * n * n;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < n; ++k) {
        const int g = (i * n + j) * n + k;
        const int idx[3] = {i, j, k};
        for (int c = 0; c < 3; ++c) {
          const double v = (n == 1) ? a0 : a0 + (a1 - a0) * idx[c] / (double)(n - 1);
          mu[g * 3 + c] = (float)v;
          sigma[g * 3 + c] = (float)sqrt(variance);   // np.sqrt(gmm.covariances_)  test_n_est_w_experts.py:146
        }
        w[g] = (float)(1.0 / G);                       // utils/utils.py:89
      }
  return 0;
}

int nesti_model_describe(const nesti_config_t* cfg, int* n_tensors, nesti_tensor_t* infos, int max_infos) {
  if (!cfg || !n_tensors) NESTI_FAIL("nesti_model_describe: null argument");
  Graph g;
  if (build_graph(cfg, &g)) return 1;
  static thread_local std::vector<std::string> names;
  std::vector<std::pair<std::string, std::vector<int64_t>>> all;
  for (const LayerDesc& d : g.layers) layer_tensors(d, &all);
  *n_tensors = (int)all.size();
  if (!infos) return 0;
  if (max_infos < (int)all.size()) NESTI_FAIL("nesti_model_describe: infos array too small");
  names.clear();
  names.reserve(all.size());
  for (size_t i = 0; i < all.size(); ++i) {
    names.push_back(all[i].first);
    infos[i].name = names.back().c_str();
    infos[i].data = nullptr;
    infos[i].ndim = (int)all[i].second.size();
    for (int d = 0; d < 5; ++d) infos[i].dims[d] = d < infos[i].ndim ? all[i].second[d] : 0;
  }
  return 0;
}

size_t nesti_tower_workspace_bytes(const nesti_config_t* cfg, int dtype, int tower, int batch) {
  if (!cfg || batch <= 0) return 0;
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 0;
  if (tower < -1 || tower >= (int)g.experts.size()) return 0;
  // the gating net of the two-stage models is quoted for its filter pass
  return tower_bytes(g.tower(tower), batch, pass_dtype(tower < 0 && dtype_cascade(dtype), main_dtype(dtype)));
}

size_t nesti_estimate_workspace_bytes_for_config(const nesti_config_t* cfg, int dtype, int batch) {
  if (!cfg || batch <= 0) return 0;
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 0;
  return est_workspace_bytes({g, main_dtype(dtype), dtype_cascade(dtype)}, batch);
}

int nesti_debug_gate_stage2_plan(const nesti_config_t* cfg, int dtype, int batch, nesti_debug_stage2_t* out) {
  if (!cfg || !out) NESTI_FAIL("nesti_debug_gate_stage2_plan: null argument");
  if (batch <= 0) NESTI_FAIL("nesti_debug_gate_stage2_plan: batch must be positive");
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 1;
  const Mode m = {g, main_dtype(dtype), dtype_cascade(dtype)};
  const Stage2Plan S = stage2_plan(m, batch);
  const WsLayout L = ws_layout(m, batch);
  memset(out, 0, sizeof(*out));
  out->cap = S.cap; out->rounds = S.rounds;
  out->tower_bytes = (int64_t)S.tower_bytes; out->residual = (int64_t)S.residual; out->logits2 = (int64_t)S.logits2;
  out->margin2 = (int64_t)S.margin2; out->end = (int64_t)S.end;
  out->arena_offset = (int64_t)L.tower; out->arena_bytes = (int64_t)(L.total - L.tower);
  return 0;
}

// ---- test hook: one tower, launch by launch (include/nesti_hip.h) -----------------------------------------------------------
int nesti_debug_tower_ops(const nesti_config_t* cfg, int dtype, int tower, int batch, const nesti_debug_pass_t* pass,
                          nesti_debug_buf_t* bufs, int max_bufs, int* n_bufs, nesti_debug_op_t* ops, int max_ops, int* n_ops,
                          int32_t* in_pos, int max_in_pos, int* n_in_pos, size_t* ws_bytes) {
  if (!cfg || !n_bufs || !n_ops) NESTI_FAIL("nesti_debug_tower_ops: null argument");
  if (batch <= 0) NESTI_FAIL("nesti_debug_tower_ops: batch must be positive");
  const nesti_debug_pass_t& ps = pass ? *pass : kMainPass;
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 1;
  if (check_pass("nesti_debug_tower_ops", g, dtype_cascade(dtype), tower, ps)) return 1;
  const Tower& T = g.tower(tower, ps.x8_mask);
  Pass run;
  run.tower = tower; run.fast = ps.fast != 0; run.x8_mask = ps.x8_mask; run.x8_fmt = ps.x8_fmt == 8 ? 8 : 6;
  const int mdt = main_dtype(dtype), dt = pass_dtype(run.fast, mdt);
  const Placement P = place_tower(T, batch, dt);
  int npos = 0;
  for (const Op& op : T.ops) if (op.kind == Op::CONV) npos += g.layers[op.layer].cin;
  *n_bufs = (int)T.bufs.size();
  *n_ops = (int)T.ops.size();
  if (n_in_pos) *n_in_pos = npos;
  if (ws_bytes) *ws_bytes = P.total;
  if ((bufs && max_bufs < *n_bufs) || (ops && max_ops < *n_ops) || (in_pos && max_in_pos < npos))
    NESTI_FAIL("nesti_debug_tower_ops: output arrays too small");
  for (int i = 0; bufs && i < *n_bufs; ++i) {
    const BufSpec& b = T.bufs[i];
    nesti_debug_buf_t& o = bufs[i];
    memset(&o, 0, sizeof(o));
    o.offset = i == 0 ? -1 : (int64_t)P.off[i];
    o.bytes = i == 0 || P.last[i] < 0 ? 0 : (int64_t)buf_bytes(b, batch, dt);
    o.log2S = b.log2S; o.C = b.C; o.f32 = b.f32; o.aux8 = b.aux8;
    o.planes = b.aux8 || b.f32 ? 1 : act_planes(i == 0 ? mdt : dt);   // buffer 0, the MuPS tensor, keeps the model's layout
    o.elem = b.aux8 ? -1 : b.f32 ? NESTI_F32 : kernel_dtype(i == 0 ? mdt : dt);
    o.first = i == 0 ? -1 : P.first[i] == (1 << 30) ? -1 : P.first[i];
    o.last = P.last[i];
  }
  static thread_local std::vector<std::string> names;
  names.clear();
  names.reserve(2 * T.ops.size());
  int pos = 0;
  for (int k = 0; ops && k < *n_ops; ++k) {
    const Op& op = T.ops[k];
    const OpPlan pl = plan_op(g, T, op, run, mdt);
    nesti_debug_op_t& o = ops[k];
    memset(&o, 0, sizeof(o));
    o.kind = op.kind == Op::CONV ? NESTI_DEBUG_OP_CONV : op.kind == Op::MAX ? NESTI_DEBUG_OP_MAX : NESTI_DEBUG_OP_MAX3;
    o.family = pl.form.family; o.form = pl.form.form; o.layer = -1; o.in_pos_off = -1;
    o.elem = pl.elem; o.planes = pl.planes;
    o.in_buf = op.in_buf; o.in_coff = op.in_coff; o.in_cstride = pl.in_cstride; o.in_planes = pl.in_planes;
    o.out_buf = op.out_buf; o.out_coff = op.out_coff; o.out_coff2 = op.out_coff2; o.out_f32 = op.out_f32;
    o.mp_buf = op.mp_buf; o.mp_mode = op.mp_mode; o.mp_mode2 = op.mp_mode2;
    o.aux_in_buf = form_x8(pl.form.form) ? op.aux_in_buf : -1; o.aux_layer = form_x8(pl.form.form) ? op.aux_layer : -1;
    o.aux_out_buf = pl.form.producer ? op.aux_out_buf : -1;
    o.log2S = op.log2S; o.C = op.C;
    if (op.kind != Op::CONV) continue;
    const LayerDesc& d = g.layers[op.layer];
    names.push_back(d.scope);
    o.scope = names.back().c_str();
    names.push_back(d.scope2);
    o.scope2 = names.back().c_str();
    o.layer = op.layer; o.k = d.k; o.log2S = d.log2S; o.s_real = d.s_real; o.is_fc = d.is_fc; o.bn = d.bn; o.relu = d.relu;
    o.pool_k = d.pool_k; o.n_taps = layer_taps(d);
    o.cin = d.cin; o.cout = d.cout; o.Cin_p = d.Cin_p; o.Cout_p = d.Cout_p;
    o.in_pos_off = pos;
    for (int c = 0; c < d.cin; ++c, ++pos) if (in_pos) in_pos[pos] = d.in_pos[c];
  }
  return 0;
}

}  // extern "C"
