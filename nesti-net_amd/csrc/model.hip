// Host side of libnesti_hip.so that touches the device: C-ABI entry points, the kernel profiler, the form of every launch, the
// workspace planner, the tower runner and the forward paths.  The graph (graph.cpp) and batch-norm folding and weight repacking
// for the MFMA kernels (pack.cpp) are host-only units of their own.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "pack.h"

#ifndef NESTI_GUARD_WALK_GRID     // measurement builds may override it (scripts/ab_guard.sh); 1 = the default walking grid (kWalkGrid)
#define NESTI_GUARD_WALK_GRID 64
#endif
#ifndef NESTI_GUARD_LANES         // auxiliary streams of the conditioning guard, one per caller stream (measurement builds: 1)
#define NESTI_GUARD_LANES 2
#endif
#ifndef NESTI_GATE_WIDEN_WALK_GRID    // the two-stage gate's widening passes hold at most a few hundred rows (normally none)
#define NESTI_GATE_WIDEN_WALK_GRID 1
#endif
#ifndef NESTI_GUARD_WIDEN_WALK_GRID   // the guard's widening pass is normally EMPTY: its launches only have to be dispatched and retire
#define NESTI_GUARD_WIDEN_WALK_GRID 8
#endif

namespace nesti {

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_error;
// nesti_experiment_mix_enable: models created while this is set also pack their tap layers for the single-product experiments
// (nesti_model_set_expert_mix / _gate_mix); off by default, so product models neither pay the packing time nor hold the copies
static bool g_experiment_mix = false;
void set_error(const std::string& msg) { g_error = msg; }

// ------------------------------------------------------------------------------------------
// optional per-category kernel timing with hipEvents on the launch stream (bench.py roofline leg)
// ------------------------------------------------------------------------------------------
constexpr int kProfSlots = NESTI_PROF_PHASES * NESTI_PROF_CATEGORIES;   // slot = phase * NESTI_PROF_CATEGORIES + category
struct ProfState {
  bool on = false;
  int phase = NESTI_PHASE_INPUT;     // set by the forward path (prof_phase); launches are booked under it
  std::vector<hipEvent_t> pool;      // recycled events
  std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[kProfSlots];
  double ms[kProfSlots] = {0};
  long long launches[kProfSlots] = {0};
};
static ProfState g_prof;
static std::mutex g_prof_mu;   // forward calls may come from several host threads (one stream each)

static hipEvent_t prof_event() {
  if (!g_prof.pool.empty()) { hipEvent_t e = g_prof.pool.back(); g_prof.pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
// A stream that is being captured into a hipGraph records nothing: events captured into a graph cannot be
// synchronised on or timed afterwards.
static bool prof_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs != hipStreamCaptureStatusNone;
}
void prof_phase(int phase) { if (g_prof.on) g_prof.phase = phase; }
// prof_begin returns a token for prof_end (-1: nothing recorded): slot * 2^20 + index of the span within the slot
int prof_begin(int cat, hipStream_t st) {
  if (!g_prof.on || prof_capturing(st)) return -1;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  // the input kernels are launched between forward passes, whatever phase the last one ended in
  const int phase = (cat == NESTI_PROF_MUPS || cat == NESTI_PROF_PATCHES) ? NESTI_PHASE_INPUT : g_prof.phase;
  const int slot = phase * NESTI_PROF_CATEGORIES + cat;
  if (g_prof.spans[slot].size() >= (1u << 20)) return -1;
  hipEvent_t a = prof_event(), b = prof_event();
  (void)hipEventRecord(a, st);
  g_prof.spans[slot].push_back({a, b});
  return (slot << 20) | ((int)g_prof.spans[slot].size() - 1);
}
void prof_end(int, int token, hipStream_t st) {
  if (token < 0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const int slot = token >> 20, idx = token & ((1 << 20) - 1);
  if (slot < kProfSlots && idx < (int)g_prof.spans[slot].size()) (void)hipEventRecord(g_prof.spans[slot][idx].second, st);
}
static void prof_collect() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int c = 0; c < kProfSlots; ++c) {
    for (auto& sp : g_prof.spans[c]) {
      (void)hipEventSynchronize(sp.second);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, sp.first, sp.second) == hipSuccess) g_prof.ms[c] += ms;
      g_prof.launches[c] += 1;
      g_prof.pool.push_back(sp.first);
      g_prof.pool.push_back(sp.second);
    }
    g_prof.spans[c].clear();
  }
}

namespace {

// ------------------------------------------------------------------------------------------
// device-resident packed layers
// ------------------------------------------------------------------------------------------
// A packed layer in device memory (upload): the packer's metadata and where its bytes went
struct PackedLayer : PackMeta {
  void* wpk = nullptr;
  float* bias = nullptr;
};

// The one place packed bytes go to the device: the image pack_form made of a layer, for every form
int upload(const PackedImage& img, PackedLayer* pl) {
  static_cast<PackMeta&>(*pl) = img;
  NESTI_CHECK_HIP(hipMalloc(&pl->wpk, img.w.size()));
  NESTI_CHECK_HIP(hipMemcpy(pl->wpk, img.w.data(), img.w.size(), hipMemcpyHostToDevice));
  NESTI_CHECK_HIP(hipMalloc((void**)&pl->bias, img.bias.size() * sizeof(float)));
  NESTI_CHECK_HIP(hipMemcpy(pl->bias, img.bias.data(), img.bias.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace
}  // namespace nesti

struct nesti_model {
  nesti::Graph graph;
  int dtype = NESTI_BF16;                      // compute dtype of everything that reaches the outputs (NESTI_F16X3C -> NESTI_F16X3)
  // every (packing, layer) launch_form names over the passes a model of this dtype runs (nesti_model_create), device-resident
  std::map<std::pair<int, int>, nesti::PackedLayer> packed;
  const nesti::PackedLayer* packing(int form, int layer) const {
    auto it = packed.find({nesti::form_packing(form), layer});
    return it == packed.end() ? nullptr : &it->second;
  }
  // the layers in the model's own dtype: every layer has this one
  const nesti::PackedLayer& main_packing(int layer) const {
    return *packing(nesti::act_planes(dtype) > 1 ? NESTI_DEBUG_FORM_PAIR : NESTI_DEBUG_FORM_PLAIN, layer);
  }
  // NESTI_F16X3C: the two-stage gate (its filter pass runs the gating net's tap layers on plain-f16 packings), the gate margin and
  // the device counters (include/nesti_hip.h: nesti_cascade_stats_t)
  bool cascade = false;
  // EXPERIMENT: models created after nesti_experiment_mix_enable(1) also hold kFormMix packings of their tap layers; expert_mix /
  // gate_mix switch them on
  bool has_mix = false;
  int expert_mix = 0;
  // NESTI_F16X8 / NESTI_F16X8C: x8_mask picks which of the experts' tap layers at 8^3 run their cross terms in FP8 / FP6
  // (include/nesti_hip.h: nesti_model_set_x8_layers), x8_fmt which of the two forms forward calls use (8 or 6; nesti_model_set_x8_format)
  int x8_mask = 0;
  int x8_fmt = 6;
  // ... and their conditioning guard (pool.hip: x8_guard_*): outputs with |n| below max(x8_guard_thr, NESTI_X8_GUARD_WIDEN x largest
  // measured |dn| / theta) are re-evaluated in f16x3 proper; gstat = the device counters (include/nesti_hip.h: nesti_x8_guard_stats_t)
  float x8_guard_thr = NESTI_X8_GUARD_DEFAULT;
  int x8_guard_walk = NESTI_GUARD_WALK_GRID;   // workgroups of the guard towers' walking launches (kernels.h: ConvParams::walk)
  unsigned long long* gstat = nullptr;
  // a guard tower sees a handful of rows, so it is latency-bound (one workgroup walks a layer's whole K loop: ~3 ms per tower): expert
  // e's guard runs on ONE auxiliary stream while the caller's stream goes on with expert e + 1 (events in both directions).  One
  // stream, not E: with more streams than hardware queues (4 by default) the event waits of one stream block the kernels of another
  // that shares its queue -- measured: E side streams cost the two-stream mode 3 %
  // kGuardLanes such sets, keyed by the caller's stream (two library batches in flight on two streams -- the way the command line runs --
  // get an auxiliary stream each: 2 + 2 = the 4 hardware queues; a third caller stream shares lane 0)
  static constexpr int kGuardLanes = NESTI_GUARD_LANES;
  struct GuardLane {
    hipStream_t gstream = nullptr;
    hipEvent_t gev_done[NESTI_MAX_EXPERTS] = {}, gev_join = nullptr;
    hipStream_t owner = nullptr;
    bool owned = false;
    std::mutex gmu;
  };
  mutable GuardLane glane[kGuardLanes];
  mutable std::mutex glane_mu;
  GuardLane* guard_lane(hipStream_t caller) const {
    std::lock_guard<std::mutex> lk(glane_mu);
    for (int i = 0; i < kGuardLanes; ++i) if (glane[i].owned && glane[i].owner == caller) return &glane[i];
    for (int i = 0; i < kGuardLanes; ++i) if (!glane[i].owned) { glane[i].owned = true; glane[i].owner = caller; return &glane[i]; }
    return &glane[0];
  }
  int gate_mix = 0;          // EXPERIMENT (nesti_model_set_gate_mix): the f16x3 gating passes run their tap layers single-product
  float tau = 0.25f;
  unsigned long long* cstat = nullptr;
  // nesti_model_set_reproducible: rstat = the mode's own 64-byte counter block ([0] gate_violations, [1] guard_violations), allocated
  // with cstat / gstat; forward calls hand it to the kernels only while the mode is on (frozen() below), and then no decision of
  // theirs reads cstat / gstat
  bool reproducible = false;
  unsigned long long* rstat = nullptr;
  unsigned long long* frozen() const { return reproducible ? rstat : nullptr; }
  ~nesti_model() {
    for (auto& p : packed) {
      if (p.second.wpk) (void)hipFree(p.second.wpk);
      if (p.second.bias) (void)hipFree(p.second.bias);
    }
    if (cstat) (void)hipFree(cstat);
    if (gstat) (void)hipFree(gstat);
    if (rstat) (void)hipFree(rstat);
    for (auto& gl : glane) {
      if (gl.gstream) (void)hipStreamDestroy(gl.gstream);
      for (auto& ev : gl.gev_done) if (ev) (void)hipEventDestroy(ev);
      if (gl.gev_join) (void)hipEventDestroy(gl.gev_join);
    }
  }
};

namespace nesti {
namespace {

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

// EXPERIMENT: the bit of Pass::mix that switches a layer of a pair-mode model to kFormMix (-1: none) -- the tap layers on
// conv8n_kernel / conv4n_kernel; the gating net's share one bit, the experts' are "inception<B>Expert_<i>_conv<2|3>" of blocks
// 1, 2 (8^3) and 4 (4^3), two bits per block (conv2, the smaller kernel, first)
constexpr int kGateMixBit = 8;
int mix_bit(const LayerDesc& d, int tower, int mdt) {
  if (act_planes(mdt) == 1 || layer_kind(d, mdt) < 2) return -1;
  if (tower < 0) return kGateMixBit;
  const int blk = d.scope.size() > 9 ? d.scope[9] - '0' : 0;
  const int idx = blk == 1 ? 0 : blk == 2 ? 1 : blk == 4 ? 2 : -1;
  return idx < 0 ? -1 : 2 * idx + (d.scope.back() == '3' ? 1 : 0);
}

struct LaunchForm {
  int form;        // NESTI_DEBUG_FORM_* or kFormMix
  int family;      // PackedLayer::kind of the packing the launch runs on
  bool producer;   // an 8^3 block's conv1 that also writes the FP8 / FP6 planes of its outputs for the block's tap layers
};
// How the conv launch `op` of a pass computes, for a model whose main dtype is mdt.  THE place that decides it: nesti_model_create
// packs what it names, run_op launches it and nesti_debug_tower_ops reports it.  A function of the configuration alone.
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
// workspace planning and tower execution
// ------------------------------------------------------------------------------------------
size_t buf_bytes(const BufSpec& b, int NB, int dtype) {
  const size_t e = b.aux8 ? 2 : b.f32 ? 4 : dtype_size(dtype) * act_planes(dtype);
  return align_up(((size_t)NB << (3 * b.log2S)) * b.C * e, 256);
}
// Workspace placement of a tower's buffers: a buffer lives from the first launch that writes it to the last launch that
// reads it (the tower's output until the end); buffers whose lifetimes do not overlap share memory (first fit), which
// brings the gating tower from 2.5 to 1.6 MB per query in 16-bit and lets one library batch cover a 100k-point cloud.
struct Placement {
  std::vector<size_t> off;   // per buffer (index 0 = the external MuPS tensor: unused)
  std::vector<int> first, last;   // per buffer: the first op that writes it, the last op that reads it (n_ops: the tower's output)
  size_t total = 0;
};
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
  struct Block { size_t off, size; int until; };
  std::vector<Block> live, freeb;
  Placement P;
  P.off.assign(n, 0);
  P.first = first; P.last = last;
  for (int i : order) {
    // release what is no longer read, coalescing neighbours
    for (size_t j = 0; j < live.size();) {
      if (live[j].until < first[i]) { freeb.push_back(live[j]); live.erase(live.begin() + j); } else ++j;
    }
    std::sort(freeb.begin(), freeb.end(), [](const Block& a, const Block& b) { return a.off < b.off; });
    for (size_t j = 0; j + 1 < freeb.size();) {
      if (freeb[j].off + freeb[j].size == freeb[j + 1].off) { freeb[j].size += freeb[j + 1].size; freeb.erase(freeb.begin() + j + 1); } else ++j;
    }
    const size_t need = buf_bytes(T.bufs[i], NB, dtype);
    size_t at = (size_t)-1;
    for (size_t j = 0; j < freeb.size(); ++j) {
      if (freeb[j].size >= need) {
        at = freeb[j].off;
        freeb[j].off += need; freeb[j].size -= need;
        if (freeb[j].size == 0) freeb.erase(freeb.begin() + j);
        break;
      }
    }
    if (at == (size_t)-1) {
      // grow at the top; a free block that ends at the top is extended instead of wasted
      if (!freeb.empty() && freeb.back().off + freeb.back().size == P.total) {
        at = freeb.back().off;
        P.total = at + need;
        freeb.pop_back();
      } else {
        at = P.total;
        P.total += need;
      }
    }
    P.off[i] = at;
    live.push_back({at, need, last[i]});
  }
  return P;
}
size_t tower_bytes(const Tower& T, int NB, int dtype) { return place_tower(T, NB, dtype).total; }

// Which k^3 layers use the Latin-square tile layout (kernels.h: ConvParams::remap): those where a 32-row tile can
// fall entirely on padding -- 5^3 taps at 8^3 (|d| = 2 clears a y/z pair) and every multi-tap layer at 4^3.  3^3 at
// 8^3 only ever clears single planes, which no 32-row tile shape can balance over four SIMDs.
int conv_remap(int k, int log2S, int n_taps) {
  if (n_taps <= 1) return 0;
  if (log2S == 1) return 2;              // 2^3: single-voxel tiles of 32 points (conv.hip: remap == 2)
  if (log2S != 2 && log2S != 3) return 0;
  return (log2S == 2 || k >= 4) ? 1 : 0;
}

// which NESTI_PROF_* conv category a layer's launch is booked under
int conv_category(const LayerDesc& d, const PackedLayer& pl) {
  if (pl.kind == 2) return d.k == 5 ? NESTI_PROF_CONV8_K5 : NESTI_PROF_CONV8_K3;
  return pl.n_taps > 1 ? NESTI_PROF_TAPS : NESTI_PROF_ONE_BY_ONE;
}

struct RunCtx {
  const nesti_model* m;
  Pass pass;
  int NB;                        // capacity (points)
  const int32_t* npoints_ptr;    // device-side live count or NULL
  const int32_t* point_index;    // gather for reads of bufs 0/1, or NULL
  hipStream_t stream;
  int walk;                      // this pass over a device-side list is probably empty (a later round, a widening pass): its conv
                                 // launches use small walking grids (kernels.h: ConvParams::walk)
};
// The RunCtx of a pass of the product: the gating net (tower -1) of gate_impl and of gate_cascade, filter pass (fast) and recheck;
// the expert towers of experts_impl with the model's x8_mask, and with x8_mask 0 -- the three-product loop everywhere -- for the
// conditioning guard's re-evaluation.  The experiment switches ride along: expert_mix on the experts, gate_mix on the gating net
// of a model without the two-stage gate
RunCtx pass_ctx(const nesti_model* m, int tower, bool fast, int x8_mask, int NB, const int32_t* npoints_ptr, const int32_t* point_index,
                hipStream_t stream, int walk) {
  Pass ps;
  ps.tower = tower; ps.fast = fast; ps.x8_mask = x8_mask; ps.x8_fmt = m->x8_fmt;
  if (tower >= 0) ps.mix = m->expert_mix;
  else if (!m->cascade && m->gate_mix) { ps.mix = 1 << kGateMixBit; ps.zero_lo = m->gate_mix == 2; }
  return RunCtx{m, ps, NB, npoints_ptr, point_index, stream, walk};
}

// The buffers of a tower in a workspace laid out by place_tower (ptr[0] = the MuPS tensor X0 the tower reads)
int tower_ptrs(const RunCtx& rc, const Tower& T, const void* X0, unsigned char* ws, size_t ws_bytes, std::vector<unsigned char*>* ptr) {
  const int dtype = rc.pass.fast ? NESTI_F16 : rc.m->dtype;
  ptr->assign(T.bufs.size(), nullptr);
  (*ptr)[0] = (unsigned char*)X0;
  const Placement P = place_tower(T, rc.NB, dtype);
  for (size_t i = 1; i < T.bufs.size(); ++i) (*ptr)[i] = ws + P.off[i];
  if (P.total > ws_bytes) NESTI_FAIL("workspace too small for this batch");
  return 0;
}

// One launch of a tower: the body of run_tower's loop, also reached alone through nesti_debug_tower_step
int run_op(const RunCtx& rc, const Tower& T, const Op& op, const std::vector<unsigned char*>& ptr) {
  const Pass& ps = rc.pass;
  const int dtype = ps.fast ? NESTI_F16 : rc.m->dtype;
  const int x0_planes = act_planes(rc.m->dtype);
  const bool ext_in = op.in_buf < 1;
  if (op.kind == Op::CONV) {
    const LayerDesc& d = rc.m->graph.layers[op.layer];
    const LaunchForm f = launch_form(rc.m->graph, op, ps, rc.m->dtype);
    const PackedLayer* plp = rc.m->packing(f.form, op.layer);
    if (!plp || plp->kind != f.family)
      NESTI_FAIL("internal: layer " + d.scope + " is not packed for form " + std::to_string(f.form) + " of this pass");
    const PackedLayer& pl = *plp;
    const bool mixl = f.form == kFormMix, x2l = f.form == NESTI_DEBUG_FORM_X2;
    const bool x8l = f.form == NESTI_DEBUG_FORM_X8 || f.form == NESTI_DEBUG_FORM_X6, x6 = ps.x8_fmt == 6;
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in_pair = mixl ? 1 : 0;
    p.x2 = x2l ? 1 : 0;
    p.in = ptr[op.in_buf]; p.out = ptr[op.out_buf]; p.wpk = pl.wpk; p.bias = pl.bias;
    p.npoints_ptr = rc.npoints_ptr; p.point_index = ext_in ? rc.point_index : nullptr;
    p.npoints = rc.NB;
    // pair modes: strides and the input offset are physical (a 64-aligned logical offset x 3), output column
    // offsets stay logical (kernels.h: ConvParams::split); an fp32 output buffer is an ordinary one
    const int planes = act_planes(dtype);
    p.split = planes > 1 ? (ps.zero_lo ? 2 : 1) : 0;
    const int in_planes = ext_in ? x0_planes : planes;
    p.in_cstride = (op.in_cstride ? op.in_cstride : T.bufs[op.in_buf].C) * in_planes; p.in_coff = op.in_coff * in_planes;
    // distance between consecutive K chunks of a PLAIN kernel's input row: 128 B, except in the NESTI_F16X3C filter pass,
    // whose plain-f16 first layer reads the hi plane of each 64-channel group [hi | lo] of the pair-layout MuPS tensor
    p.in_chunk_bytes = kRowBytes * (planes == 1 ? in_planes : 1);
    p.out_cstride = T.bufs[op.out_buf].C * (op.out_f32 ? 1 : planes); p.out_coff = op.out_coff;
    p.n_chunks = pl.n_chunks; p.n_taps = pl.n_taps; p.tap_k = d.k; p.log2S = d.log2S; p.s_real = d.s_real;
    p.relu = d.relu ? 1 : 0; p.out_f32 = op.out_f32 ? 1 : 0; p.acc_scale = pl.acc_scale; p.x3native = (pl.x3n && !x2l) ? 1 : 0;
    const long long rows = (long long)rc.NB << (3 * d.log2S);
    p.m_tiles = pl.kind == 3 ? (rc.NB + 15) / 16 : pl.kind == 2 ? (rc.NB + 3) / 4 : (int)((rows + kTileM - 1) / kTileM);
    p.n_tiles = pl.n_tiles; p.split_tile = pl.split_tile; p.out_coff2 = op.out_coff2; p.pool_k = d.pool_k;
    if (op.mp_buf >= 0) { p.mp_out = ptr[op.mp_buf]; p.mp_cstride = T.bufs[op.mp_buf].C * planes; p.mp_mode = op.mp_mode; p.mp_mode2 = op.mp_mode2; }
    if (x8l) {                                   // consumer: the FP8 cross-term loop on the planes the block's conv1 wrote
      const int sc = rc.m->main_packing(op.aux_layer).x8_sc;
      p.x8 = 1; p.aux8_in = ptr[op.aux_in_buf]; p.aux8_stride = T.bufs[op.aux_in_buf].C * 2;
      p.x8_scale_a = 127 - (sc + 11); p.x8_scale_b = 127 - pl.x8_sb;
      p.x8_fmt = x6 ? 6 : 8;
    }
    if (f.producer) {
      p.aux8_out = ptr[op.aux_out_buf]; p.aux8_stride = T.bufs[op.aux_out_buf].C * 2;
      p.x8_sc = rc.m->main_packing(op.layer).x8_sc; p.x8_sa = p.x8_sc + 11;
      p.x8_fmt = x6 ? 6 : 8;
    }
    memcpy(p.tap, pl.tap, sizeof(p.tap));
    p.remap = conv_remap(d.k, d.log2S, pl.n_taps);
    p.walk = rc.walk;
    const int cat = conv_category(d, pl);
    const int tok = prof_begin(cat, rc.stream);
    // (a mixed layer is a plain f16 / bf16 kernel inside a pair-mode tower: kernel_dtype is the same element type either way)
    const int rcv = pl.kind == 2   ? launch_conv8n(p, kernel_dtype(dtype), d.k, rc.stream)
                    : pl.kind == 3 ? launch_conv4n(p, kernel_dtype(dtype), d.k, rc.stream)
                                   : launch_conv(p, kernel_dtype(dtype), pl.TN, rc.stream);
    prof_end(cat, tok, rc.stream);
    if (rcv) return 1;
  } else {
    PoolParams p;
    memset(&p, 0, sizeof(p));
    p.in = ptr[op.in_buf]; p.out = ptr[op.out_buf];
    p.npoints_ptr = rc.npoints_ptr;
    p.npoints = rc.NB;
    const int planes = act_planes(dtype);
    p.split = planes > 1 ? 1 : 0;
    p.in_cstride = T.bufs[op.in_buf].C * planes; p.in_coff = op.in_coff;
    p.out_cstride = T.bufs[op.out_buf].C * planes; p.out_coff = op.out_coff;
    p.C = op.C; p.log2S = op.log2S;
    const int tok = prof_begin(NESTI_PROF_POOL, rc.stream);
    const int rcp = op.kind == Op::MAX3 ? launch_maxpool3s2(p, kernel_dtype(dtype), rc.stream)
                                        : launch_maxpool2(p, kernel_dtype(dtype), rc.stream);
    prof_end(NESTI_PROF_POOL, tok, rc.stream);
    if (rcp) return 1;
  }
  return 0;
}

int run_tower(const RunCtx& rc, const Tower& T, const void* X0, unsigned char* ws, size_t ws_bytes, float** out) {
  std::vector<unsigned char*> ptr;
  if (tower_ptrs(rc, T, X0, ws, ws_bytes, &ptr)) return 1;
  for (const Op& op : T.ops)
    if (run_op(rc, T, op, ptr)) return 1;
  *out = reinterpret_cast<float*>(ptr[T.out_buf]);
  return 0;
}

// channel stride of the MuPS rows the towers read, in elements (pair modes: two planes per 64-channel group)
int mups_stride(const nesti_model* m) { return m->graph.mups_cstride * act_planes(m->dtype); }

// NESTI_F16X3C: the f16x3 gate re-decides the flagged rows `cap` at a time (its workspace is 3x the filter's per row, and
// only a fraction of a batch is flagged): small batches in one round, large ones in quarters
int cascade_cap(int NB) { return NB <= 4096 ? NB : (int)align_up((size_t)(NB + 3) / 4, 256); }
int cascade_rounds(int NB) { return (NB + cascade_cap(NB) - 1) / cascade_cap(NB); }

// A routed expert sees about 1 / E of a batch, so its tower is sized for a quarter of a large batch and run in up to four
// rounds over its routing list (rounds beyond the list's length launch empty grids: ~0.2 % of a 100k batch); the workspace of a
// batch is then set by the gating net alone and a whole 100k-point cloud is one library batch in every mode but f16x3 / f32.
int expert_cap(int NB) { return NB <= 8192 ? NB : (int)align_up((size_t)(NB + 3) / 4, 256); }
// rows of ONE expert the conditioning guard can re-evaluate per pass (a fraction of a per cent of a batch are flagged at all)
int guard_cap(int NB) { return std::min(expert_cap(NB), 2048); }

size_t max_tower_bytes(const nesti_model* m, int NB) {
  size_t t = m->cascade ? std::max(tower_bytes(m->graph.gate, NB, NESTI_F16), tower_bytes(m->graph.gate, cascade_cap(NB), m->dtype))
                        : tower_bytes(m->graph.gate, NB, m->dtype);
  for (const Tower& e : m->graph.experts) t = std::max(t, tower_bytes(e, expert_cap(NB), m->dtype));
  return t;
}

struct WsLayout {
  size_t x0, probs, expert, counts, lists, ecounts, glist, keep, flags, fcounts, tower, total;
};
WsLayout ws_layout(const nesti_model* m, int NB) {
  WsLayout L;
  const size_t act = align_up(((size_t)NB << (3 * m->graph.gate_x0_log2S())) * mups_stride(m) * dtype_size(m->dtype), 256);
  size_t o = 0;
  L.x0 = o; o += act;
  L.probs = o; o += align_up((size_t)NB * NESTI_MAX_EXPERTS * 4, 256);
  L.expert = o; o += align_up((size_t)NB * 4, 256);
  L.counts = o; o += 256;
  L.lists = o; o += align_up((size_t)NB * NESTI_MAX_EXPERTS * 4, 256);
  L.ecounts = o; o += 1024;          // [E][rounds] rows of each expert round; words 128-135 / 140-141: the conditioning guard's list lengths and |n| band
  L.glist = o;
  if (m->graph.x8) o += align_up((size_t)NESTI_MAX_EXPERTS * guard_cap(NB) * 4, 256);   // the conditioning guard's row lists, one per expert
  L.keep = L.flags = L.fcounts = o;
  if (m->cascade) {   // the f16 gate's logits, the flag list, [flag count | per-round counts]
    L.keep = o; o += align_up((size_t)NB * NESTI_MAX_EXPERTS * 4, 256);
    L.flags = o; o += align_up((size_t)NB * 4, 256);
    L.fcounts = o; o += 512;          // kernels.h: the two-stage gate's per-call counters
  }
  L.tower = o; o += max_tower_bytes(m, NB);
  L.total = o;
  return L;
}

// NESTI_F16X3C (include/nesti_hip.h): the gating net in plain f16 over the batch, then in f16x3 over the rows whose f16
// top-2 margin is below tau (gathered through the flag list like a routed expert gathers its rows), `cap` rows per round;
// the routing lists are built from the final arg-max.  ws = the forward workspace (ws_layout), capacity NB >= B.
int gate_cascade(const nesti_model* m, const void* X0, int B, unsigned char* ws, const WsLayout& L, int NB, float* probs,
                 int32_t* expert, int32_t* counts, int32_t* lists, hipStream_t stream) {
  const int E = m->graph.cfg.n_experts;
  unsigned char* tower_ws = ws + L.tower;
  const size_t tower_bytes_ = L.total - L.tower;
  float* keep = (float*)(ws + L.keep);
  int32_t* flag_list = (int32_t*)(ws + L.flags);
  int32_t* fcounts = (int32_t*)(ws + L.fcounts);           // kernels.h: kRoundCountsOff, kTauEffOff, kWidenCountOff, kWidenRoundsOff
  const int lstride = m->graph.gate.bufs[m->graph.gate.out_buf].C;
  float* logits = nullptr;
  const RunCtx fast = pass_ctx(m, -1, /*fast=*/true, 0, B, nullptr, nullptr, stream, 0);
  prof_phase(NESTI_PHASE_GATE);
  if (run_tower(fast, m->graph.gate, X0, tower_ws, tower_bytes_, &logits)) return 1;
  prof_phase(NESTI_PHASE_RECHECK);
  const int cap = std::min(cascade_cap(NB), B), rounds = (B + cap - 1) / cap;
  unsigned long long* rstat = m->frozen();   // reproducible mode: the threshold is tau itself and pass 0 is the only pass
  if (launch_gate_flag(logits, lstride, B, E, m->tau, NESTI_GATE_WIDEN, probs, expert, keep, fcounts, flag_list, cap, rounds,
                       m->cstat, rstat, stream))
    return 1;
  // pass 0: the rows below the call's threshold; passes 1 .. NESTI_GATE_WIDEN_PASSES: widening passes -- the band between the
  // threshold reached so far and NESTI_GATE_WIDEN x the largest error measured up to the start of the pass, so an error first
  // seen inside a widening pass is covered by the next one of the SAME call (normally every pass is empty: its launches find a
  // zero row count on the device and return; no host synchronisation, so the whole call stays graph-capturable)
  for (int pass = 0; pass <= (rstat ? 0 : NESTI_GATE_WIDEN_PASSES); ++pass) {
    if (pass >= 1 && launch_gate_widen(keep, B, E, NESTI_GATE_WIDEN, fcounts, flag_list, cap, rounds, m->cstat, stream)) return 1;
    const int32_t* round_counts = fcounts + (pass == 0 ? kRoundCountsOff : kWidenRoundsOff);
    for (int r = 0; r < rounds; ++r) {
      // round 0 of pass 0 holds the flagged rows; everything after it is normally empty
      const RunCtx exact = pass_ctx(m, -1, false, 0, cap, round_counts + r, flag_list + (size_t)r * cap, stream,
                                    pass >= 1 ? NESTI_GATE_WIDEN_WALK_GRID : r >= 1 ? 1 : 0);
      if (run_tower(exact, m->graph.gate, X0, tower_ws, tower_bytes_, &logits)) return 1;
      if (launch_gate_recheck(logits, lstride, flag_list + (size_t)r * cap, round_counts + r, cap, E, keep, probs, expert,
                              m->cstat, fcounts, NESTI_GATE_WIDEN, rstat, stream))
        return 1;
    }
  }
  if (counts) return launch_route(expert, B, E, counts, lists, stream);
  return 0;
}

int gate_impl(const nesti_model* m, const void* X0, int B, unsigned char* tower_ws, size_t tower_bytes_,
              float* probs, int32_t* expert, int32_t* counts, int32_t* lists, hipStream_t stream) {
  const RunCtx rc = pass_ctx(m, -1, false, 0, B, nullptr, nullptr, stream, 0);
  float* logits = nullptr;
  prof_phase(NESTI_PHASE_GATE);
  if (run_tower(rc, m->graph.gate, X0, tower_ws, tower_bytes_, &logits)) return 1;
  const int lstride = m->graph.gate.bufs[m->graph.gate.out_buf].C;
  if (m->graph.cfg.arch == NESTI_ARCH_SWITCH)   // noise_est < 0.015 -> small, else large (models/ms_sw_n_est.py:80-82)
    return launch_switch_finish(logits, lstride, B, 0.015f, probs, expert, counts, lists, stream);
  return launch_gate_finish(logits, lstride, B, m->graph.cfg.n_experts, probs, expert, counts, lists, stream);
}

// NB = the batch capacity the workspace was laid out for (ws_layout); ecounts = its per-(expert, round) counter block; glist = the
// conditioning guard's row list (x8 models, top-1 routing)
constexpr int kGuardCountOff = 128, kGuardSlotOff = 140;      // int32 words of the ecounts block: [E] list lengths, the |n| band
int experts_impl(const nesti_model* m, const void* X0, int B, int NB, unsigned char* tower_ws, size_t tower_bytes_,
                 const int32_t* counts, const int32_t* lists, int32_t* ecounts, int32_t* glist, float* normals, hipStream_t stream) {
  const int E = m->graph.cfg.n_experts;
  const int cap = std::min(expert_cap(NB), B), rounds = (B + cap - 1) / cap;
  prof_phase(NESTI_PHASE_EXPERTS);
  if (counts && launch_round_counts(counts, E, cap, rounds, ecounts, stream)) return 1;
  const size_t x0_row = ((size_t)1 << (3 * m->graph.gate_x0_log2S())) * mups_stride(m) * dtype_size(m->dtype);   // one query's MuPS rows
  // the conditioning guard of the FP8 cross-term layers (pool.hip): once expert e's rows are written, those whose |n| falls inside the
  // pass's band go through the SAME tower in f16x3 proper, which replaces them and measures |dn|; a second pass covers the band a
  // larger measurement of THIS call may have opened (normally empty).  A guard tower sees a handful of rows, so it is latency-bound
  // (~3 ms: one workgroup walks a layer's whole K loop): in the first pass expert e's guard runs on the model's auxiliary stream, in its
  // own slice of the tower workspace, while the caller's stream goes on with expert e + 1
  const bool guard = counts && glist && m->x8_mask && m->gstat && m->x8_guard_thr >= 0.f;
  const int gcap = std::min(guard_cap(NB), B);
  float* gslot = guard ? reinterpret_cast<float*>(ecounts + kGuardSlotOff) : nullptr;
  int32_t* gcount = guard ? ecounts + kGuardCountOff : nullptr;                 // [E]
  const float gscale = NESTI_X8_GUARD_WIDEN / sqrtf(2.f * NESTI_X8_GUARD_BAR);
  unsigned long long* rstat = m->frozen();   // reproducible mode: the band is [0, thr) and pass 0 is the only pass
  size_t main_bytes = 0, guard_bytes = 0;
  for (int e = 0; e < E && guard; ++e) {
    main_bytes = std::max(main_bytes, align_up(tower_bytes(m->graph.experts[e], cap, m->dtype), 256));
    guard_bytes = std::max(guard_bytes, tower_bytes(m->graph.experts[e], gcap, m->dtype));
  }
  // (a stream that is being captured into a hipGraph keeps everything on itself: the guard then runs on the caller's stream, one
  // tower after the other, like it does when the two workspace slices do not fit)
  nesti_model::GuardLane* lane = guard ? m->guard_lane(stream) : nullptr;
  const bool side = guard && lane->gstream && main_bytes + guard_bytes <= tower_bytes_ && !prof_capturing(stream);
  std::unique_lock<std::mutex> glk;
  if (side) glk = std::unique_lock<std::mutex>(lane->gmu);   // the lane's auxiliary stream and events: one call enqueues on them at a time
  auto guard_expert = [&](int e, hipStream_t st, unsigned char* arena, size_t arena_bytes, int walk_grid) -> int {
    const Tower& T = m->graph.experts[e];
    int32_t* gl = glist + (size_t)e * gcap;
    if (launch_x8_guard_flag(lists + (size_t)e * B, counts + e, B, normals, gslot, gl, gcount + e, gcap, m->gstat, st)) return 1;
    float* out = nullptr;
    const RunCtx rc = pass_ctx(m, e, false, /*x8_mask=*/0, gcap, gcount + e, gl, st, walk_grid);   // a small walking grid (a few dozen rows)
    if (run_tower(rc, T, X0, arena, arena_bytes, &out)) return 1;
    return launch_x8_guard_fix(out, T.bufs[T.out_buf].C, gl, gcount + e, gcap, normals, m->gstat, m->x8_guard_thr, gscale, rstat, st);
  };
  if (guard && launch_x8_guard_begin(0, m->x8_guard_thr, gscale, B, m->gstat, gslot, rstat, stream)) return 1;
  for (int e = 0; e < E; ++e) {
    const Tower& T = m->graph.experts[e];
    const int ostride = T.bufs[T.out_buf].C;
    for (int r = 0; r < rounds; ++r) {
      float* out = nullptr;
      if (counts) {   // top-1 routing: only the points whose arg-max is e (test_n_est_w_experts.py:150-152), `cap` of them per round
        const int32_t* list = lists + (size_t)e * B + (size_t)r * cap;
        const int32_t* cnt = ecounts + e * rounds + r;
        // an expert sees ~1 / E of a batch: rounds after the first are normally empty
        const RunCtx rc = pass_ctx(m, e, false, m->x8_mask, cap, cnt, list, stream, /*walk=*/r >= 1);
        if (run_tower(rc, T, X0, tower_ws, tower_bytes_, &out)) return 1;
        if (launch_scatter3(out, ostride, list, cnt, cap, normals, stream)) return 1;
      } else {        // reference behaviour: every expert on every point -> [E,B,3], rows [r * cap, ...) of the batch per round
        const int take = std::min(cap, B - r * cap);
        const RunCtx rc = pass_ctx(m, e, false, m->x8_mask, take, nullptr, nullptr, stream, 0);
        if (run_tower(rc, T, (const unsigned char*)X0 + (size_t)r * cap * x0_row, tower_ws, tower_bytes_, &out)) return 1;
        if (launch_scatter3(out, ostride, nullptr, nullptr, take, normals + ((size_t)e * B + (size_t)r * cap) * 3, stream)) return 1;
      }
    }
    if (guard) {
      prof_phase(NESTI_PHASE_GUARD);
      if (side) {
        NESTI_CHECK_HIP(hipEventRecord(lane->gev_done[e], stream));
        NESTI_CHECK_HIP(hipStreamWaitEvent(lane->gstream, lane->gev_done[e], 0));
        if (guard_expert(e, lane->gstream, tower_ws + main_bytes, tower_bytes_ - main_bytes, m->x8_guard_walk)) return 1;
      } else if (guard_expert(e, stream, tower_ws, tower_bytes_, m->x8_guard_walk)) {
        return 1;
      }
      prof_phase(NESTI_PHASE_EXPERTS);
    }
  }
  if (guard) {
    if (side) {
      NESTI_CHECK_HIP(hipEventRecord(lane->gev_join, lane->gstream));
      NESTI_CHECK_HIP(hipStreamWaitEvent(stream, lane->gev_join, 0));
      glk.unlock();
    }
    prof_phase(NESTI_PHASE_GUARD);
    for (int pass = 1; pass <= (rstat ? 0 : NESTI_X8_GUARD_WIDEN_PASSES); ++pass) {
      if (launch_x8_guard_begin(pass, m->x8_guard_thr, gscale, B, m->gstat, gslot, nullptr, stream)) return 1;
      for (int e = 0; e < E; ++e)
        if (guard_expert(e, stream, tower_ws, tower_bytes_, NESTI_GUARD_WIDEN_WALK_GRID)) return 1;
    }
  }
  return 0;
}

}  // namespace
}  // namespace nesti

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace nesti;

extern "C" {

const char* nesti_last_error(void) { return g_error.c_str(); }
const char* nesti_version(void) {
  return "nesti-hip 0.6 (gfx950)"   // measurement builds are named
#ifdef NESTI_ATTRIBUTION
         " [measurement build: NESTI_ATTRIBUTION]"
#endif
#ifdef NESTI_EXPERIMENT_XW
         " [measurement build: NESTI_EXPERIMENT_XW]"
#endif
      ;
}

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

int nesti_mups_forward(const nesti_config_t* cfg, const float* points_dev, const int32_t* n_eff_dev, int B,
                       void* out_dev, int out_dtype, int out_cstride, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!cfg || !points_dev || !n_eff_dev || !out_dev) NESTI_FAIL("nesti_mups_forward: null argument");
  const int tok = prof_begin(NESTI_PROF_MUPS, (hipStream_t)stream);
  const int rc = launch_mups(cfg, points_dev, n_eff_dev, B, out_dev, out_dtype, out_cstride, /*embed4=*/0, (hipStream_t)stream);
  prof_end(NESTI_PROF_MUPS, tok, (hipStream_t)stream);
  return rc;
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

int nesti_model_create(const nesti_config_t* cfg, const nesti_tensor_t* tensors, int n_tensors, int dtype,
                       nesti_model_t** out) {
  if (!cfg || !tensors || !out) NESTI_FAIL("nesti_model_create: null argument");
  if (dtype != NESTI_F32 && dtype != NESTI_BF16 && dtype != NESTI_F16 && dtype != NESTI_BF16X3 && dtype != NESTI_F16X3 &&
      dtype != NESTI_F16X3C && dtype != NESTI_F16X8 && dtype != NESTI_F16X8C)
    NESTI_FAIL("nesti_model_create: bad dtype");
  if (dtype_cascade(dtype) && cfg->arch != NESTI_ARCH_EXPERTS)
    NESTI_FAIL("nesti_model_create: NESTI_F16X3C / NESTI_F16X8C is the two-stage gate of experts_n_est; use NESTI_F16X3 for the other models");
  if (dtype_x8(dtype) && (cfg->arch != NESTI_ARCH_EXPERTS || cfg->grid_n != 8))
    NESTI_FAIL("nesti_model_create: NESTI_F16X8 / NESTI_F16X8C (FP8 cross terms in the expert towers) is for experts_n_est on the 8^3 grid");
  std::unique_ptr<nesti_model> m(new nesti_model());
  m->cascade = dtype_cascade(dtype);
  const bool x8 = dtype_x8(dtype);
  dtype = main_dtype(dtype);
  m->dtype = dtype;
  if (build_graph(cfg, &m->graph, x8)) return 1;
  TensorTable tt;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name) tt.by_name[tensors[i].name] = &tensors[i];
  // the 8^3 tap kernel's x padding relies on out-of-range LDS reads returning zero: checked once per device, and only for
  // models that have such layers
  bool any_conv8 = false;
  for (const LayerDesc& d : m->graph.layers) any_conv8 = any_conv8 || layer_kind(d, dtype) == 2;
  if (any_conv8 && conv8_selftest()) return 1;
  // the passes a model of this dtype runs, per tower (-1: the gating net): the main pass; the filter pass of the two-stage gate; the
  // experts' cross-term passes in both formats (x8_mask 0, the guard's re-evaluation, is the main pass); the experiment's
  // single-product passes.  Every (packing, layer) launch_form names over them is packed once
  m->has_mix = g_experiment_mix && act_planes(dtype) > 1 && cfg->arch == NESTI_ARCH_EXPERTS && cfg->grid_n == 8;
  for (int t = -1; t < (int)m->graph.experts.size(); ++t) {
    std::vector<Pass> passes(1);
    if (m->cascade && t < 0) { passes.push_back(Pass()); passes.back().fast = true; }
    for (int fmt : {8, 6})
      if (x8 && t >= 0) { passes.push_back(Pass()); passes.back().x8_mask = 0xF; passes.back().x8_fmt = fmt; }
    if (m->has_mix) { passes.push_back(Pass()); passes.back().mix = t < 0 ? 1 << kGateMixBit : 0x3F; }
    for (Pass& ps : passes) {
      ps.tower = t;
      for (const Op& op : (t < 0 ? m->graph.gate : m->graph.experts[t]).ops) {
        if (op.kind != Op::CONV) continue;
        const LayerDesc& d = m->graph.layers[op.layer];
        const LaunchForm f = launch_form(m->graph, op, ps, dtype);
        const int packing = form_packing(f.form);
        PackedLayer& pl = m->packed[{packing, op.layer}];
        PackedImage img;
        if (!pl.wpk && (pack_form(d, tt, packing, dtype, &img) || upload(img, &pl))) return 1;
        if (f.producer) pl.x8_sc = x8_activation_exponent(d, tt);   // the pre-scale of the planes it writes
      }
    }
  }
  if (x8) {
    m->x8_mask = 0xF;         // all four tap layers at 8^3 (include/nesti_hip.h: nesti_model_set_x8_layers)
    NESTI_CHECK_HIP(hipMalloc((void**)&m->gstat, 64));
    NESTI_CHECK_HIP(hipMemset(m->gstat, 0, 64));
    for (auto& gl : m->glane) {
      NESTI_CHECK_HIP(hipStreamCreateWithFlags(&gl.gstream, hipStreamNonBlocking));
      NESTI_CHECK_HIP(hipEventCreateWithFlags(&gl.gev_join, hipEventDisableTiming));
      for (int e = 0; e < cfg->n_experts; ++e) NESTI_CHECK_HIP(hipEventCreateWithFlags(&gl.gev_done[e], hipEventDisableTiming));
    }
  }
  if (m->cascade) {
    NESTI_CHECK_HIP(hipMalloc((void**)&m->cstat, 64));
    NESTI_CHECK_HIP(hipMemset(m->cstat, 0, 64));
  }
  if (m->cstat || m->gstat) {   // the reproducible mode's own counters (nesti_model_set_reproducible)
    NESTI_CHECK_HIP(hipMalloc((void**)&m->rstat, 64));
    NESTI_CHECK_HIP(hipMemset(m->rstat, 0, 64));
  }
  NESTI_CHECK_HIP(hipDeviceSynchronize());
  *out = m.release();
  return 0;
}

void nesti_model_destroy(nesti_model_t* m) { delete m; }

int nesti_model_set_gate_margin(nesti_model_t* m, float tau) {
  if (!m || !m->cascade) NESTI_FAIL("nesti_model_set_gate_margin: not a NESTI_F16X3C model");
  if (!(tau >= 0.f)) NESTI_FAIL("nesti_model_set_gate_margin: tau must be >= 0");
  m->tau = tau;
  return 0;
}

int nesti_experiment_mix_enable(int on) {
  g_experiment_mix = on != 0;
  return 0;
}

int nesti_model_set_expert_mix(nesti_model_t* m, int mask) {
  if (!m) NESTI_FAIL("nesti_model_set_expert_mix: null model");
  if (mask && !m->has_mix) NESTI_FAIL("nesti_model_set_expert_mix: pair-mode experts_n_est models (8^3 grid) created after nesti_experiment_mix_enable(1) only");
  if (mask < 0 || mask >= (1 << 6)) NESTI_FAIL("nesti_model_set_expert_mix: mask has six bits");
  m->expert_mix = mask;
  return 0;
}

int nesti_model_set_x8_layers(nesti_model_t* m, int mask) {
  if (!m) NESTI_FAIL("nesti_model_set_x8_layers: null model");
  if (!m->graph.x8) NESTI_FAIL("nesti_model_set_x8_layers: not an NESTI_F16X8 / NESTI_F16X8C model");
  if (mask < 0 || mask > 0xF) NESTI_FAIL("nesti_model_set_x8_layers: mask has four bits (inception1 conv2 / conv3, inception2 conv2 / conv3)");
  m->x8_mask = mask;
  return 0;
}

int nesti_model_set_x8_format(nesti_model_t* m, int bits) {
  if (!m) NESTI_FAIL("nesti_model_set_x8_format: null model");
  if (!m->graph.x8) NESTI_FAIL("nesti_model_set_x8_format: not an NESTI_F16X8 / NESTI_F16X8C model");
  if (bits != 8 && bits != 6) NESTI_FAIL("nesti_model_set_x8_format: 8 (e4m3, one scale per layer) or 6 (e2m3, one scale per 16-channel block)");
  m->x8_fmt = bits;
  return 0;
}

int nesti_model_set_x8_guard(nesti_model_t* m, float thr) {
  if (!m || !m->gstat) NESTI_FAIL("nesti_model_set_x8_guard: not an NESTI_F16X8 / NESTI_F16X8C model");
  if (thr != thr) NESTI_FAIL("nesti_model_set_x8_guard: threshold is NaN");
  m->x8_guard_thr = thr;
  return 0;
}

int nesti_model_x8_guard_stats(const nesti_model_t* m, nesti_x8_guard_stats_t* out, int reset, void* stream) {
  if (!m || !m->gstat || !out) NESTI_FAIL("nesti_model_x8_guard_stats: not an NESTI_F16X8 / NESTI_F16X8C model / null argument");
  unsigned long long h[8];
  NESTI_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  NESTI_CHECK_HIP(hipMemcpy(h, m->gstat, sizeof(h), hipMemcpyDeviceToHost));
  if (reset) NESTI_CHECK_HIP(hipMemset(m->gstat, 0, 64));
  out->queries = h[0]; out->rechecked = h[1]; out->dropped = h[3];
  const uint32_t bits = (uint32_t)h[2];
  memcpy(&out->max_dn, &bits, 4);
  out->thr = m->x8_guard_thr;
  out->thr_eff = m->x8_guard_thr < 0.f || m->reproducible ? m->x8_guard_thr
                                       : std::max(m->x8_guard_thr, NESTI_X8_GUARD_WIDEN * out->max_dn / sqrtf(2.f * NESTI_X8_GUARD_BAR));
  return 0;
}

int nesti_model_set_gate_mix(nesti_model_t* m, int on) {
  if (!m) NESTI_FAIL("nesti_model_set_gate_mix: null model");
  if (on && !m->has_mix) NESTI_FAIL("nesti_model_set_gate_mix: pair-mode experts_n_est models (8^3 grid) created after nesti_experiment_mix_enable(1) only");
#ifndef NESTI_EXPERIMENT_XW
  if (on == 2) NESTI_FAIL("nesti_model_set_gate_mix: mode 2 (the exact-weight filter emulation of profiles/r05_gate_medium.txt) needs a "
                          "library built with EXTRA_CXXFLAGS=-DNESTI_EXPERIMENT_XW");
#endif
  m->gate_mix = on == 2 ? 2 : on ? 1 : 0;   // 2: additionally every layer's OUTPUT is rounded to 16 bits (lo = 0): the numerics of a
                                            // plain-f16 gate whose 1x1x1 / FC layers multiply by the exact weights (hi * W_hi + hi * W_lo)
  return 0;
}

int nesti_model_cascade_stats(const nesti_model_t* m, nesti_cascade_stats_t* out, int reset, void* stream) {
  if (!m || !m->cascade || !out) NESTI_FAIL("nesti_model_cascade_stats: not a NESTI_F16X3C model");
  unsigned long long h[8];
  NESTI_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  NESTI_CHECK_HIP(hipMemcpy(h, m->cstat, sizeof(h), hipMemcpyDeviceToHost));
  if (reset) NESTI_CHECK_HIP(hipMemset(m->cstat, 0, 64));
  out->queries = h[0]; out->rechecked = h[1]; out->changed = h[2];
  const uint32_t bits = (uint32_t)h[3];
  memcpy(&out->max_margin_err, &bits, 4);
  out->tau = m->tau;
  memcpy(&out->sum_sq_pair_err, &h[4], 8);
  out->pairs = h[5];
  out->widened = h[6];
  out->widen_events = h[7];
  out->tau_eff = m->reproducible ? m->tau : std::max(m->tau, NESTI_GATE_WIDEN * out->max_margin_err);
  return 0;
}

int nesti_model_set_reproducible(nesti_model_t* m, int on) {
  if (!m) NESTI_FAIL("nesti_model_set_reproducible: null model");
  m->reproducible = on != 0;   // a model with neither two-stage gate nor guard has no rstat: frozen() stays null, nothing changes
  return 0;
}

int nesti_model_reproducible_stats(const nesti_model_t* m, nesti_reproducible_stats_t* out, int reset, void* stream) {
  if (!m || !out) NESTI_FAIL("nesti_model_reproducible_stats: null model / null argument");
  unsigned long long r[8] = {}, c[8] = {}, g[8] = {};
  NESTI_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (m->rstat) NESTI_CHECK_HIP(hipMemcpy(r, m->rstat, sizeof(r), hipMemcpyDeviceToHost));
  if (m->cstat) NESTI_CHECK_HIP(hipMemcpy(c, m->cstat, sizeof(c), hipMemcpyDeviceToHost));
  if (m->gstat) NESTI_CHECK_HIP(hipMemcpy(g, m->gstat, sizeof(g), hipMemcpyDeviceToHost));
  if (reset) {
    if (m->rstat) NESTI_CHECK_HIP(hipMemset(m->rstat, 0, 64));
    if (m->cstat) NESTI_CHECK_HIP(hipMemset(m->cstat, 0, 64));
    if (m->gstat) NESTI_CHECK_HIP(hipMemset(m->gstat, 0, 64));
  }
  memset(out, 0, sizeof(*out));
  out->on = m->reproducible ? 1 : 0;
  out->gate_violations = r[0]; out->guard_violations = r[1]; out->guard_dropped = g[3];
  const uint32_t eb = (uint32_t)c[3], db = (uint32_t)g[2];
  memcpy(&out->max_margin_err, &eb, 4);
  memcpy(&out->max_dn, &db, 4);
  out->tau = m->cascade ? m->tau : 0.f;
  out->thr = m->gstat ? m->x8_guard_thr : -1.f;
  return 0;
}

int nesti_model_gate_error_export(const nesti_model_t* m, float* dst_dev, void* stream) {
  if (!m || !m->cascade || !dst_dev) NESTI_FAIL("nesti_model_gate_error_export: not a NESTI_F16X3C model / null argument");
  return launch_stat_max_export(m->cstat + 3, dst_dev, (hipStream_t)stream);
}

int nesti_model_gate_error_import(nesti_model_t* m, const float* src_dev, int n, void* stream) {
  if (!m || !m->cascade || (n > 0 && !src_dev)) NESTI_FAIL("nesti_model_gate_error_import: not a NESTI_F16X3C model / null argument");
  return launch_stat_max_import(m->cstat + 3, src_dev, n, (hipStream_t)stream);
}

int nesti_model_guard_error_export(const nesti_model_t* m, float* dst_dev, void* stream) {
  if (!m || !m->gstat || !dst_dev) NESTI_FAIL("nesti_model_guard_error_export: not an NESTI_F16X8 / NESTI_F16X8C model / null argument");
  return launch_stat_max_export(m->gstat + 2, dst_dev, (hipStream_t)stream);
}

int nesti_model_guard_error_import(nesti_model_t* m, const float* src_dev, int n, void* stream) {
  if (!m || !m->gstat || (n > 0 && !src_dev)) NESTI_FAIL("nesti_model_guard_error_import: not an NESTI_F16X8 / NESTI_F16X8C model / null argument");
  return launch_stat_max_import(m->gstat + 2, src_dev, n, (hipStream_t)stream);
}

size_t nesti_tower_workspace_bytes(const nesti_config_t* cfg, int dtype, int tower, int batch) {
  if (!cfg || batch <= 0) return 0;
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 0;
  if (tower < -1 || tower >= (int)g.experts.size()) return 0;
  const int dt = tower < 0 && dtype_cascade(dtype) ? NESTI_F16 : main_dtype(dtype);
  return tower_bytes(tower < 0 ? g.gate : g.experts[tower], batch, dt);
}

size_t nesti_workspace_bytes(const nesti_model_t* m, int max_batch) {
  if (!m || max_batch <= 0) return 0;
  return ws_layout(m, max_batch).total;
}

int nesti_model_mups_cstride(const nesti_model_t* m) { return m ? nesti::mups_stride(m) : 0; }
int nesti_model_mups_rows(const nesti_model_t* m) { return m ? 1 << (3 * m->graph.gate_x0_log2S()) : 0; }

int nesti_model_mups(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev, int B, void* mups_out_dev,
                     void* stream) {
  if (B <= 0) return 0;
  if (!m || !points_dev || !n_eff_dev || !mups_out_dev) NESTI_FAIL("nesti_model_mups: null argument");
  const int tok = prof_begin(NESTI_PROF_MUPS, (hipStream_t)stream);
  const int rc = launch_mups(&m->graph.cfg, points_dev, n_eff_dev, B, mups_out_dev, m->dtype, mups_stride(m),
                             /*embed4=*/m->graph.cfg.grid_n == 3, (hipStream_t)stream);
  prof_end(NESTI_PROF_MUPS, tok, (hipStream_t)stream);
  return rc;
}

int nesti_gate_forward(const nesti_model_t* m, const void* mups_dev, int B, void* ws_dev, size_t ws_bytes,
                       float* probs_out_dev, int32_t* expert_out_dev, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!m || !mups_dev || !ws_dev) NESTI_FAIL("nesti_gate_forward: null argument");
  if (m->graph.cfg.arch != NESTI_ARCH_EXPERTS && m->graph.cfg.arch != NESTI_ARCH_SWITCH)
    NESTI_FAIL("nesti_gate_forward: this model has no gating net");
  if (B <= 0) return 0;
  const WsLayout L = ws_layout(m, B);
  if (L.total > ws_bytes) NESTI_FAIL("nesti_gate_forward: workspace too small (see nesti_workspace_bytes)");
  unsigned char* ws = (unsigned char*)ws_dev;
  hipStream_t st = (hipStream_t)stream;
  if (m->cascade)
    return gate_cascade(m, mups_dev, B, ws, L, B, probs_out_dev, expert_out_dev ? expert_out_dev : (int32_t*)(ws + L.expert),
                        nullptr, nullptr, st);
  return gate_impl(m, mups_dev, B, ws + L.tower, L.total - L.tower, probs_out_dev, expert_out_dev, nullptr,
                   nullptr, st);
}

int nesti_experts_forward(const nesti_model_t* m, const void* mups_dev, const int32_t* expert_dev, int B, void* ws_dev,
                          size_t ws_bytes, float* normals_out_dev, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!m || !mups_dev || !ws_dev || !normals_out_dev) NESTI_FAIL("nesti_experts_forward: null argument");
  if (B <= 0) return 0;
  const WsLayout L = ws_layout(m, B);
  if (L.total > ws_bytes) NESTI_FAIL("nesti_experts_forward: workspace too small (see nesti_workspace_bytes)");
  unsigned char* ws = (unsigned char*)ws_dev;
  hipStream_t st = (hipStream_t)stream;
  int32_t* counts = nullptr;
  int32_t* lists = nullptr;
  if (expert_dev) {
    counts = (int32_t*)(ws + L.counts);
    lists = (int32_t*)(ws + L.lists);
    if (launch_route(expert_dev, B, m->graph.cfg.n_experts, counts, lists, st)) return 1;
  }
  return experts_impl(m, mups_dev, B, B, ws + L.tower, L.total - L.tower, counts, lists, (int32_t*)(ws + L.ecounts),
                      m->graph.x8 ? (int32_t*)(ws + L.glist) : nullptr, normals_out_dev, st);
}

// gate -> routing -> experts on a MuPS tensor X0 that already sits in the workspace
static int forward_tail(const nesti_model_t* m, const void* X0, int B, int NB, unsigned char* ws, const WsLayout& L,
                        float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, hipStream_t st) {
  if (m->graph.cfg.arch == NESTI_ARCH_SINGLE || m->graph.cfg.arch == NESTI_ARCH_MULTI)   // single-tower ablations: the tower's output IS n_pred (test_n_est.py:136-141)
    return experts_impl(m, X0, B, NB, ws + L.tower, L.total - L.tower, nullptr, nullptr, nullptr, nullptr, normals_out_dev, st);
  float* probs = probs_out_dev ? probs_out_dev : (float*)(ws + L.probs);
  int32_t* expert = expert_out_dev ? expert_out_dev : (int32_t*)(ws + L.expert);
  int32_t* counts = (int32_t*)(ws + L.counts);
  int32_t* lists = (int32_t*)(ws + L.lists);
  if (m->cascade ? gate_cascade(m, X0, B, ws, L, NB, probs, expert, counts, lists, st)
                 : gate_impl(m, X0, B, ws + L.tower, L.total - L.tower, probs, expert, counts, lists, st))
    return 1;
  return experts_impl(m, X0, B, NB, ws + L.tower, L.total - L.tower, counts, lists, (int32_t*)(ws + L.ecounts),
                      m->graph.x8 ? (int32_t*)(ws + L.glist) : nullptr, normals_out_dev, st);
}

int nesti_forward(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev, int B, void* ws_dev,
                  size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!m || !points_dev || !n_eff_dev || !ws_dev || !normals_out_dev) NESTI_FAIL("nesti_forward: null argument");
  const WsLayout L = ws_layout(m, B);
  if (L.total > ws_bytes) NESTI_FAIL("nesti_forward: workspace too small (see nesti_workspace_bytes)");
  unsigned char* ws = (unsigned char*)ws_dev;
  hipStream_t st = (hipStream_t)stream;
  void* X0 = ws + L.x0;
  const int tok = prof_begin(NESTI_PROF_MUPS, st);
  const int rcm = launch_mups(&m->graph.cfg, points_dev, n_eff_dev, B, X0, m->dtype, mups_stride(m),
                              /*embed4=*/m->graph.cfg.grid_n == 3, st);
  prof_end(NESTI_PROF_MUPS, tok, st);
  if (rcm) return 1;
  return forward_tail(m, X0, B, B, ws, L, normals_out_dev, expert_out_dev, probs_out_dev, st);
}

// ---- fused end-to-end entry: search grid + ball query + MuPS + gate + routed experts, batch by batch ---------------
// 8^3 Gaussian grid: patches_mups_kernel goes from the cloud to the MuPS tensor in one kernel (the patch tensors are never
// written); 3^3 grid: patches_kernel + mups3_kernel through a staging buffer in the workspace.
static size_t est_points_bytes(const nesti_model* m, int batch) {
  if (m->graph.cfg.grid_n == 8) return 0;
  return align_up((size_t)batch * m->graph.cfg.n_scales * m->graph.cfg.points_per_scale * 3 * sizeof(float), 256);
}
static size_t est_neff_bytes(const nesti_model* m, int batch) {
  return align_up((size_t)batch * m->graph.cfg.n_scales * sizeof(int32_t), 256);
}

size_t nesti_estimate_workspace_bytes(const nesti_model_t* m, int batch) {
  if (!m || batch <= 0) return 0;
  return est_points_bytes(m, batch) + est_neff_bytes(m, batch) + ws_layout(m, batch).total;
}

size_t nesti_estimate_workspace_bytes_for_config(const nesti_config_t* cfg, int dtype, int batch) {
  if (!cfg || batch <= 0) return 0;
  // the layout functions only look at the graph and the mode flags: a model shell without weights sizes exactly like the real one
  nesti_model shell;
  shell.cascade = dtype_cascade(dtype);
  shell.dtype = main_dtype(dtype);
  if (build_graph(cfg, &shell.graph, dtype_x8(dtype))) return 0;
  return nesti_estimate_workspace_bytes(&shell, batch);
}

// nesti_estimate_normals (centres = cloud points) and nesti_estimate_normals_at (centres = positions, `at`): one body.  The
// position form also applies the sentinel of queries without a neighbourhood, after each batch's outputs are complete
// (forward_tail ends with the conditioning guard joined on `st`), and can hand out the uncapped ball sizes.
static int estimate_impl(const char* who, bool at, const nesti_model_t* m, const float* cloud_dev, int N, const int32_t* query_idx_dev,
                         const float* query_xyz_dev, int M, const double* r_abs, uint64_t seed, int query_row0, int batch,
                         int build_grid, void* grid_ws_dev, size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes, float* normals_out_dev,
                         int32_t* expert_out_dev, float* probs_out_dev, int32_t* n_ball_out_dev, void* stream) {
  const std::string w(who);
  if (M <= 0) return 0;   // no queries: nothing to do
  if (!m || !cloud_dev || !r_abs || !grid_ws_dev || !ws_dev || !normals_out_dev) NESTI_FAIL(w + ": null argument");
  if (at && !query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (batch <= 0) NESTI_FAIL(w + ": batch must be positive");
  if (at && query_row0 < 0) NESTI_FAIL(w + ": query_row0 must be >= 0");
  if (!at && (query_row0 < 0 || (!query_idx_dev && (long long)query_row0 + M > (long long)N)))
    NESTI_FAIL(w + ": query rows [query_row0, query_row0 + M) exceed the cloud (N points)");
  if (nesti_estimate_workspace_bytes(m, batch) > ws_bytes)
    NESTI_FAIL(w + ": workspace too small (see nesti_estimate_workspace_bytes)");
  if (grid_ws_bytes < nesti_patches_workspace_bytes(N)) NESTI_FAIL(w + ": grid workspace too small");
  const nesti_config_t* cfg = &m->graph.cfg;
  for (int s = 0; s < cfg->n_scales; ++s)
    if (!(r_abs[s] > 0.0)) NESTI_FAIL(w + ": radii must be positive");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  float* points = (float*)ws;
  int32_t* n_eff = (int32_t*)(ws + est_points_bytes(m, batch));
  unsigned char* fwd_ws = ws + est_points_bytes(m, batch) + est_neff_bytes(m, batch);
  const WsLayout L = ws_layout(m, batch);
  if (build_grid && nesti_patches_grid(cfg, cloud_dev, N, r_abs, grid_ws_dev, grid_ws_bytes, stream)) return 1;
  const int E = m->graph.cfg.arch == NESTI_ARCH_SWITCH ? 1 : m->graph.cfg.n_experts;   // columns of probs_out
  const int S = cfg->n_scales;
  const bool fused = cfg->grid_n == 8;
  for (int done = 0; done < M; done += batch) {
    const int take = std::min(batch, M - done);
    const int32_t* qidx = query_idx_dev ? query_idx_dev + done : nullptr;
    const float* qxyz = at ? query_xyz_dev + (size_t)done * 3 : nullptr;
    int32_t* b_out = n_ball_out_dev ? n_ball_out_dev + (size_t)done * S : nullptr;
    float* n_out = normals_out_dev + (size_t)done * 3;
    int32_t* e_out = expert_out_dev ? expert_out_dev + done : nullptr;
    float* p_out = probs_out_dev ? probs_out_dev + (size_t)done * E : nullptr;
    if (fused) {
      const int tok = prof_begin(NESTI_PROF_MUPS, st);
      const int rcf = launch_patches_mups(cfg, cloud_dev, N, qidx, qxyz, take, r_abs, seed, query_row0 + done, grid_ws_dev,
                                          fwd_ws + L.x0, m->dtype, mups_stride(m), n_eff, b_out, st);
      prof_end(NESTI_PROF_MUPS, tok, st);
      if (rcf) return 1;
      if (forward_tail(m, fwd_ws + L.x0, take, batch, fwd_ws, L, n_out, e_out, p_out, st)) return 1;
    } else {
      if (at ? nesti_patches_query_at(cfg, cloud_dev, N, qxyz, take, r_abs, seed, query_row0 + done, points, n_eff, nullptr, b_out,
                                      grid_ws_dev, grid_ws_bytes, stream)
             : nesti_patches_query(cfg, cloud_dev, N, qidx, take, r_abs, seed, query_row0 + done, points, n_eff, nullptr, nullptr,
                                   grid_ws_dev, grid_ws_bytes, stream))
        return 1;
      if (nesti_forward(m, points, n_eff, take, fwd_ws, L.total, n_out, e_out, p_out, stream)) return 1;
    }
    if (at && launch_mask_empty_queries(n_eff, take, S, n_out, e_out, p_out, E, st)) return 1;
  }
  return 0;
}

int nesti_estimate_normals(const nesti_model_t* m, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                           const double* r_abs, uint64_t seed, int query_row0, int batch, int build_grid,
                           void* grid_ws_dev, size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes,
                           float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, void* stream) {
  return estimate_impl("nesti_estimate_normals", false, m, cloud_dev, N, query_idx_dev, nullptr, M, r_abs, seed, query_row0, batch,
                       build_grid, grid_ws_dev, grid_ws_bytes, ws_dev, ws_bytes, normals_out_dev, expert_out_dev, probs_out_dev,
                       nullptr, stream);
}

int nesti_estimate_normals_at(const nesti_model_t* m, const float* cloud_dev, int N, const float* query_xyz_dev, int M,
                              const double* r_abs, uint64_t seed, int query_row0, int batch, int build_grid,
                              void* grid_ws_dev, size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes,
                              float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, int32_t* n_ball_out_dev,
                              void* stream) {
  return estimate_impl("nesti_estimate_normals_at", true, m, cloud_dev, N, nullptr, query_xyz_dev, M, r_abs, seed, query_row0, batch,
                       build_grid, grid_ws_dev, grid_ws_bytes, ws_dev, ws_bytes, normals_out_dev, expert_out_dev, probs_out_dev,
                       n_ball_out_dev, stream);
}

int nesti_mask_empty_queries(const int32_t* n_eff_dev, int M, int S, float* normals_dev, int32_t* expert_dev, float* probs_dev, int E,
                             void* stream) {
  if (M <= 0) return 0;   // no rows: nothing to do
  if (!n_eff_dev || !normals_dev) NESTI_FAIL("nesti_mask_empty_queries: null argument");
  if (S < 1 || S > NESTI_MAX_SCALES) NESTI_FAIL("nesti_mask_empty_queries: bad n_scales");
  if (probs_dev && E < 1) NESTI_FAIL("nesti_mask_empty_queries: probs_dev needs E >= 1 columns");
  return launch_mask_empty_queries(n_eff_dev, M, S, normals_dev, expert_dev, probs_dev, E, (hipStream_t)stream);
}

// one item of nesti_estimate_normals_multi / _multi_at
struct EstItem {
  const float* cloud_dev;
  int n_points;
  const int32_t* query_idx_dev;
  const float* query_xyz_dev;
  int n_queries;
  const double* r_abs;
  uint64_t seed;
  int query_row0;
  const void* grid_ws_dev;
  size_t grid_ws_bytes;
};

static int estimate_multi_impl(const char* who, bool at, const nesti_model_t* m, const std::vector<EstItem>& items, int batch,
                               void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev,
                               void* stream) {
  const std::string w(who);
  const int n_items = (int)items.size();
  if (!m || !ws_dev || !normals_out_dev) NESTI_FAIL(w + ": null argument");
  if (batch <= 0) NESTI_FAIL(w + ": batch must be positive");
  const nesti_config_t* cfg = &m->graph.cfg;
  if (cfg->grid_n != 8) NESTI_FAIL(w + ": the 8^3 Gaussian grid only (use nesti_estimate_normals per shape)");
  if (nesti_estimate_workspace_bytes(m, batch) > ws_bytes)
    NESTI_FAIL(w + ": workspace too small (see nesti_estimate_workspace_bytes)");
  long long total = 0;
  for (int i = 0; i < n_items; ++i) {
    const EstItem& it = items[i];
    if (it.n_queries < 0 || (it.n_queries > 0 && (!it.cloud_dev || !it.grid_ws_dev || it.n_points <= 0)))
      NESTI_FAIL(w + ": bad item");
    if (at && it.n_queries > 0 && !it.query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev in an item");
    if (at && it.query_row0 < 0) NESTI_FAIL(w + ": query_row0 of an item must be >= 0");
    if (!at && (it.query_row0 < 0 || (!it.query_idx_dev && (long long)it.query_row0 + it.n_queries > (long long)it.n_points)))
      NESTI_FAIL(w + ": query rows of an item exceed its cloud");
    if (it.n_queries > 0 && it.grid_ws_bytes < nesti_patches_workspace_bytes(it.n_points))
      NESTI_FAIL(w + ": grid workspace of an item too small");
    for (int s = 0; s < cfg->n_scales; ++s)
      if (it.n_queries > 0 && !(it.r_abs[s] > 0.0)) NESTI_FAIL(w + ": radii must be positive");
    total += it.n_queries;
  }
  if (total == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int32_t* n_eff = (int32_t*)((unsigned char*)ws_dev + est_points_bytes(m, batch));   // [batch, S]: position queries only
  unsigned char* fwd_ws = (unsigned char*)ws_dev + est_points_bytes(m, batch) + est_neff_bytes(m, batch);
  const WsLayout L = ws_layout(m, batch);
  unsigned char* X0 = fwd_ws + L.x0;
  const size_t row_bytes = (size_t)nesti_model_mups_rows(m) * mups_stride(m) * dtype_size(m->dtype);   // one query's MuPS
  const int E = m->graph.cfg.arch == NESTI_ARCH_SWITCH ? 1 : m->graph.cfg.n_experts;
  const int S = cfg->n_scales;
  long long done = 0;           // rows emitted so far
  int item = 0, item_done = 0;  // cursor into the items
  while (done < total) {
    int fill = 0;
    const int tok = prof_begin(NESTI_PROF_MUPS, st);
    while (fill < batch && item < n_items) {
      const EstItem& it = items[item];
      const int take = std::min(batch - fill, it.n_queries - item_done);
      if (take > 0 &&
          launch_patches_mups(cfg, it.cloud_dev, it.n_points, it.query_idx_dev ? it.query_idx_dev + item_done : nullptr,
                              at ? it.query_xyz_dev + (size_t)item_done * 3 : nullptr, take, it.r_abs, it.seed,
                              it.query_row0 + item_done, it.grid_ws_dev, X0 + (size_t)fill * row_bytes, m->dtype, mups_stride(m),
                              at ? n_eff + (size_t)fill * S : nullptr, nullptr, st)) {
        prof_end(NESTI_PROF_MUPS, tok, st);      // close the timing span on the error path too
        return 1;
      }
      fill += take;
      item_done += take;
      if (item_done >= it.n_queries) { ++item; item_done = 0; }
    }
    prof_end(NESTI_PROF_MUPS, tok, st);
    float* n_out = normals_out_dev + (size_t)done * 3;
    int32_t* e_out = expert_out_dev ? expert_out_dev + done : nullptr;
    float* p_out = probs_out_dev ? probs_out_dev + (size_t)done * E : nullptr;
    if (forward_tail(m, X0, fill, batch, fwd_ws, L, n_out, e_out, p_out, st)) return 1;
    if (at && launch_mask_empty_queries(n_eff, fill, S, n_out, e_out, p_out, E, st)) return 1;
    done += fill;
  }
  return 0;
}

int nesti_estimate_normals_multi(const nesti_model_t* m, const nesti_shape_queries_t* items, int n_items, int batch,
                                 void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev,
                                 float* probs_out_dev, void* stream) {
  {
    long long any = 0;
    for (int i = 0; items && i < n_items; ++i) any += items[i].n_queries > 0 ? items[i].n_queries : 0;
    if (any == 0) return 0;   // no queries: nothing to do
  }
  if (!items) NESTI_FAIL("nesti_estimate_normals_multi: null argument");
  std::vector<EstItem> v;
  for (int i = 0; i < n_items; ++i)
    v.push_back({items[i].cloud_dev, items[i].n_points, items[i].query_idx_dev, nullptr, items[i].n_queries, items[i].r_abs,
                 items[i].seed, items[i].query_row0, items[i].grid_ws_dev, items[i].grid_ws_bytes});
  return estimate_multi_impl("nesti_estimate_normals_multi", false, m, v, batch, ws_dev, ws_bytes, normals_out_dev, expert_out_dev,
                             probs_out_dev, stream);
}

int nesti_estimate_normals_multi_at(const nesti_model_t* m, const nesti_shape_positions_t* items, int n_items, int batch,
                                    void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev,
                                    float* probs_out_dev, void* stream) {
  {
    long long any = 0;
    for (int i = 0; items && i < n_items; ++i) any += items[i].n_queries > 0 ? items[i].n_queries : 0;
    if (any == 0) return 0;   // no queries: nothing to do
  }
  if (!items) NESTI_FAIL("nesti_estimate_normals_multi_at: null argument");
  std::vector<EstItem> v;
  for (int i = 0; i < n_items; ++i)
    v.push_back({items[i].cloud_dev, items[i].n_points, nullptr, items[i].query_xyz_dev, items[i].n_queries, items[i].r_abs,
                 items[i].seed, items[i].query_row0, items[i].grid_ws_dev, items[i].grid_ws_bytes});
  return estimate_multi_impl("nesti_estimate_normals_multi_at", true, m, v, batch, ws_dev, ws_bytes, normals_out_dev, expert_out_dev,
                             probs_out_dev, stream);
}

int nesti_profile_enable(int on) {
  prof_collect();
  for (int c = 0; c < kProfSlots; ++c) { g_prof.ms[c] = 0; g_prof.launches[c] = 0; }
  g_prof.on = on != 0;
  g_prof.phase = NESTI_PHASE_INPUT;
  return 0;
}

int nesti_profile_read(double* ms, long long* launches) {
  prof_collect();   // synchronises on the recorded events
  for (int c = 0; c < kProfSlots; ++c) {
    if (ms) ms[c] = g_prof.ms[c];
    if (launches) launches[c] = g_prof.launches[c];
  }
  return 0;
}

int nesti_model_macs(const nesti_model_t* m, int tower, int kind, double* nominal, double* useful, double* issued) {
  if (!m) NESTI_FAIL("nesti_model_macs: null model");
  if (kind < -1 || kind > NESTI_PROF_ONE_BY_ONE) NESTI_FAIL("nesti_model_macs: kind must be -1 or a conv category");
  const int E = m->graph.cfg.n_experts;
  if (tower < -1 || tower >= E) NESTI_FAIL("nesti_model_macs: tower must be -1 (gate) or an expert index");
  const Tower& T = tower < 0 ? m->graph.gate : m->graph.experts[tower];
  double nom = 0, use = 0, iss = 0;
  for (const Op& op : T.ops) {
    if (op.kind != Op::CONV) continue;
    const LayerDesc& d = m->graph.layers[op.layer];
    const PackedLayer& pl = m->main_packing(op.layer);
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
  return 0;
}

// ---- test hooks: one tower, launch by launch (include/nesti_hip.h) ----------------------------------------------------------
static const nesti_debug_pass_t kMainPass = {0, 0, 0};

int nesti_debug_pack_layer(const nesti_config_t* cfg, const nesti_tensor_t* tensors, int n_tensors, int dtype, int form, int layer,
                           nesti_debug_pack_t* info, void* w, size_t max_w, float* bias, size_t max_bias) {
  if (!cfg || !tensors || !info) NESTI_FAIL("nesti_debug_pack_layer: null argument");
  if (dtype < NESTI_F32 || dtype > NESTI_F16X8C) NESTI_FAIL("nesti_debug_pack_layer: bad dtype");
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 1;
  if (layer < 0 || layer >= (int)g.layers.size()) NESTI_FAIL("nesti_debug_pack_layer: layer index outside the model");
  const LayerDesc& d = g.layers[layer];
  const int mdt = main_dtype(dtype), packing = form_packing(form);
  const bool x8 = packing == NESTI_DEBUG_FORM_X8 || packing == NESTI_DEBUG_FORM_X6;
  if (packing != NESTI_DEBUG_FORM_PLAIN && packing != NESTI_DEBUG_FORM_PAIR && !x8) NESTI_FAIL("nesti_debug_pack_layer: form is NESTI_DEBUG_FORM_*");
  if (packing == NESTI_DEBUG_FORM_PAIR && act_planes(mdt) == 1)
    NESTI_FAIL("nesti_debug_pack_layer: the pair packing is for the pair dtypes (NESTI_BF16X3, NESTI_F16X3 and the modes built on it)");
  if (x8 && !(g.x8 && use_conv8(d)))
    NESTI_FAIL("nesti_debug_pack_layer: the X8 / X6 packings are for the k^3 tap layers at 8^3 of NESTI_F16X8 / NESTI_F16X8C models; " + d.scope +
               " is not one");
  TensorTable tt;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name) tt.by_name[tensors[i].name] = &tensors[i];
  PackedImage img;
  if (pack_form(d, tt, packing, mdt, &img)) return 1;
  memset(info, 0, sizeof(*info));
  info->kind = img.kind; info->TN = img.TN; info->n_tiles = img.n_tiles; info->split_tile = img.split_tile;
  info->n_chunks = img.n_chunks; info->n_taps = img.n_taps; info->x3n = img.x3n ? 1 : 0; info->acc_scale = img.acc_scale;
  info->x8_sb = img.x8_sb; info->x8_sc = x8_activation_exponent(d, tt);
  info->w_bytes = (int64_t)img.w.size(); info->n_bias = (int64_t)img.bias.size();
  memcpy(info->tap, img.tap, sizeof(info->tap));
  if ((w && max_w < img.w.size()) || (bias && max_bias < img.bias.size())) NESTI_FAIL("nesti_debug_pack_layer: output arrays too small");
  if (w) memcpy(w, img.w.data(), img.w.size());
  if (bias) memcpy(bias, img.bias.data(), img.bias.size() * sizeof(float));
  return 0;
}

// the pass arguments of the two hooks against the graph (cascade: a model with the two-stage gate); `who` prefixes the message
static int check_pass(const std::string& who, const Graph& g, bool cascade, int tower, const nesti_debug_pass_t& ps) {
  if (tower < -1 || tower >= (int)g.experts.size()) NESTI_FAIL(who + ": tower must be -1 (gate) or an expert index");
  if (tower < 0 && g.cfg.arch != NESTI_ARCH_EXPERTS && g.cfg.arch != NESTI_ARCH_SWITCH) NESTI_FAIL(who + ": this model has no gating net");
  if (ps.fast && !(cascade && tower < 0)) NESTI_FAIL(who + ": the filter pass is the gating net's of NESTI_F16X3C / NESTI_F16X8C models");
  if (ps.x8_mask < 0 || ps.x8_mask > 0xF || (ps.x8_mask && !(g.x8 && tower >= 0)))
    NESTI_FAIL(who + ": x8_mask has four bits and applies to the expert towers of NESTI_F16X8 / NESTI_F16X8C models");
  if (ps.x8_fmt != 0 && ps.x8_fmt != 6 && ps.x8_fmt != 8) NESTI_FAIL(who + ": x8_fmt is 0 (= 6), 6 or 8");
  return 0;
}

int nesti_debug_tower_ops(const nesti_config_t* cfg, int dtype, int tower, int batch, const nesti_debug_pass_t* pass,
                          nesti_debug_buf_t* bufs, int max_bufs, int* n_bufs, nesti_debug_op_t* ops, int max_ops, int* n_ops,
                          int32_t* in_pos, int max_in_pos, int* n_in_pos, size_t* ws_bytes) {
  if (!cfg || !n_bufs || !n_ops) NESTI_FAIL("nesti_debug_tower_ops: null argument");
  if (batch <= 0) NESTI_FAIL("nesti_debug_tower_ops: batch must be positive");
  const nesti_debug_pass_t& ps = pass ? *pass : kMainPass;
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 1;
  if (check_pass("nesti_debug_tower_ops", g, dtype_cascade(dtype), tower, ps)) return 1;
  const Tower& T = tower < 0 ? g.gate : g.experts[tower];
  Pass run;
  run.tower = tower; run.fast = ps.fast != 0; run.x8_mask = ps.x8_mask; run.x8_fmt = ps.x8_fmt == 8 ? 8 : 6;
  const int mdt = main_dtype(dtype), dt = ps.fast ? NESTI_F16 : mdt;   // as run_op
  const int planes = act_planes(dt);
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
    o.planes = b.aux8 || b.f32 ? 1 : act_planes(i == 0 ? mdt : dt);
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
    nesti_debug_op_t& o = ops[k];
    memset(&o, 0, sizeof(o));
    o.kind = op.kind == Op::CONV ? NESTI_DEBUG_OP_CONV : op.kind == Op::MAX ? NESTI_DEBUG_OP_MAX : NESTI_DEBUG_OP_MAX3;
    o.family = -1; o.layer = -1; o.in_pos_off = -1;
    o.elem = kernel_dtype(dt); o.planes = planes;
    o.in_buf = op.in_buf; o.in_coff = op.in_coff; o.in_cstride = op.in_cstride ? op.in_cstride : T.bufs[op.in_buf].C;
    o.in_planes = op.in_buf < 1 ? act_planes(mdt) : planes;
    o.out_buf = op.out_buf; o.out_coff = op.out_coff; o.out_coff2 = op.out_coff2; o.out_f32 = op.out_f32;
    o.mp_buf = op.mp_buf; o.mp_mode = op.mp_mode; o.mp_mode2 = op.mp_mode2;
    o.aux_in_buf = o.aux_out_buf = o.aux_layer = -1;
    o.form = planes > 1 ? NESTI_DEBUG_FORM_PAIR : NESTI_DEBUG_FORM_PLAIN;
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
    const LaunchForm f = launch_form(g, op, run, mdt);
    o.family = f.family; o.form = f.form;
    if (f.form == NESTI_DEBUG_FORM_X8 || f.form == NESTI_DEBUG_FORM_X6) { o.aux_in_buf = op.aux_in_buf; o.aux_layer = op.aux_layer; }
    if (f.producer) o.aux_out_buf = op.aux_out_buf;
    o.in_pos_off = pos;
    for (int c = 0; c < d.cin; ++c, ++pos) if (in_pos) in_pos[pos] = d.in_pos[c];
  }
  return 0;
}

int nesti_debug_tower_step(const nesti_model_t* m, int tower, const nesti_debug_pass_t* pass, int op, const void* mups_dev, int batch,
                           const int32_t* point_index_dev, const int32_t* npoints_dev, int walk, void* ws_dev, size_t ws_bytes,
                           void* stream) {
  if (!m || !mups_dev || !ws_dev) NESTI_FAIL("nesti_debug_tower_step: null argument");
  if (batch <= 0) NESTI_FAIL("nesti_debug_tower_step: batch must be positive");
  const nesti_debug_pass_t& ps = pass ? *pass : kMainPass;
  const Graph& g = m->graph;
  if (check_pass("nesti_debug_tower_step", g, m->cascade, tower, ps)) return 1;
  if (ps.x8_fmt != 0 && ps.x8_fmt != m->x8_fmt) NESTI_FAIL("nesti_debug_tower_step: x8_fmt differs from the model's (nesti_model_set_x8_format)");
  if (walk < 0 || (walk > 1 && walk % 8)) NESTI_FAIL("nesti_debug_tower_step: walk is 0, 1 or a multiple of 8");
  const Tower& T = tower < 0 ? g.gate : g.experts[tower];
  if (op < 0 || op >= (int)T.ops.size()) NESTI_FAIL("nesti_debug_tower_step: op index outside the tower");
  const RunCtx rc = pass_ctx(m, tower, ps.fast != 0, ps.x8_mask, batch, npoints_dev, point_index_dev, (hipStream_t)stream, walk);
  std::vector<unsigned char*> ptr;
  if (tower_ptrs(rc, T, mups_dev, (unsigned char*)ws_dev, ws_bytes, &ptr)) return 1;
  return run_op(rc, T, T.ops[op], ptr);
}

}  // extern "C"

