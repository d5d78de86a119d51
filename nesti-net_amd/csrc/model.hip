// The model on the device and its forward paths: the model object with its packed layers and counter blocks, the tower runner, the
// gate (one pass or the two-stage cascade), the routed experts with their conditioning guard, and the C-ABI entries that create,
// configure, read and run a model.  What a launch is and where its buffers live is decided by the planner (plan.cpp); here a launch
// gets its device addresses and goes out.  The deciding kernels (decide.hip), the kernel profiler (prof.hip), the graph (graph.cpp),
// batch-norm folding and weight repacking (pack.cpp) and the planner are units of their own.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "decide.h"
#include "kernels.h"
#include "plan.h"

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

// A 64-byte block of device counters (include/nesti_hip.h: nesti_cascade_stats_t, nesti_x8_guard_stats_t,
// nesti_reproducible_stats_t): owned here, handed to the kernels as the raw pointer `dev`
struct StatBlock {
  unsigned long long* dev = nullptr;
  StatBlock() = default;
  StatBlock(const StatBlock&) = delete;
  StatBlock& operator=(const StatBlock&) = delete;
  ~StatBlock() { if (dev) (void)hipFree(dev); }
  explicit operator bool() const { return dev != nullptr; }
  int alloc() { NESTI_CHECK_HIP(hipMalloc((void**)&dev, 64)); return reset(); }
  int reset() const { NESTI_CHECK_HIP(hipMemset(dev, 0, 64)); return 0; }
  // the eight words into h (zeros when the model has no such block), zeroed on the device afterwards if `then_reset`
  int read(unsigned long long (&h)[8], int then_reset) const {
    memset(h, 0, sizeof(h));
    if (dev) NESTI_CHECK_HIP(hipMemcpy(h, dev, sizeof(h), hipMemcpyDeviceToHost));
    return dev && then_reset ? reset() : 0;
  }
};

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
  nesti::Mode mode() const { return {graph, dtype, cascade}; }   // what the planner's sizing functions read (plan.h)
  // EXPERIMENT: models created after nesti_experiment_mix_enable(1) also hold kFormMix packings of their tap layers; expert_mix /
  // gate_mix switch them on
  bool has_mix = false;
  int expert_mix = 0;
  // NESTI_F16X8 / NESTI_F16X8C: x8_mask picks which of the experts' tap layers at 8^3 run their cross terms in FP8 / FP6
  // (include/nesti_hip.h: nesti_model_set_x8_layers), x8_fmt which of the two forms forward calls use (8 or 6; nesti_model_set_x8_format)
  int x8_mask = 0;
  int x8_fmt = 6;
  // ... and their conditioning guard (decide.hip: x8_guard_*): outputs with |n| below max(x8_guard_thr, NESTI_X8_GUARD_WIDEN x largest
  // measured |dn| / theta) are re-evaluated in f16x3 proper; gstat = the device counters (include/nesti_hip.h: nesti_x8_guard_stats_t)
  float x8_guard_thr = NESTI_X8_GUARD_DEFAULT;
  int x8_guard_walk = NESTI_GUARD_WALK_GRID;   // workgroups of the guard towers' walking launches (host.h: ConvParams::walk)
  nesti::StatBlock gstat;
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
  nesti::StatBlock cstat;
  // NESTI_F16X8C: recheck stage 2 (gate_cascade) -- the flagged rows first go through the gating net with its 8^3 tap layers in the FP6
  // form (graph.h: Graph::gate2); only those whose stage-2 margin is below tau2_eff reach the f16x3 gate.  cstat2 = its counters
  // (host.h: C2Stat).  On while the model's cross-term format is 6, nesti_model_set_gate_stage2 has not switched it off and a second
  // margin has been SET (nesti_model_set_gate_margin2; the calibration does): the stage's error is two orders below the filter's, and
  // no constant is a safe margin for weights nobody has measured -- until then every flagged row is the f16x3 gate's, as without the stage
  float tau2 = 0.f;
  bool tau2_set = false;
  bool stage2 = true;
  nesti::StatBlock cstat2;
  bool stage2_on() const { return cascade && cstat2 && stage2 && tau2_set && x8_fmt == 6; }
  // nesti_model_set_reproducible: rstat = the mode's own 64-byte counter block (host.h: RStat), allocated
  // with cstat / gstat; forward calls hand it to the kernels only while the mode is on (frozen() below), and then no decision of
  // theirs reads cstat / gstat
  bool reproducible = false;
  nesti::StatBlock rstat;
  unsigned long long* frozen() const { return reproducible ? rstat.dev : nullptr; }
  ~nesti_model() {
    for (auto& p : packed) {
      if (p.second.wpk) (void)hipFree(p.second.wpk);
      if (p.second.bias) (void)hipFree(p.second.bias);
    }
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
// tower execution
// ------------------------------------------------------------------------------------------
struct RunCtx {
  const nesti_model* m;
  Pass pass;
  int NB;                        // capacity (points)
  const int32_t* npoints_ptr;    // device-side live count or NULL
  const int32_t* point_index;    // gather for reads of bufs 0/1, or NULL
  hipStream_t stream;
  int walk;                      // this pass over a device-side list is probably empty (a later round, a widening pass): its conv
                                 // launches use small walking grids (host.h: ConvParams::walk)
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
  ptr->assign(T.bufs.size(), nullptr);
  (*ptr)[0] = (unsigned char*)X0;
  const Placement P = place_tower(T, rc.NB, pass_dtype(rc.pass.fast, rc.m->dtype));
  for (size_t i = 1; i < T.bufs.size(); ++i) (*ptr)[i] = ws + P.off[i];
  if (P.total > ws_bytes) NESTI_FAIL("workspace too small for this batch");
  return 0;
}

// One launch of a tower: the body of run_tower's loop, also reached alone through nesti_debug_tower_step.  What the launch is comes
// from the planner (plan.cpp: plan_op, the derivation nesti_debug_tower_ops reports); here it gets its addresses, its timing span
// and its kernel
int run_op(const RunCtx& rc, const Tower& T, const Op& op, const std::vector<unsigned char*>& ptr) {
  const nesti_model* m = rc.m;
  const OpPlan plan = plan_op(m->graph, T, op, rc.pass, m->dtype);
  if (op.kind != Op::CONV) {
    PoolParams p = pool_params(T, op, plan, rc.NB);
    p.in = ptr[op.in_buf]; p.out = ptr[op.out_buf]; p.npoints_ptr = rc.npoints_ptr;
    const int tok = prof_begin(NESTI_PROF_POOL, rc.stream);
    const int rcp = op.kind == Op::MAX3 ? launch_maxpool3s2(p, plan.elem, rc.stream) : launch_maxpool2(p, plan.elem, rc.stream);
    prof_end(NESTI_PROF_POOL, tok, rc.stream);
    return rcp ? 1 : 0;
  }
  const LayerDesc& d = m->graph.layers[op.layer];
  const PackedLayer* pk = m->packing(plan.form.form, op.layer);
  if (!pk || pk->kind != plan.form.family)
    NESTI_FAIL("internal: layer " + d.scope + " is not packed for form " + std::to_string(plan.form.form) + " of this pass");
  ConvParams p = conv_params(m->graph, T, op, rc.pass, plan, *pk, plan.x8_sc_layer >= 0 ? m->main_packing(plan.x8_sc_layer).x8_sc : 0, rc.NB);
  p.in = ptr[op.in_buf]; p.out = ptr[op.out_buf]; p.wpk = pk->wpk; p.bias = pk->bias;
  p.npoints_ptr = rc.npoints_ptr; p.point_index = op.in_buf < 1 ? rc.point_index : nullptr;
  if (op.mp_buf >= 0) p.mp_out = ptr[op.mp_buf];
  if (p.x8) p.aux8_in = ptr[op.aux_in_buf];
  if (plan.form.producer) p.aux8_out = ptr[op.aux_out_buf];
  p.walk = rc.walk;
  const int cat = conv_category(d, *pk);
  const int tok = prof_begin(cat, rc.stream);
  const int rcv = pk->kind == 2   ? launch_conv8n(p, plan.elem, d.k, rc.stream)
                  : pk->kind == 3 ? launch_conv4n(p, plan.elem, d.k, rc.stream)
                                  : launch_conv(p, plan.elem, pk->TN, rc.stream);
  prof_end(cat, tok, rc.stream);
  return rcv ? 1 : 0;
}

int run_tower(const RunCtx& rc, const Tower& T, const void* X0, unsigned char* ws, size_t ws_bytes, float** out) {
  std::vector<unsigned char*> ptr;
  if (tower_ptrs(rc, T, X0, ws, ws_bytes, &ptr)) return 1;
  for (const Op& op : T.ops)
    if (run_op(rc, T, op, ptr)) return 1;
  *out = reinterpret_cast<float*>(ptr[T.out_buf]);
  return 0;
}

// The forward arena of one call: the caller's workspace and its layout for the batch capacity NB >= the call's rows (plan.cpp:
// ws_layout).  Travels as one value; whoever needs a part takes it here
struct Arena {
  unsigned char* ws;
  int NB;
  WsLayout L;
  Arena(const nesti_model* m, void* ws_dev, int NB) : ws((unsigned char*)ws_dev), NB(NB), L(ws_layout(m->mode(), NB)) {}
  template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  unsigned char* tower() const { return ws + L.tower; }      // where every tower pass is placed (run_tower), and its size
  size_t tower_size() const { return L.total - L.tower; }
};

// NESTI_F16X3C (include/nesti_hip.h): the gating net in plain f16 over the batch, then in f16x3 over the rows whose f16
// top-2 margin is below tau (gathered through the flag list like a routed expert gathers its rows), `cap` rows per round;
// the routing lists are built from the final arg-max.
int gate_cascade(const nesti_model* m, const void* X0, int B, const Arena& A, float* probs, int32_t* expert, int32_t* counts,
                 int32_t* lists, hipStream_t stream) {
  const int E = m->graph.cfg.n_experts;
  if (!expert) expert = A.at<int32_t>(A.L.expert);   // the recheck needs the arg-max whether or not the caller wants it
  float* keep = A.at<float>(A.L.keep);
  int32_t* flag_list = A.at<int32_t>(A.L.flags);
  int32_t* fcounts = A.at<int32_t>(A.L.fcounts);         // host.h: kRoundCountsOff, kTauEffOff, kWidenCountOff, kWidenRoundsOff
  const int lstride = m->graph.gate.bufs[m->graph.gate.out_buf].C;
  float* logits = nullptr;
  const RunCtx fast = pass_ctx(m, -1, /*fast=*/true, 0, B, nullptr, nullptr, stream, 0);
  prof_phase(NESTI_PHASE_GATE);
  if (run_tower(fast, m->graph.gate, X0, A.tower(), A.tower_size(), &logits)) return 1;
  prof_phase(NESTI_PHASE_RECHECK);
  const int cap = std::min(cascade_cap(A.NB), B), rounds = (B + cap - 1) / cap;
  unsigned long long* rstat = m->frozen();   // reproducible mode: the threshold is tau itself and pass 0 is the only pass
  if (launch_gate_flag(logits, lstride, B, E, m->tau, NESTI_GATE_WIDEN, probs, expert, keep, fcounts, flag_list, cap, rounds,
                       m->cstat.dev, rstat, stream))
    return 1;
  // pass 0: the rows below the call's threshold; passes 1 .. NESTI_GATE_WIDEN_PASSES: widening passes -- the band between the
  // threshold reached so far and NESTI_GATE_WIDEN x the largest error measured up to the start of the pass, so an error first
  // seen inside a widening pass is covered by the next one of the SAME call (normally every pass is empty: its launches find a
  // zero row count on the device and return; no host synchronisation, so the whole call stays graph-capturable)
  // recheck stage 2 (NESTI_F16X8C, format 6): in pass 0 a round's rows go through the gating net in its FP6 form first; the rows whose
  // stage-2 margin stays below tau2_eff -- the round's residual list, a fraction of a per cent of a batch -- then go through the f16x3
  // gate as walking launches.  The widening passes of the filter's margin (normally empty) keep the two-pass form
  // The stage's buffers sit inside the tower arena (plan.h: Stage2Plan), in rounds of S2.cap rows of the flag list
  const Stage2Plan S2 = m->stage2_on() ? stage2_plan(m->mode(), A.NB) : Stage2Plan();
  const bool s2 = S2.cap > 0;
  const int cap2 = std::min(S2.cap, B), rounds2 = s2 ? (B + cap2 - 1) / cap2 : 0;
  int32_t* residual = reinterpret_cast<int32_t*>(A.tower() + S2.residual);
  float* logits2 = reinterpret_cast<float*>(A.tower() + S2.logits2);
  float* margin2 = reinterpret_cast<float*>(A.tower() + S2.margin2);
  // stage 3 over the current residual list: the f16x3 gate on fcounts[kResCountOff] rows
  auto stage3 = [&](const float* l2) {
    const RunCtx exact = pass_ctx(m, -1, false, 0, S2.cap, fcounts + kResCountOff, residual, stream, NESTI_GATE_WIDEN_WALK_GRID);
    if (run_tower(exact, m->graph.gate, X0, A.tower(), S2.tower_bytes, &logits)) return 1;
    return launch_gate3_recheck(logits, lstride, residual, S2.cap, E, keep, l2, probs, expert, m->cstat.dev, m->cstat2.dev, fcounts,
                                NESTI_GATE_WIDEN, rstat, stream);
  };
  if (s2 && (launch_gate2_begin(fcounts, m->cstat2.dev, m->tau2, NESTI_GATE_WIDEN, rstat, stream) ||
             launch_round_counts(fcounts, 1, cap2, rounds2, fcounts + kRound2Off, stream)))
    return 1;
  for (int pass = 0; pass <= (rstat ? 0 : NESTI_GATE_WIDEN_PASSES); ++pass) {
    if (pass >= 1 && launch_gate_widen(keep, B, E, NESTI_GATE_WIDEN, fcounts, flag_list, cap, rounds, m->cstat.dev, stream)) return 1;
    const int32_t* round_counts = fcounts + (pass == 0 ? kRoundCountsOff : kWidenRoundsOff);
    for (int r = 0; s2 && pass == 0 && r < rounds2; ++r) {
      const int32_t* list = flag_list + (size_t)r * cap2;
      const int32_t* count = fcounts + kRound2Off + r;
      const RunCtx fp6 = pass_ctx(m, -1, false, 0x3F, S2.cap, count, list, stream, r >= 1 ? 1 : 0);
      if (run_tower(fp6, m->graph.gate2, X0, A.tower(), S2.tower_bytes, &logits)) return 1;
      if (launch_gate2_decide(logits, lstride, list, count, cap2, E, keep, probs, expert, m->cstat.dev, m->cstat2.dev, fcounts,
                              NESTI_GATE_WIDEN, rstat, residual, logits2, margin2 + (size_t)r * cap2, stream))
        return 1;
      if (stage3(logits2)) return 1;
    }
    if (s2 && pass == 0) {
      // the stage's widening round: what this call has measured since its tau2_eff was taken (normally nothing: an empty list)
      if (!rstat && (launch_gate2_widen(B, fcounts, flag_list, margin2, residual, S2.cap, m->cstat2.dev, NESTI_GATE_WIDEN, stream) || stage3(nullptr)))
        return 1;
      continue;
    }
    for (int r = 0; r < rounds; ++r) {
      // round 0 of pass 0 holds the flagged rows; everything after it is normally empty
      const RunCtx exact = pass_ctx(m, -1, false, 0, cap, round_counts + r, flag_list + (size_t)r * cap, stream,
                                    pass >= 1 ? NESTI_GATE_WIDEN_WALK_GRID : r >= 1 ? 1 : 0);
      if (run_tower(exact, m->graph.gate, X0, A.tower(), A.tower_size(), &logits)) return 1;
      if (launch_gate_recheck(logits, lstride, flag_list + (size_t)r * cap, round_counts + r, cap, E, keep, probs, expert,
                              m->cstat.dev, fcounts, NESTI_GATE_WIDEN, rstat, stream))
        return 1;
    }
  }
  if (counts) return launch_route(expert, B, E, counts, lists, stream);
  return 0;
}

// The gating net over B rows: the two-stage gate of a NESTI_F16X3C / NESTI_F16X8C model, else one pass and the softmax / switch
int gate_impl(const nesti_model* m, const void* X0, int B, const Arena& A, float* probs, int32_t* expert, int32_t* counts,
              int32_t* lists, hipStream_t stream) {
  if (m->cascade) return gate_cascade(m, X0, B, A, probs, expert, counts, lists, stream);
  const RunCtx rc = pass_ctx(m, -1, false, 0, B, nullptr, nullptr, stream, 0);
  float* logits = nullptr;
  prof_phase(NESTI_PHASE_GATE);
  if (run_tower(rc, m->graph.gate, X0, A.tower(), A.tower_size(), &logits)) return 1;
  const int lstride = m->graph.gate.bufs[m->graph.gate.out_buf].C;
  if (m->graph.cfg.arch == NESTI_ARCH_SWITCH)   // noise_est < 0.015 -> small, else large (models/ms_sw_n_est.py:80-82)
    return launch_switch_finish(logits, lstride, B, 0.015f, probs, expert, counts, lists, stream);
  return launch_gate_finish(logits, lstride, B, m->graph.cfg.n_experts, probs, expert, counts, lists, stream);
}

// The conditioning guard of the FP8 cross-term layers (decide.hip) over one experts_impl call: once expert e's rows are written, those
// whose |n| falls inside the pass's band go through the SAME tower in f16x3 proper, which replaces them and measures |dn|; a second
// pass covers the band a larger measurement of THIS call may have opened (normally empty).  A guard tower sees a handful of rows, so it
// is latency-bound (~3 ms: one workgroup walks a layer's whole K loop): in the first pass expert e's guard runs on the model's
// auxiliary stream (nesti_model::GuardLane), in its own slice of the tower workspace, while the caller's stream goes on with expert e + 1
struct Guard {
  const nesti_model* m;
  const void* X0;
  const int B;
  const Arena& A;
  const int32_t *counts, *lists;   // the routing
  float* normals;
  hipStream_t stream;              // the caller's
  bool on, side = false;           // side: the first pass runs on the lane's stream, in [main_bytes, ...) of the tower arena
  nesti_model::GuardLane* lane = nullptr;
  std::unique_lock<std::mutex> lock;   // the lane's auxiliary stream and events: one call enqueues on them at a time
  size_t main_bytes = 0;
  int32_t* glist;                  // [E][gcap] row lists
  const int gcap;
  float* gslot = nullptr;          // the |n| band and the [E] list lengths: words of the ecounts block (host.h)
  int32_t* gcount = nullptr;
  const float scale = x8_guard_scale();
  unsigned long long* rstat;       // reproducible mode: the band is [0, thr) and pass 0 is the only pass

  // cap: rows of a routed expert's round (the caller's stream keeps a tower workspace of that many rows)
  Guard(const nesti_model* m, const void* X0, int B, const Arena& A, const int32_t* counts, const int32_t* lists, float* normals, int cap,
        hipStream_t stream)
      : m(m), X0(X0), B(B), A(A), counts(counts), lists(lists), normals(normals), stream(stream),
        glist(m->graph.x8 ? A.at<int32_t>(A.L.glist) : nullptr), gcap(std::min(guard_cap(A.NB), B)), rstat(m->frozen()) {
    on = counts && glist && m->x8_mask && m->gstat && m->x8_guard_thr >= 0.f;
    if (!on) return;
    gslot = A.at<float>(A.L.ecounts) + kGuardSlotOff;
    gcount = A.at<int32_t>(A.L.ecounts) + kGuardCountOff;
    size_t guard_bytes = 0;
    for (const Tower& T : m->graph.experts) {
      main_bytes = std::max(main_bytes, align_up(tower_bytes(T, cap, m->dtype), 256));
      guard_bytes = std::max(guard_bytes, tower_bytes(T, gcap, m->dtype));
    }
    // (a stream that is being captured into a hipGraph keeps everything on itself: the guard then runs on the caller's stream, one
    // tower after the other, like it does when the two workspace slices do not fit)
    lane = m->guard_lane(stream);
    side = lane->gstream && main_bytes + guard_bytes <= A.tower_size() && !stream_capturing(stream);
    if (side) lock = std::unique_lock<std::mutex>(lane->gmu);
  }

  // expert e's rows inside the current band: flag, re-evaluate, replace
  int expert(int e, hipStream_t st, unsigned char* arena, size_t arena_bytes, int walk_grid) {
    const Tower& T = m->graph.experts[e];
    int32_t* gl = glist + (size_t)e * gcap;
    if (launch_x8_guard_flag(lists + (size_t)e * B, counts + e, B, normals, gslot, gl, gcount + e, gcap, m->gstat.dev, st)) return 1;
    float* out = nullptr;
    const RunCtx rc = pass_ctx(m, e, false, /*x8_mask=*/0, gcap, gcount + e, gl, st, walk_grid);   // a small walking grid (a few dozen rows)
    if (run_tower(rc, T, X0, arena, arena_bytes, &out)) return 1;
    return launch_x8_guard_fix(out, T.bufs[T.out_buf].C, gl, gcount + e, gcap, normals, m->gstat.dev, m->x8_guard_thr, scale, rstat, st);
  }

  // before the first expert: the band of the first pass
  int begin() { return on && launch_x8_guard_begin(0, m->x8_guard_thr, scale, B, m->gstat.dev, gslot, rstat, stream); }

  // after expert e's rounds are enqueued on the caller's stream: its first pass
  int after_expert(int e) {
    if (!on) return 0;
    prof_phase(NESTI_PHASE_GUARD);
    if (side) {
      NESTI_CHECK_HIP(hipEventRecord(lane->gev_done[e], stream));
      NESTI_CHECK_HIP(hipStreamWaitEvent(lane->gstream, lane->gev_done[e], 0));
      if (expert(e, lane->gstream, A.tower() + main_bytes, A.tower_size() - main_bytes, m->x8_guard_walk)) return 1;
    } else if (expert(e, stream, A.tower(), A.tower_size(), m->x8_guard_walk)) {
      return 1;
    }
    prof_phase(NESTI_PHASE_EXPERTS);
    return 0;
  }

  // after the last expert: the lane joins the caller's stream, then the widening passes on it
  int finish() {
    if (!on) return 0;
    if (side) {
      NESTI_CHECK_HIP(hipEventRecord(lane->gev_join, lane->gstream));
      NESTI_CHECK_HIP(hipStreamWaitEvent(stream, lane->gev_join, 0));
      lock.unlock();
    }
    prof_phase(NESTI_PHASE_GUARD);
    for (int pass = 1; pass <= (rstat ? 0 : NESTI_X8_GUARD_WIDEN_PASSES); ++pass) {
      if (launch_x8_guard_begin(pass, m->x8_guard_thr, scale, B, m->gstat.dev, gslot, nullptr, stream)) return 1;
      for (int e = 0; e < (int)m->graph.experts.size(); ++e)
        if (expert(e, stream, A.tower(), A.tower_size(), NESTI_GUARD_WIDEN_WALK_GRID)) return 1;
    }
    return 0;
  }
};

// counts / lists = the routing (null: every expert on every point); ecounts = the arena's per-(expert, round) counter block
int experts_impl(const nesti_model* m, const void* X0, int B, const Arena& A, const int32_t* counts, const int32_t* lists, float* normals,
                 hipStream_t stream) {
  int32_t* ecounts = A.at<int32_t>(A.L.ecounts);
  const int E = m->graph.cfg.n_experts;
  const int cap = std::min(expert_cap(A.NB), B), rounds = (B + cap - 1) / cap;
  prof_phase(NESTI_PHASE_EXPERTS);
  if (counts && launch_round_counts(counts, E, cap, rounds, ecounts, stream)) return 1;
  const size_t x0_row = mups_row_bytes(m->mode());
  Guard guard(m, X0, B, A, counts, lists, normals, cap, stream);
  if (guard.begin()) return 1;
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
        if (run_tower(rc, T, X0, A.tower(), A.tower_size(), &out)) return 1;
        if (launch_scatter3(out, ostride, list, cnt, cap, normals, stream)) return 1;
      } else {        // reference behaviour: every expert on every point -> [E,B,3], rows [r * cap, ...) of the batch per round
        const int take = std::min(cap, B - r * cap);
        const RunCtx rc = pass_ctx(m, e, false, m->x8_mask, take, nullptr, nullptr, stream, 0);
        if (run_tower(rc, T, (const unsigned char*)X0 + (size_t)r * cap * x0_row, A.tower(), A.tower_size(), &out)) return 1;
        if (launch_scatter3(out, ostride, nullptr, nullptr, take, normals + ((size_t)e * B + (size_t)r * cap) * 3, stream)) return 1;
      }
    }
    if (guard.after_expert(e)) return 1;
  }
  return guard.finish();
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

int nesti_mups_forward(const nesti_config_t* cfg, const float* points_dev, const int32_t* n_eff_dev, int B,
                       void* out_dev, int out_dtype, int out_cstride, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!cfg || !points_dev || !n_eff_dev || !out_dev) NESTI_FAIL("nesti_mups_forward: null argument");
  const int tok = prof_begin(NESTI_PROF_MUPS, (hipStream_t)stream);
  const int rc = launch_mups(cfg, points_dev, n_eff_dev, B, out_dev, out_dtype, out_cstride, /*embed4=*/0, (hipStream_t)stream);
  prof_end(NESTI_PROF_MUPS, tok, (hipStream_t)stream);
  return rc;
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
  const TensorTable tt = tensor_table(tensors, n_tensors);
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
    if (m->cascade && t < 0 && m->graph.has_gate2()) { passes.push_back(Pass()); passes.back().x8_mask = 0x3F; passes.back().x8_fmt = 6; }
    for (int fmt : {8, 6})
      if (x8 && t >= 0) { passes.push_back(Pass()); passes.back().x8_mask = 0xF; passes.back().x8_fmt = fmt; }
    if (m->has_mix) { passes.push_back(Pass()); passes.back().mix = t < 0 ? 1 << kGateMixBit : 0x3F; }
    for (Pass& ps : passes) {
      ps.tower = t;
      for (const Op& op : m->graph.tower(t, ps.x8_mask).ops) {
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
    if (m->gstat.alloc()) return 1;
    for (auto& gl : m->glane) {
      NESTI_CHECK_HIP(hipStreamCreateWithFlags(&gl.gstream, hipStreamNonBlocking));
      NESTI_CHECK_HIP(hipEventCreateWithFlags(&gl.gev_join, hipEventDisableTiming));
      for (int e = 0; e < cfg->n_experts; ++e) NESTI_CHECK_HIP(hipEventCreateWithFlags(&gl.gev_done[e], hipEventDisableTiming));
    }
  }
  if (m->cascade && m->cstat.alloc()) return 1;
  if (m->cascade && m->graph.has_gate2() && m->cstat2.alloc()) return 1;
  if ((m->cstat || m->gstat) && m->rstat.alloc()) return 1;   // the reproducible mode's own counters (nesti_model_set_reproducible)
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

int nesti_model_set_gate_margin2(nesti_model_t* m, float tau2) {
  if (!m || !m->cstat2) NESTI_FAIL("nesti_model_set_gate_margin2: not a NESTI_F16X8C model");
  if (!(tau2 >= 0.f)) NESTI_FAIL("nesti_model_set_gate_margin2: tau2 must be >= 0");
  m->tau2 = tau2;
  m->tau2_set = true;
  return 0;
}

int nesti_model_set_gate_stage2(nesti_model_t* m, int on) {
  if (!m || !m->cstat2) NESTI_FAIL("nesti_model_set_gate_stage2: not a NESTI_F16X8C model");
  m->stage2 = on != 0;
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
  if (m->gstat.read(h, reset)) return 1;
  out->queries = h[kGQueries]; out->rechecked = h[kGRechecked]; out->dropped = h[kGDropped];
  out->max_dn = counter_float(h[kGMaxDnBits]);
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
  if (m->cstat.read(h, reset)) return 1;
  out->queries = h[kCQueries]; out->rechecked = h[kCRechecked]; out->changed = h[kCChanged];
  out->max_margin_err = counter_float(h[kCMaxErrBits]);
  out->tau = m->tau;
  memcpy(&out->sum_sq_pair_err, &h[kCSumSq], 8);
  out->pairs = h[kCPairs];
  out->widened = h[kCWidened];
  out->widen_events = h[kCWidenEvents];
  out->tau_eff = m->reproducible ? m->tau : gate_tau_eff(m->tau, NESTI_GATE_WIDEN, out->max_margin_err);
  unsigned long long h2[8];
  if (m->cstat2.read(h2, reset)) return 1;
  out->stage2 = m->stage2_on() ? 1 : 0;
  out->stage2_rows = h2[kC2Rows]; out->stage2_decided = h2[kC2Decided]; out->stage2_residual = h2[kC2Residual];
  out->max_margin_err2 = counter_float(h2[kC2MaxErrBits]);
  out->tau2 = m->cstat2 ? m->tau2 : 0.f;
  memcpy(&out->sum_sq_pair_err2, &h2[kC2SumSq], 8);
  out->pairs2 = h2[kC2Pairs];
  out->stage2_widened = h2[kC2Widened]; out->stage2_dropped = h2[kC2Dropped];
  out->tau2_eff = !m->cstat2 ? 0.f : m->reproducible ? m->tau2 : gate_tau_eff(m->tau2, NESTI_GATE_WIDEN, out->max_margin_err2);
  return 0;
}

int nesti_model_set_reproducible(nesti_model_t* m, int on) {
  if (!m) NESTI_FAIL("nesti_model_set_reproducible: null model");
  m->reproducible = on != 0;   // a model with neither two-stage gate nor guard has no rstat: frozen() stays null, nothing changes
  return 0;
}

int nesti_model_reproducible_stats(const nesti_model_t* m, nesti_reproducible_stats_t* out, int reset, void* stream) {
  if (!m || !out) NESTI_FAIL("nesti_model_reproducible_stats: null model / null argument");
  unsigned long long r[8], c[8], g[8];
  NESTI_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long c2[8];
  if (m->rstat.read(r, reset) || m->cstat.read(c, reset) || m->gstat.read(g, reset) || m->cstat2.read(c2, reset)) return 1;
  memset(out, 0, sizeof(*out));
  out->on = m->reproducible ? 1 : 0;
  out->gate_violations = r[kRGateViolations]; out->guard_violations = r[kRGuardViolations]; out->guard_dropped = g[kGDropped];
  out->max_margin_err = counter_float(c[kCMaxErrBits]);
  out->max_dn = counter_float(g[kGMaxDnBits]);
  out->tau = m->cascade ? m->tau : 0.f;
  out->thr = m->gstat ? m->x8_guard_thr : -1.f;
  return 0;
}

int nesti_model_gate_error_export(const nesti_model_t* m, float* dst_dev, void* stream) {
  if (!m || !m->cascade || !dst_dev) NESTI_FAIL("nesti_model_gate_error_export: not a NESTI_F16X3C model / null argument");
  return launch_stat_max_export(m->cstat.dev + kCMaxErrBits, dst_dev, (hipStream_t)stream);
}

int nesti_model_gate_error_import(nesti_model_t* m, const float* src_dev, int n, void* stream) {
  if (!m || !m->cascade || (n > 0 && !src_dev)) NESTI_FAIL("nesti_model_gate_error_import: not a NESTI_F16X3C model / null argument");
  return launch_stat_max_import(m->cstat.dev + kCMaxErrBits, src_dev, n, (hipStream_t)stream);
}

int nesti_model_gate_error2_export(const nesti_model_t* m, float* dst_dev, void* stream) {
  if (!m || !m->cstat2 || !dst_dev) NESTI_FAIL("nesti_model_gate_error2_export: not a NESTI_F16X8C model / null argument");
  return launch_stat_max_export(m->cstat2.dev + kC2MaxErrBits, dst_dev, (hipStream_t)stream);
}

int nesti_model_gate_error2_import(nesti_model_t* m, const float* src_dev, int n, void* stream) {
  if (!m || !m->cstat2 || (n > 0 && !src_dev)) NESTI_FAIL("nesti_model_gate_error2_import: not a NESTI_F16X8C model / null argument");
  return launch_stat_max_import(m->cstat2.dev + kC2MaxErrBits, src_dev, n, (hipStream_t)stream);
}

int nesti_model_guard_error_export(const nesti_model_t* m, float* dst_dev, void* stream) {
  if (!m || !m->gstat || !dst_dev) NESTI_FAIL("nesti_model_guard_error_export: not an NESTI_F16X8 / NESTI_F16X8C model / null argument");
  return launch_stat_max_export(m->gstat.dev + kGMaxDnBits, dst_dev, (hipStream_t)stream);
}

int nesti_model_guard_error_import(nesti_model_t* m, const float* src_dev, int n, void* stream) {
  if (!m || !m->gstat || (n > 0 && !src_dev)) NESTI_FAIL("nesti_model_guard_error_import: not an NESTI_F16X8 / NESTI_F16X8C model / null argument");
  return launch_stat_max_import(m->gstat.dev + kGMaxDnBits, src_dev, n, (hipStream_t)stream);
}

size_t nesti_workspace_bytes(const nesti_model_t* m, int max_batch) {
  if (!m || max_batch <= 0) return 0;
  return ws_layout(m->mode(), max_batch).total;
}

int nesti_model_mups_cstride(const nesti_model_t* m) { return m ? mups_stride(m->mode()) : 0; }
int nesti_model_mups_rows(const nesti_model_t* m) { return m ? 1 << (3 * m->graph.gate_x0_log2S()) : 0; }

// MuPS of B patches in the model's own layout, inside its profiler span
static int run_mups(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev, int B, void* out_dev, hipStream_t st) {
  const int tok = prof_begin(NESTI_PROF_MUPS, st);
  const int rc = launch_mups(&m->graph.cfg, points_dev, n_eff_dev, B, out_dev, m->dtype, mups_stride(m->mode()),
                             /*embed4=*/m->graph.cfg.grid_n == 3, st);
  prof_end(NESTI_PROF_MUPS, tok, st);
  return rc;
}

int nesti_model_mups(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev, int B, void* mups_out_dev,
                     void* stream) {
  if (B <= 0) return 0;
  if (!m || !points_dev || !n_eff_dev || !mups_out_dev) NESTI_FAIL("nesti_model_mups: null argument");
  return run_mups(m, points_dev, n_eff_dev, B, mups_out_dev, (hipStream_t)stream);
}

int nesti_gate_forward(const nesti_model_t* m, const void* mups_dev, int B, void* ws_dev, size_t ws_bytes,
                       float* probs_out_dev, int32_t* expert_out_dev, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!m || !mups_dev || !ws_dev) NESTI_FAIL("nesti_gate_forward: null argument");
  if (m->graph.cfg.arch != NESTI_ARCH_EXPERTS && m->graph.cfg.arch != NESTI_ARCH_SWITCH)
    NESTI_FAIL("nesti_gate_forward: this model has no gating net");
  const Arena A(m, ws_dev, B);
  if (A.L.total > ws_bytes) NESTI_FAIL("nesti_gate_forward: workspace too small (see nesti_workspace_bytes)");
  return gate_impl(m, mups_dev, B, A, probs_out_dev, expert_out_dev, nullptr, nullptr, (hipStream_t)stream);
}

int nesti_experts_forward(const nesti_model_t* m, const void* mups_dev, const int32_t* expert_dev, int B, void* ws_dev,
                          size_t ws_bytes, float* normals_out_dev, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!m || !mups_dev || !ws_dev || !normals_out_dev) NESTI_FAIL("nesti_experts_forward: null argument");
  const Arena A(m, ws_dev, B);
  if (A.L.total > ws_bytes) NESTI_FAIL("nesti_experts_forward: workspace too small (see nesti_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  int32_t* counts = expert_dev ? A.at<int32_t>(A.L.counts) : nullptr;
  int32_t* lists = expert_dev ? A.at<int32_t>(A.L.lists) : nullptr;
  if (expert_dev && launch_route(expert_dev, B, m->graph.cfg.n_experts, counts, lists, st)) return 1;
  return experts_impl(m, mups_dev, B, A, counts, lists, normals_out_dev, st);
}

// gate -> routing -> experts on B rows of a MuPS tensor X0
static int forward_tail(const nesti_model_t* m, const void* X0, int B, const Arena& A, float* normals_out_dev, int32_t* expert_out_dev,
                        float* probs_out_dev, hipStream_t st) {
  if (m->graph.cfg.arch == NESTI_ARCH_SINGLE || m->graph.cfg.arch == NESTI_ARCH_MULTI)   // single-tower ablations: the tower's output IS n_pred (test_n_est.py:136-141)
    return experts_impl(m, X0, B, A, nullptr, nullptr, normals_out_dev, st);
  float* probs = probs_out_dev ? probs_out_dev : A.at<float>(A.L.probs);
  int32_t* expert = expert_out_dev ? expert_out_dev : A.at<int32_t>(A.L.expert);
  int32_t* counts = A.at<int32_t>(A.L.counts);
  int32_t* lists = A.at<int32_t>(A.L.lists);
  if (gate_impl(m, X0, B, A, probs, expert, counts, lists, st)) return 1;
  return experts_impl(m, X0, B, A, counts, lists, normals_out_dev, st);
}

int nesti_forward(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev, int B, void* ws_dev,
                  size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, void* stream) {
  if (B <= 0) return 0;   // empty batch: nothing to do
  if (!m || !points_dev || !n_eff_dev || !ws_dev || !normals_out_dev) NESTI_FAIL("nesti_forward: null argument");
  const Arena A(m, ws_dev, B);
  if (A.L.total > ws_bytes) NESTI_FAIL("nesti_forward: workspace too small (see nesti_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  void* X0 = A.ws + A.L.x0;
  if (run_mups(m, points_dev, n_eff_dev, B, X0, st)) return 1;
  return forward_tail(m, X0, B, A, normals_out_dev, expert_out_dev, probs_out_dev, st);
}

// ---- fused end-to-end entry: search grid + ball query + MuPS + gate + routed experts, batch by batch ---------------
// (plan.h: est_workspace_bytes lays the workspace out as [points (3^3 grid only) | n_eff | forward workspace])
size_t nesti_estimate_workspace_bytes(const nesti_model_t* m, int batch) {
  if (!m || batch <= 0) return 0;
  return est_workspace_bytes(m->mode(), batch);
}

// one shape of a fused call: the _multi entries take a list, nesti_estimate_normals / _at on the 8^3 grid are a list of one
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
  int32_t* n_ball_out_dev;   // position queries: the uncapped ball sizes [n_queries, S], or NULL
};
static EstItem est_item(const nesti_shape_queries_t& s) {
  return {s.cloud_dev, s.n_points, s.query_idx_dev, nullptr, s.n_queries, s.r_abs, s.seed, s.query_row0, s.grid_ws_dev, s.grid_ws_bytes, nullptr};
}
static EstItem est_item(const nesti_shape_positions_t& s) {
  return {s.cloud_dev, s.n_points, nullptr, s.query_xyz_dev, s.n_queries, s.r_abs, s.seed, s.query_row0, s.grid_ws_dev, s.grid_ws_bytes, nullptr};
}

// The two checks every fused entry makes of a shape: its query rows (the single and the multi entries word the refusals
// differently) and its radii
static int check_rows(const std::string& w, bool at, const EstItem& it, const char* row0_msg, const char* rows_msg) {
  if (at && it.query_row0 < 0) NESTI_FAIL(w + row0_msg);
  if (!at && (it.query_row0 < 0 || (!it.query_idx_dev && (long long)it.query_row0 + it.n_queries > (long long)it.n_points)))
    NESTI_FAIL(w + rows_msg);
  return 0;
}
static int check_radii(const std::string& w, const EstItem& it, int S) {
  for (int s = 0; s < S && it.n_queries > 0; ++s) if (!(it.r_abs[s] > 0.0)) NESTI_FAIL(w + ": radii must be positive");
  return 0;
}

// The batch loop of the fused entries on the 8^3 grid: the items' queries, `batch` at a time across item boundaries, from the cloud
// to the MuPS tensor in one kernel per item and batch, then gate -> routing -> experts.  Output rows follow the items' order.  The
// position form (at) also applies the sentinel of queries without a neighbourhood, after each batch's outputs are complete
// (forward_tail ends with the conditioning guard joined on `st`).  Arguments are checked by the callers
static int estimate_batches(bool at, const nesti_model_t* m, const EstItem* items, int n_items, long long total, int batch, void* ws_dev,
                            float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, hipStream_t st) {
  const nesti_config_t* cfg = &m->graph.cfg;
  const Mode mode = m->mode();
  unsigned char* staging = (unsigned char*)ws_dev + est_points_bytes(m->graph, batch);
  int32_t* n_eff = (int32_t*)staging;   // [batch, S]: position queries only
  const Arena A(m, staging + est_neff_bytes(m->graph, batch), batch);
  unsigned char* X0 = A.ws + A.L.x0;
  const size_t row_bytes = mups_row_bytes(mode);
  const int E = probs_cols(m->graph), S = cfg->n_scales;
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
                              it.query_row0 + item_done, it.grid_ws_dev, X0 + (size_t)fill * row_bytes, m->dtype, mups_stride(mode),
                              at ? n_eff + (size_t)fill * S : nullptr,
                              it.n_ball_out_dev ? it.n_ball_out_dev + (size_t)item_done * S : nullptr, st)) {
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
    if (forward_tail(m, X0, fill, A, n_out, e_out, p_out, st)) return 1;
    if (at && launch_mask_empty_queries(n_eff, fill, S, n_out, e_out, p_out, E, st)) return 1;
    done += fill;
  }
  return 0;
}

// nesti_estimate_normals (centres = cloud points) and nesti_estimate_normals_at (centres = positions, `at`): one body.  The
// position form can hand out the uncapped ball sizes.  8^3 grid: estimate_batches with one item; 3^3 grid: patches_kernel +
// mups3_kernel through the staging buffer, batch by batch
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
  const EstItem it = {cloud_dev, N, query_idx_dev, query_xyz_dev, M, r_abs, seed, query_row0, grid_ws_dev, grid_ws_bytes, n_ball_out_dev};
  if (check_rows(w, at, it, ": query_row0 must be >= 0", ": query rows [query_row0, query_row0 + M) exceed the cloud (N points)")) return 1;
  if (nesti_estimate_workspace_bytes(m, batch) > ws_bytes)
    NESTI_FAIL(w + ": workspace too small (see nesti_estimate_workspace_bytes)");
  if (grid_ws_bytes < nesti_patches_workspace_bytes(N)) NESTI_FAIL(w + ": grid workspace too small");
  const nesti_config_t* cfg = &m->graph.cfg;
  if (check_radii(w, it, cfg->n_scales)) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (build_grid && nesti_patches_grid(cfg, cloud_dev, N, r_abs, grid_ws_dev, grid_ws_bytes, stream)) return 1;
  if (cfg->grid_n == 8) return estimate_batches(at, m, &it, 1, M, batch, ws_dev, normals_out_dev, expert_out_dev, probs_out_dev, st);
  float* points = (float*)ws_dev;
  int32_t* n_eff = (int32_t*)((unsigned char*)ws_dev + est_points_bytes(m->graph, batch));
  unsigned char* fwd_ws = (unsigned char*)n_eff + est_neff_bytes(m->graph, batch);
  const size_t fwd_bytes = ws_layout(m->mode(), batch).total;
  const int E = probs_cols(m->graph), S = cfg->n_scales;
  for (int done = 0; done < M; done += batch) {
    const int take = std::min(batch, M - done);
    int32_t* b_out = n_ball_out_dev ? n_ball_out_dev + (size_t)done * S : nullptr;
    float* n_out = normals_out_dev + (size_t)done * 3;
    int32_t* e_out = expert_out_dev ? expert_out_dev + done : nullptr;
    float* p_out = probs_out_dev ? probs_out_dev + (size_t)done * E : nullptr;
    if (at ? nesti_patches_query_at(cfg, cloud_dev, N, query_xyz_dev + (size_t)done * 3, take, r_abs, seed, query_row0 + done, points, n_eff,
                                    nullptr, b_out, grid_ws_dev, grid_ws_bytes, stream)
           : nesti_patches_query(cfg, cloud_dev, N, query_idx_dev ? query_idx_dev + done : nullptr, take, r_abs, seed, query_row0 + done,
                                 points, n_eff, nullptr, nullptr, grid_ws_dev, grid_ws_bytes, stream))
      return 1;
    if (nesti_forward(m, points, n_eff, take, fwd_ws, fwd_bytes, n_out, e_out, p_out, stream)) return 1;
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

}  // extern "C"

// nesti_estimate_normals_multi / _multi_at: one body over the item type (nesti_shape_queries_t, nesti_shape_positions_t; `at` for the latter)
template <class Item>
static int estimate_multi(const char* who, bool at, const nesti_model_t* m, const Item* items, int n_items, int batch, void* ws_dev,
                          size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev, void* stream) {
  const std::string w(who);
  long long total = 0;
  for (int i = 0; items && i < n_items; ++i) total += items[i].n_queries > 0 ? items[i].n_queries : 0;
  if (total == 0) return 0;   // no queries: nothing to do
  if (!m || !ws_dev || !normals_out_dev) NESTI_FAIL(w + ": null argument");
  if (batch <= 0) NESTI_FAIL(w + ": batch must be positive");
  if (m->graph.cfg.grid_n != 8) NESTI_FAIL(w + ": the 8^3 Gaussian grid only (use nesti_estimate_normals per shape)");
  if (nesti_estimate_workspace_bytes(m, batch) > ws_bytes)
    NESTI_FAIL(w + ": workspace too small (see nesti_estimate_workspace_bytes)");
  std::vector<EstItem> v;
  for (int i = 0; i < n_items; ++i) {
    const EstItem it = est_item(items[i]);
    if (it.n_queries < 0 || (it.n_queries > 0 && (!it.cloud_dev || !it.grid_ws_dev || it.n_points <= 0))) NESTI_FAIL(w + ": bad item");
    if (at && it.n_queries > 0 && !it.query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev in an item");
    if (check_rows(w, at, it, ": query_row0 of an item must be >= 0", ": query rows of an item exceed its cloud")) return 1;
    if (it.n_queries > 0 && it.grid_ws_bytes < nesti_patches_workspace_bytes(it.n_points))
      NESTI_FAIL(w + ": grid workspace of an item too small");
    if (check_radii(w, it, m->graph.cfg.n_scales)) return 1;
    v.push_back(it);
  }
  return estimate_batches(at, m, v.data(), n_items, total, batch, ws_dev, normals_out_dev, expert_out_dev, probs_out_dev, (hipStream_t)stream);
}

extern "C" {

int nesti_estimate_normals_multi(const nesti_model_t* m, const nesti_shape_queries_t* items, int n_items, int batch,
                                 void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev,
                                 float* probs_out_dev, void* stream) {
  return estimate_multi("nesti_estimate_normals_multi", false, m, items, n_items, batch, ws_dev, ws_bytes, normals_out_dev, expert_out_dev,
                        probs_out_dev, stream);
}

int nesti_estimate_normals_multi_at(const nesti_model_t* m, const nesti_shape_positions_t* items, int n_items, int batch,
                                    void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev,
                                    float* probs_out_dev, void* stream) {
  return estimate_multi("nesti_estimate_normals_multi_at", true, m, items, n_items, batch, ws_dev, ws_bytes, normals_out_dev,
                        expert_out_dev, probs_out_dev, stream);
}

int nesti_model_macs(const nesti_model_t* m, int tower, int kind, double* nominal, double* useful, double* issued) {
  if (!m) NESTI_FAIL("nesti_model_macs: null model");
  if (kind < -1 || kind > NESTI_PROF_ONE_BY_ONE) NESTI_FAIL("nesti_model_macs: kind must be -1 or a conv category");
  if (tower < -1 || tower >= m->graph.cfg.n_experts) NESTI_FAIL("nesti_model_macs: tower must be -1 (gate) or an expert index");
  tower_macs(m->graph, tower, kind, [m](int layer) -> const PackMeta& { return m->main_packing(layer); }, nominal, useful, issued);
  return 0;
}

// ---- test hook: one launch of a tower alone (include/nesti_hip.h; plan.cpp has nesti_debug_tower_ops, which describes it) ----------
int nesti_debug_tower_step(const nesti_model_t* m, int tower, const nesti_debug_pass_t* pass, int op, const void* mups_dev, int batch,
                           const int32_t* point_index_dev, const int32_t* npoints_dev, int walk, void* ws_dev, size_t ws_bytes,
                           void* stream) {
  if (!m || !mups_dev || !ws_dev) NESTI_FAIL("nesti_debug_tower_step: null argument");
  if (batch <= 0) NESTI_FAIL("nesti_debug_tower_step: batch must be positive");
  const nesti_debug_pass_t& ps = pass ? *pass : kMainPass;
  if (check_pass("nesti_debug_tower_step", m->graph, m->cascade, tower, ps)) return 1;
  if (ps.x8_fmt != 0 && ps.x8_fmt != m->x8_fmt) NESTI_FAIL("nesti_debug_tower_step: x8_fmt differs from the model's (nesti_model_set_x8_format)");
  if (walk < 0 || (walk > 1 && walk % 8)) NESTI_FAIL("nesti_debug_tower_step: walk is 0, 1 or a multiple of 8");
  const Tower& T = m->graph.tower(tower, ps.x8_mask);
  if (op < 0 || op >= (int)T.ops.size()) NESTI_FAIL("nesti_debug_tower_step: op index outside the tower");
  const RunCtx rc = pass_ctx(m, tower, ps.fast != 0, ps.x8_mask, batch, npoints_dev, point_index_dev, (hipStream_t)stream, walk);
  std::vector<unsigned char*> ptr;
  if (tower_ptrs(rc, T, mups_dev, (unsigned char*)ws_dev, ws_bytes, &ptr)) return 1;
  return run_op(rc, T, T.ops[op], ptr);
}

}  // extern "C"
