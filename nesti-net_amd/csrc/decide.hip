// The kernels that decide, and their launchers (decide.h): the gate's softmax + arg-max, the two-stage gate of NESTI_F16X3C, the
// routing lists and the final scatter, the counter words that travel between ranks, the conditioning guard of the FP8 / FP6
// cross-term experts and the sentinel of position queries.  Memory- or latency-bound, element-wise over the rows of a batch.
// tests/decision_ref.py restates each in numpy; nesti_debug_decision_step (below) runs one launcher alone on caller buffers.
#include "decide.h"

namespace nesti {
namespace {

// softmax (models/experts_n_est.py:177) + np.argmax first-index tie-break (test_n_est_w_experts.py:150) of one row: l = its E
// logits, replaced by exp(l - mx); mx = their fmaxf maximum; probs_row = where the probabilities go, or null
__device__ __forceinline__ int softmax_argmax(float* l, int E, float mx, float* __restrict__ probs_row) {
  float sum = 0.f;
  for (int e = 0; e < E; ++e) { l[e] = expf(l[e] - mx); sum += l[e]; }
  int best = 0;
  float pb = -1.f;
  for (int e = 0; e < E; ++e) {
    const float pr = l[e] / sum;
    if (probs_row) probs_row[e] = pr;
    if (pr > pb) { pb = pr; best = e; }
  }
  return best;
}

// the gate of a model without the two-stage gate: softmax_argmax + optional routing lists for top-1 execution.
__global__ void gate_finish_kernel(const float* __restrict__ logits, int lstride, int B, int E,
                                   float* __restrict__ probs, int32_t* __restrict__ expert,
                                   int32_t* __restrict__ counts, int32_t* __restrict__ lists) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float l[NESTI_MAX_EXPERTS], mx = -INFINITY;
  for (int e = 0; e < E; ++e) { l[e] = logits[(size_t)b * lstride + e]; mx = fmaxf(mx, l[e]); }
  const int best = softmax_argmax(l, E, mx, probs ? probs + (size_t)b * E : nullptr);
  if (expert) expert[b] = best;
  if (counts) {
    const int pos = atomicAdd(&counts[best], 1);
    lists[(size_t)best * B + pos] = b;
  }
}

// ---- NESTI_F16X3C: the two-stage gate (include/nesti_hip.h) -----------------------------------------------------------
// cstat: device counters of the model (host.h: CStat).  The stats are accumulated with atomics in flag-list order, which is not
// deterministic: the double sum may differ in its last bits from run to run (it only feeds sigma, a diagnostic and one input of the
// calibration).
//
// The margin REACTS to what the gate measures (it does not just report it): the threshold of a forward call is
//   tau_eff = max(tau, NESTI_GATE_WIDEN * max_margin_err so far)       (host.h: gate_tau_eff),
// snapshotted into the call's workspace by gate_begin_kernel (forward calls on other streams share the counters and may raise
// them while this one runs), and after the call's own recheck rounds up to NESTI_GATE_WIDEN_PASSES widening passes flag the band
// [tau_eff, NESTI_GATE_WIDEN * max_margin_err) again, each against a snapshot taken when it starts, so that an error the call
// has just measured -- in its recheck rounds or in an earlier widening pass -- is covered for the rows of the same call.
// Unrechecked rows therefore keep a margin of at least NESTI_GATE_WIDEN x the largest error seen on any row decided twice up to
// the start of the call's last widening pass.  The guarantee is per call: two calls in flight on two streams share the
// counters, and an error one of them measures after the other's last snapshot protects the other only from its next call on.
//
// REPRODUCIBLE MODE (nesti_model_set_reproducible): the kernels below that take `rstat` -- the model's third counter block (host.h:
// RStat) -- get a null pointer in the default mode and behave as described above.  With the block, no DECISION reads a counter: the
// call's threshold is tau itself, no widening pass is enqueued, and a row decided twice whose error would have widened the margin is
// counted in rstat[kRGateViolations] instead.  Everything that measures keeps running.
__global__ void gate_begin_kernel(int32_t* __restrict__ fcounts, const unsigned long long* __restrict__ cstat, float tau,
                                  float widen, const unsigned long long* __restrict__ rstat) {
  if (threadIdx.x != 0) return;
  fcounts[0] = 0;                                    // flag count of the filter pass
  fcounts[kWidenCountOff] = 0;                       // ... of the widening round
  const float m = counter_float(cstat[kCMaxErrBits]);
  reinterpret_cast<float*>(fcounts)[kTauEffOff] = rstat ? tau : gate_tau_eff(tau, widen, m);
}

__device__ __forceinline__ float top2_margin(const float* l, int E, bool* nonfinite) {
  float mx = -INFINITY, second = -INFINITY;
  bool bad = false;
  for (int e = 0; e < E; ++e) {
    bad |= !(fabsf(l[e]) < INFINITY);     // NaN, +inf, -inf
    if (l[e] > mx) { second = mx; mx = l[e]; } else second = fmaxf(second, l[e]);
  }
  *nonfinite = bad;
  return mx - second;
}

// The filter (on the plain-f16 gate's logits): softmax + first-index arg-max like gate_finish_kernel; the logits are kept for
// the recheck's error measurement and every row whose top-2 logit margin is below tau_eff -- or that holds a logit that is not finite:
// fmaxf and the > comparisons above skip NaNs, so a NaN row could otherwise keep a large finite margin; a +inf logit gives the
// margin inf (never below tau_eff) and NaN probabilities, a -inf one hides an expert -- is appended to flag_list.
__global__ void gate_flag_kernel(const float* __restrict__ logits, int lstride, int B, int E,
                                 float* __restrict__ probs, int32_t* __restrict__ expert, float* __restrict__ keep,
                                 int32_t* __restrict__ fcounts, int32_t* __restrict__ flag_list,
                                 unsigned long long* __restrict__ cstat) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float tau = reinterpret_cast<const float*>(fcounts)[kTauEffOff];
  float l[NESTI_MAX_EXPERTS], mx = -INFINITY;
  for (int e = 0; e < E; ++e) {
    l[e] = logits[(size_t)b * lstride + e];
    keep[(size_t)b * NESTI_MAX_EXPERTS + e] = l[e];
    mx = fmaxf(mx, l[e]);
  }
  bool nonfinite;
  const float margin = top2_margin(l, E, &nonfinite);
  const bool flag = nonfinite || !(margin >= tau);
  expert[b] = softmax_argmax(l, E, mx, probs ? probs + (size_t)b * E : nullptr);
  if (flag) flag_list[atomicAdd(&fcounts[0], 1)] = b;
  // one counter update per wave
  const unsigned long long fm = __ballot(flag), am = __ballot(true);
  if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)am) - 1u) {
    atomicAdd(&cstat[kCQueries], (unsigned long long)__popcll(am));
    if (fm) atomicAdd(&cstat[kCRechecked], (unsigned long long)__popcll(fm));
  }
}

// One widening pass (model.hip: gate_cascade runs up to NESTI_GATE_WIDEN_PASSES of them after the recheck rounds, each normally
// empty).  gate_widen_begin_kernel snapshots the pass's upper bound = widen x the largest error measured so far -- by this call's
// own recheck rounds or by calls on other streams -- into the call's workspace, so that every thread of the pass flags against
// the same band; gate_widen_kernel appends the rows whose f16 margin lies in [tau_eff, upper) to the flag list (the previous
// list is dead by then, its storage is reused); gate_widen_end_kernel writes the tower-round counts and raises the call's tau_eff
// to `upper`, so the next pass starts where this one ended: an error first measured INSIDE a widening pass is covered by the
// following pass of the same call.
__global__ void gate_widen_begin_kernel(int32_t* __restrict__ fcounts, const unsigned long long* __restrict__ cstat, float widen) {
  if (threadIdx.x != 0) return;
  fcounts[kWidenCountOff] = 0;
  reinterpret_cast<float*>(fcounts)[kWidenUpperOff] = widen * counter_float(cstat[kCMaxErrBits]);
}
__global__ void gate_widen_kernel(const float* __restrict__ keep, int B, int E, int32_t* __restrict__ fcounts,
                                  int32_t* __restrict__ flag_list, unsigned long long* __restrict__ cstat) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float lower = reinterpret_cast<const float*>(fcounts)[kTauEffOff];
  const float upper = reinterpret_cast<const float*>(fcounts)[kWidenUpperOff];
  if (!(upper > lower)) return;
  float l[NESTI_MAX_EXPERTS];
  for (int e = 0; e < E; ++e) l[e] = keep[(size_t)b * NESTI_MAX_EXPERTS + e];
  bool nonfinite;
  const float margin = top2_margin(l, E, &nonfinite);
  if (nonfinite || !(margin >= lower && margin < upper)) return;    // rows with a non-finite logit went through the first list
  const int pos = atomicAdd(&fcounts[kWidenCountOff], 1);
  flag_list[pos] = b;
  atomicAdd(&cstat[kCRechecked], 1ull);
  atomicAdd(&cstat[kCWidened], 1ull);
  if (pos == 0) atomicAdd(&cstat[kCWidenEvents], 1ull);
}
__global__ void gate_widen_end_kernel(int32_t* __restrict__ fcounts, int cap, int n_rounds) {
  const int t = threadIdx.x;
  if (t < n_rounds) fcounts[kWidenRoundsOff + t] = max(0, min(cap, fcounts[kWidenCountOff] - t * cap));
  if (t == 0) {
    float* f = reinterpret_cast<float*>(fcounts);
    if (f[kWidenUpperOff] > f[kTauEffOff]) f[kTauEffOff] = f[kWidenUpperOff];
  }
}

// multi-GPU: the largest error of the f16 gate as a device float, and the other ranks' values folded back in (dist.py); word = the
// counter that holds the float's bits (cstat[kCMaxErrBits]: max_margin_err; gstat[kGMaxDnBits]: the conditioning guard's max_dn)
__global__ void stat_max_export_kernel(const unsigned long long* __restrict__ word, float* __restrict__ dst) {
  if (threadIdx.x == 0) dst[0] = counter_float(word[0]);
}
__global__ void stat_max_import_kernel(unsigned long long* __restrict__ word, const float* __restrict__ src, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = src[i];
  if (v > 0.f && v < INFINITY) atomicMax(word, (unsigned long long)__float_as_uint(v));   // NaN compares false
}

// rows [r * cap, r * cap + cap) of list i are one round of a tower that runs `cap` rows at a time:
// out[i * n_rounds + r] = how many of them exist (the flag list of the two-stage gate: one list; the routing lists: E)
__global__ void round_counts_kernel(const int32_t* __restrict__ counts, int n_lists, int cap, int n_rounds, int32_t* __restrict__ out) {
  const int t = threadIdx.x;
  if (t < n_lists * n_rounds) out[t] = max(0, min(cap, counts[t / n_rounds] - (t % n_rounds) * cap));
}

// What deciding row b from the logits l of a more exact pass takes (l is replaced by exp(l - mx)): the final probabilities and
// arg-max, and the f16 gate's error on the logit differences against its own arg-max (gate_recheck_kernel; stage 2 below)
__device__ __forceinline__ void recheck_row(float* l, float mx, int b, int E, const float* __restrict__ keep, float* __restrict__ probs,
                                            int32_t* __restrict__ expert, unsigned long long* __restrict__ cstat,
                                            const int32_t* __restrict__ fcounts, float widen, unsigned long long* __restrict__ rstat) {
  const int a = expert[b];                       // the f16 gate's arg-max
  float err = 0.f, sq = 0.f;
  int pairs = 0;
  for (int e = 0; e < E; ++e) {
    const float d16 = keep[(size_t)b * NESTI_MAX_EXPERTS + a] - keep[(size_t)b * NESTI_MAX_EXPERTS + e];
    const float pe = fabsf(d16 - (l[a] - l[e]));      // the f16 pass's error on the logit difference (a, e); 0 for e == a
    if (!(pe < INFINITY)) continue;                   // a non-finite logit on either side: the pair measures nothing
    err = fmaxf(err, pe);
    sq += pe * pe;
    pairs += e != a;
  }
  const int best = softmax_argmax(l, E, mx, probs ? probs + (size_t)b * E : nullptr);
  expert[b] = best;
  if (best != a) atomicAdd(&cstat[kCChanged], 1ull);
  atomicMax(&cstat[kCMaxErrBits], (unsigned long long)__float_as_uint(err));
  atomicAdd(reinterpret_cast<double*>(&cstat[kCSumSq]), (double)sq);
  atomicAdd(&cstat[kCPairs], (unsigned long long)pairs);
  // reproducible mode: the error that would have widened the call's margin is counted, not acted on
  if (rstat && widen * err > reinterpret_cast<const float*>(fcounts)[kTauEffOff]) atomicAdd(&rstat[kRGateViolations], 1ull);
}

// The recheck (on the f16x3 gate's logits of one round, compact rows j <-> query flag_list[j]): the final probabilities and
// arg-max of those queries, and the f16 gate's error on the logit differences against its own arg-max.
__global__ void gate_recheck_kernel(const float* __restrict__ logits, int lstride, const int32_t* __restrict__ flag_list,
                                    const int32_t* __restrict__ count_ptr, int cap, int E, const float* __restrict__ keep,
                                    float* __restrict__ probs, int32_t* __restrict__ expert,
                                    unsigned long long* __restrict__ cstat, const int32_t* __restrict__ fcounts, float widen,
                                    unsigned long long* __restrict__ rstat) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(cap, *count_ptr)) return;
  float l[NESTI_MAX_EXPERTS], mx = -INFINITY;
  for (int e = 0; e < E; ++e) { l[e] = logits[(size_t)j * lstride + e]; mx = fmaxf(mx, l[e]); }
  recheck_row(l, mx, flag_list[j], E, keep, probs, expert, cstat, fcounts, widen, rstat);
}

// ---- NESTI_F16X8C: recheck stage 2 (model.hip: gate_cascade) ----------------------------------------------------------------------
// The flagged rows first go through the gating net with its six 8^3 tap layers in the FP6 cross-term form (conv8n.hip X6), whose
// error on a logit difference is far below the filter's.  A row whose stage-2 top-2 margin is at least
//   tau2_eff = max(tau2, NESTI_GATE_WIDEN * largest stage-2 error measured so far)       (snapshotted per call, like tau_eff)
// is final: gate2_decide_kernel does for it what gate_recheck_kernel does, with the stage-2 logits.  The others -- and every row
// with a logit that is not finite -- form the round's residual list, with their stage-2 logits kept; stage 3 is today's f16x3 gate
// over that list, and gate3_recheck_kernel measures BOTH errors on it: the filter's (exactly as gate_recheck_kernel) and stage 2's,
// |(l_a - l_k)_stage2 - (l_a - l_k)_f16x3| over all k with a = the stage-2 arg-max.  Every rechecked row therefore measures the filter
// once, against the pass that decides it.  After the rounds one widening round (gate2_widen_kernel) passes the rows stage 2 decided
// with a margin in [tau2_eff, NESTI_GATE_WIDEN * the largest stage-2 error now known) on to stage 3 as well (normally none: the
// tower's launches find a zero count).  Reproducible mode (rstat): tau2_eff = tau2, no widening round, and a residual row whose
// stage-2 error would have widened the margin is counted in rstat[kRGateViolations].
//   margin2[i]: the stage-2 margin of flag-list position i (+inf for a row passed on), what the widening round reads
__global__ void gate2_begin_kernel(int32_t* __restrict__ fcounts, const unsigned long long* __restrict__ cstat2, float tau2, float widen,
                                   const unsigned long long* __restrict__ rstat) {
  if (threadIdx.x != 0) return;
  reinterpret_cast<float*>(fcounts)[kTau2EffOff] = rstat ? tau2 : gate_tau_eff(tau2, widen, counter_float(cstat2[kC2MaxErrBits]));
}

__global__ void gate2_decide_kernel(const float* __restrict__ logits, int lstride, const int32_t* __restrict__ flag_list,
                                    const int32_t* __restrict__ count_ptr, int cap, int E, const float* __restrict__ keep,
                                    float* __restrict__ probs, int32_t* __restrict__ expert, unsigned long long* __restrict__ cstat,
                                    unsigned long long* __restrict__ cstat2, int32_t* __restrict__ fcounts, float widen,
                                    unsigned long long* __restrict__ rstat, int32_t* __restrict__ residual,
                                    float* __restrict__ logits2, float* __restrict__ margin2) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(cap, *count_ptr)) return;
  const int b = flag_list[j];
  float l[NESTI_MAX_EXPERTS], mx = -INFINITY;
  for (int e = 0; e < E; ++e) { l[e] = logits[(size_t)j * lstride + e]; mx = fmaxf(mx, l[e]); }
  bool nonfinite;
  const float margin = top2_margin(l, E, &nonfinite);
  const bool pass_on = nonfinite || !(margin >= reinterpret_cast<const float*>(fcounts)[kTau2EffOff]);
  margin2[j] = pass_on ? INFINITY : margin;
  if (pass_on) {
    const int pos = atomicAdd(&fcounts[kResCountOff], 1);      // at most the round's rows: pos < cap
    residual[pos] = b;
    for (int e = 0; e < E; ++e) logits2[(size_t)pos * NESTI_MAX_EXPERTS + e] = l[e];
  } else {
    recheck_row(l, mx, b, E, keep, probs, expert, cstat, fcounts, widen, rstat);
  }
  const unsigned long long pm = __ballot(pass_on), am = __ballot(true);
  if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)am) - 1u) {
    atomicAdd(&cstat2[kC2Rows], (unsigned long long)__popcll(am));
    if (am & ~pm) atomicAdd(&cstat2[kC2Decided], (unsigned long long)__popcll(am & ~pm));
    if (pm) atomicAdd(&cstat2[kC2Residual], (unsigned long long)__popcll(pm));
  }
}

// Stage 3 over the residual list (compact rows j <-> query residual[j], fcounts[kResCountOff] of them): final probabilities and
// arg-max from the f16x3 logits.  logits2 != null (a round's residual): both error measurements; null (the widening round, whose
// rows stage 2 had already decided and measured the filter with): none
__global__ void gate3_recheck_kernel(const float* __restrict__ logits, int lstride, const int32_t* __restrict__ residual, int cap, int E,
                                     const float* __restrict__ keep, const float* __restrict__ logits2, float* __restrict__ probs,
                                     int32_t* __restrict__ expert, unsigned long long* __restrict__ cstat,
                                     unsigned long long* __restrict__ cstat2, const int32_t* __restrict__ fcounts, float widen,
                                     unsigned long long* __restrict__ rstat) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(cap, fcounts[kResCountOff])) return;
  const int b = residual[j];
  float l[NESTI_MAX_EXPERTS], mx = -INFINITY;
  for (int e = 0; e < E; ++e) { l[e] = logits[(size_t)j * lstride + e]; mx = fmaxf(mx, l[e]); }
  if (!logits2) {
    expert[b] = softmax_argmax(l, E, mx, probs ? probs + (size_t)b * E : nullptr);
    return;
  }
  float l3[NESTI_MAX_EXPERTS];
  for (int e = 0; e < E; ++e) l3[e] = l[e];
  recheck_row(l, mx, b, E, keep, probs, expert, cstat, fcounts, widen, rstat);     // replaces l by exp(l - mx)
  const float* l2 = logits2 + (size_t)j * NESTI_MAX_EXPERTS;
  int a = 0;
  for (int e = 1; e < E; ++e) if (l2[e] > l2[a]) a = e;                            // the stage-2 arg-max (first index on ties)
  float err = 0.f, sq = 0.f;
  int pairs = 0;
  for (int e = 0; e < E; ++e) {
    const float pe = fabsf((l2[a] - l2[e]) - (l3[a] - l3[e]));
    if (!(pe < INFINITY)) continue;
    err = fmaxf(err, pe);
    sq += pe * pe;
    pairs += e != a;
  }
  atomicMax(&cstat2[kC2MaxErrBits], (unsigned long long)__float_as_uint(err));
  atomicAdd(reinterpret_cast<double*>(&cstat2[kC2SumSq]), (double)sq);
  atomicAdd(&cstat2[kC2Pairs], (unsigned long long)pairs);
  if (rstat && widen * err > reinterpret_cast<const float*>(fcounts)[kTau2EffOff]) atomicAdd(&rstat[kRGateViolations], 1ull);
}

// The stage's widening round: the rows of the call's flag list (n_flagged = fcounts[0] positions) that stage 2 decided with a margin
// inside [tau2_eff, widen x the largest stage-2 error known now) become the residual list once more (at most cap of them; the rest
// are counted in cstat2[kC2Dropped])
__global__ void gate2_widen_begin_kernel(int32_t* __restrict__ fcounts, const unsigned long long* __restrict__ cstat2, float widen) {
  if (threadIdx.x != 0) return;
  fcounts[kResCountOff] = 0;
  reinterpret_cast<float*>(fcounts)[kTau2UpperOff] = widen * counter_float(cstat2[kC2MaxErrBits]);
}
__global__ void gate2_widen_kernel(int B, int32_t* __restrict__ fcounts, const int32_t* __restrict__ flag_list,
                                   const float* __restrict__ margin2, int32_t* __restrict__ residual, int cap,
                                   unsigned long long* __restrict__ cstat2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= min(B, fcounts[0])) return;
  const float lower = reinterpret_cast<const float*>(fcounts)[kTau2EffOff];
  const float upper = reinterpret_cast<const float*>(fcounts)[kTau2UpperOff];
  const float m = margin2[i];
  if (!(m >= lower && m < upper)) return;
  const int pos = atomicAdd(&fcounts[kResCountOff], 1);
  if (pos < cap) { residual[pos] = flag_list[i]; atomicAdd(&cstat2[kC2Widened], 1ull); }
  else atomicAdd(&cstat2[kC2Dropped], 1ull);
}

// tf.where(noise_est < 0.015, n_est_small, n_est_large) as a routing decision (models/ms_sw_n_est.py:80-82)
__global__ void switch_finish_kernel(const float* __restrict__ logits, int lstride, int B, float threshold,
                                     float* __restrict__ probs, int32_t* __restrict__ expert,
                                     int32_t* __restrict__ counts, int32_t* __restrict__ lists) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float noise = logits[(size_t)b * lstride];
  const int pick = (noise < threshold) ? 0 : 1;   // a NaN compares false -> large, like tf.where
  if (probs) probs[b] = noise;
  if (expert) expert[b] = pick;
  if (counts) {
    const int pos = atomicAdd(&counts[pick], 1);
    lists[(size_t)pick * B + pos] = b;
  }
}

__global__ void route_kernel(const int32_t* __restrict__ expert, int B, int E,
                             int32_t* __restrict__ counts, int32_t* __restrict__ lists) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int e = expert[b];
  if (e < 0 || e >= E) return;
  const int pos = atomicAdd(&counts[e], 1);
  lists[(size_t)e * B + pos] = b;
}

__global__ void scatter3_kernel(const float* __restrict__ src, int sstride, const int32_t* __restrict__ index,
                                const int32_t* __restrict__ count_ptr, int count_cap, float* __restrict__ out) {
  int n = count_cap;
  if (count_ptr) n = min(n, *count_ptr);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const long long d = index ? index[j] : j;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[d * 3 + c] = src[(size_t)j * sstride + c];
}

// Zeroes the routing counters.  A kernel, not hipMemsetAsync: inside a captured hipGraph the memset node of this
// 4*E-byte region did not take effect on replay (ROCm 7.2, gfx950) -- the counters then accumulated from replay to
// replay and the expert towers read stale list entries.
__global__ void zero_counts_kernel(int32_t* __restrict__ counts, int n) {
  if ((int)threadIdx.x < n) counts[threadIdx.x] = 0;
}

}  // namespace

// ---- the conditioning guard of the FP8 cross-term experts (NESTI_F16X8 / NESTI_F16X8C; model.hip: Guard) ----------------------------
// The FP8 residual moves an expert's output n by |dn| ~ 5e-5 (<= 2e-4 on 100 000 queries), independent of |n|; 1 - cos against the
// three-product result is (|dn| / |n|)^2 / 2, so only outputs of very small norm can be tilted by more than the bar.  A query whose
// |n| is below thr = widen x (largest |dn| measured so far) / theta, theta = sqrt(2 x 2.5e-6), is therefore evaluated AGAIN by its
// expert in f16x3 proper and the result replaces the X8 one; the rows decided twice measure |dn| (it does not depend on |n|), and the
// threshold follows the measurement like the two-stage gate's margin does.
//   gstat (device, per model): host.h: GStat
//   slot  (device, per call):  [0] lower, [1] upper end of the current pass's |n| band (floats)
// Reproducible mode (rstat != null, see the two-stage gate above): the band of pass 0 is [0, thr) whatever has been measured, no
// further pass is enqueued, and a re-evaluated row whose |dn| would have raised the threshold is counted in rstat[kRGuardViolations].
__global__ void x8_guard_begin_kernel(int pass, float thr, float scale, int B, unsigned long long* __restrict__ gstat, float* __restrict__ slot,
                                      const unsigned long long* __restrict__ rstat) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float hi = rstat ? thr : fmaxf(thr, scale * counter_float(gstat[kGMaxDnBits]));      // scale = widen / theta (host.h: x8_guard_scale)
  if (pass == 0) {
    slot[0] = 0.f;
    slot[1] = hi;
    atomicAdd(&gstat[kGQueries], (unsigned long long)B);
  } else {
    slot[0] = slot[1];
    slot[1] = fmaxf(hi, slot[1]);
  }
}
// expert e's routing list -> the rows whose |n| lies in the band, compacted into glist (at most cap of them)
__global__ void x8_guard_flag_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ count_ptr, int count_cap,
                                     const float* __restrict__ normals, const float* __restrict__ slot, int32_t* __restrict__ glist,
                                     int32_t* __restrict__ gcount, int cap, unsigned long long* __restrict__ gstat) {
  const int n = min(count_cap, *count_ptr);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int i = list[j];
  const float x = normals[(size_t)i * 3], y = normals[(size_t)i * 3 + 1], z = normals[(size_t)i * 3 + 2];
  const float r = sqrtf(x * x + y * y + z * z);
  if (!(r >= slot[0] && r < slot[1]) && r == r) return;                            // a NaN output is re-evaluated too
  const int pos = atomicAdd(gcount, 1);
  if (pos < cap) glist[pos] = i;
  else atomicAdd(&gstat[kGDropped], 1ull);
}
// the f16x3 results of the flagged rows replace the X8 ones; |dn| is measured on the way
__global__ void x8_guard_fix_kernel(const float* __restrict__ src, int sstride, const int32_t* __restrict__ glist,
                                    const int32_t* __restrict__ gcount, int cap, float* __restrict__ normals,
                                    unsigned long long* __restrict__ gstat, float thr, float scale,
                                    unsigned long long* __restrict__ rstat) {
  const int n = min(cap, *gcount);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0 && n > 0) atomicAdd(&gstat[kGRechecked], (unsigned long long)n);
  if (j >= n) return;
  const long long i = glist[j];
  float d2 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float nw = src[(size_t)j * sstride + c], od = normals[i * 3 + c];
    d2 += (nw - od) * (nw - od);
    normals[i * 3 + c] = nw;
  }
  const float dn = sqrtf(d2);
  if (dn > 0.f && dn < INFINITY) atomicMax(&gstat[kGMaxDnBits], (unsigned long long)__float_as_uint(dn));
  if (rstat && dn < INFINITY && scale * dn > thr) atomicAdd(&rstat[kRGuardViolations], 1ull);
}

// ---- position queries (nesti_*_at): a query whose balls are empty at EVERY scale has no neighbourhood ----------------------------
// Its MuPS rows are zeros and went through the towers like any row; what comes out is the sentinel: normal (0, 0, 0), expert -1,
// probabilities 0.  Element-wise over the rows of a batch, enqueued after everything that writes the batch's outputs.
__global__ void mask_empty_queries_kernel(const int32_t* __restrict__ n_eff, int M, int S, float* __restrict__ normals,
                                          int32_t* __restrict__ expert, float* __restrict__ probs, int E) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  for (int s = 0; s < S; ++s)
    if (n_eff[(size_t)i * S + s] > 0) return;
  normals[(size_t)i * 3] = 0.f; normals[(size_t)i * 3 + 1] = 0.f; normals[(size_t)i * 3 + 2] = 0.f;
  if (expert) expert[i] = -1;
  if (probs)
    for (int e = 0; e < E; ++e) probs[(size_t)i * E + e] = 0.f;
}

int launch_gate_finish(const float* logits, int lstride, int B, int E, float* probs, int32_t* expert,
                       int32_t* counts, int32_t* lists, hipStream_t stream) {
  if (B <= 0) return 0;
  if (E > NESTI_MAX_EXPERTS) NESTI_FAIL("gate_finish: too many experts");
  if (counts) hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(64), 0, stream, counts, E);
  hipLaunchKernelGGL(gate_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, logits, lstride, B, E,
                     probs, expert, counts, lists);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate_flag(const float* logits, int lstride, int B, int E, float tau, float widen, float* probs, int32_t* expert,
                     float* keep, int32_t* fcounts, int32_t* flag_list, int cap, int n_rounds, unsigned long long* cstat,
                     const unsigned long long* rstat, hipStream_t stream) {
  if (B <= 0) return 0;
  if (E > NESTI_MAX_EXPERTS || n_rounds > kMaxCascadeRounds) NESTI_FAIL("gate_flag: too many experts / rounds");
  hipLaunchKernelGGL(gate_begin_kernel, dim3(1), dim3(64), 0, stream, fcounts, cstat, tau, widen, rstat);
  hipLaunchKernelGGL(gate_flag_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, logits, lstride, B, E, probs,
                     expert, keep, fcounts, flag_list, cstat);
  hipLaunchKernelGGL(round_counts_kernel, dim3(1), dim3(64), 0, stream, fcounts, 1, cap, n_rounds, fcounts + kRoundCountsOff);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate_widen(const float* keep, int B, int E, float widen, int32_t* fcounts, int32_t* flag_list, int cap, int n_rounds,
                      unsigned long long* cstat, hipStream_t stream) {
  if (B <= 0) return 0;
  if (n_rounds > kMaxCascadeRounds) NESTI_FAIL("gate_widen: too many rounds");
  hipLaunchKernelGGL(gate_widen_begin_kernel, dim3(1), dim3(64), 0, stream, fcounts, cstat, widen);
  hipLaunchKernelGGL(gate_widen_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, keep, B, E, fcounts, flag_list, cstat);
  hipLaunchKernelGGL(gate_widen_end_kernel, dim3(1), dim3(64), 0, stream, fcounts, cap, n_rounds);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_stat_max_export(const unsigned long long* word, float* dst, hipStream_t stream) {
  hipLaunchKernelGGL(stat_max_export_kernel, dim3(1), dim3(64), 0, stream, word, dst);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}
int launch_stat_max_import(unsigned long long* word, const float* src, int n, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(stat_max_import_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, word, src, n);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_round_counts(const int32_t* counts, int n_lists, int cap, int n_rounds, int32_t* out, hipStream_t stream) {
  if (n_lists * n_rounds > 256) NESTI_FAIL("round_counts: too many lists x rounds");
  hipLaunchKernelGGL(round_counts_kernel, dim3(1), dim3(256), 0, stream, counts, n_lists, cap, n_rounds, out);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate_recheck(const float* logits, int lstride, const int32_t* flag_list, const int32_t* count_ptr, int cap, int E,
                        const float* keep, float* probs, int32_t* expert, unsigned long long* cstat, const int32_t* fcounts,
                        float widen, unsigned long long* rstat, hipStream_t stream) {
  if (cap <= 0) return 0;
  hipLaunchKernelGGL(gate_recheck_kernel, dim3((cap + 255) / 256), dim3(256), 0, stream, logits, lstride, flag_list,
                     count_ptr, cap, E, keep, probs, expert, cstat, fcounts, widen, rstat);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate2_begin(int32_t* fcounts, const unsigned long long* cstat2, float tau2, float widen, const unsigned long long* rstat,
                       hipStream_t stream) {
  hipLaunchKernelGGL(gate2_begin_kernel, dim3(1), dim3(64), 0, stream, fcounts, cstat2, tau2, widen, rstat);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate2_decide(const float* logits, int lstride, const int32_t* flag_list, const int32_t* count_ptr, int cap, int E,
                        const float* keep, float* probs, int32_t* expert, unsigned long long* cstat, unsigned long long* cstat2,
                        int32_t* fcounts, float widen, unsigned long long* rstat, int32_t* residual, float* logits2, float* margin2,
                        hipStream_t stream) {
  if (cap <= 0) return 0;
  hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(64), 0, stream, fcounts + kResCountOff, 1);
  hipLaunchKernelGGL(gate2_decide_kernel, dim3((cap + 255) / 256), dim3(256), 0, stream, logits, lstride, flag_list, count_ptr, cap, E,
                     keep, probs, expert, cstat, cstat2, fcounts, widen, rstat, residual, logits2, margin2);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate3_recheck(const float* logits, int lstride, const int32_t* residual, int cap, int E, const float* keep,
                         const float* logits2, float* probs, int32_t* expert, unsigned long long* cstat, unsigned long long* cstat2,
                         const int32_t* fcounts, float widen, unsigned long long* rstat, hipStream_t stream) {
  if (cap <= 0) return 0;
  hipLaunchKernelGGL(gate3_recheck_kernel, dim3((cap + 255) / 256), dim3(256), 0, stream, logits, lstride, residual, cap, E, keep,
                     logits2, probs, expert, cstat, cstat2, fcounts, widen, rstat);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gate2_widen(int B, int32_t* fcounts, const int32_t* flag_list, const float* margin2, int32_t* residual, int cap,
                       unsigned long long* cstat2, float widen, hipStream_t stream) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(gate2_widen_begin_kernel, dim3(1), dim3(64), 0, stream, fcounts, cstat2, widen);
  hipLaunchKernelGGL(gate2_widen_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, fcounts, flag_list, margin2, residual, cap, cstat2);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_switch_finish(const float* logits, int lstride, int B, float threshold, float* probs, int32_t* expert,
                         int32_t* counts, int32_t* lists, hipStream_t stream) {
  if (B <= 0) return 0;
  if (counts) hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(64), 0, stream, counts, 2);
  hipLaunchKernelGGL(switch_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, logits, lstride, B, threshold,
                     probs, expert, counts, lists);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_x8_guard_begin(int pass, float thr, float scale, int B, unsigned long long* gstat, float* slot,
                          const unsigned long long* rstat, hipStream_t stream) {
  hipLaunchKernelGGL(x8_guard_begin_kernel, dim3(1), dim3(64), 0, stream, pass, thr, scale, B, gstat, slot, rstat);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}
int launch_x8_guard_flag(const int32_t* list, const int32_t* count_ptr, int count_cap, const float* normals, const float* slot,
                         int32_t* glist, int32_t* gcount, int cap, unsigned long long* gstat, hipStream_t stream) {
  if (count_cap <= 0) return 0;
  hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(64), 0, stream, gcount, 1);
  hipLaunchKernelGGL(x8_guard_flag_kernel, dim3((count_cap + 255) / 256), dim3(256), 0, stream, list, count_ptr, count_cap, normals,
                     slot, glist, gcount, cap, gstat);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}
int launch_x8_guard_fix(const float* src, int sstride, const int32_t* glist, const int32_t* gcount, int cap, float* normals,
                        unsigned long long* gstat, float thr, float scale, unsigned long long* rstat, hipStream_t stream) {
  if (cap <= 0) return 0;
  // a walking-size grid: the list is normally a few dozen rows; a full one is walked by the same threads
  hipLaunchKernelGGL(x8_guard_fix_kernel, dim3((cap + 255) / 256), dim3(256), 0, stream, src, sstride, glist, gcount, cap, normals, gstat,
                     thr, scale, rstat);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_mask_empty_queries(const int32_t* n_eff, int M, int S, float* normals, int32_t* expert, float* probs, int E,
                              hipStream_t stream) {
  if (M <= 0) return 0;
  hipLaunchKernelGGL(mask_empty_queries_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, n_eff, M, S, normals, expert, probs, E);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_route(const int32_t* expert, int B, int E, int32_t* counts, int32_t* lists, hipStream_t stream) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(64), 0, stream, counts, E);
  hipLaunchKernelGGL(route_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, expert, B, E, counts, lists);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_scatter3(const float* src, int sstride, const int32_t* index, const int32_t* count_ptr,
                    int count_cap, float* out, hipStream_t stream) {
  if (count_cap <= 0) return 0;
  hipLaunchKernelGGL(scatter3_kernel, dim3((count_cap + 255) / 256), dim3(256), 0, stream, src, sstride,
                     index, count_ptr, count_cap, out);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_mask_empty_queries(const int32_t* n_eff_dev, int M, int S, float* normals_dev, int32_t* expert_dev, float* probs_dev, int E,
                             void* stream) {
  if (M <= 0) return 0;   // no rows: nothing to do
  if (!n_eff_dev || !normals_dev) NESTI_FAIL("nesti_mask_empty_queries: null argument");
  if (S < 1 || S > NESTI_MAX_SCALES) NESTI_FAIL("nesti_mask_empty_queries: bad n_scales");
  if (probs_dev && E < 1) NESTI_FAIL("nesti_mask_empty_queries: probs_dev needs E >= 1 columns");
  return launch_mask_empty_queries(n_eff_dev, M, S, normals_dev, expert_dev, probs_dev, E, (hipStream_t)stream);
}

// ---- test hook: one launcher of the deciding kernels alone, on caller buffers (include/nesti_hip.h) --------------------------------
int nesti_debug_decision_step(int op, const nesti_debug_decision_t* a, void* stream) {
  const std::string who = "nesti_debug_decision_step: ";
  if (!a) NESTI_FAIL(who + "null argument");
  if (op < 0 || op >= NESTI_DECISION_OPS) NESTI_FAIL(who + "unknown op");
  const hipStream_t st = (hipStream_t)stream;
  auto u64 = [](uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); };
  const bool uses_E = op == NESTI_DECISION_GATE_FINISH || op == NESTI_DECISION_GATE_FLAG || op == NESTI_DECISION_GATE_WIDEN ||
                      op == NESTI_DECISION_GATE_RECHECK || op == NESTI_DECISION_ROUTE;
  if (uses_E && (a->E < 1 || a->E > NESTI_MAX_EXPERTS)) NESTI_FAIL(who + "E outside 1 .. NESTI_MAX_EXPERTS");
  if (a->n_rounds > kMaxCascadeRounds) NESTI_FAIL(who + "n_rounds above kMaxCascadeRounds");
#define NESTI_NEED(cond, what) if (!(cond)) NESTI_FAIL(who + "null pointer: " what)
  switch (op) {
    case NESTI_DECISION_GATE_FINISH:
      NESTI_NEED(a->logits && (!a->counts || a->lists), "logits, lists");
      return launch_gate_finish(a->logits, a->lstride, a->B, a->E, a->probs, a->expert, a->counts, a->lists, st);
    case NESTI_DECISION_GATE_FLAG:
      NESTI_NEED(a->logits && a->expert && a->keep && a->fcounts && a->flag_list && a->cstat, "logits, expert, keep, fcounts, flag_list, cstat");
      return launch_gate_flag(a->logits, a->lstride, a->B, a->E, a->tau, a->widen, a->probs, a->expert, a->keep, a->fcounts, a->flag_list,
                              a->cap, a->n_rounds, u64(a->cstat), u64(a->rstat), st);
    case NESTI_DECISION_GATE_WIDEN:
      NESTI_NEED(a->keep && a->fcounts && a->flag_list && a->cstat, "keep, fcounts, flag_list, cstat");
      return launch_gate_widen(a->keep, a->B, a->E, a->widen, a->fcounts, a->flag_list, a->cap, a->n_rounds, u64(a->cstat), st);
    case NESTI_DECISION_GATE_RECHECK:
      NESTI_NEED(a->logits && a->flag_list && a->count_ptr && a->keep && a->expert && a->cstat && (!a->rstat || a->fcounts),
                 "logits, flag_list, count_ptr, keep, expert, cstat, fcounts");
      return launch_gate_recheck(a->logits, a->lstride, a->flag_list, a->count_ptr, a->cap, a->E, a->keep, a->probs, a->expert,
                                 u64(a->cstat), a->fcounts, a->widen, u64(a->rstat), st);
    case NESTI_DECISION_ROUND_COUNTS:
      NESTI_NEED(a->counts && a->round_out, "counts, round_out");
      return launch_round_counts(a->counts, a->n_lists, a->cap, a->n_rounds, a->round_out, st);
    case NESTI_DECISION_SWITCH_FINISH:
      NESTI_NEED(a->logits && (!a->counts || a->lists), "logits, lists");
      return launch_switch_finish(a->logits, a->lstride, a->B, a->thr, a->probs, a->expert, a->counts, a->lists, st);
    case NESTI_DECISION_X8_GUARD_BEGIN:
      NESTI_NEED(a->gstat && a->slot, "gstat, slot");
      return launch_x8_guard_begin(a->pass, a->thr, a->scale, a->B, u64(a->gstat), a->slot, u64(a->rstat), st);
    case NESTI_DECISION_X8_GUARD_FLAG:
      NESTI_NEED(a->lists && a->count_ptr && a->normals && a->slot && a->glist && a->gcount && a->gstat,
                 "lists, count_ptr, normals, slot, glist, gcount, gstat");
      return launch_x8_guard_flag(a->lists, a->count_ptr, a->B, a->normals, a->slot, a->glist, a->gcount, a->cap, u64(a->gstat), st);
    case NESTI_DECISION_X8_GUARD_FIX:
      NESTI_NEED(a->src && a->glist && a->gcount && a->normals && a->gstat, "src, glist, gcount, normals, gstat");
      return launch_x8_guard_fix(a->src, a->sstride, a->glist, a->gcount, a->cap, a->normals, u64(a->gstat), a->thr, a->scale,
                                 u64(a->rstat), st);
    case NESTI_DECISION_ROUTE:
      NESTI_NEED(a->expert && a->counts && a->lists, "expert, counts, lists");
      return launch_route(a->expert, a->B, a->E, a->counts, a->lists, st);
    case NESTI_DECISION_SCATTER3:
      NESTI_NEED(a->src && a->normals, "src, normals");
      return launch_scatter3(a->src, a->sstride, a->index, a->count_ptr, a->cap, a->normals, st);
    case NESTI_DECISION_STAT_MAX_EXPORT:
      NESTI_NEED(a->word && a->dst, "word, dst");
      return launch_stat_max_export(u64(a->word), a->dst, st);
    default:   // NESTI_DECISION_STAT_MAX_IMPORT
      NESTI_NEED(a->word && a->src, "word, src");
      return launch_stat_max_import(u64(a->word), a->src, a->B, st);
  }
#undef NESTI_NEED
}

}  // extern "C"
