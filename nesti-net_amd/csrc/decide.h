// Launchers of the kernels that decide (decide.hip): the gate's softmax + arg-max, the two-stage gate, the routing helpers, the
// counter words that travel between ranks, the conditioning guard and the sentinel of position queries.  The words of the counter
// blocks (cstat, gstat, rstat) and of the per-call workspace blocks (fcounts, ecounts) they take are host.h's.
#pragma once
#include "common.h"

namespace nesti {

// softmax over the first E logits of each row + first-index arg-max
// (models/experts_n_est.py:177, test_n_est_w_experts.py:150); optional routing lists.
int launch_gate_finish(const float* logits, int lstride, int B, int E, float* probs,
                       int32_t* expert, int32_t* counts /*[E] or NULL*/,
                       int32_t* lists /*[E][B] or NULL*/, hipStream_t stream);
// NESTI_F16X3C, the two-stage gate: keep [B, NESTI_MAX_EXPERTS] f32 (the f16 pass's logits), flag_list [B], cstat = the model's
// device counters, fcounts = the kFcountsBytes block of the call's workspace (host.h)
int launch_gate_flag(const float* logits, int lstride, int B, int E, float tau, float widen, float* probs, int32_t* expert,
                     float* keep, int32_t* fcounts, int32_t* flag_list, int cap, int n_rounds, unsigned long long* cstat,
                     const unsigned long long* rstat, hipStream_t stream);
// after the recheck rounds, one widening pass: snapshot upper = widen * max_margin_err, flag list (storage reused) of the rows
// in [tau_eff, upper), its round counts, then tau_eff = max(tau_eff, upper)
int launch_gate_widen(const float* keep, int B, int E, float widen, int32_t* fcounts, int32_t* flag_list, int cap, int n_rounds,
                      unsigned long long* cstat, hipStream_t stream);
// rstat = the counter block of the reproducible mode (nesti_model_set_reproducible), null in the default mode: with it the call's
// threshold is tau itself and gate_recheck counts the rows whose widen x error exceeds fcounts[kTauEffOff] instead of anything
// acting on them
int launch_gate_recheck(const float* logits, int lstride, const int32_t* flag_list, const int32_t* count_ptr, int cap, int E,
                        const float* keep, float* probs, int32_t* expert, unsigned long long* cstat, const int32_t* fcounts,
                        float widen, unsigned long long* rstat, hipStream_t stream);
// NESTI_F16X8C, recheck stage 2 (decide.hip): cstat2 = the model's second counter block (host.h: C2Stat); residual [cap], logits2
// [cap, NESTI_MAX_EXPERTS] and margin2 (one float per flag-list position; a round passes its slice) are the call's workspace.
// _begin snapshots tau2_eff; _decide finishes the rows of a round whose stage-2 margin reaches it and lists the others; _gate3_recheck
// finishes the listed rows from the f16x3 logits (logits2 null: the widening round, nothing measured); _widen lists the rows the
// call's later measurements no longer cover
int launch_gate2_begin(int32_t* fcounts, const unsigned long long* cstat2, float tau2, float widen, const unsigned long long* rstat,
                       hipStream_t stream);
int launch_gate2_decide(const float* logits, int lstride, const int32_t* flag_list, const int32_t* count_ptr, int cap, int E,
                        const float* keep, float* probs, int32_t* expert, unsigned long long* cstat, unsigned long long* cstat2,
                        int32_t* fcounts, float widen, unsigned long long* rstat, int32_t* residual, float* logits2, float* margin2,
                        hipStream_t stream);
int launch_gate3_recheck(const float* logits, int lstride, const int32_t* residual, int cap, int E, const float* keep,
                         const float* logits2, float* probs, int32_t* expert, unsigned long long* cstat, unsigned long long* cstat2,
                         const int32_t* fcounts, float widen, unsigned long long* rstat, hipStream_t stream);
int launch_gate2_widen(int B, int32_t* fcounts, const int32_t* flag_list, const float* margin2, int32_t* residual, int cap,
                       unsigned long long* cstat2, float widen, hipStream_t stream);
// a float maximum kept as bits in one counter word (cstat[kCMaxErrBits], gstat[kGMaxDnBits]) <-> a device float (multi-GPU: every
// rank works with the largest value any rank has measured, nesti_model_gate_error_export / _import and the _guard_ twins)
int launch_stat_max_export(const unsigned long long* word, float* dst, hipStream_t stream);
int launch_stat_max_import(unsigned long long* word, const float* src, int n, hipStream_t stream);
// out[i * n_rounds + r] = clamp(counts[i] - r * cap, 0, cap): the rows of list i that round r of a `cap`-row tower covers
int launch_round_counts(const int32_t* counts, int n_lists, int cap, int n_rounds, int32_t* out, hipStream_t stream);
// ms_sw_n_est's switch (models/ms_sw_n_est.py:80-82): noise = logits[b*lstride]; expert = noise < threshold ? 0 : 1;
// probs[b] = noise (one column); optional routing lists over the 2 towers.
int launch_switch_finish(const float* logits, int lstride, int B, float threshold, float* probs,
                         int32_t* expert, int32_t* counts /*[2] or NULL*/, int32_t* lists /*[2][B] or NULL*/,
                         hipStream_t stream);
// the conditioning guard of the FP8 cross-term experts: band of |n| for this pass, flag expert e's rows inside it, replace them by
// their f16x3 re-evaluation and measure |dn|
int launch_x8_guard_begin(int pass, float thr, float scale, int B, unsigned long long* gstat, float* slot,
                          const unsigned long long* rstat, hipStream_t stream);
int launch_x8_guard_flag(const int32_t* list, const int32_t* count_ptr, int count_cap, const float* normals, const float* slot,
                         int32_t* glist, int32_t* gcount, int cap, unsigned long long* gstat, hipStream_t stream);
int launch_x8_guard_fix(const float* src, int sstride, const int32_t* glist, const int32_t* gcount, int cap, float* normals,
                        unsigned long long* gstat, float thr, float scale, unsigned long long* rstat, hipStream_t stream);
// position queries: rows whose n_eff is 0 at every scale get the sentinel normal (0,0,0), expert -1, probs 0 (expert / probs may be NULL)
int launch_mask_empty_queries(const int32_t* n_eff, int M, int S, float* normals, int32_t* expert, float* probs, int E,
                              hipStream_t stream);
// build routing lists from a caller-supplied expert assignment
int launch_route(const int32_t* expert, int B, int E, int32_t* counts, int32_t* lists,
                 hipStream_t stream);
// out[index[j]*3 + c] = src[j*sstride + c] for j < *count (or count_cap when count_ptr NULL)
int launch_scatter3(const float* src, int sstride, const int32_t* index, const int32_t* count_ptr,
                    int count_cap, float* out, hipStream_t stream);

}  // namespace nesti
