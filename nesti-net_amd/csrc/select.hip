// Scale-selected plane fit over neighbour lists (DESIGN.md 2 "Scale-selected plane fit"): the plane fit of nesti_pca_normals_nbr at every
// neighbour count of a ladder of up to NESTI_SELECT_MAX_L counts, and per row the choice of one of them -- the candidate of smallest
// surface variation e0 / (e0 + e1 + e2), Pauly, Keiser and Gross's multi-scale surface variation (2003) read as a selector, standing in
// for the bias / variance trade of Mitra and Nguyen (2003).  The conventions are the library's own (no parity with any published selector
// is claimed); the score uses only + - x / and comparisons on the f32 eigenvalues as written, so a caller recomputes every choice from
// the outputs (tests/_select_fixture.py).
//
// THE ENTRY (nesti_pca_select_nbr, nesti_pca_select_nbr_at).  Centres, the list nbr_dev [M, K], its valid prefix and the untrusted-list
// rule are exactly those of nesti_pca_normals_nbr (nbr_dev.h).  ks [L] on the host: strictly ascending, in 1 .. K; slack: fp64, >= 0.
//  1 CANDIDATE c.  n_c = min(ks[c], valid prefix); r2_c = the largest d2 among the first n_c slots (a prefix maximum).
//  2 FIT.  nesti_pca_normals_nbr with ks = {ks[c]}, bit for bit: slot i is added in lane i mod 64, a lane adds its slots in ascending
//    order from +0.0, every total goes through the xor-butterfly of wave_sum (offsets 32, 16, ..., 1), then plane_solve as it stands.
//    n_c < 3 or r2_c == 0: zeros.
//  3 SCORE.  den = ((double)e0 + (double)e1) + (double)e2, v_c = (double)e0 / den; eligible iff n_c >= 3, r2_c > 0 and den > 0.
//  4 SELECTION.  v_min over the eligible; thr = v_min + v_min slack; sel = the largest eligible c with v_c <= thr; none eligible: -1.
//  5 OUTPUTS.  The selected normal, eigenvalues, sel, n_sel, (float)sqrt(r2_sel); per candidate (float)v_c (0 where not eligible),
//    normal, eigenvalues, radius and count.  Any may be NULL.
// DETERMINISM.  No atomics.  A row's bits are a pure function of (cloud, centre, list prefix, ladder, slack).
//
// THE KERNEL.  One wave per row, four rows per workgroup, no LDS, no scratch; L is a run-time value, one kernel serves every ladder.
//  - A lane owns at most kNbrTrips = 4 slots (lane, lane + 64, ...), so its partial sum for ANY candidate is one of four running prefix
//    sums of its own terms (or +0.0): they are formed once, 4 x 9 fp64 sums and 4 prefix maxima of d2, whatever L is.  The 4-scale
//    kernel keeps S x 9 sums per lane and walks every term S times; that does not stretch to a ladder.
//  - The butterflies of the candidates are folded into one (fold below): at offset 32 a lane keeps half of the candidates and hands
//    its partner the other half, at 16 a quarter, ... so a total over 32 candidates costs 16 + 8 + 4 + 2 + 1 + 1 = 32 shuffles in place
//    of 32 x 6.  Every addition pairs the same two operands as wave_sum does at that offset (a + b and b + a are the same bits), so the
//    totals are wave_sum's.  One of the nine sums is folded at a time: at most 32 fp64 values in flight, not 288.
//  - The fold is W = 8, 16 or 32 candidates wide, the smallest that holds L: a branch on L that the whole grid takes the same way,
//    inside the one kernel.  A narrower fold selects and shuffles proportionally less; candidates from L on repeat the top and are
//    never written.
//  - The 64 / W lanes from lane c (64 / W) on end up with the totals of candidate c: plane_solve runs once for all candidates in parallel, as
//    lane s solves scale s in the 4-scale kernels.  The selection is one fmin butterfly and one ballot.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // query_centre, centre_lost; its ball_d2 is not used here

// every product and sum below is rounded on its own, like the list kernels of knn.hip whose bits step 2 restates
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"

namespace nesti {
namespace {

constexpr int kMaxL = NESTI_SELECT_MAX_L;
static_assert(kMaxL == 32 && kWave == 2 * kMaxL, "the widest fold leaves candidate c in lanes 2c and 2c + 1");

struct SelectParams {
  NbrParams np;                       // np.ks[*] = the top of the ladder; np.radius_out and np.count_out are not used
  int L;
  int ks[kMaxL];                      // the ladder; entries from L on repeat the top
  double slack;
  float* normals_out;                 // [M, 3]
  float* eig_out;                     // [M, 3]
  int32_t* sel_out;                   // [M]
  int32_t* k_out;                     // [M]
  float* radius_out;                  // [M]
  float* variation_all_out;           // [M, L]
  float* normals_all_out;             // [M, L, 3]
  float* eig_all_out;                 // [M, L, 3]
  float* radius_all_out;              // [M, L]
  int32_t* count_all_out;             // [M, L]
};

struct FoldAdd {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};
struct FoldMax {
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};

// The folded butterfly from the stage at offset OFF on.  While HALF >= 1: of the 2 HALF values a lane still holds it keeps HALF -- the
// upper ones where its bit OFF is set -- and combines each with the partner's value for the same candidate, own operand first as in
// wave_sum.  Once one value is left (HALF == 0) the remaining offsets are the plain butterfly.
template <int HALF, int OFF, int W, class Op>
__device__ __forceinline__ void fold_from(double (&v)[W], int lane, Op op) {
  if constexpr (HALF >= 1) {
    const bool hi = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
      const double a = v[i], b = v[i + HALF];
      const double keep = hi ? b : a, send = hi ? a : b;
      v[i] = op(keep, __shfl_xor(send, OFF, kWave));
    }
    fold_from<HALF / 2, OFF / 2>(v, lane, op);
  } else if constexpr (OFF >= 1) {
    v[0] = op(v[0], __shfl_xor(v[0], OFF, kWave));
    fold_from<0, OFF / 2>(v, lane, op);
  }
}
// The wave totals of v[c], c = 0 .. W - 1, each by the xor-butterfly of wave_sum / wave_max (offsets 32, 16, 8, 4, 2, 1): lane l returns
// the total of candidate l / (64 / W).
template <int W, class Op>
__device__ __forceinline__ double fold(double (&v)[W], int lane, Op op) {
  fold_from<W / 2, kWave / 2>(v, lane, op);
  return v[0];
}

// The totals of the nine sums and r2 of candidate lane / (64 / W), for a ladder of at most W counts: per candidate the lane's partial
// is the running sum behind its last slot below n_c (none: +0.0), and the partials of all candidates meet in one fold per sum.
template <int W>
__device__ __forceinline__ void candidate_totals(const int (&ks)[kMaxL], int prefix, int lane, const double (&run)[kNbrTrips][kSums],
                                                 const double (&rmax)[kNbrTrips], double (&sum)[kSums], double& r2) {
  static_assert(W == 8 || W == 16 || W == kMaxL, "a fold width");
  int mine[W];                          // how many of the lane's slots lie below n_c (0 .. 4; a slot that was not walked is never counted)
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const int nc = min(ks[c], prefix);
    mine[c] = max(0, min(kNbrTrips, (nc - lane + kWave - 1) >> 6));
  }
  double v[W];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
#pragma unroll
    for (int c = 0; c < W; ++c) {
      double x = 0.0;
#pragma unroll
      for (int t = 0; t < kNbrTrips; ++t) x = mine[c] == t + 1 ? run[t][k] : x;
      v[c] = x;
    }
    sum[k] = fold<W>(v, lane, FoldAdd{});
  }
#pragma unroll
  for (int c = 0; c < W; ++c) {
    double x = 0.0;
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t) x = mine[c] == t + 1 ? rmax[t] : x;
    v[c] = x;
  }
  r2 = fold<W>(v, lane, FoldMax{});
}

__device__ __forceinline__ double wave_fmin(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, kWave));
  return v;
}

__global__ __launch_bounds__(kThreads) void pca_select_kernel(const SelectParams sp) {
  const NbrParams& np = sp.np;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= np.p.M) return;                                    // whole waves leave: the shuffles below see full waves
  const float* centre = query_centre(np.p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const int L = sp.L;
  int j[kNbrTrips];
  const int prefix = nbr_row_upto(np, q, lane, centre_lost(cf0, cf1, cf2), sp.ks[kMaxL - 1], j);   // min(top of the ladder, valid prefix)
  // ---- the lane's running prefix sums: run[t] = ((0 + term of slot 0) + ...) + term of slot t, rmax[t] the largest d2 so far ---------
  double run[kNbrTrips][kSums], rmax[kNbrTrips];
#pragma unroll
  for (int t = 0; t < kNbrTrips; ++t) {
    rmax[t] = 0.0;
#pragma unroll
    for (int k = 0; k < kSums; ++k) run[t][k] = 0.0;
  }
  walk_list(np.p.cloud, j, prefix, lane, (double)cf0, (double)cf1, (double)cf2, [&](int i, double dx, double dy, double dz, double d2) {
    const PlaneTerms term = plane_terms(dx, dy, dz);
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t) {
      if (i == lane + t * kWave) {                            // known at compile time once walk_list is unrolled
        rmax[t] = fmax(t ? rmax[t ? t - 1 : 0] : 0.0, d2);
#pragma unroll
        for (int k = 0; k < kSums; ++k) run[t][k] = (t ? run[t ? t - 1 : 0][k] : 0.0) + term.v[k];
      }
    }
  });
  // ---- the totals of candidate lane >> shift: the narrowest fold that holds the ladder (L is the same for the whole grid) ---------------
  double sum[kSums], r2;
  int shift;
  if (L <= 8) {
    candidate_totals<8>(sp.ks, prefix, lane, run, rmax, sum, r2);
    shift = 3;
  } else if (L <= 16) {
    candidate_totals<16>(sp.ks, prefix, lane, run, rmax, sum, r2);
    shift = 2;
  } else {
    candidate_totals<kMaxL>(sp.ks, prefix, lane, run, rmax, sum, r2);
    shift = 1;
  }
  // ---- the lanes of candidate c solve it ---------------------------------------------------------------------------------------------------
  const int c = lane >> shift;
  int kc = 0;
#pragma unroll
  for (int i = 0; i < kMaxL; ++i) kc = c == i ? sp.ks[i] : kc;
  const int n = min(kc, prefix);
  const bool live = c < L;
  float nrm[3], ev[3];
  plane_solve(sum, (live && r2 > 0.0) ? n : 0, r2, nrm, ev);
  // ---- score and selection ---------------------------------------------------------------------------------------------------------------
  const double den = ((double)ev[0] + (double)ev[1]) + (double)ev[2];
  const bool eligible = live && n >= 3 && r2 > 0.0 && den > 0.0;
  const double var = eligible ? (double)ev[0] / den : 0.0;
  const double vmin = wave_fmin(eligible ? var : (double)INFINITY);
  const double thr = vmin + vmin * sp.slack;
  const unsigned long long pass = __ballot(eligible && var <= thr);
  const int sel = pass ? (63 - __builtin_clzll(pass)) >> shift : -1;   // the highest lane that passed holds the largest candidate
  // ---- outputs: the first lane of a candidate writes it -----------------------------------------------------------------------------------
  const float rad = (float)sqrt(r2);
  if (live && (lane & ((1 << shift) - 1)) == 0) {
    const size_t o = (size_t)q * L + c;
    if (sp.variation_all_out) sp.variation_all_out[o] = (float)var;
    if (sp.normals_all_out) { sp.normals_all_out[o * 3] = nrm[0]; sp.normals_all_out[o * 3 + 1] = nrm[1]; sp.normals_all_out[o * 3 + 2] = nrm[2]; }
    if (sp.eig_all_out) { sp.eig_all_out[o * 3] = ev[0]; sp.eig_all_out[o * 3 + 1] = ev[1]; sp.eig_all_out[o * 3 + 2] = ev[2]; }
    if (sp.radius_all_out) sp.radius_all_out[o] = rad;
    if (sp.count_all_out) sp.count_all_out[o] = n;
  }
  if (lane == (sel < 0 ? 0 : sel << shift)) {
    const bool none = sel < 0;
    const size_t o = (size_t)q;
    if (sp.normals_out) {
      sp.normals_out[o * 3] = none ? 0.f : nrm[0]; sp.normals_out[o * 3 + 1] = none ? 0.f : nrm[1]; sp.normals_out[o * 3 + 2] = none ? 0.f : nrm[2];
    }
    if (sp.eig_out) { sp.eig_out[o * 3] = none ? 0.f : ev[0]; sp.eig_out[o * 3 + 1] = none ? 0.f : ev[1]; sp.eig_out[o * 3 + 2] = none ? 0.f : ev[2]; }
    if (sp.sel_out) sp.sel_out[o] = sel;
    if (sp.k_out) sp.k_out[o] = none ? 0 : n;
    if (sp.radius_out) sp.radius_out[o] = none ? 0.f : rad;
  }
}

// nesti_pca_select_nbr and nesti_pca_select_nbr_at: one body
int select_impl(const char* who, bool at, const float* cloud_dev, int N, const int32_t* query_idx_dev, const float* query_xyz_dev, int M,
                int query_row0, const int32_t* nbr_dev, int K, const int32_t* ks, int L, double slack, float* normals_out_dev,
                float* eig_out_dev, int32_t* sel_out_dev, int32_t* k_out_dev, float* radius_out_dev, float* variation_all_out_dev,
                float* normals_all_out_dev, float* eig_all_out_dev, float* radius_all_out_dev, int32_t* count_all_out_dev, void* stream) {
  const std::string w(who);
  if (!cloud_dev || !nbr_dev || !ks) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (refuse_knn_k(w, K)) return 1;
  if (L < 1 || L > kMaxL) NESTI_FAIL(w + ": L must be in 1 .. " + std::to_string(kMaxL));
  for (int c = 0; c < L; ++c)
    if (ks[c] < 1 || ks[c] > K || (c && ks[c] <= ks[c - 1])) NESTI_FAIL(w + ": the ladder must be strictly ascending and in 1 .. K");
  if (!std::isfinite(slack) || slack < 0.0) NESTI_FAIL(w + ": slack must be finite and >= 0");
  SelectParams sp;
  const int32_t top[1] = {ks[L - 1]};
  // the rest of what the list fits refuse (M, the rows, the positions), and their parameter block
  if (nbr_params_fill(w, at, &sp.np, cloud_dev, N, query_idx_dev, query_xyz_dev, M, query_row0, nbr_dev, K, top, 1, nullptr, nullptr))
    return 1;
  if (M == 0) return 0;
  sp.L = L;
  for (int c = 0; c < kMaxL; ++c) sp.ks[c] = ks[c < L ? c : L - 1];
  sp.slack = slack;
  sp.normals_out = normals_out_dev;
  sp.eig_out = eig_out_dev;
  sp.sel_out = sel_out_dev;
  sp.k_out = k_out_dev;
  sp.radius_out = radius_out_dev;
  sp.variation_all_out = variation_all_out_dev;
  sp.normals_all_out = normals_all_out_dev;
  sp.eig_all_out = eig_all_out_dev;
  sp.radius_all_out = radius_all_out_dev;
  sp.count_all_out = count_all_out_dev;
  return launch_wave_rows(pca_select_kernel, sp, M, stream);
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_pca_select_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                         int K, const int32_t* ks, int L, double slack, float* normals_out_dev, float* eig_out_dev, int32_t* sel_out_dev,
                         int32_t* k_out_dev, float* radius_out_dev, float* variation_all_out_dev, float* normals_all_out_dev,
                         float* eig_all_out_dev, float* radius_all_out_dev, int32_t* count_all_out_dev, void* stream) {
  return select_impl("nesti_pca_select_nbr", false, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, L, slack,
                     normals_out_dev, eig_out_dev, sel_out_dev, k_out_dev, radius_out_dev, variation_all_out_dev, normals_all_out_dev,
                     eig_all_out_dev, radius_all_out_dev, count_all_out_dev, stream);
}

int nesti_pca_select_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                            const int32_t* ks, int L, double slack, float* normals_out_dev, float* eig_out_dev, int32_t* sel_out_dev,
                            int32_t* k_out_dev, float* radius_out_dev, float* variation_all_out_dev, float* normals_all_out_dev,
                            float* eig_all_out_dev, float* radius_all_out_dev, int32_t* count_all_out_dev, void* stream) {
  return select_impl("nesti_pca_select_nbr_at", true, cloud_dev, N, nullptr, query_xyz_dev, M, 0, nbr_dev, K, ks, L, slack,
                     normals_out_dev, eig_out_dev, sel_out_dev, k_out_dev, radius_out_dev, variation_all_out_dev, normals_all_out_dev,
                     eig_all_out_dev, radius_all_out_dev, count_all_out_dev, stream);
}

}  // extern "C"
