// Robust plane-fit normals over neighbour lists (DESIGN.md 2 "Robust plane fit"): an M-estimator of the plane through a neighbourhood,
// solved by iteratively re-weighted least squares -- the robust fits of Mederos et al. (2003), Fleishman et al. (2005) and the RIMLS of
// Oztireli et al. (2009) read as a normal estimator.  Residuals to the current plane down-weight the points of the other face of a
// crease, so the fit leans to one face where the plane fit averages both; the normal stays continuous (no bins, no triplets).  The
// conventions are the library's own (no parity with any published code is claimed): fp64 throughout, every operation rounded on its
// own, only + - x / sqrt, comparisons and integer arithmetic; tests/_robust_fixture.py predicts every byte.
//
// THE ENTRY (nesti_robust_normals_nbr, nesti_robust_normals_nbr_at).  Centres, the list nbr_dev [M, K], ks [S], the valid prefix, n_s, d,
// d2 and r2_s are exactly those of nesti_pca_normals_nbr (nbr_dev.h).  Per row and scale, over the first n = n_s slots:
//  0 START.  plane = the plane fit of nesti_pca_normals_nbr, bit for bit (always computed).  g = init[row, s] where an init is given, else
//    plane.  The row is 0 0 0 with iters_done, support, inliers and moments 0 if n < 3, r2 == 0, a d2 of the prefix is not finite, or g
//    is 0 0 0 or not finite.  Otherwise g is put under the sign rule (the first non-zero of (g_z, g_y, g_x) positive, on the f32 values).
//  ONE ITERATION from the f32 normal g:
//  1 v = (double)g / sqrt((g_x g_x + g_y g_y) + g_z g_z).
//  2 h_i = (v_x dx_i + v_y dy_i) + v_z dz_i; c = the element of rank n / 2 (0-based, ascending) of the h_i; res_i = h_i - c.
//  3 med = the element of rank n / 2 of the |res_i|; sig = max(sigma med, floor sqrt(r2)).
//  4 x_i = res_i / sig, t_i = 1 / (1 + x_i x_i), u_i = 1 - falloff (d2_i / r2), a_i = u_i t_i, w_i = a_i a_i.
//  5 Ten sums: sw = sum w_i and sum w_i T_i[k] for the nine terms T_i of the plane fit (plane_terms: d, then the six rounded products
//    xx xy xz yy yz zz).  Slot i is added in lane i mod 64, a lane adds its slots in ascending order from +0.0, each total goes through
//    the xor-butterfly of wave_sum.
//  6 plane_solve_mass with sw in the place of the count: the plane fit's solve, rounding and sign rule.
//  7 The iteration FAILS if not sw > 0, if fewer than 3 slots have w_i > 0, or if the new normal is 0 0 0 or not finite: g stays and the
//    row stops.
//  After `iters` iterations (or a failure) the output is g: the state between iterations is the f32 normal alone, so iters = T equals T
//  chained calls of iters = 1 through init, bit for bit.  iters = 0: (float)v of step 1, under the sign rule once more.
// DETERMINISM.  No atomics.  A row's bits are a pure function of (cloud, centre, list prefix, ks, the parameters, its init row).
//
// THE KERNEL.  One wave per row, four rows per workgroup, no LDS.  A lane owns at most kNbrTrips = 4 slots; their d and d2 are read
// once and stay in registers across scales and iterations.  Every total ends up in every lane (the butterfly), so every lane runs the
// same solve on the same values and the state g is wave-uniform: no lane is singled out, no value is broadcast.
//  - The two order statistics are exact and need no LDS and no shuffle: a double maps to a 64-bit key whose unsigned order is the order
//    of the values; the key of rank r is found bit by bit from the top (the largest T with #(key < T) <= r), each round one 64-bit
//    compare per owned slot whose ballot is counted on the scalar unit: at most 64 rounds of at most 4 ballots, and the rounds end
//    as soon as one key is left that shares the bits found so far (wave_rank_key).
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // query_centre, centre_lost; its ball_d2 is not used here

// every product and sum below is rounded on its own, like the list kernels of knn.hip whose plane fit step 0 restates
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"

namespace nesti {
namespace {

constexpr int kMoments = 1 + kSums;   // sw, then the nine weighted sums in the order of plane_terms

struct RobustParams {
  NbrParams np;
  int iters;
  double sigma, falloff, floor;
  const float* init;                  // [M, S, 3] or NULL: the start normals
  float* normals_out;                 // [M, S, 3]
  float* plane_out;                   // [M, S, 3]
  float* support_out;                 // [M, S]
  int32_t* inliers_out;               // [M, S]
  int32_t* iters_out;                 // [M, S]
  double* moments_out;                // [M, S, 10]
};

// a finite double -> a key whose unsigned order is the order of the values (-0 sorts below +0; they are equal values and either serves)
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double order_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// The key of 0-based rank r among the keys of the slots below n (key[t]: slot lane + 64 t; a slot from n on holds ~0 and is never
// counted), 0 <= r < n: the largest T with #(key < T) <= r, built from the top bit down.  Wave-uniform.  With the bits above b fixed
// to `have`, `lo` keys lie below have and `bucket` keys share those bits, lo <= r < lo + bucket; once one key is left in the bucket it is
// the answer and is read from its lane -- a neighbourhood's heights part within some twenty bits, so most of the 64 rounds never run.
// Equal keys never part: they take all 64 rounds and have is the answer.
__device__ __forceinline__ unsigned long long wave_rank_key(const unsigned long long (&key)[kNbrTrips], int n, int r, int lane) {
  unsigned long long have = 0;
  int lo = 0, bucket = n, b = 63;
#pragma unroll 1
  for (; b >= 0 && bucket > 1; --b) {
    const unsigned long long cand = have | (1ull << b);
    int below = 0;
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t)
      if (t * kWave < n) below += __popcll(__ballot(key[t] < cand));
    if (below <= r) {
      bucket -= below - lo;
      lo = below;
      have = cand;
    } else {
      bucket = below - lo;
    }
  }
  if (b >= 0) {                                               // bits b .. 0 are open and one key shares the fixed ones: fetch it
    const unsigned long long open = (2ull << b) - 1ull;       // b = 63 (n = 1): every bit, by wrap-around
    const unsigned long long fixed = have;
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t) {
      const unsigned long long hit = __ballot(lane + t * kWave < n && (key[t] & ~open) == fixed);
      if (hit) {
        const int src = __builtin_ctzll(hit);
        have = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(key[t] >> 32), src) << 32) |
               (unsigned)__builtin_amdgcn_readlane((int)key[t], src);
      }
    }
  }
  return have;
}

__device__ __forceinline__ bool f32_finite(float v) { return fabsf(v) < INFINITY; }

// the sign rule of the library on f32 values: the first non-zero of (z, y, x) positive, zeros +0
__device__ __forceinline__ void sign_rule(float (&g)[3]) {
  const float lead = g[2] != 0.f ? g[2] : (g[1] != 0.f ? g[1] : g[0]);
  if (lead < 0.f) { g[0] = -g[0]; g[1] = -g[1]; g[2] = -g[2]; }
  g[0] = g[0] + 0.f; g[1] = g[1] + 0.f; g[2] = g[2] + 0.f;
}

template <int S>
__global__ __launch_bounds__(kThreads) void robust_nbr_kernel(const RobustParams rp) {
  const NbrParams& np = rp.np;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= np.p.M) return;                                    // whole waves leave: the shuffles and ballots below see full waves
  const float* centre = query_centre(np.p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  int j[kNbrTrips], ns[S];
  nbr_row<S>(np, q, lane, centre_lost(cf0, cf1, cf2), j, ns);
  // ---- the lane's slots: read once, kept across scales and iterations ---------------------------------------------------------------
  double dx[kNbrTrips], dy[kNbrTrips], dz[kNbrTrips], d2[kNbrTrips];
#pragma unroll
  for (int t = 0; t < kNbrTrips; ++t) { dx[t] = 0.0; dy[t] = 0.0; dz[t] = 0.0; d2[t] = 0.0; }
  walk_list(np.p.cloud, j, ns[S - 1], lane, (double)cf0, (double)cf1, (double)cf2, [&](int i, double x, double y, double z, double dd) {
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t) {
      if (i == lane + t * kWave) { dx[t] = x; dy[t] = y; dz[t] = z; d2[t] = dd; }   // known at compile time once walk_list is unrolled
    }
  });
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int n = ns[s];
    // ---- step 0: the plane fit of the list kernel (plane_fit_nbr of knn.hip: the same terms in the same order), every total in every lane
    double acc[kSums], rmax = 0.0;
    bool wild = false;                                        // a d2 of the prefix that is not finite
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t) {
      if (lane + t * kWave < n) {
        rmax = fmax(rmax, d2[t]);
        plane_add(acc, plane_terms(dx[t], dy[t], dz[t]));
        wild = wild || !(d2[t] < (double)INFINITY);
      }
    }
    const double r2 = wave_max(rmax);
    double sum[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = wave_sum(acc[k]);
    float plane[3], ev[3];
    plane_solve(sum, r2 > 0.0 ? n : 0, r2, plane, ev);
    // ---- the start normal -----------------------------------------------------------------------------------------------------------
    const size_t o = (size_t)q * S + s;
    float g[3] = {plane[0], plane[1], plane[2]};
    if (rp.init) { g[0] = rp.init[o * 3]; g[1] = rp.init[o * 3 + 1]; g[2] = rp.init[o * 3 + 2]; }
    const bool start = f32_finite(g[0]) && f32_finite(g[1]) && f32_finite(g[2]) && (g[0] != 0.f || g[1] != 0.f || g[2] != 0.f);
    const bool fit = n >= 3 && r2 > 0.0 && __ballot(wild) == 0ull && start;
    double mom[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) mom[k] = 0.0;
    int done = 0, inliers = 0;
    if (!fit) {
      g[0] = 0.f; g[1] = 0.f; g[2] = 0.f;
    } else {
      sign_rule(g);
      const double rad = sqrt(r2);
#pragma unroll 1
      for (int it = 0; it < max(rp.iters, 1); ++it) {
        // ---- step 1 -----------------------------------------------------------------------------------------------------------------
        const double gx = (double)g[0], gy = (double)g[1], gz = (double)g[2];
        const double len = sqrt((gx * gx + gy * gy) + gz * gz);
        const double vx = gx / len, vy = gy / len, vz = gz / len;
        if (rp.iters == 0) {                                  // no iteration: the start normal, renormalised
          g[0] = (float)vx; g[1] = (float)vy; g[2] = (float)vz;
          sign_rule(g);
          break;
        }
        // ---- steps 2 and 3: heights, the two order statistics, the scale of the residuals ------------------------------------------------
        double res[kNbrTrips];
        unsigned long long key[kNbrTrips];
#pragma unroll
        for (int t = 0; t < kNbrTrips; ++t) {
          res[t] = (vx * dx[t] + vy * dy[t]) + vz * dz[t];
          key[t] = lane + t * kWave < n ? order_key(res[t]) : ~0ull;
        }
        const double c = order_value(wave_rank_key(key, n, n >> 1, lane));
#pragma unroll
        for (int t = 0; t < kNbrTrips; ++t) {
          res[t] = res[t] - c;
          key[t] = lane + t * kWave < n ? order_key(fabs(res[t])) : ~0ull;
        }
        const double med = order_value(wave_rank_key(key, n, n >> 1, lane));
        const double sig = fmax(rp.sigma * med, rp.floor * rad);
        // ---- steps 4 and 5: the weights and the ten sums ------------------------------------------------------------------------------
        double wacc[kMoments];
#pragma unroll
        for (int k = 0; k < kMoments; ++k) wacc[k] = 0.0;
        int heavy = 0, inside = 0;
#pragma unroll
        for (int t = 0; t < kNbrTrips; ++t) {
          const bool on = lane + t * kWave < n;
          double w = 0.0;
          if (on) {
            const double x = res[t] / sig;
            const double tt = 1.0 / (1.0 + x * x);
            const double u = 1.0 - rp.falloff * (d2[t] / r2);
            const double a = u * tt;
            w = a * a;
            const PlaneTerms term = plane_terms(dx[t], dy[t], dz[t]);
            wacc[0] += w;
#pragma unroll
            for (int k = 0; k < kSums; ++k) wacc[1 + k] += w * term.v[k];
          }
          if (t * kWave < n) {
            heavy += __popcll(__ballot(on && w > 0.0));
            inside += __popcll(__ballot(on && fabs(res[t]) <= sig));
          }
        }
        double tot[kMoments];
#pragma unroll
        for (int k = 0; k < kMoments; ++k) tot[k] = wave_sum(wacc[k]);
        // ---- steps 6 and 7 --------------------------------------------------------------------------------------------------------------
        if (!(tot[0] > 0.0) || heavy < 3) break;
        double wsum[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) wsum[k] = tot[1 + k];
        float nrm[3], wev[3];
        plane_solve_mass(wsum, tot[0], r2, nrm, wev);
        if (!(f32_finite(nrm[0]) && f32_finite(nrm[1]) && f32_finite(nrm[2])) || (nrm[0] == 0.f && nrm[1] == 0.f && nrm[2] == 0.f)) break;
        g[0] = nrm[0]; g[1] = nrm[1]; g[2] = nrm[2];
#pragma unroll
        for (int k = 0; k < kMoments; ++k) mom[k] = tot[k];
        inliers = inside;
        ++done;
      }
    }
    if (lane == 0) {
      if (rp.normals_out) { rp.normals_out[o * 3] = g[0]; rp.normals_out[o * 3 + 1] = g[1]; rp.normals_out[o * 3 + 2] = g[2]; }
      if (rp.plane_out) { rp.plane_out[o * 3] = plane[0]; rp.plane_out[o * 3 + 1] = plane[1]; rp.plane_out[o * 3 + 2] = plane[2]; }
      if (rp.support_out) rp.support_out[o] = (float)mom[0];
      if (rp.inliers_out) rp.inliers_out[o] = inliers;
      if (rp.iters_out) rp.iters_out[o] = done;
      if (rp.moments_out) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) rp.moments_out[o * kMoments + k] = mom[k];
      }
      if (np.radius_out) np.radius_out[o] = (float)sqrt(r2);
      if (np.count_out) np.count_out[o] = n;
    }
  }
}

// nesti_robust_normals_nbr and nesti_robust_normals_nbr_at: one body
int robust_nbr_impl(const char* who, bool at, const float* cloud_dev, int N, const int32_t* query_idx_dev, const float* query_xyz_dev,
                    int M, int query_row0, const int32_t* nbr_dev, int K, const int32_t* ks, int S, int iters, double sigma, double falloff,
                    double floor, const float* init_normals_dev, float* normals_out_dev, float* plane_out_dev, float* support_out_dev,
                    int32_t* inliers_out_dev, int32_t* iters_out_dev, double* moments_out_dev, float* radius_out_dev,
                    int32_t* count_out_dev, void* stream) {
  const std::string w(who);
  RobustParams rp;
  if (nbr_params_fill(w, at, &rp.np, cloud_dev, N, query_idx_dev, query_xyz_dev, M, query_row0, nbr_dev, K, ks, S, radius_out_dev,
                      count_out_dev))
    return 1;
  if (iters < 0 || iters > NESTI_ROBUST_MAX_ITERS) NESTI_FAIL(w + ": iters must be in 0 .. " + std::to_string(NESTI_ROBUST_MAX_ITERS));
  if (!(sigma > 0.0 && sigma <= 1e6)) NESTI_FAIL(w + ": sigma must be finite and in (0, 1e6]");
  if (!(falloff >= 0.0 && falloff <= 1.0)) NESTI_FAIL(w + ": falloff must be in [0, 1]");
  if (!(floor >= 1e-6 && floor <= 1.0)) NESTI_FAIL(w + ": floor must be in [1e-6, 1]");
  if (M == 0) return 0;
  rp.iters = iters;
  rp.sigma = sigma;
  rp.falloff = falloff;
  rp.floor = floor;
  rp.init = init_normals_dev;
  rp.normals_out = normals_out_dev;
  rp.plane_out = plane_out_dev;
  rp.support_out = support_out_dev;
  rp.inliers_out = inliers_out_dev;
  rp.iters_out = iters_out_dev;
  rp.moments_out = moments_out_dev;
  return with_scales(S, [&](auto s) { return launch_wave_rows(robust_nbr_kernel<decltype(s)::value>, rp, M, stream); });
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_robust_normals_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                             int K, const int32_t* ks, int S, int iters, double sigma, double falloff, double floor,
                             const float* init_normals_dev, float* normals_out_dev, float* plane_out_dev, float* support_out_dev,
                             int32_t* inliers_out_dev, int32_t* iters_out_dev, double* moments_out_dev, float* radius_out_dev,
                             int32_t* count_out_dev, void* stream) {
  return robust_nbr_impl("nesti_robust_normals_nbr", false, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, S, iters,
                         sigma, falloff, floor, init_normals_dev, normals_out_dev, plane_out_dev, support_out_dev, inliers_out_dev,
                         iters_out_dev, moments_out_dev, radius_out_dev, count_out_dev, stream);
}

int nesti_robust_normals_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                                const int32_t* ks, int S, int iters, double sigma, double falloff, double floor,
                                const float* init_normals_dev, float* normals_out_dev, float* plane_out_dev, float* support_out_dev,
                                int32_t* inliers_out_dev, int32_t* iters_out_dev, double* moments_out_dev, float* radius_out_dev,
                                int32_t* count_out_dev, void* stream) {
  return robust_nbr_impl("nesti_robust_normals_nbr_at", true, cloud_dev, N, nullptr, query_xyz_dev, M, 0, nbr_dev, K, ks, S, iters, sigma,
                         falloff, floor, init_normals_dev, normals_out_dev, plane_out_dev, support_out_dev, inliers_out_dev,
                         iters_out_dev, moments_out_dev, radius_out_dev, count_out_dev, stream);
}

}  // extern "C"
