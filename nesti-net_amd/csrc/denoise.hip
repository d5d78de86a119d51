// Point denoising over neighbour lists (DESIGN.md 2 "Point denoising"): one pass of the bilateral point filter of Fleishman, Drori and
// Cohen-Or, "Bilateral Mesh Denoising" (2003) and Digne and de Franchis, "The Bilateral Filter for Point Clouds" (2017) -- the
// projection step of Huang et al., "Edge-Aware Point Set Resampling" (2013), whose normal half is smooth.hip -- a row's point moves
// along its own normal by the weighted mean of its neighbours' heights over its tangent plane, the weight falling to zero where a
// neighbour's normal leaves a cone round the row's own (smoothing's cone weight) and with the height itself (the Geman-McClure weight
// of robust.hip), so a face is flattened and a crease is not rounded off -- with conventions of the library's own, chosen so that a
// restatement in plain IEEE arithmetic (tests/_denoise_fixture.py) predicts every output bit: fp64 throughout, every operation
// rounded on its own; only + - x / sqrt, comparisons and integer arithmetic.  It moves positions; normals are read, never written.
//
// THE PASS (nesti_denoise_points_nbr).  Centres (query_idx_dev / query_row0, M rows), the list nbr_dev [M, K] and its valid prefix are
// exactly as for nesti_smooth_normals_nbr (nbr_dev.h): the list is untrusted, the prefix ends at the first entry outside [0, N), a
// non-finite centre position has an empty prefix.  normals_in_dev [N, 3] f32 holds a normal for every cloud point, indexed like the
// cloud.  k in 1 .. K: the leading entries used; cos_t in [0, 0.999999], falloff in [0, 1], sigma in (0, 1e6] (the height scale in
// neighbourhood radii) and step in (0, 1], fp64 on the host.  There is no _at entry: a position that is not a cloud point has nothing
// to move.
//  1 ELIGIBILITY.  As in smoothing, on the bits: a normal is eligible iff its three components are finite and one is non-zero.
//    c = the centre's cloud index; p_c = cloud[c]; n_c = normals_in[c]; q_c = (x x + y y) + z z of n_c in fp64.  A row whose n_c is
//    not eligible, whose prefix is empty or whose centre is not finite moves nothing: the three floats of p_c are copied bit for bit,
//    delta, support and count are 0.
//  2 PREFIX.  n = min(k, valid prefix); d = (double)p - (double)c and d2 = (dx dx + dy dy) + dz dz per slot as the list fits form them;
//    r2 = the largest d2 of the prefix; rad = sqrt(r2).
//  3 CENTRE NORMAL.  v = (double)n_c / sqrt(q_c), component by component.
//  4 SLOT i < n with neighbour j = nbr[i], n_j = normals_in[j] eligible (an ineligible one adds nothing), q_j like q_c:
//      t: smoothing's step 3, the one cone_weight of group_dev.h -- dd = (n_c.x n_j.x + n_c.y n_j.y) + n_c.z n_j.z;
//      ca = |dd| / sqrt(q_c q_j);  t = (ca - cos_t) / (1 - cos_t);  if not t > 0 the slot adds nothing (NaN included);  t = min(t, 1);
//      u = 1 - (falloff d2) / r2 if r2 > 0, else u = 1;
//      h = (v.x dx + v.y dy) + v.z dz;  x = h / (sigma rad) if r2 > 0, else x = 0;  g = 1 / (1 + x x);
//      a = (u t) g;  W = a a;  H += W h;  Wsum += W;  cnt += 1 (integer).
//  5 ORDER.  Smoothing's step 4: lane l of a 64-lane wave adds its slots l, l + 64, ... in ascending order into partial sums that
//    start at +0.0; the lanes meet in wave_sum (pca_dev.h: xor offsets 32, 16, ..., 1).
//  6 RESULT.  If Wsum > 0 and delta = step (H / Wsum) is finite, the output is (float)((double)p_c + delta v) per component, the
//    product and the sum rounded separately; otherwise the input row is copied bit for bit and delta is 0 (support and count are
//    still the sums of step 4).
//  7 OUTPUTS (device; any may be NULL):  points_out_dev [M,3] f32;  delta_out_dev [M] f32 = (float)delta, the signed displacement
//    along the centre's normal;  support_out_dev [M] f32 = (float)Wsum;  count_out_dev [M] int32.
// DETERMINISM.  No atomics.  A row's bits are a pure function of (cloud, centre, list prefix, the normals it reads, k, cos_t, falloff,
// sigma, step): independent of batching, streams and the grid.  Every term is even in the sign of n_j and H is odd in the sign of
// n_c, as is v: the output position does not depend on the sign of any input normal, delta takes the sign of the centre's.  The pass
// is a Jacobi step -- rows read their neighbours' INPUT positions -- so the output must not lie inside the cloud.
//
// THE KERNEL.  The form of smooth_nbr_kernel: a dependent gather, list entry -> position (walk_list, which gives r2 before any weight
// is formed) -> normal.  A slot's d2 and h stay in registers between the two walks (v needs the centre's normal alone), so the list
// and the positions are read once.  A row is served by a GROUP of G lanes, the smallest of 16, 32 and 64 that holds k: 64 / G rows
// per wave, four waves per workgroup; groups never meet and whole groups leave for q >= M -- group_row, group_centre_lost and
// group_nbr_row of nbr_dev.h, the very definitions smooth_nbr_kernel runs.  No LDS, no scratch.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // query_centre, centre_lost, finite_bits; its ball_d2 is not used here

// every product and sum below is rounded on its own: the CPU restatement (tests/_denoise_fixture.py) predicts every bit
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"
#include "group_dev.h"

namespace nesti {
namespace {

struct DenoiseParams {
  NbrParams np;                       // np.ks[*] = k; np.radius_out and np.count_out are not used
  const float* normals_in;            // [N, 3]
  double cos_t, falloff, sigma, step;
  float* points_out;                  // [M, 3] or NULL
  float* delta_out;                   // [M] or NULL
  float* support_out;                 // [M] or NULL
  int32_t* count_out;                 // [M] or NULL
};

// G = 64: one row per wave.  G = 16, 32 (k <= G): 64 / G rows per wave, one per group of G lanes; a lane holds at most one slot, its
// partial sums are 0 + the slot's terms, and the butterfly of the group is the tail (offsets G / 2, ..., 1) of the wave's, whose head
// would add the +0.0 of lanes without a slot: the bytes of the 64-lane statement.
template <int G>
__global__ __launch_bounds__(kThreads) void denoise_nbr_kernel(const DenoiseParams dp) {
  constexpr int kTrips = G == kWave ? kNbrTrips : 1;          // slots per lane
  const NbrParams& np = dp.np;
  const GroupRow row = group_row<G>();
  const int q = row.q, sl = row.sl;                           // sl: the lane within its group
  if (q >= np.p.M) return;                                    // whole groups leave: the shuffles below stay inside a group
  const float* centre = query_centre(np.p, q);                // a cloud point: there is no positions form
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const double cx = cf0, cy = cf1, cz = cf2;
  const float* nc = dp.normals_in + (centre - np.p.cloud);    // the normal of the same (clamped) cloud index
  const float ncf0 = nc[0], ncf1 = nc[1], ncf2 = nc[2];
  int j[kNbrTrips];
  const int prefix = group_nbr_row<G>(np, q, sl, group_centre_lost<G>(cf0, cf1, cf2), j);
  const int n = eligible_normal(ncf0, ncf1, ncf2) ? prefix : 0;   // an ineligible centre normal walks nothing
  // ---- step 3: the centre's unit normal (n = 0: never used) ---------------------------------------------------------------------------
  const double ncx = ncf0, ncy = ncf1, ncz = ncf2;
  const double qc = knn_d2(ncx, ncy, ncz);
  const double lc = sqrt(qc);
  const double vx = ncx / lc, vy = ncy / lc, vz = ncz / lc;
  // ---- step 2: d2 and h of every slot, kept for step 4, and r2 ------------------------------------------------------------------------
  double d2s[kTrips], hs[kTrips], r2 = 0.0;
#pragma unroll
  for (int t = 0; t < kTrips; ++t) { d2s[t] = 0.0; hs[t] = 0.0; }
  walk_list(np.p.cloud, j, n, sl, cx, cy, cz, [&](int i, double dx, double dy, double dz, double d2) {
    const double h = (vx * dx + vy * dy) + vz * dz;
#pragma unroll
    for (int t = 0; t < kTrips; ++t)
      if (i == sl + t * kWave) { d2s[t] = d2; hs[t] = h; }
    r2 = fmax(r2, d2);
  });
  r2 = group_max<G>(r2);
  // ---- step 4: the slots of this lane, ascending ---------------------------------------------------------------------------------------
  const double span = 1.0 - dp.cos_t;
  const double hscale = dp.sigma * sqrt(r2);                  // sigma rad
  double H = 0.0, Wsum = 0.0;
  int cnt = 0;
#pragma unroll
  for (int t = 0; t < kTrips; ++t) {
    const int i = sl + t * kWave;
    if (i < n) {                                              // j[t] lies in [0, N): checked above
      const float* nj = dp.normals_in + (size_t)j[t] * 3;
      const ConeWeight c = cone_weight(ncx, ncy, ncz, qc, nj[0], nj[1], nj[2], dp.cos_t, span);
      if (c.counts) {
        const double u = cone_falloff(dp.falloff, d2s[t], r2);
        const double h = hs[t];
        const double x = r2 > 0.0 ? h / hscale : 0.0;
        const double g = 1.0 / (1.0 + x * x);
        const double a = (u * c.tt) * g;
        const double W = a * a;
        H = H + W * h;
        Wsum = Wsum + W;
        ++cnt;
      }
    }
  }
  H = group_sum<G>(H);
  Wsum = group_sum<G>(Wsum);
  cnt = group_sum<G>(cnt);
  // ---- step 6 ----------------------------------------------------------------------------------------------------------------------------
  float fx = cf0, fy = cf1, fz = cf2;                         // the input row, bit for bit
  double delta = 0.0;
  if (n > 0 && Wsum > 0.0) {
    const double dl = dp.step * (H / Wsum);
    if (fabs(dl) < INFINITY) {                                // false for NaN
      delta = dl;
      fx = (float)(cx + dl * vx); fy = (float)(cy + dl * vy); fz = (float)(cz + dl * vz);
    }
  }
  if (sl == 0) {
    if (dp.points_out) { dp.points_out[(size_t)q * 3] = fx; dp.points_out[(size_t)q * 3 + 1] = fy; dp.points_out[(size_t)q * 3 + 2] = fz; }
    if (dp.delta_out) dp.delta_out[q] = (float)delta;
    if (dp.support_out) dp.support_out[q] = n > 0 ? (float)Wsum : 0.f;
    if (dp.count_out) dp.count_out[q] = n > 0 ? cnt : 0;
  }
}

// nesti_debug_denoise_lanes: 0 = the smallest group that holds k
std::atomic<int> g_denoise_lanes{0};

// [a, a + na) and [b, b + nb) share a byte, or b lies inside [a, a + na) (an empty range still has a place)
inline bool ranges_meet(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return (b0 >= a0 && b0 - a0 < std::max(na, (size_t)1)) || (a0 >= b0 && a0 - b0 < std::max(nb, (size_t)1));
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_denoise_points_nbr(const float* cloud_dev, int N, const float* normals_in_dev, const int32_t* query_idx_dev, int M,
                             int query_row0, const int32_t* nbr_dev, int K, int k, double cos_t, double falloff, double sigma,
                             double step, float* points_out_dev, float* delta_out_dev, float* support_out_dev, int32_t* count_out_dev,
                             void* stream) {
  const std::string w("nesti_denoise_points_nbr");
  DenoiseParams dp;
  const int32_t ks[1] = {k};
  if (refuse_knn_k(w, K)) return 1;
  if (k < 1 || k > K) NESTI_FAIL(w + ": k must be in 1 .. K");
  if (nbr_params_fill(w, false, &dp.np, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, 1, nullptr, nullptr)) return 1;
  if (!normals_in_dev) NESTI_FAIL(w + ": null normals_in_dev");
  if (!std::isfinite(cos_t) || cos_t < 0.0 || cos_t > 0.999999) NESTI_FAIL(w + ": cos_t must be finite and in [0, 0.999999]");
  if (!std::isfinite(falloff) || falloff < 0.0 || falloff > 1.0) NESTI_FAIL(w + ": falloff must be finite and in [0, 1]");
  if (!std::isfinite(sigma) || !(sigma > 0.0) || sigma > 1e6) NESTI_FAIL(w + ": sigma must be finite and in (0, 1e6]");
  if (!std::isfinite(step) || !(step > 0.0) || step > 1.0) NESTI_FAIL(w + ": step must be finite and in (0, 1]");
  if (points_out_dev && ranges_meet(cloud_dev, (size_t)N * 3 * sizeof(float), points_out_dev, (size_t)M * 3 * sizeof(float)))
    NESTI_FAIL(w + ": points_out_dev must not lie inside the cloud (a Jacobi step: rows read their neighbours' input positions)");
  if (M == 0) return 0;
  dp.normals_in = normals_in_dev;
  dp.cos_t = cos_t;
  dp.falloff = falloff;
  dp.sigma = sigma;
  dp.step = step;
  dp.points_out = points_out_dev;
  dp.delta_out = delta_out_dev;
  dp.support_out = support_out_dev;
  dp.count_out = count_out_dev;
  // the lane group: the smallest of 16, 32, 64 that holds k, or a wider one asked for (nesti_debug_denoise_lanes)
  return with_lane_group(k, g_denoise_lanes.load(std::memory_order_relaxed), [&](auto g) {
    return launch_group_rows<decltype(g)::value>(denoise_nbr_kernel<decltype(g)::value>, dp, M, stream);
  });
}

int nesti_debug_denoise_lanes(int lanes) { return set_lane_group("nesti_debug_denoise_lanes", g_denoise_lanes, lanes); }

}  // extern "C"
