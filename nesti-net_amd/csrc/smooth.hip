// Feature-preserving normal smoothing over neighbour lists (DESIGN.md 2 "Normal smoothing"): one pass of a bilateral filter of
// normals after Jones, Durand and Zwicker, "Normal Improvement for Point Rendering" (2004), Sun et al., "Fast and Effective
// Feature-Preserving Mesh Denoising" (2007) and the anisotropic normal smoothing of Huang et al., "Edge-Aware Point Set Resampling"
// (2013) -- a row's normal becomes the weighted mean of its neighbours' normals, the weight falling to zero where a neighbour's normal
// leaves a cone round the row's own, so rows agree along a face and not across a crease -- with conventions of the library's own,
// chosen so that a restatement in plain IEEE arithmetic (tests/_smooth_fixture.py) predicts every output bit: fp64 throughout, every
// operation rounded on its own; only + - x / sqrt, comparisons and integer arithmetic.  It filters normals; positions never move.
//
// THE PASS (nesti_smooth_normals_nbr).  Centres (query_idx_dev / query_row0, M rows), the list nbr_dev [M, K] and its valid prefix are
// exactly as for nesti_pca_normals_nbr (nbr_dev.h): the list is untrusted, the prefix ends at the first entry outside [0, N), a
// non-finite centre position has an empty prefix.  normals_in_dev [N, 3] f32 holds a normal for every cloud point, indexed like the
// cloud.  k in 1 .. K: the leading entries used; cos_t in [0, 0.999999] and falloff in [0, 1], fp64 on the host.  There is no _at
// entry: a position has no normal of its own to compare with.
//  1 ELIGIBILITY.  A normal is eligible iff its three components are finite and one is non-zero, tested on the bits (orient.hip's
//    rule).  c = the centre's cloud index; n_c = normals_in[c]; q_c = (x x + y y) + z z of n_c in fp64.  A row whose n_c is not
//    eligible, or whose prefix is empty, gets the three floats of normals_in[c] copied bit for bit, support 0 and count 0.
//  2 PREFIX.  n = min(k, valid prefix); d = (double)p - (double)c and d2 = (dx dx + dy dy) + dz dz per slot as the list fits form them;
//    r2 = the largest d2 of the prefix.
//  3 SLOT i < n with neighbour j = nbr[i], n_j = normals_in[j] eligible (an ineligible one adds nothing), q_j like q_c:
//      d = (n_c.x n_j.x + n_c.y n_j.y) + n_c.z n_j.z;  ca = |d| / sqrt(q_c q_j);  t = (ca - cos_t) / (1 - cos_t);
//      if not t > 0 the slot adds nothing (NaN included);  t = min(t, 1);
//      u = 1 - (falloff d2) / r2 if r2 > 0, else u = 1;  W = (u u) (t t);  g = W / sqrt(q_j), negated if d < 0 (the unoriented
//      alignment: a neighbour counts on the centre's side);  X += g n_j.x, Y += g n_j.y, Z += g n_j.z;  Wsum += W;  cnt += 1 (integer).
//  4 ORDER.  Lane l of a 64-lane wave adds its slots l, l + 64, ... in ascending order into partial sums that start at +0.0; the lanes
//    meet in wave_sum (pca_dev.h: xor offsets 32, 16, ..., 1) -- the order of the other list fits.
//  5 RESULT.  nn = (X X + Y Y) + Z Z; if nn > 0 and finite the output is (X, Y, Z) / sqrt(nn), rounded to f32 once, zeros written as
//    +0; otherwise the input row is copied bit for bit (support and count are still the sums of step 3).  No sign rule: every term lies
//    in the centre's closed half-space, so an oriented field stays oriented and an unoriented one keeps each row's side.
//  6 OUTPUTS (device; any may be NULL):  normals_out_dev [M,3] f32;  support_out_dev [M] f32 = (float)Wsum;  count_out_dev [M] int32.
// DETERMINISM.  No atomics.  A row's bits are a pure function of (cloud, centre, list prefix, the normals it reads, k, cos_t, falloff):
// independent of batching, streams and the grid.  The pass is a Jacobi step -- rows read their neighbours' INPUT normals -- so the
// output must not be the input.
//
// THE KERNEL.  The pass is a dependent gather: list entry -> position (walk_list, which also gives r2 before any weight is formed) ->
// normal.  The slot's d2 stays in registers between the two, so the list and the positions are read once.  At the working point
// k = 16 .. 32 one wave per row would leave most lanes without a slot, so a row is served by a GROUP of G lanes, the smallest of 16, 32
// and 64 that holds k: 64 / G rows per wave, four waves per workgroup; groups never meet (every shuffle stays inside one) and whole
// groups leave for q >= M.  G = 64 is the one-wave-per-row form of pca_nbr_kernel, over nbr_row and walk_list as they stand; a smaller
// group forms the prefix of its one trip itself (group_nbr_row, nbr_dev.h) and walks it with the same walk_list.  No LDS, no scratch.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // query_centre, centre_lost, finite_bits; its ball_d2 is not used here

// every product and sum below is rounded on its own: the CPU restatement (tests/_smooth_fixture.py) predicts every bit
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"
#include "group_dev.h"

namespace nesti {
namespace {

struct SmoothParams {
  NbrParams np;                       // np.ks[*] = k; np.radius_out and np.count_out are not used
  const float* normals_in;            // [N, 3]
  double cos_t, falloff;
  float* normals_out;                 // [M, 3] or NULL
  float* support_out;                 // [M] or NULL
  int32_t* count_out;                 // [M] or NULL
};

// eligible_normal, cone_weight and the host side of a lane group: group_dev.h; its row and list: nbr_dev.h; its reductions: wave_dev.h

// G = 64: one row per wave.  G = 16, 32 (k <= G): 64 / G rows per wave, one per group of G lanes; a lane holds at most one slot, its
// partial sums are 0 + the slot's terms, and the butterfly of the group is the tail (offsets G / 2, ..., 1) of the wave's, whose head
// would add the +0.0 of lanes without a slot: the bytes of the 64-lane statement.
template <int G>
__global__ __launch_bounds__(kThreads) void smooth_nbr_kernel(const SmoothParams sp) {
  constexpr int kTrips = G == kWave ? kNbrTrips : 1;          // slots per lane
  const NbrParams& np = sp.np;
  const GroupRow row = group_row<G>();
  const int q = row.q, sl = row.sl;                           // sl: the lane within its group
  if (q >= np.p.M) return;                                    // whole groups leave: the shuffles below stay inside a group
  const float* centre = query_centre(np.p, q);                // a cloud point: there is no positions form
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const double cx = cf0, cy = cf1, cz = cf2;
  const float* nc = sp.normals_in + (centre - np.p.cloud);    // the normal of the same (clamped) cloud index
  const float ncf0 = nc[0], ncf1 = nc[1], ncf2 = nc[2];
  int j[kNbrTrips];
  const int prefix = group_nbr_row<G>(np, q, sl, group_centre_lost<G>(cf0, cf1, cf2), j);
  const int n = eligible_normal(ncf0, ncf1, ncf2) ? prefix : 0;   // an ineligible centre normal walks nothing
  // ---- step 2: d2 of every slot, kept for step 3, and r2 -----------------------------------------------------------------------------
  double d2s[kTrips], r2 = 0.0;
#pragma unroll
  for (int t = 0; t < kTrips; ++t) d2s[t] = 0.0;
  walk_list(np.p.cloud, j, n, sl, cx, cy, cz, [&](int i, double, double, double, double d2) {
#pragma unroll
    for (int t = 0; t < kTrips; ++t)
      if (i == sl + t * kWave) d2s[t] = d2;
    r2 = fmax(r2, d2);
  });
  r2 = group_max<G>(r2);
  // ---- step 3: the slots of this lane, ascending ---------------------------------------------------------------------------------------
  const double ncx = ncf0, ncy = ncf1, ncz = ncf2;
  const double qc = knn_d2(ncx, ncy, ncz);
  const double span = 1.0 - sp.cos_t;
  double X = 0.0, Y = 0.0, Z = 0.0, Wsum = 0.0;
  int cnt = 0;
#pragma unroll
  for (int t = 0; t < kTrips; ++t) {
    const int i = sl + t * kWave;
    if (i < n) {                                              // j[t] lies in [0, N): checked above
      const float* nj = sp.normals_in + (size_t)j[t] * 3;
      const ConeWeight c = cone_weight(ncx, ncy, ncz, qc, nj[0], nj[1], nj[2], sp.cos_t, span);
      if (c.counts) {
        const double u = cone_falloff(sp.falloff, d2s[t], r2);
        const double W = (u * u) * (c.tt * c.tt);
        double g = W / sqrt(c.qj);
        if (c.dd < 0.0) g = -g;
        X = X + g * c.nx; Y = Y + g * c.ny; Z = Z + g * c.nz;
        Wsum = Wsum + W;
        ++cnt;
      }
    }
  }
  X = group_sum<G>(X); Y = group_sum<G>(Y); Z = group_sum<G>(Z);
  Wsum = group_sum<G>(Wsum);
  cnt = group_sum<G>(cnt);
  // ---- step 5 ----------------------------------------------------------------------------------------------------------------------------
  const double nn = (X * X + Y * Y) + Z * Z;
  float fx = ncf0, fy = ncf1, fz = ncf2;                      // the input row, bit for bit
  if (n > 0 && nn > 0.0 && nn < INFINITY) {
    const double len = sqrt(nn);
    fx = (float)(X / len) + 0.f; fy = (float)(Y / len) + 0.f; fz = (float)(Z / len) + 0.f;   // -0 + +0 = +0: no negative zero leaves
  }
  if (sl == 0) {
    if (sp.normals_out) { sp.normals_out[(size_t)q * 3] = fx; sp.normals_out[(size_t)q * 3 + 1] = fy; sp.normals_out[(size_t)q * 3 + 2] = fz; }
    if (sp.support_out) sp.support_out[q] = n > 0 ? (float)Wsum : 0.f;
    if (sp.count_out) sp.count_out[q] = n > 0 ? cnt : 0;
  }
}

// nesti_debug_smooth_lanes: 0 = the smallest group that holds k
std::atomic<int> g_smooth_lanes{0};

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_smooth_normals_nbr(const float* cloud_dev, int N, const float* normals_in_dev, const int32_t* query_idx_dev, int M,
                             int query_row0, const int32_t* nbr_dev, int K, int k, double cos_t, double falloff, float* normals_out_dev,
                             float* support_out_dev, int32_t* count_out_dev, void* stream) {
  const std::string w("nesti_smooth_normals_nbr");
  SmoothParams sp;
  const int32_t ks[1] = {k};
  if (refuse_knn_k(w, K)) return 1;
  if (k < 1 || k > K) NESTI_FAIL(w + ": k must be in 1 .. K");
  if (nbr_params_fill(w, false, &sp.np, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, 1, nullptr, nullptr)) return 1;
  if (!normals_in_dev) NESTI_FAIL(w + ": null normals_in_dev");
  if (!std::isfinite(cos_t) || cos_t < 0.0 || cos_t > 0.999999) NESTI_FAIL(w + ": cos_t must be finite and in [0, 0.999999]");
  if (!std::isfinite(falloff) || falloff < 0.0 || falloff > 1.0) NESTI_FAIL(w + ": falloff must be finite and in [0, 1]");
  if (normals_out_dev == normals_in_dev)
    NESTI_FAIL(w + ": normals_out_dev must not be normals_in_dev (a Jacobi step: rows read their neighbours' input)");
  if (M == 0) return 0;
  sp.normals_in = normals_in_dev;
  sp.cos_t = cos_t;
  sp.falloff = falloff;
  sp.normals_out = normals_out_dev;
  sp.support_out = support_out_dev;
  sp.count_out = count_out_dev;
  // the lane group: the smallest of 16, 32, 64 that holds k, or a wider one asked for (nesti_debug_smooth_lanes)
  return with_lane_group(k, g_smooth_lanes.load(std::memory_order_relaxed), [&](auto g) {
    return launch_group_rows<decltype(g)::value>(smooth_nbr_kernel<decltype(g)::value>, sp, M, stream);
  });
}

int nesti_debug_smooth_lanes(int lanes) { return set_lane_group("nesti_debug_smooth_lanes", g_smooth_lanes, lanes); }

}  // extern "C"
