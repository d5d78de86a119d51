// The walk of an untrusted neighbour list by one wave (DESIGN.md 2 "k-nearest neighbourhoods"), shared by the list kernels of knn.hip
// (plane fit, quadric fit), by hough.hip, select.hip and robust.hip: the parameter block, the valid prefix of a row, the per-slot
// differences and what every list entry refuses on the host -- and the same row served by a group of 16 or 32 lanes, for the list
// passes of smooth.hip, denoise.hip and outlier.hip.  One definition, so the prefix, d, d2 and r2_s of every list entry are the same
// values.
//
// For the including unit: include patches_dev.h first, then `#pragma clang fp contract(off)`, then pca_dev.h and this header -- every
// product and sum below is rounded on its own.
#pragma once
#include "pca_dev.h"

namespace nesti {
namespace {

constexpr int kNbrTrips = NESTI_KNN_MAX_K / kWave;          // slots per lane of a neighbour list
static_assert(NESTI_KNN_MAX_K % kWave == 0, "a list is whole trips of the wave");

// (dx dx + dy dy) + dz dz in fp64, each operation rounded on its own (contraction is off in the including file)
__device__ __forceinline__ double knn_d2(double dx, double dy, double dz) {
  const double s = dx * dx + dy * dy;
  return s + dz * dz;
}

// the lanes of one wave see each other's LDS writes after this; waves of a workgroup run different queries and never meet
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- the cut of a wave's candidate pairs, shared by the grid search (knn.hip) and the image-window search (window.hip) ---------------
constexpr int kKnnCap = 1024;                               // pairs per wave
static_assert(NESTI_KNN_MAX_K + kWave <= kKnnCap, "a cut leaves room for the next trip");

// Sorts the wave's pairs [0, cnt) ascending by (d2, j) -- bitonic, over the next power of two >= 64, padded with (+inf, INT_MAX) -- and
// returns min(cnt, K), the number kept.  cnt <= kKnnCap, the same in every lane.
__device__ __forceinline__ int knn_cut(double* bd, int* bj, int cnt, int K, int lane) {
  int n2 = kWave;
  while (n2 < cnt) n2 <<= 1;
  for (int i = cnt + lane; i < n2; i += kWave) {
    bd[i] = INFINITY;
    bj[i] = 0x7fffffff;
  }
  wave_lds_fence();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int t = lane; t < (n2 >> 1); t += kWave) {
        const int a = ((t & ~(s - 1)) << 1) | (t & (s - 1)), b = a | s;
        const bool up = (a & k) == 0;
        const double da = bd[a], db = bd[b];
        const int ja = bj[a], jb = bj[b];
        const bool a_after_b = da > db || (da == db && ja > jb);
        if (a_after_b == up) {
          bd[a] = db; bd[b] = da;
          bj[a] = jb; bj[b] = ja;
        }
      }
      wave_lds_fence();
    }
  }
  return min(cnt, K);
}

struct NbrParams {
  PatchParams p;                      // cloud, query_idx / query_xyz, M, N, row0 (no grid)
  const int32_t* nbr;                 // [M, K]
  int K;
  int ks[NESTI_MAX_SCALES];           // ascending, 1 <= ks[s] <= K
  float* radius_out;                  // [M, S] or NULL
  int32_t* count_out;                 // [M, S] or NULL
};

// The list of row q: slot lane + 64 t into j[t] (0 where the slot is not used), and n[s] = min(ks[s], valid prefix) in every lane.
template <int S>
__device__ __forceinline__ void nbr_row(const NbrParams& np, int q, int lane, bool lost, int (&j)[kNbrTrips], int (&n)[S]) {
  const int kmax = np.ks[S - 1];
  int bad = lost ? 0 : kmax;                                  // the first slot whose entry lies outside [0, N)
#pragma unroll
  for (int t = 0; t < kNbrTrips; ++t) {
    const int i = lane + t * kWave;
    j[t] = 0;
    if (i < kmax) {
      const int v = np.nbr[(size_t)q * np.K + i];
      if ((unsigned)v >= (unsigned)np.p.N) bad = min(bad, i);
      else j[t] = v;
    }
  }
  bad = wave_min(bad);
#pragma unroll
  for (int s = 0; s < S; ++s) n[s] = min(np.ks[s], bad);
}

// nbr_row for a count that is not a template argument (select.hip: the top of a ladder): the slots below kmax into j[t] by the same
// reads and the same test; returns min(kmax, valid prefix) in every lane
__device__ __forceinline__ int nbr_row_upto(const NbrParams& np, int q, int lane, bool lost, int kmax, int (&j)[kNbrTrips]) {
  int bad = lost ? 0 : kmax;
#pragma unroll
  for (int t = 0; t < kNbrTrips; ++t) {
    const int i = lane + t * kWave;
    j[t] = 0;
    if (i < kmax) {
      const int v = np.nbr[(size_t)q * np.K + i];
      if ((unsigned)v >= (unsigned)np.p.N) bad = min(bad, i);
      else j[t] = v;
    }
  }
  return wave_min(bad);
}

// ---- a row by a GROUP of G lanes, G = 16, 32 or 64 (smooth.hip, denoise.hip, outlier.hip): 64 / G rows per wave, one per group -------
// The row of this lane's group and the lane within it.  G = 64 is wave_row(): the row stays in a scalar register.  The caller lets
// whole groups leave for q >= M, so every shuffle of the others stays inside a full group.
struct GroupRow {
  int q, sl;
};
template <int G>
__device__ __forceinline__ GroupRow group_row() {
  static_assert(G == 16 || G == 32 || G == kWave, "a lane group");
  const int lane = threadIdx.x & (kWave - 1);
  const int q = G == kWave ? wave_row() : (int)(blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6)) * (kWave / G) + lane / G;
  return {q, lane & (G - 1)};
}
// centre_lost (patches_dev.h) ties its argument to a scalar register: right for the wave's one row, not for a group's
template <int G>
__device__ __forceinline__ bool group_centre_lost(float x, float y, float z) {
  return G == kWave ? centre_lost(x, y, z) : !(finite_bits(x) && finite_bits(y) && finite_bits(z));
}
// nbr_row for a group: the slots of row q into j[] and min(ks[0], valid prefix), the same in every lane of the group.  G = 64 is
// nbr_row<1> as it stands; a smaller group holds the whole list in one trip -- the host picks G >= ks[0] (with_lane_group, group_dev.h)
template <int G>
__device__ __forceinline__ int group_nbr_row(const NbrParams& np, int q, int sl, bool lost, int (&j)[kNbrTrips]) {
  if constexpr (G == kWave) {
    int ns[1];
    nbr_row<1>(np, q, sl, lost, j, ns);
    return ns[0];
  } else {
    const int k = np.ks[0];
    int bad = lost ? 0 : k;
#pragma unroll
    for (int t = 0; t < kNbrTrips; ++t) j[t] = 0;
    if (sl < k) {
      const int v = np.nbr[(size_t)q * np.K + sl];
      if ((unsigned)v >= (unsigned)np.p.N) bad = sl;
      else j[0] = v;
    }
    return min(min(k, G), group_min<G>(bad));                 // k <= G; said so, the walk's trips beyond the first fall away
  }
}

// body(slot, dx, dy, dz, d2) for the slots lane, lane + 64, ... below n of the list: the walk of the list kernels
template <class Body>
__device__ __forceinline__ void walk_list(const float* cloud, const int (&j)[kNbrTrips], int n, int lane, double cx, double cy, double cz,
                                          Body&& body) {
#pragma unroll
  for (int t = 0; t < kNbrTrips; ++t) {
    const int i = lane + t * kWave;
    if (i < n) {
      const float* pt = cloud + (size_t)j[t] * 3;
      const double dx = (double)pt[0] - cx, dy = (double)pt[1] - cy, dz = (double)pt[2] - cz;
      body(i, dx, dy, dz, knn_d2(dx, dy, dz));
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

inline int refuse_knn_k(const std::string& w, int K) {
  if (K < 1 || K > NESTI_KNN_MAX_K) NESTI_FAIL(w + ": K must be in 1 .. " + std::to_string(NESTI_KNN_MAX_K));
  return 0;
}

// what the list entries refuse, under the entry's name, and their parameter block
inline int nbr_params_fill(const std::string& w, bool at, NbrParams* np, const float* cloud_dev, int N, const int32_t* query_idx_dev,
                           const float* query_xyz_dev, int M, int query_row0, const int32_t* nbr_dev, int K, const int32_t* ks, int S,
                           float* radius_out_dev, int32_t* count_out_dev) {
  if (!cloud_dev || !nbr_dev || !ks) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (refuse_knn_k(w, K)) return 1;
  if (S < 1 || S > NESTI_MAX_SCALES) NESTI_FAIL(w + ": bad n_scales");
  for (int s = 0; s < S; ++s)
    if (ks[s] < 1 || ks[s] > K || (s && ks[s] < ks[s - 1])) NESTI_FAIL(w + ": ks must be ascending and in 1 .. K");
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (refuse_query_rows(w, N, !at && !query_idx_dev, M, query_row0)) return 1;
  if (M > 0 && at && !query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev");
  memset(np, 0, sizeof(*np));
  np->p.cloud = cloud_dev;
  np->p.query_idx = query_idx_dev;
  np->p.query_xyz = at ? query_xyz_dev : nullptr;
  np->p.M = M; np->p.N = N; np->p.S = S; np->p.row0 = query_row0;
  np->nbr = nbr_dev;
  np->K = K;
  for (int s = 0; s < NESTI_MAX_SCALES; ++s) np->ks[s] = ks[s < S ? s : S - 1];
  np->radius_out = radius_out_dev;
  np->count_out = count_out_dev;
  return 0;
}

}  // namespace
}  // namespace nesti
