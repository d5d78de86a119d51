// Outlier removal before estimation (DESIGN.md 2 "Outlier removal"): the two textbook filters of a point cloud -- statistical (a row
// leaves when the mean distance to its k nearest other points exceeds the cloud's mean of that figure by std_ratio standard deviations;
// Rusu et al., "Towards 3D Point Cloud Based Object Maps for Household Environments", 2008) and radius (a row leaves when fewer than
// min_neighbours other points lie within a radius) -- as three passes over the sorted lists nesti_knn returns: scores per row, the
// statistics of a score array, an ordered compaction.  The conventions are the library's own, chosen so that a restatement in plain
// IEEE arithmetic (tests/_outliers_fixture.py) predicts every output bit: fp64 throughout, every operation rounded on its own; only
// + - x / sqrt, comparisons and integer arithmetic; no atomics.  No parity with any published code is claimed.
//
// SCORES (nesti_outlier_scores_nbr).  Row q is cloud point c = query_row0 + q; nbr_dev [M, K] is untrusted, as for the list fits
// (nbr_dev.h): P = min(k + 1, valid prefix), the prefix ending at the first entry outside [0, N); d = (double)p - (double)c and
// d2 = (dx dx + dy dy) + dz dz per slot as nesti_knn forms them.  Of the slots below P the first one whose INDEX is c is skipped (the
// index, not d2 == 0: duplicates tie and sort by index); where none is, the slots below min(k, P) are used.  n_other = the slots used.
//   mean   = (sum of sqrt(d2) over the used slots) / n_other;  +inf where n_other == 0
//   kth_d2 = the largest d2 used where n_other == k, else +inf
// The sum has the list fits' order: slot i is added in lane i mod 64, a lane's slots ascending from +0.0, the lanes meet in the xor
// butterfly 32 .. 1.  Every term is >= +0, so a skipped slot and an idle lane change no bit -- which is why a row may be served by a
// GROUP of 16, 32 or 64 lanes, the smallest that holds k + 1 (group_row of nbr_dev.h), with the bytes of the 64-lane statement.  A used
// slot whose d2 is NaN (a cloud point with a NaN coordinate, in a list of the caller's) makes mean and kth_d2 the canonical quiet NaN
// (0x7ff8000000000000); so does a centre with a non-finite coordinate, whose n_other is 0.
//
// STATISTICS (nesti_outlier_threshold).  A non-finite score (tested on the bits) is absent: value +0, count 0.  Blocks of 256
// consecutive rows are reduced in LDS by stride halving (128, 64, .. 1: v[t] = v[t] + v[t + s]); ONE workgroup of 256 then reduces the
// block partials -- thread t adds partials t, t + 256, .. in ascending order to +0.0, then the same stride halving.  Pass 1: S, n,
// mean = S / n.  Pass 2: Q = the sum of (s - mean)(s - mean) by the same tree.  std = sqrt(Q / (n - 1)) for n >= 2, else 0;
// thr = mean + std_ratio std.  n == 0: mean = std = 0, thr = +inf.  Four launches, nothing read back.
//
// COMPACTION (nesti_outlier_compact).  A row is kept iff its score is finite and <= the threshold (a tie stays; NaN and +-inf leave).
// Per-block counts (ballot / popcount in a wave, LDS across waves), one single-workgroup scan of the block counts, a scatter in row
// order: compact_dev.h, shared with depth.hip and voxel.hip.  No atomics, no workgroup waits on another: kept_idx is ascending.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // query_centre, centre_lost, finite_bits; its ball_d2 is not used here

// every product and sum below is rounded on its own: the CPU restatement (tests/_outliers_fixture.py) predicts every bit
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"
#include "group_dev.h"
#include "compact_dev.h"

namespace nesti {
namespace {

constexpr unsigned long long kQuietNaN = 0x7ff8000000000000ull;

__device__ __forceinline__ bool finite_bits64(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// ---- scores ----------------------------------------------------------------------------------------------------------------------------
struct ScoreParams {
  NbrParams np;                       // np.ks[*] = k + 1; np.radius_out and np.count_out are not used
  int k;
  double* mean_out;                   // [M] or NULL
  double* kth_out;                    // [M] or NULL
  int32_t* n_other_out;               // [M] or NULL
};

// G = 64: one row per wave.  G = 16, 32 (k + 1 <= G): 64 / G rows per wave, one per group of G lanes; a lane holds at most one slot and
// the butterfly of the group is the tail (offsets G / 2, .., 1) of the wave's, whose head would add the +0.0 of lanes without a slot.
// The group's row and list: group_row, group_centre_lost, group_nbr_row (nbr_dev.h), shared with smooth.hip and denoise.hip.
template <int G>
__global__ __launch_bounds__(kThreads) void outlier_scores_kernel(const ScoreParams sp) {
  const NbrParams& np = sp.np;
  const GroupRow row = group_row<G>();
  const int q = row.q, sl = row.sl;                           // sl: the lane within its group
  if (q >= np.p.M) return;                                    // whole groups leave: the shuffles below stay inside a group
  const int own = np.p.row0 + q;                              // in [0, N): refused on the host otherwise
  const float* centre = np.p.cloud + (size_t)own * 3;
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const double cx = cf0, cy = cf1, cz = cf2;
  const bool lost = group_centre_lost<G>(cf0, cf1, cf2);
  const int k = sp.k;
  int j[kNbrTrips];
  const int P = group_nbr_row<G>(np, q, sl, lost, j);         // min(k + 1, valid prefix): np.ks[0] = k + 1
  // the first slot below P that holds the row's own index (kNone: absent)
  constexpr int kNone = NESTI_KNN_MAX_K;
  int self = kNone;
#pragma unroll
  for (int t = 0; t < (G == kWave ? kNbrTrips : 1); ++t) {
    const int i = sl + t * kWave;
    if (i < P && j[t] == own) self = min(self, i);
  }
  self = group_min<G>(self);
  const int limit = self != kNone ? P : min(k, P);            // slots below limit are used, but for slot `self`
  const int n_other = self != kNone ? P - 1 : limit;
  double sum = 0.0, top = 0.0;
  walk_list(np.p.cloud, j, limit, sl, cx, cy, cz, [&](int i, double, double, double, double d2) {
    if (i != self) {
      sum = sum + sqrt(d2);
      top = fmax(top, d2);                                    // a NaN d2 is caught through the sum below
    }
  });
  sum = group_sum<G>(sum);
  top = group_max<G>(top);
  double mean = n_other > 0 ? sum / (double)n_other : (double)INFINITY;
  double kth = n_other == k ? top : (double)INFINITY;
  int n_out = n_other;
  if (lost || sum != sum) {
    mean = __longlong_as_double((long long)kQuietNaN);
    kth = mean;
    if (lost) n_out = 0;
  }
  if (sl == 0) {
    if (sp.mean_out) sp.mean_out[q] = mean;
    if (sp.kth_out) sp.kth_out[q] = kth;
    if (sp.n_other_out) sp.n_other_out[q] = n_out;
  }
}

// nesti_debug_outlier_lanes: 0 = the smallest group that holds k + 1
std::atomic<int> g_outlier_lanes{0};

// ---- statistics --------------------------------------------------------------------------------------------------------------------------
struct OutlierLayout {
  size_t part_sum, part_cnt, block_cnt, total;
};
inline OutlierLayout outlier_layout(size_t n) {
  OutlierLayout L;
  size_t o = 0;
  L.part_sum = o; o += align_up(blocks_of(n) * 8, 256);
  L.part_cnt = o; o += align_up(blocks_of(n) * 4, 256);
  L.block_cnt = o; o += align_up(blocks_of(n) * 4, 256);
  L.total = o;
  return L;
}

// stride halving over the 256 values of a workgroup: v[t] = v[t] + v[t + s] for s = 128, 64, .., 1; the total in v[0] after the call
__device__ __forceinline__ void block_halving(double* v, int* c) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      v[t] = v[t] + v[t + s];
      c[t] += c[t + s];
    }
    __syncthreads();
  }
}

// SQUARES = false: the present scores themselves; true: (s - mean)(s - mean) with mean = stats[1] of pass 1
template <bool SQUARES>
__global__ __launch_bounds__(kThreads) void outlier_partial_kernel(const double* __restrict__ scores, int M, const double* __restrict__ stats,
                                                                   double* __restrict__ part_sum, int32_t* __restrict__ part_cnt) {
  __shared__ double v[kThreads];
  __shared__ int c[kThreads];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  double val = 0.0;
  int cnt = 0;
  if (i < M) {
    const double s = scores[i];
    if (finite_bits64(s)) {
      cnt = 1;
      if (SQUARES) {
        const double e = s - stats[1];
        val = e * e;
      } else {
        val = s;
      }
    }
  }
  v[threadIdx.x] = val;
  c[threadIdx.x] = cnt;
  block_halving(v, c);
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = v[0];
    part_cnt[blockIdx.x] = c[0];
  }
}

// ONE workgroup: the block partials -> the total, then the statistics.  stats = {n, mean, std, thr}
template <bool SQUARES>
__global__ __launch_bounds__(kThreads) void outlier_final_kernel(const double* __restrict__ part_sum, const int32_t* __restrict__ part_cnt,
                                                                 int nb, double std_ratio, double* __restrict__ stats) {
  __shared__ double v[kThreads];
  __shared__ int c[kThreads];
  double acc = 0.0;
  int cnt = 0;
  for (int b = threadIdx.x; b < nb; b += kThreads) {
    acc = acc + part_sum[b];
    cnt += part_cnt[b];
  }
  v[threadIdx.x] = acc;
  c[threadIdx.x] = cnt;
  block_halving(v, c);
  if (threadIdx.x != 0) return;
  const int n = c[0];
  if (!SQUARES) {
    stats[0] = (double)n;
    stats[1] = n > 0 ? v[0] / (double)n : 0.0;
  } else {
    const double sd = n >= 2 ? sqrt(v[0] / (double)(n - 1)) : 0.0;
    const double scaled = std_ratio * sd;
    stats[2] = sd;
    stats[3] = n > 0 ? stats[1] + scaled : (double)INFINITY;
  }
}

// ---- ordered compaction: count per block, one scan, scatter (block_rank and compact_scan_kernel: compact_dev.h) ----------------------
struct CompactParams {
  const float* cloud;                 // [N, 3]; NULL with xyz_out NULL
  const double* scores;               // [N]
  const double* thr_dev;              // or NULL: thr
  double thr;
  int N;
  float* xyz_out;
  int32_t* kept_idx_out;
  int32_t* new_of_old_out;
  uint8_t* keep_out;
};

__device__ __forceinline__ bool row_kept(const CompactParams& p, long long i) {
  if (i >= p.N) return false;
  const double s = p.scores[i];
  const double thr = p.thr_dev ? *p.thr_dev : p.thr;
  return finite_bits64(s) && s <= thr;
}

__global__ __launch_bounds__(kThreads) void outlier_count_kernel(const CompactParams p, int32_t* __restrict__ block_count) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  int total;
  block_rank(row_kept(p, i), &total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void outlier_scatter_kernel(const CompactParams p, const int32_t* __restrict__ block_start) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool pred = row_kept(p, i);
  int total;
  const int pos = block_start[blockIdx.x] + block_rank(pred, &total);     // < the number of kept rows <= N
  if (i >= p.N) return;
  if (p.keep_out) p.keep_out[i] = pred ? 1 : 0;
  if (p.new_of_old_out) p.new_of_old_out[i] = pred ? pos : -1;
  if (!pred) return;
  if (p.kept_idx_out) p.kept_idx_out[pos] = (int32_t)i;
  if (p.xyz_out) {                                          // a bit copy: -0.0 stays -0.0, a payload stays a payload
    const uint32_t* src = (const uint32_t*)p.cloud + (size_t)i * 3;
    uint32_t* dst = (uint32_t*)p.xyz_out + (size_t)pos * 3;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  }
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

size_t nesti_outlier_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return outlier_layout((size_t)n).total;
}

int nesti_outlier_scores_nbr(const float* cloud_dev, int N, int query_row0, int M, const int32_t* nbr_dev, int K, int k,
                             double* mean_out_dev, double* kth_d2_out_dev, int32_t* n_other_out_dev, void* stream) {
  const std::string w("nesti_outlier_scores_nbr");
  ScoreParams sp;
  if (refuse_knn_k(w, K)) return 1;
  if (k < 1 || k >= K) NESTI_FAIL(w + ": k must be in 1 .. K - 1 (the list holds the row itself and k others)");
  const int32_t ks[1] = {k + 1};
  if (nbr_params_fill(w, false, &sp.np, cloud_dev, N, nullptr, nullptr, M, query_row0, nbr_dev, K, ks, 1, nullptr, nullptr)) return 1;
  if (M == 0) return 0;
  sp.k = k;
  sp.mean_out = mean_out_dev;
  sp.kth_out = kth_d2_out_dev;
  sp.n_other_out = n_other_out_dev;
  // the lane group: the smallest of 16, 32, 64 that holds k + 1, or a wider one asked for (nesti_debug_outlier_lanes)
  return with_lane_group(k + 1, g_outlier_lanes.load(std::memory_order_relaxed), [&](auto g) {
    return launch_group_rows<decltype(g)::value>(outlier_scores_kernel<decltype(g)::value>, sp, M, stream);
  });
}

int nesti_debug_outlier_lanes(int lanes) { return set_lane_group("nesti_debug_outlier_lanes", g_outlier_lanes, lanes); }

int nesti_outlier_threshold(const double* scores_dev, int M, double std_ratio, double* stats_out_dev, void* ws_dev, size_t ws_bytes,
                            void* stream) {
  const std::string w("nesti_outlier_threshold");
  if (!scores_dev || !stats_out_dev || !ws_dev) NESTI_FAIL(w + ": null argument");
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (!std::isfinite(std_ratio) || std_ratio < 0.0) NESTI_FAIL(w + ": std_ratio must be finite and >= 0");
  if (M == 0) return 0;
  const OutlierLayout L = outlier_layout((size_t)M);
  if (ws_bytes < L.total) NESTI_FAIL(w + ": workspace too small (nesti_outlier_workspace_bytes(M))");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  double* part_sum = (double*)(ws + L.part_sum);
  int32_t* part_cnt = (int32_t*)(ws + L.part_cnt);
  const int nb = (int)blocks_of((size_t)M);
  const int tok = prof_begin(NESTI_PROF_PATCHES, st);
  hipLaunchKernelGGL(outlier_partial_kernel<false>, dim3(nb), dim3(kThreads), 0, st, scores_dev, M, (const double*)stats_out_dev, part_sum,
                     part_cnt);
  hipLaunchKernelGGL(outlier_final_kernel<false>, dim3(1), dim3(kThreads), 0, st, (const double*)part_sum, (const int32_t*)part_cnt, nb,
                     std_ratio, stats_out_dev);
  hipLaunchKernelGGL(outlier_partial_kernel<true>, dim3(nb), dim3(kThreads), 0, st, scores_dev, M, (const double*)stats_out_dev, part_sum,
                     part_cnt);
  hipLaunchKernelGGL(outlier_final_kernel<true>, dim3(1), dim3(kThreads), 0, st, (const double*)part_sum, (const int32_t*)part_cnt, nb,
                     std_ratio, stats_out_dev);
  prof_end(NESTI_PROF_PATCHES, tok, st);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int nesti_outlier_compact(const float* cloud_dev, int N, const double* scores_dev, const double* thr_dev, double thr, float* xyz_out_dev,
                          int32_t* kept_idx_out_dev, int32_t* new_of_old_out_dev, uint8_t* keep_out_dev, int32_t* n_kept_out_dev,
                          void* ws_dev, size_t ws_bytes, void* stream) {
  const std::string w("nesti_outlier_compact");
  if (!scores_dev || !n_kept_out_dev || !ws_dev || (xyz_out_dev && !cloud_dev)) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (!thr_dev && (!std::isfinite(thr) || thr < 0.0)) NESTI_FAIL(w + ": thr must be finite and >= 0 (or given on the device: thr_dev)");
  const OutlierLayout L = outlier_layout((size_t)N);
  if (ws_bytes < L.total) NESTI_FAIL(w + ": workspace too small (nesti_outlier_workspace_bytes(N))");
  hipStream_t st = (hipStream_t)stream;
  int32_t* block_cnt = (int32_t*)((unsigned char*)ws_dev + L.block_cnt);
  CompactParams p;
  p.cloud = cloud_dev; p.scores = scores_dev; p.thr_dev = thr_dev; p.thr = thr; p.N = N;
  p.xyz_out = xyz_out_dev; p.kept_idx_out = kept_idx_out_dev; p.new_of_old_out = new_of_old_out_dev; p.keep_out = keep_out_dev;
  const int nb = (int)blocks_of((size_t)N);
  const int tok = prof_begin(NESTI_PROF_PATCHES, st);
  hipLaunchKernelGGL(outlier_count_kernel, dim3(nb), dim3(kThreads), 0, st, p, block_cnt);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, block_cnt, (long long)nb, n_kept_out_dev);
  hipLaunchKernelGGL(outlier_scatter_kernel, dim3(nb), dim3(kThreads), 0, st, p, (const int32_t*)block_cnt);
  prof_end(NESTI_PROF_PATCHES, tok, st);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
