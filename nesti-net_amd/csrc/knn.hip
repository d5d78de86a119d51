// k-nearest-neighbour neighbourhoods (DESIGN.md 2 "k-nearest neighbourhoods"): an exact k-NN search on the uniform search grid of
// patches.hip, and the plane fit (pca_dev.h) and quadric fit (quadric_dev.h) over neighbour lists instead of balls.  No model, no weights.
//
// THE SEARCH (nesti_knn / nesti_knn_at).  For a centre c, over ALL N cloud points j: d = (double)p_j - (double)c,
// d2_j = (dx dx + dy dy) + dz dz with each of the five operations rounded on its own (knn_d2 below; NOT the fused ball_d2 of
// patches_dev.h), and the result is the K smallest pairs (d2_j, j) in lexicographic order, ascending.  The pairs are all different, so
// the result is a pure function of (cloud, centre, K): it does not depend on the grid, on the order inside a cell or on the batching.
// A cloud point with a NaN coordinate has a NaN d2, which comes before no threshold: it is never a neighbour, and the count of a query
// falls below min(K, N) where fewer than K other points exist (a numpy sort would put it last instead).  provider.CloudPatches refuses
// such a cloud; through the C entries it is the caller's.
//
// One wave per query, four per workgroup.  The wave visits the grid shell by shell round the centre's (clamped) cell: shell R is the
// cells at Chebyshev distance R, walked as x-spans of start[] -- row (z, y) of the block goes to lane (row mod 64), a row on a y or z
// face is one contiguous span of 2R + 1 cells, an inner row is its two end cells -- so an empty shell costs two loads per row and
// nothing per cell.  The non-empty spans are then streamed by the whole wave, 64 candidates a trip.  A candidate below the current
// threshold pair is appended to the wave's LDS buffer (1 024 pairs: 12 KiB per wave, 48 KiB per workgroup) by ballot compaction: no
// atomics.  The buffer is cut back to its K smallest pairs (a bitonic sort over the next power of two) when the next trip might not fit
// and at each shell's end; the threshold pair is the K-th pair of the last cut (+inf before K candidates are held), so a cell with more
// points than the buffer -- 1 500 copies of one point, a 1 x 1 x 1 grid -- streams through it: capacity never decides a result.
//
// THE STOP RULE.  After shell R the visited block is cells [c - R, c + R] per axis, clipped to the grid.  The search stops when K pairs
// are held and the K-th d2 is STRICTLY below the square of the proven distance: the smallest distance from the centre to a face of the
// block that still has grid beyond it (a face at or past the grid's border is infinitely far: every cloud point lies in a grid cell,
// and a position outside the bounding box starts from the clamped border cell with the faces on its outer side infinitely far).  Strict,
// because an unvisited point at equal distance with a smaller index would win the tie.  When the block covers the grid every face is
// infinitely far and the search stops.
// THE MARGIN.  A point's cell is floor((v - minv) inv_cell) in fp64, so a point of an unvisited cell with index >= m satisfies
// fl(fl(v - minv) inv_cell) >= m, hence v - minv >= (m / inv_cell) (1 - 2 eps) to first order (eps = 2^-53: one rounding each for the
// difference and the product, and floor is monotonic).  The face is computed as minv + m / inv_cell and the distance as its difference
// to the centre's coordinate: three more roundings, each relative to a magnitude of at most |minv| + |m / inv_cell| + |c|.  All five
// together move the proven distance by less than 5 eps (|minv| + |m / inv_cell| + |c|); the margin subtracted is 8 eps times that sum
// (2^-50).  The same holds mirrored for a low face (index <= m - 1 means v - minv < (m / inv_cell) (1 + 2 eps)).  The proven distance
// is then scaled by (1 - 2^-50) before it is squared, which covers the rounding of the square itself and of the unvisited point's own
// d2 >= fl(dx dx) >= dx^2 (1 - eps) with dx = fl(v - c): the computed d2 of every unvisited point is > the computed bound.
//
// THE FITS OVER LISTS (nesti_pca_normals_nbr*, nesti_quadric_fit_nbr*).  The list nbr[M, K] is untrusted device data: the valid prefix
// of a row ends at its first entry outside [0, N).  Scale s is the first n_s = min(k_s, valid prefix) entries; r2_s is the largest d2
// among them (d and d2 as in the search).  Slot i goes to lane i mod 64 (at most four slots per lane, in ascending order) and the lanes
// meet in the xor-butterfly of pca_dev.h, so a row's output bits are a pure function of (cloud, centre, list prefix): with the search's
// list, of (cloud, centre, ks) -- independent of batching, of streams, of the grid and of the grid BUILD, which the ball kernels, whose
// sums follow the order inside a cell, do not promise.  plane_solve, quadric_solve and quadric_curvatures run unchanged with r2 = r2_s
// and r = sqrt(r2_s); n_s < 3 or r2_s == 0 gives the plane fit's sentinel, and with it a failed quadric fit.  A centre with a non-finite
// coordinate has an empty prefix.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // the grid's layout, cells and centres; its ball_d2 is not used here

// every product and sum below -- the plane fit of pca_dev.h and the solve of quadric_solve.h included -- is rounded on its own: the CPU
// restatement (tests/_knn_fixture.py) predicts every bit of the search
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"       // the list's parameter block, prefix and walk (shared with hough.hip); knn_d2, wave_lds_fence
#include "quadric_dev.h"

namespace nesti {
namespace {

// kKnnCap, the pairs per wave, and knn_cut: nbr_dev.h (shared with window.hip)

struct KnnParams {
  PatchParams p;                      // cloud, sorted, start, header, query_idx / query_xyz, M, N, row0
  int K;
  int32_t* nbr_out;                   // [M, K]
  double* d2_out;                     // [M, K] or NULL
  int32_t* count_out;                 // [M] or NULL
};

struct KnnShared {
  double d2[kRowsPerBlock][kKnnCap];
  int j[kRowsPerBlock][kKnnCap];
};

__global__ __launch_bounds__(kThreads) void knn_kernel(const KnnParams kp) {
  __shared__ KnnShared sh;
  const PatchParams& p = kp.p;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= p.M) return;                                       // whole waves leave: the ballots below see full waves
  double* bd = sh.d2[threadIdx.x >> 6];
  int* bj = sh.j[threadIdx.x >> 6];
  const int K = kp.K;
  const float* centre = query_centre(p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  int cnt = 0;
  if (!centre_lost(cf0, cf1, cf2)) {
    const GridHeader h = *p.header;
    const double c[3] = {(double)cf0, (double)cf1, (double)cf2};
    // dims clamped into what the workspace holds, whatever a workspace that does not belong to the cloud says
    const int dim[3] = {min(max(h.dims[0], 1), kMaxDim), min(max(h.dims[1], 1), kMaxDim), min(max(h.dims[2], 1), kMaxDim)};
    int ic[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ic[a] = uniform(cell_axis(c[a], h.minv[a], h.inv_cell, dim[a]));
    double td = INFINITY;                                     // the threshold pair: a candidate must come before it
    int tj = 0x7fffffff;
    int sorted_cnt = 0;                                       // pairs [0, sorted_cnt) are the last cut's, in order
    for (int R = 0;; ++R) {
      const int x0 = max(ic[0] - R, 0), x1 = min(ic[0] + R, dim[0] - 1);
      const int y0 = max(ic[1] - R, 0), y1 = min(ic[1] + R, dim[1] - 1);
      const int z0 = max(ic[2] - R, 0), z1 = min(ic[2] + R, dim[2] - 1);
      const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
      for (int base = 0; base < rows; base += kWave) {
        // row base + lane of the block: one span if it lies on a y or z face of the shell, else its two end cells
        int sb[2] = {0, 0}, se[2] = {0, 0};
        const int r = base + lane;
        if (r < rows) {
          const int zz = z0 + r / ny, yy = y0 + r % ny;
          const int row0 = (zz * dim[1] + yy) * dim[0];
          if (abs(zz - ic[2]) == R || abs(yy - ic[1]) == R) {
            sb[0] = p.start[row0 + x0];
            se[0] = p.start[row0 + x1 + 1];
          } else {
            if (ic[0] - R >= 0) { sb[0] = p.start[row0 + ic[0] - R]; se[0] = p.start[row0 + ic[0] - R + 1]; }
            if (ic[0] + R < dim[0]) { sb[1] = p.start[row0 + ic[0] + R]; se[1] = p.start[row0 + ic[0] + R + 1]; }
          }
#pragma unroll
          for (int e = 0; e < 2; ++e) {                       // a span never leaves the cell-ordered copy
            sb[e] = max(sb[e], 0);
            se[e] = min(se[e], p.N);
          }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          unsigned long long live = __ballot(sb[e] < se[e]);
          while (live) {
            const int src = __builtin_ctzll(live);
            live &= live - 1;
            const int b = __builtin_amdgcn_readlane(sb[e], src), end = __builtin_amdgcn_readlane(se[e], src);
            for (int i0 = b; i0 < end; i0 += kWave) {
              if (cnt > kKnnCap - kWave) {                    // the next trip might not fit: keep the K smallest
                wave_lds_fence();
                cnt = knn_cut(bd, bj, cnt, K, lane);
                sorted_cnt = cnt;
                if (cnt >= K) { td = bd[K - 1]; tj = bj[K - 1]; }
              }
              const int i = i0 + lane;
              bool pass = false;
              double d2 = 0.0;
              int j = 0;
              if (i < end) {
                const float4 cand = p.sorted[i];
                d2 = knn_d2((double)cand.x - c[0], (double)cand.y - c[1], (double)cand.z - c[2]);
                j = __float_as_int(cand.w);
                pass = d2 < td || (d2 == td && j < tj);
              }
              const unsigned long long m = __ballot(pass);
              if (pass) {
                const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                bd[pos] = d2;
                bj[pos] = j;
              }
              cnt += __builtin_popcountll(m);
            }
          }
        }
      }
      // the shell's end: cut, unless nothing came since the last cut (an empty shell)
      if (cnt != sorted_cnt) {
        wave_lds_fence();
        cnt = knn_cut(bd, bj, cnt, K, lane);
        sorted_cnt = cnt;
        if (cnt >= K) { td = bd[K - 1]; tj = bj[K - 1]; }
      }
      // the proven distance (see the header): the nearest face of the block with grid beyond it, less the margin
      double proven = INFINITY;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int lo = ic[a] - R, hi = ic[a] + R + 1;
        if (lo > 0) {
          const double off = (double)lo / h.inv_cell;
          proven = fmin(proven, (c[a] - (h.minv[a] + off)) - 0x1p-50 * ((fabs(h.minv[a]) + fabs(off)) + fabs(c[a])));
        }
        if (hi < dim[a]) {
          const double off = (double)hi / h.inv_cell;
          proven = fmin(proven, ((h.minv[a] + off) - c[a]) - 0x1p-50 * ((fabs(h.minv[a]) + fabs(off)) + fabs(c[a])));
        }
      }
      if (proven == INFINITY) break;                          // the block covers the grid
      proven = fmax(proven, 0.0) * (1.0 - 0x1p-50);
      if (cnt >= K && td < proven * proven) break;
    }
  }
  wave_lds_fence();
  for (int i = lane; i < K; i += kWave) {
    const size_t o = (size_t)q * K + i;
    kp.nbr_out[o] = i < cnt ? bj[i] : -1;
    if (kp.d2_out) kp.d2_out[o] = i < cnt ? bd[i] : INFINITY;
  }
  if (kp.count_out && lane == 0) kp.count_out[q] = cnt;
}

// ---- the fits over neighbour lists --------------------------------------------------------------------------------------------------

// NbrParams, nbr_row and walk_list: nbr_dev.h

// The plane fit of every scale over the list: plane_sums of pca_dev.h with a prefix in place of a ball.  Lane s ends up with the sums,
// the count n_s and r2_s of scale s; the solve sees n = 0 where r2_s == 0.  Writes the radius and the count of the lane's scale.
template <int S>
__device__ __forceinline__ void plane_fit_nbr(const NbrParams& np, const int (&j)[kNbrTrips], const int (&ns)[S], int q, int lane,
                                              double cx, double cy, double cz, int& n, double& r2, float (&nrm)[3], float (&ev)[3]) {
  double acc[S][kSums], r2s[S];
  int cnt[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    cnt[s] = 0;
    r2s[s] = 0.0;
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[s][k] = 0.0;
  }
  walk_list(np.p.cloud, j, ns[S - 1], lane, cx, cy, cz, [&](int i, double dx, double dy, double dz, double d2) {
    const PlaneTerms t = plane_terms(dx, dy, dz);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (i < ns[s]) {
        ++cnt[s];
        r2s[s] = fmax(r2s[s], d2);
        plane_add(acc[s], t);
      }
    }
  });
#pragma unroll
  for (int s = 0; s < S; ++s) r2s[s] = wave_max(r2s[s]);
  double sum[kSums];
  plane_totals<S>(acc, cnt, r2s, lane, sum, n, r2);
  plane_solve(sum, (lane < S && r2 > 0.0) ? n : 0, r2, nrm, ev);
  if (lane < S) {
    const size_t o = (size_t)q * S + lane;
    if (np.radius_out) np.radius_out[o] = (float)sqrt(r2);
    if (np.count_out) np.count_out[o] = n;
  }
}

struct PcaNbrParams {
  NbrParams np;
  float* normals_out;                 // [M, S, 3] or NULL
  float* eig_out;                     // [M, S, 3] or NULL
};

template <int S>
__global__ __launch_bounds__(kThreads) void pca_nbr_kernel(const PcaNbrParams pp) {
  const NbrParams& np = pp.np;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= np.p.M) return;                                    // whole waves leave: the shuffles below see full waves
  const float* centre = query_centre(np.p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  int j[kNbrTrips], ns[S], n;
  nbr_row<S>(np, q, lane, centre_lost(cf0, cf1, cf2), j, ns);
  double r2;
  float nrm[3], ev[3];
  plane_fit_nbr<S>(np, j, ns, q, lane, (double)cf0, (double)cf1, (double)cf2, n, r2, nrm, ev);
  if (lane >= S) return;                                      // lane s solved scale s
  const size_t o = (size_t)q * S + lane;
  if (pp.normals_out) { pp.normals_out[o * 3] = nrm[0]; pp.normals_out[o * 3 + 1] = nrm[1]; pp.normals_out[o * 3 + 2] = nrm[2]; }
  if (pp.eig_out) { pp.eig_out[o * 3] = ev[0]; pp.eig_out[o * 3 + 1] = ev[1]; pp.eig_out[o * 3 + 2] = ev[2]; }
}

struct QuadricNbrParams {
  NbrParams np;
  QuadricOut out;                     // count unused: NbrParams::count_out
};

template <int S>
__global__ __launch_bounds__(kThreads) void quadric_nbr_kernel(const QuadricNbrParams qp) {
  const NbrParams& np = qp.np;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= np.p.M) return;                                    // whole waves leave: the shuffles below see full waves
  const float* centre = query_centre(np.p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const double cx = cf0, cy = cf1, cz = cf2;
  int j[kNbrTrips], ns[S], n;
  nbr_row<S>(np, q, lane, centre_lost(cf0, cf1, cf2), j, ns);
  // ---- pass 1: the plane fit of the list kernel, bit for bit; lane s solves scale s ------------------------------------------------
  double r2;
  float nrm[3], ev[3];
  plane_fit_nbr<S>(np, j, ns, q, lane, cx, cy, cz, n, r2, nrm, ev);
  // ---- the frame and the radius sqrt(r2_s) of every scale, the same in every lane; a scale that cannot be fitted gets an empty prefix
  double fr[S][9], rad[S];
  bool live[S];
  int nlive[S];
  quadric_frames<S>(nrm, (lane < S && r2 > 0.0) ? n : 0, fr, live);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    nlive[s] = live[s] ? ns[s] : 0;
    rad[s] = wave_uniform(sqrt(__shfl(r2, s, kWave)));
  }
  // ---- pass 2: the moments over the same prefixes ---------------------------------------------------------------------------------
  double acc[S][kQSums];
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int k = 0; k < kQSums; ++k) acc[s][k] = 0.0;
  }
  walk_list(np.p.cloud, j, ns[S - 1], lane, cx, cy, cz, [&](int i, double dx, double dy, double dz, double) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (i < nlive[s]) quadric_add(acc[s], fr[s], rad[s], dx, dy, dz);
    }
  });
  double m[kQuadricMoments], f[9], r = 1.0;
#pragma unroll
  for (int k = 0; k < kQuadricMoments; ++k) m[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) quadric_totals(acc[s], fr[s], rad[s], lane == s, m, f, r);
  if (lane >= S) return;
  // ---- lane s: solve, normal, curvatures.  r2_s == 0 left no plane normal, so the fit fails ---------------------------------------
  QuadricOut out = qp.out;
  out.count = nullptr;                                        // plane_fit_nbr wrote the count
  quadric_solve_write(m, f, r, n, nrm, (size_t)q * S + lane, out);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

// refuse_knn_k and nbr_params_fill (what the list fits refuse, and their parameter block): nbr_dev.h

// nesti_knn (centres = cloud points, by index or row) and nesti_knn_at (centres = positions): one body
int knn_impl(const char* who, bool at, const float* cloud_dev, int N, const int32_t* query_idx_dev, const float* query_xyz_dev, int M,
             int query_row0, int K, int32_t* nbr_out_dev, double* d2_out_dev, int32_t* count_out_dev, const void* grid_ws_dev,
             size_t grid_ws_bytes, void* stream) {
  const std::string w(who);
  if (!cloud_dev || !grid_ws_dev || !nbr_out_dev) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (refuse_knn_k(w, K)) return 1;
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (grid_ws_bytes < patch_ws_layout(N).total) NESTI_FAIL(w + ": grid workspace too small");
  if (refuse_query_rows(w, N, !at && !query_idx_dev, M, query_row0)) return 1;
  if (M == 0) return 0;
  if (at && !query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev");
  KnnParams kp;
  memset(&kp, 0, sizeof(kp));
  patch_params_grid(&kp.p, N, grid_ws_dev);
  kp.p.cloud = cloud_dev;
  kp.p.query_idx = query_idx_dev;
  kp.p.query_xyz = at ? query_xyz_dev : nullptr;
  kp.p.M = M; kp.p.N = N; kp.p.row0 = query_row0;
  kp.K = K;
  kp.nbr_out = nbr_out_dev;
  kp.d2_out = d2_out_dev;
  kp.count_out = count_out_dev;
  return launch_wave_rows(knn_kernel, kp, M, stream);
}

// nesti_pca_normals_nbr and nesti_pca_normals_nbr_at: one body
int pca_nbr_impl(const char* who, bool at, const float* cloud_dev, int N, const int32_t* query_idx_dev, const float* query_xyz_dev, int M,
                 int query_row0, const int32_t* nbr_dev, int K, const int32_t* ks, int S, float* normals_out_dev, float* eig_out_dev,
                 float* radius_out_dev, int32_t* count_out_dev, void* stream) {
  PcaNbrParams pp;
  if (nbr_params_fill(who, at, &pp.np, cloud_dev, N, query_idx_dev, query_xyz_dev, M, query_row0, nbr_dev, K, ks, S, radius_out_dev,
                      count_out_dev))
    return 1;
  if (M == 0) return 0;
  pp.normals_out = normals_out_dev;
  pp.eig_out = eig_out_dev;
  return with_scales(S, [&](auto s) { return launch_wave_rows(pca_nbr_kernel<decltype(s)::value>, pp, M, stream); });
}

// nesti_quadric_fit_nbr and nesti_quadric_fit_nbr_at: one body
int quadric_nbr_impl(const char* who, bool at, const float* cloud_dev, int N, const int32_t* query_idx_dev, const float* query_xyz_dev,
                     int M, int query_row0, const int32_t* nbr_dev, int K, const int32_t* ks, int S, float* normals_out_dev,
                     float* curv_out_dev, float* plane_out_dev, float* radius_out_dev, int32_t* count_out_dev, void* stream) {
  QuadricNbrParams qp;
  if (nbr_params_fill(who, at, &qp.np, cloud_dev, N, query_idx_dev, query_xyz_dev, M, query_row0, nbr_dev, K, ks, S, radius_out_dev,
                      count_out_dev))
    return 1;
  if (M == 0) return 0;
  qp.out = QuadricOut{normals_out_dev, curv_out_dev, plane_out_dev, nullptr};
  return with_scales(S, [&](auto s) { return launch_wave_rows(quadric_nbr_kernel<decltype(s)::value>, qp, M, stream); });
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_knn(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, int K, int32_t* nbr_out_dev,
              double* d2_out_dev, int32_t* count_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  return knn_impl("nesti_knn", false, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, K, nbr_out_dev, d2_out_dev, count_out_dev,
                  grid_ws_dev, grid_ws_bytes, stream);
}

int nesti_knn_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, int K, int32_t* nbr_out_dev, double* d2_out_dev,
                 int32_t* count_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  return knn_impl("nesti_knn_at", true, cloud_dev, N, nullptr, query_xyz_dev, M, 0, K, nbr_out_dev, d2_out_dev, count_out_dev,
                  grid_ws_dev, grid_ws_bytes, stream);
}

int nesti_pca_normals_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                          int K, const int32_t* ks, int S, float* normals_out_dev, float* eig_out_dev, float* radius_out_dev,
                          int32_t* count_out_dev, void* stream) {
  return pca_nbr_impl("nesti_pca_normals_nbr", false, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, S,
                      normals_out_dev, eig_out_dev, radius_out_dev, count_out_dev, stream);
}

int nesti_pca_normals_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                             const int32_t* ks, int S, float* normals_out_dev, float* eig_out_dev, float* radius_out_dev,
                             int32_t* count_out_dev, void* stream) {
  return pca_nbr_impl("nesti_pca_normals_nbr_at", true, cloud_dev, N, nullptr, query_xyz_dev, M, 0, nbr_dev, K, ks, S, normals_out_dev,
                      eig_out_dev, radius_out_dev, count_out_dev, stream);
}

int nesti_quadric_fit_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                          int K, const int32_t* ks, int S, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                          float* radius_out_dev, int32_t* count_out_dev, void* stream) {
  return quadric_nbr_impl("nesti_quadric_fit_nbr", false, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, S,
                          normals_out_dev, curv_out_dev, plane_out_dev, radius_out_dev, count_out_dev, stream);
}

int nesti_quadric_fit_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                             const int32_t* ks, int S, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                             float* radius_out_dev, int32_t* count_out_dev, void* stream) {
  return quadric_nbr_impl("nesti_quadric_fit_nbr_at", true, cloud_dev, N, nullptr, query_xyz_dev, M, 0, nbr_dev, K, ks, S,
                          normals_out_dev, curv_out_dev, plane_out_dev, radius_out_dev, count_out_dev, stream);
}

}  // extern "C"
