// Image-window neighbour lists (DESIGN.md 2 "Image-window neighbourhoods"): the neighbours of a depth frame's point among the points of
// the pixels round its own pixel, and a PROOF of when that list is the exact k-NN list of nesti_knn.  A depth frame is an organized
// cloud: nesti_depth_to_cloud leaves rank[H W], the cloud row of every pixel, and the image is the search structure -- no grid is built
// and no shell is walked.
//
// THE LIST (nesti_depth_window_knn).  The centre is cloud row i (query_idx_dev[q] clamped into the cloud, or query_row0 + q); its pixel
// is p = pix[i], v0 = p / W, u0 = p % W.  One candidate per pixel of [u0 - R, u0 + R] x [v0 - R, v0 + R], clipped to the image, whose rank
// entry j lies in [0, N); d2_j is the search's (knn_d2 of nbr_dev.h over the f32 rows: five operations, each rounded on its own, a NaN d2
// never a neighbour); the result is the K smallest pairs (d2_j, j), ascending, -1 / +inf beyond count = min(K, candidates).  rank and
// pix are untrusted: an entry outside its range is no candidate, resp. gives a row of count 0 -- never an out-of-bounds read.
//
// THE PROOF.  In the camera frame a pixel with u >= u0 + R + 1 holds a point with x / z >= (u0 + R + 1 - cx) / fx (for fx > 0; mirrored
// otherwise), which lies beyond the plane through the camera centre and the image line u = u0 + R + 0.5: x - a z = 0 with
// a = (u0 + R + 0.5 - cx) / fx.  So every point outside the window lies beyond one of (at most) four such planes, and the distance
// from the centre to the nearest of them bounds the distance to every such point from below.  A side at or past the image's border has
// nothing beyond it.  With a pose T (camera -> world, rigid) the plane's normal is m_r = T[r][axis] - a T[r][2] and the centre relative
// to the camera is rel_r = c_r - T[r][3]; dist = |m . rel| / sqrt(1 + a a).
// THE MARGIN.  Every stored coordinate is ONE f32 rounding of its fp64 value: it moves by at most 2^-24 of itself.  A point whose exact
// position is L from the (stored) centre c has a norm of at most |c| + L, so it is stored at least L - 2^-24 (|c| + L) =
// L (1 - 2^-24) - 2^-24 |c| from c, and that grows with L, so L may be replaced by the plane distance.  The constants used are 8 x
// that, 2^-21 on both terms, with |c| taken as the 1-norm; the half pixel between the edge and the first pixel centre outside covers the
// fp64 roundings of nesti_depth_to_cloud and of dist itself, which are of the order 2^-50 against a slope step of 1 / (2 fx).
// b = max(0, bound (1 - 2^-21) - 2^-21 ((|c0| + |c1|) + |c2|)) and proven = (count == K) && d2[K - 1] < b b, STRICTLY: a point outside at
// equal distance with a smaller index would win the tie.  The proof presumes that xyz, pix, rank and the camera come from ONE
// nesti_depth_to_cloud call, that the points have not moved since and that the pose is rigid; otherwise the lists are still as defined
// and proven means nothing.
//
// One wave per row, four per workgroup.  Lanes stride over the window row by row: the rank reads of a window row are contiguous and the
// xyz gathers nearly so (the compaction is in pixel order).  The pairs go to the wave's LDS buffer by ballot compaction and are cut once
// by the search's bitonic knn_cut.  Two instantiations: 256 pairs (R <= 7: 12 KiB a workgroup) and 1 024 pairs (48 KiB).  No atomics,
// no dependence on which workgroup runs first; whole waves leave before any ballot.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // centre_lost, refuse_query_rows; its ball_d2 is not used here

// every product, quotient and sum below is rounded on its own: the CPU restatement (tests/_window_fixture.py) predicts every bit
#pragma clang fp contract(off)

#include "pca_dev.h"       // wave_row, launch_wave_rows
#include "nbr_dev.h"       // knn_d2, knn_cut, kKnnCap, wave_lds_fence, refuse_knn_k

namespace nesti {
namespace {

constexpr long long kMaxPixels = 1ll << 26;
constexpr int kSmallCap = 256;                              // pairs per wave of the small instantiation
constexpr int kSmallR = 7;                                  // (2 * 7 + 1)^2 = 225 <= 256
static_assert((2 * kSmallR + 1) * (2 * kSmallR + 1) <= kSmallCap, "a small window fits the small buffer");
static_assert((2 * NESTI_WINDOW_MAX_R + 1) * (2 * NESTI_WINDOW_MAX_R + 1) <= kKnnCap, "the largest window is one fill of the pair buffer");
static_assert(NESTI_KNN_MAX_K <= kSmallCap, "the list is written from the buffer");

struct WindowParams {
  const float* xyz;                   // [N, 3]
  const int32_t* pix;                 // [N]
  const int32_t* rank;                // [H W]
  const int32_t* query_idx;           // [M] or NULL
  int N, H, W, M, row0, R, K;
  double fx, fy, cx, cy;
  double T[12];                       // the pose, or the identity
  int32_t* nbr_out;                   // [M, K]
  double* d2_out;                     // [M, K] or NULL
  int32_t* count_out;                 // [M] or NULL
  int32_t* proven_out;                // [M] or NULL
};

template <int CAP>
struct WindowShared {
  double d2[kRowsPerBlock][CAP];
  int j[kRowsPerBlock][CAP];
};

// the distance from the centre c to the plane through the camera centre and the image line `axis` = e (axis 0: u, 1: v)
__device__ __forceinline__ double side_dist(const WindowParams& wp, const double (&c)[3], int axis, double e) {
  const double a = axis == 0 ? (e - wp.cx) / wp.fx : (e - wp.cy) / wp.fy;
  double m[3], rel[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    m[r] = wp.T[4 * r + axis] - a * wp.T[4 * r + 2];
    rel[r] = c[r] - wp.T[4 * r + 3];
  }
  const double s = (m[0] * rel[0] + m[1] * rel[1]) + m[2] * rel[2];
  return fabs(s) / sqrt(1.0 + a * a);
}

template <int CAP>
__global__ __launch_bounds__(kThreads) void window_kernel(const WindowParams wp) {
  __shared__ WindowShared<CAP> sh;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= wp.M) return;                                      // whole waves leave: the ballots below see full waves
  double* bd = sh.d2[threadIdx.x >> 6];
  int* bj = sh.j[threadIdx.x >> 6];
  const int K = wp.K, R = wp.R;
  int qi = wp.query_idx ? wp.query_idx[q] : wp.row0 + q;
  qi = uniform(min(max(qi, 0), wp.N - 1));
  const float* centre = wp.xyz + (size_t)qi * 3;
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const int p = uniform(wp.pix[qi]);
  int cnt = 0, proven = 0;
  if ((unsigned)p < (unsigned)(wp.H * wp.W) && !centre_lost(cf0, cf1, cf2)) {
    const double c[3] = {(double)cf0, (double)cf1, (double)cf2};
    const int v0 = p / wp.W, u0 = p - v0 * wp.W;
    const int ulo = max(u0 - R, 0), uhi = min(u0 + R, wp.W - 1), vlo = max(v0 - R, 0), vhi = min(v0 + R, wp.H - 1);
    const int ww = uhi - ulo + 1, total = ww * (vhi - vlo + 1);   // <= (2 R + 1)^2 <= CAP
    for (int t0 = 0; t0 < total; t0 += kWave) {
      const int t = t0 + lane;
      bool pass = false;
      double d2 = 0.0;
      int j = 0;
      if (t < total) {
        const int dv = t / ww;
        j = wp.rank[(vlo + dv) * wp.W + ulo + (t - dv * ww)];
        if ((unsigned)j < (unsigned)wp.N) {
          const float* pt = wp.xyz + (size_t)j * 3;
          d2 = knn_d2((double)pt[0] - c[0], (double)pt[1] - c[1], (double)pt[2] - c[2]);
          pass = d2 == d2;                                    // a NaN d2 is never a neighbour
        }
      }
      const unsigned long long m = __ballot(pass);
      if (pass) {
        const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        bd[pos] = d2;
        bj[pos] = j;
      }
      cnt += __builtin_popcountll(m);
    }
    wave_lds_fence();
    cnt = knn_cut(bd, bj, cnt, K, lane);
    // the proof (see the header): the nearest plane of a side with image beyond it, less the margin
    double bound = INFINITY;
    if (u0 - R > 0) bound = fmin(bound, side_dist(wp, c, 0, (double)(u0 - R) - 0.5));
    if (u0 + R < wp.W - 1) bound = fmin(bound, side_dist(wp, c, 0, (double)(u0 + R) + 0.5));
    if (v0 - R > 0) bound = fmin(bound, side_dist(wp, c, 1, (double)(v0 - R) - 0.5));
    if (v0 + R < wp.H - 1) bound = fmin(bound, side_dist(wp, c, 1, (double)(v0 + R) + 0.5));
    if (bound == INFINITY) {
      proven = 1;                                             // the window covers the image
    } else {
      const double b = fmax(0.0, bound * (1.0 - 0x1p-21) - 0x1p-21 * ((fabs(c[0]) + fabs(c[1])) + fabs(c[2])));
      proven = (cnt == K && bd[K - 1] < b * b) ? 1 : 0;
    }
  }
  wave_lds_fence();
  for (int i = lane; i < K; i += kWave) {
    const size_t o = (size_t)q * K + i;
    wp.nbr_out[o] = i < cnt ? bj[i] : -1;
    if (wp.d2_out) wp.d2_out[o] = i < cnt ? bd[i] : INFINITY;
  }
  if (lane == 0) {
    if (wp.count_out) wp.count_out[q] = cnt;
    if (wp.proven_out) wp.proven_out[q] = proven;
  }
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_depth_window_knn(const float* xyz_dev, int N, const int32_t* pix_dev, const int32_t* rank_dev, int H, int W,
                           const nesti_camera_t* camera, const int32_t* query_idx_dev, int M, int query_row0, int R, int K,
                           int32_t* nbr_out_dev, double* d2_out_dev, int32_t* count_out_dev, int32_t* proven_out_dev, void* stream) {
  const std::string w("nesti_depth_window_knn");
  if (!xyz_dev || !pix_dev || !rank_dev || !camera || !nbr_out_dev) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (H <= 0 || W <= 0) NESTI_FAIL(w + ": H and W must be > 0");
  if ((long long)H * (long long)W > kMaxPixels) NESTI_FAIL(w + ": H * W must not exceed 2^26");
  if (!std::isfinite(camera->fx) || !std::isfinite(camera->fy) || camera->fx == 0.0 || camera->fy == 0.0)
    NESTI_FAIL(w + ": fx and fy must be finite and non-zero");
  if (!std::isfinite(camera->cx) || !std::isfinite(camera->cy)) NESTI_FAIL(w + ": cx and cy must be finite");
  if (camera->has_pose)
    for (int k = 0; k < 12; ++k)
      if (!std::isfinite(camera->pose[k])) NESTI_FAIL(w + ": the pose must be finite");
  if (R < 1 || R > NESTI_WINDOW_MAX_R) NESTI_FAIL(w + ": R must be in 1 .. " + std::to_string(NESTI_WINDOW_MAX_R));
  if (refuse_knn_k(w, K)) return 1;
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (refuse_query_rows(w, N, !query_idx_dev, M, query_row0)) return 1;
  if (M == 0) return 0;
  WindowParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.xyz = xyz_dev; wp.pix = pix_dev; wp.rank = rank_dev; wp.query_idx = query_idx_dev;
  wp.N = N; wp.H = H; wp.W = W; wp.M = M; wp.row0 = query_row0; wp.R = R; wp.K = K;
  wp.fx = camera->fx; wp.fy = camera->fy; wp.cx = camera->cx; wp.cy = camera->cy;
  for (int k = 0; k < 12; ++k) wp.T[k] = camera->has_pose ? camera->pose[k] : (k % 5 == 0 ? 1.0 : 0.0);
  wp.nbr_out = nbr_out_dev; wp.d2_out = d2_out_dev; wp.count_out = count_out_dev; wp.proven_out = proven_out_dev;
  if (R <= kSmallR) return launch_wave_rows(window_kernel<kSmallCap>, wp, M, stream);
  return launch_wave_rows(window_kernel<kKnnCap>, wp, M, stream);
}

}  // extern "C"
