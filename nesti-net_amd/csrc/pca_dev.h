// The plane fit of one query by one wave (DESIGN.md 2 "Plane-fit normals"), shared by pca_kernel (pca.hip), by pass 1 of
// quadric_kernel (quadric.hip) and by the neighbour-list kernels of knn.hip: the query's spans, the nine fp64 sums and the count of
// every scale, their wave reductions, and the solve with its rounding and sign rule.  One definition, so the plane normal of the
// quadric fit IS nesti_pca_normals' normal, bit for bit.
//
// For the including unit: include patches_dev.h first, under the compiler's default contraction (ball_d2, see there), then
// `#pragma clang fp contract(off)`, then this header -- every product and sum below is rounded on its own.
#pragma once
#include "patches_dev.h"
#include "pca_eig.h"
#include "wave_dev.h"      // kThreads, kWave, kRowsPerBlock; wave_sum / wave_min / wave_max: the 64-lane case of group_sum / _min / _max

namespace nesti {
namespace {

constexpr int kSums = 9;              // sum d (3), sum d d^T (6: xx xy xz yy yz zz)

// the row of this wave (the same in every lane: said so, and the centre and its tests live in scalar registers); a wave beyond the
// last row gets M or more and leaves whole, so the shuffles of the others see full waves
__device__ __forceinline__ int wave_row() {
  return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6)));
}

// host side: f(std::integral_constant<int, S>) for the number of scales S in 1 .. NESTI_MAX_SCALES (checked by the caller) a launch
// is instantiated for, like with_elem_type (kernels.h)
static_assert(NESTI_MAX_SCALES == 4, "with_scales names every S");
template <class F>
int with_scales(int S, F&& f) {
  switch (S) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}
// host side: one launch of a one-wave-per-row kernel (wave_row) over M > 0 rows on `stream`, timed in the profiler's neighbourhood slot
template <class Params>
int launch_wave_rows(void (*kernel)(Params), const Params& params, int M, void* stream) {
  const dim3 grid((unsigned)((M + kRowsPerBlock - 1) / kRowsPerBlock)), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  const int tok = prof_begin(NESTI_PROF_PATCHES, st);
  hipLaunchKernelGGL(kernel, grid, block, 0, st, params);
  prof_end(NESTI_PROF_PATCHES, tok, st);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

// lane t < 9: x-span t of the cell block round the centre (block_span, patches_dev.h); empty for a centre that is not finite
__device__ __forceinline__ WaveSpans wave_spans(const PatchParams& p, int lane, float cf0, float cf1, float cf2) {
  WaveSpans spans = {0, 0};
  if (!centre_lost(cf0, cf1, cf2) && lane < 9) {
    const Span s = block_span(*p.header, p.start, p.N, cf0, cf1, cf2, lane);
    spans.b = s.b;
    spans.e = s.e;
  }
  return spans;
}

// The per-candidate body of the plane fit, shared by the ball walk below and the neighbour-list walk (nbr_dev.h: walk_list): the nine terms of a
// difference d -- d itself and the six products of d d^T, formed once per candidate -- and their addition to one scale's sums.
struct PlaneTerms {
  double v[kSums];
};
__device__ __forceinline__ PlaneTerms plane_terms(double dx, double dy, double dz) {
  const double xx = __dmul_rn(dx, dx), yy = __dmul_rn(dy, dy), zz = __dmul_rn(dz, dz);
  const double xy = dx * dy, xz = dx * dz, yz = dy * dz;
  return {{dx, dy, dz, xx, xy, xz, yy, yz, zz}};
}
__device__ __forceinline__ void plane_add(double (&acc)[kSums], const PlaneTerms& t) {
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] += t.v[k];
}

// The totals of the per-lane sums and counts of every scale: one fixed xor-butterfly each.  Every lane ends up with every total; lane
// s keeps those of scale s, with its r^2 (lanes >= S: of the last scale).
template <int S>
__device__ __forceinline__ void plane_totals(const double (&acc)[S][kSums], const int (&cnt)[S], const double* r2s, int lane,
                                             double (&sum)[kSums], int& n, double& r2) {
#pragma unroll
  for (int k = 0; k < kSums; ++k) sum[k] = 0.0;
  n = 0;
  r2 = 1.0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int ns = wave_sum(cnt[s]);
    const bool mine = lane == s || (s == S - 1 && lane >= S);
    if (mine) { n = ns; r2 = r2s[s]; }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
      const double t = wave_sum(acc[s][k]);
      if (mine) sum[k] = t;
    }
  }
}

// The sums of d and d d^T and the count of every scale's ball.  A candidate is tested once for all scales: the six products of d are
// formed once and added to the sums of every scale whose ball holds it.  Every lane ends up with every total; lane s keeps those of
// scale s (lanes >= S: of the last scale).
template <int S>
__device__ __forceinline__ void plane_sums(const PatchParams& p, const WaveSpans& spans, int lane, double cx, double cy, double cz,
                                           double (&sum)[kSums], int& n, double& r2) {
  double acc[S][kSums];
  int cnt[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    cnt[s] = 0;
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[s][k] = 0.0;
  }
  walk_block(p.sorted, spans, lane, kWave, cx, cy, cz, [&](const float4& c, double d2) {
    // the differences ball_d2 was given, formed again: the same operations, so the same values
    const PlaneTerms t = plane_terms((double)c.x - cx, (double)c.y - cy, (double)c.z - cz);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (d2 <= p.r2[s]) {
        ++cnt[s];
        plane_add(acc[s], t);
      }
    }
  });
  plane_totals<S>(acc, cnt, p.r2, lane, sum, n, r2);
}

// covariance in units of r^2 -> Jacobi -> the normal (normalised in fp64, rounded to f32 once, signed on the f32 values so that the
// first non-zero of (n_z, n_y, n_x) is positive, zeros +0) and the clamped eigenvalues, for sums of total mass dn: the count of the
// plane fits (plane_solve below), the sum of the weights of the robust fit (robust.hip)
__device__ __forceinline__ void plane_solve_mass(const double (&sum)[kSums], double dn, double r2, float (&nrm)[3], float (&ev)[3]) {
  const double mx = sum[0] / dn, my = sum[1] / dn, mz = sum[2] / dn;
  const double c[6] = {(sum[3] / dn - mx * mx) / r2, (sum[4] / dn - mx * my) / r2, (sum[5] / dn - mx * mz) / r2,
                       (sum[6] / dn - my * my) / r2, (sum[7] / dn - my * mz) / r2, (sum[8] / dn - mz * mz) / r2};
  double w[3], vec[3][3];
  sym3_eig(c, w, vec);
  const double len = sqrt((vec[0][0] * vec[0][0] + vec[0][1] * vec[0][1]) + vec[0][2] * vec[0][2]);
  float fx = (float)(vec[0][0] / len), fy = (float)(vec[0][1] / len), fz = (float)(vec[0][2] / len);
  const float lead = fz != 0.f ? fz : (fy != 0.f ? fy : fx);
  if (lead < 0.f) { fx = -fx; fy = -fy; fz = -fz; }
  nrm[0] = fx + 0.f; nrm[1] = fy + 0.f; nrm[2] = fz + 0.f;   // -0 + +0 = +0: no negative zero leaves
#pragma unroll
  for (int k = 0; k < 3; ++k) ev[k] = (float)fmax(0.0, w[k]);
}
// the plane fit's solve: dn = n; n < 3: all 0
__device__ __forceinline__ void plane_solve(const double (&sum)[kSums], int n, double r2, float (&nrm)[3], float (&ev)[3]) {
  nrm[0] = 0.f; nrm[1] = 0.f; nrm[2] = 0.f;
  ev[0] = 0.f; ev[1] = 0.f; ev[2] = 0.f;
  if (n >= 3) plane_solve_mass(sum, (double)n, r2, nrm, ev);
}

}  // namespace
}  // namespace nesti
