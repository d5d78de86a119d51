// The quadric fit of one query by one wave after its plane fit (DESIGN.md 2 "Quadric fit", steps 2 - 8), shared by quadric_kernel
// (quadric.hip: the neighbourhood is a ball of the search grid) and quadric_nbr_kernel (knn.hip: a prefix of a neighbour list): the
// frame of every scale, the per-candidate body of the 20 moments, their wave reductions, and the solve with its outputs.  One
// definition each, so the two kernels differ in the walk over their candidates and in nothing else.
//
// For the including unit: after `#pragma clang fp contract(off)` and after pca_dev.h -- every product and sum below is rounded on its own.
#pragma once
#include "pca_dev.h"
#include "quadric_solve.h"

namespace nesti {
namespace {

constexpr int kQSums = kQuadricMoments - 1;   // m[1..20]: m[0] = n is known from pass 1

struct QuadricOut {
  float* normals;                     // [M, S, 3] or NULL
  float* curv;                        // [M, S, 2] or NULL
  float* plane;                       // [M, S, 3] or NULL
  int32_t* count;                     // [M, S] or NULL
};

// a value that is the same in every lane, into scalar registers
__device__ __forceinline__ double wave_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// step 2: the frame (t1, t2, n0) of a plane normal, f[0..2] = t1, f[3..5] = t2, f[6..8] = n0
__device__ __forceinline__ void quadric_frame(double nx, double ny, double nz, double (&f)[9]) {
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  double cx, cy, cz;                                          // n0 x e_j
  if (ax <= ay && ax <= az) { cx = 0.0; cy = nz; cz = -ny; }
  else if (ay <= az) { cx = -nz; cy = 0.0; cz = nx; }
  else { cx = ny; cy = -nx; cz = 0.0; }
  const double len = sqrt((cx * cx + cy * cy) + cz * cz);
  f[0] = cx / len; f[1] = cy / len; f[2] = cz / len;
  f[3] = ny * f[2] - nz * f[1];
  f[4] = nz * f[0] - nx * f[2];
  f[5] = nx * f[1] - ny * f[0];
  f[6] = nx; f[7] = ny; f[8] = nz;
}

// The frame of every scale from the plane fit lane s holds for scale s (its normal nrm and count n), the same in every lane.
// live[s]: the scale can be fitted (n >= 6 and a plane normal); the frame of another scale is all zero and pass 2 adds nothing for it.
template <int S>
__device__ __forceinline__ void quadric_frames(const float (&nrm)[3], int n, double (&fr)[S][9], bool (&live)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const float bx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nrm[0]), s));
    const float by = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nrm[1]), s));
    const float bz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nrm[2]), s));
    const int ns = __builtin_amdgcn_readlane(n, s);
    live[s] = ns >= kQuadricMinPoints && (bx != 0.f || by != 0.f || bz != 0.f);
    double f[9];
    quadric_frame((double)bx, (double)by, (double)bz, f);
#pragma unroll
    for (int k = 0; k < 9; ++k) fr[s][k] = wave_uniform(live[s] ? f[k] : 0.0);
  }
}

// steps 3 and 4 for one candidate of one scale: its coordinates in the frame f, scaled by the radius, and the 20 sums
__device__ __forceinline__ void quadric_add(double (&a)[kQSums], const double (&f)[9], double rad, double dx, double dy, double dz) {
  const double u = ((f[0] * dx + f[1] * dy) + f[2] * dz) / rad;
  const double v = ((f[3] * dx + f[4] * dy) + f[5] * dz) / rad;
  const double h = ((f[6] * dx + f[7] * dy) + f[8] * dz) / rad;
  const double u2 = u * u, uv = u * v, v2 = v * v;
  const double u3 = u2 * u, u2v = u2 * v, uv2 = u * v2, v3 = v2 * v;
  a[0] += u; a[1] += v;
  a[2] += u2; a[3] += uv; a[4] += v2;
  a[5] += u3; a[6] += u2v; a[7] += uv2; a[8] += v3;
  a[9] += u2 * u2; a[10] += u3 * v; a[11] += u2 * v2; a[12] += u * v3; a[13] += v2 * v2;
  a[14] += h; a[15] += h * u; a[16] += h * v; a[17] += h * u2; a[18] += h * uv; a[19] += h * v2;
}

// The totals of one scale's sums of pass 2 (the fixed xor-butterfly; every lane ends up with every total) and, in the lane that solves
// that scale (`mine`), its moments m[1..20], frame and radius.  Per scale, with the loop over the scales left to the kernel: taking the
// [S][..] arrays through one call cost quadric_kernel<4> 166 more registers (profiles/knn_refactor_isa.txt).
__device__ __forceinline__ void quadric_totals(const double (&acc)[kQSums], const double (&fr)[9], double rad, bool mine,
                                               double (&m)[kQuadricMoments], double (&f)[9], double& r) {
  if (mine) {
    r = rad;
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = fr[k];
  }
#pragma unroll
  for (int k = 0; k < kQSums; ++k) {
    const double t = wave_sum(acc[k]);
    if (mine) m[k + 1] = t;
  }
}

// Steps 5 - 8 of one scale in one lane, and row o of the outputs.  m[1..20], f, r: the lane's totals (quadric_totals); n, nrm: its
// plane fit.
__device__ __forceinline__ void quadric_solve_write(double (&m)[kQuadricMoments], const double (&f)[9], double r, int n,
                                                    const float (&nrm)[3], size_t o, const QuadricOut& out) {
  m[0] = (double)n;
  float nu[3] = {0.f, 0.f, 0.f}, kf[2] = {0.f, 0.f};
  double a[kQuadricCoeffs];
  const bool fitted = n >= kQuadricMinPoints && (nrm[0] != 0.f || nrm[1] != 0.f || nrm[2] != 0.f);
  if (quadric_solve(m, a) && fitted) {
    const double vx = (f[6] - a[1] * f[0]) - a[2] * f[3], vy = (f[7] - a[1] * f[1]) - a[2] * f[4], vz = (f[8] - a[1] * f[2]) - a[2] * f[5];
    const double len = sqrt((vx * vx + vy * vy) + vz * vz);
    double k[2];
    quadric_curvatures(a, k);
    const float fx = (float)(vx / len), fy = (float)(vy / len), fz = (float)(vz / len);
    const float k0 = (float)(k[0] / r), k1 = (float)(k[1] / r);
    if (finite_bits(fx) && finite_bits(fy) && finite_bits(fz) && finite_bits(k0) && finite_bits(k1)) {
      nu[0] = fx + 0.f; nu[1] = fy + 0.f; nu[2] = fz + 0.f;    // -0 + +0 = +0: no negative zero leaves
      kf[0] = k0; kf[1] = k1;
    }
  }
  if (out.normals) { out.normals[o * 3] = nu[0]; out.normals[o * 3 + 1] = nu[1]; out.normals[o * 3 + 2] = nu[2]; }
  if (out.curv) { out.curv[o * 2] = kf[0]; out.curv[o * 2 + 1] = kf[1]; }
  if (out.plane) { out.plane[o * 3] = nrm[0]; out.plane[o * 3 + 1] = nrm[1]; out.plane[o * 3 + 2] = nrm[2]; }
  if (out.count) out.count[o] = n;
}

}  // namespace
}  // namespace nesti
