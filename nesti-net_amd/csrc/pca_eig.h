// Eigen-decomposition of a symmetric 3 x 3 matrix in fp64 by cyclic Jacobi rotations: the solver of the plane-fit normals
// (pca.hip, one solve per query and scale) and of the host-only entry nesti_sym3_eig, which runs the same arithmetic on the CPU.
//
// Only + - x / sqrt, every operation rounded on its own (the including unit turns contraction off), a fixed number of sweeps and
// no data-dependent loop: the result is a pure function of the six inputs.  A rotation whose pivot is an exact zero is skipped, so
// a matrix with a zero row (a planar neighbourhood in an axis plane) keeps that axis as an exact eigenvector.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NESTI_EIG_HD __host__ __device__
#else
#define NESTI_EIG_HD
#endif

namespace nesti {

// Sweeps over the pivots (0,1), (0,2), (1,2).  Cyclic Jacobi converges quadratically once the off-diagonal norm is below the
// smallest eigenvalue gap, and a 3 x 3 matrix gets there within two or three sweeps.  Measured on the matrices of tests/test_pca.py
// (2 000 random ones, equal eigenvalues, rank 0 and 1, entries spanning twelve decades), largest off-diagonal norm over ||C||:
// 3e-6 after three sweeps, 2e-24 after four, 2e-101 after five.  Four sweeps therefore already leave less than 2^-53 ||C||, the
// rounding of one operation; the fifth is the margin for a start that spends a sweep longer in the linear phase.  Its rotations have
// angles below 1e-23 (c rounds to 1), so it changes nothing in the last bit; more sweeps would add only their time.
constexpr int kSym3Sweeps = 5;

// one rotation in the (P, Q) plane, R the remaining index: Rutishauser's update (t = tan, tau = tan of the half angle)
template <int P, int Q, int R>
NESTI_EIG_HD inline void sym3_rotate(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double at = fabs(theta);
  // the root of t^2 + 2 theta t - 1 of smaller magnitude; theta^2 overflowing gives t = 0, the right limit
  double t = 1.0 / (at + sqrt(at * at + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = arp - s * (arq + tau * arp);
  a[R][Q] = arq + s * (arp - tau * arq);
  a[P][R] = a[R][P];
  a[Q][R] = a[R][Q];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = v[k][P], vq = v[k][Q];
    v[k][P] = vp - s * (vq + tau * vp);
    v[k][Q] = vq + s * (vp - tau * vq);
  }
}

// c = {xx, xy, xz, yy, yz, zz}.  w: the eigenvalues, ascending (equal ones keep the order of their diagonal positions); vec[k]: the
// eigenvector of w[k], unit up to rounding.  Non-finite input gives non-finite output and nothing else.
NESTI_EIG_HD inline void sym3_eig(const double (&c)[6], double (&w)[3], double (&vec)[3][3]) {
  double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < kSym3Sweeps; ++sweep) {
    sym3_rotate<0, 1, 2>(a, v);
    sym3_rotate<0, 2, 1>(a, v);
    sym3_rotate<1, 2, 0>(a, v);
  }
  // sort by three compare-exchanges (strict: ties stay): eigenvector k is column k of v
  double d[3] = {a[0][0], a[1][1], a[2][2]};
  double col[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    col[k][0] = v[0][k]; col[k][1] = v[1][k]; col[k][2] = v[2][k];
  }
#define NESTI_EIG_CSWAP(i, j)                                                     \
  if (d[j] < d[i]) {                                                              \
    const double td = d[i]; d[i] = d[j]; d[j] = td;                               \
    for (int k = 0; k < 3; ++k) { const double tv = col[i][k]; col[i][k] = col[j][k]; col[j][k] = tv; } \
  }
  NESTI_EIG_CSWAP(0, 1)
  NESTI_EIG_CSWAP(1, 2)
  NESTI_EIG_CSWAP(0, 1)
#undef NESTI_EIG_CSWAP
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = d[k];
    vec[k][0] = col[k][0]; vec[k][1] = col[k][1]; vec[k][2] = col[k][2];
  }
}

}  // namespace nesti
