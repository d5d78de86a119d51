// The 6 x 6 solve and the curvature arithmetic of the quadric fit (DESIGN.md 2 "Quadric fit", steps 5 and 7): what quadric.hip runs
// once per query and scale, and what the host-only entry nesti_quadric_solve runs on the CPU -- the same header, the same arithmetic.
//
// Only + - x / sqrt in fp64, every operation rounded on its own (the including unit turns contraction off), a fixed operation order and
// no data-dependent loop: the results are a pure function of the 21 moments.  Negating the moments that are odd in (u, h) negates
// a0, a2, a3, a5 and nothing else, exactly (every intermediate changes sign or does not), and with them the curvatures become
// (-k_min, -k_max), exactly: the flip property the orientation of a fitted row rests on.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NESTI_QUADRIC_HD __host__ __device__
#else
#define NESTI_QUADRIC_HD
#endif

namespace nesti {

constexpr int kQuadricMoments = 21;   // m[0..14] = sum u^p v^q, p + q <= 4, by degree and then by q; m[15..20] = sum h phi_i
constexpr int kQuadricCoeffs = 6;     // phi = (1, u, v, u^2, u v, v^2)
constexpr int kQuadricMinPoints = 6;
// a pivot s_j must exceed this times N_jj.  Cholesky of a matrix of condition kappa loses its last pivot near kappa 2^-53; 2^-44 N_jj
// stops at kappa ~ 2e13, where the solution still has two or three digits, and well before a pivot that is rounding noise.
constexpr double kQuadricPivotTol = 0x1p-44;

// the powers of u and v in phi_i, and the place of sum u^p v^q in m
NESTI_QUADRIC_HD constexpr int quadric_pu(int i) { return i == 3 ? 2 : ((i == 1 || i == 4) ? 1 : 0); }
NESTI_QUADRIC_HD constexpr int quadric_pv(int i) { return i == 5 ? 2 : ((i == 2 || i == 4) ? 1 : 0); }
NESTI_QUADRIC_HD constexpr int quadric_moment(int p, int q) { return (p + q) * (p + q + 1) / 2 + q; }
NESTI_QUADRIC_HD constexpr int quadric_n_index(int i, int j) {
  return quadric_moment(quadric_pu(i) + quadric_pu(j), quadric_pv(i) + quadric_pv(j));
}

// N a = b with N_ij = sum phi_i phi_j read from m and b = m[15..20], by Cholesky without pivoting:
//     s_j = N_jj - sum_{k<j} L_jk^2 (k ascending),  L_jj = sqrt(s_j),  L_ij = (N_ij - sum_{k<j} L_ik L_jk) / L_jj,
//     y_i = (b_i - sum_{k<i} L_ik y_k) / L_ii (i ascending),  a_i = (y_i - sum_{k>i} L_ki a_k) / L_ii (i descending, k ascending).
// Fails -- returns false and a = 0 -- unless m[0] >= 6, every s_j > 2^-44 N_jj (a zero, negative or NaN pivot fails that test) and
// every a_i is finite.
NESTI_QUADRIC_HD inline bool quadric_solve(const double (&m)[kQuadricMoments], double (&a)[kQuadricCoeffs]) {
  constexpr int K = kQuadricCoeffs;
  double L[K][K];
  bool ok = m[0] >= (double)kQuadricMinPoints;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double njj = m[quadric_n_index(j, j)];
    double s = njj;
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    ok = ok && s > kQuadricPivotTol * njj;
    const double d = sqrt(s);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double t = m[quadric_n_index(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / d;
    }
  }
  double y[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double t = m[15 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < K; ++k) t = t - L[k][i] * a[k];
    a[i] = t / L[i][i];
  }
  // a coefficient that is not finite (a NaN among the h moments, which no pivot sees; an overflow) fails the fit too: x - x is 0
  // exactly for a finite x and NaN otherwise
#pragma unroll
  for (int i = 0; i < K; ++i) ok = ok && a[i] - a[i] == 0.0;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = 0.0;
  }
  return ok;
}

// Principal curvatures of the height function h = a . phi at (u, v) = (0, 0), in the units of the fit (1 / r), positive where the
// surface bends toward the side h grows on: the eigenvalues of the shape operator written in an ORTHONORMAL tangent basis,
//     g = (a1, a2),  w = sqrt(1 + g.g),  Hh = [[2 a3, a4], [a4, 2 a5]],  P = I - g g^T / (w (1 + w)) = (I + g g^T)^(-1/2),
//     Sm = P Hh P / w  (symmetric),  k = mean +- sqrt(dif^2 + q^2).
// Symmetric, so the eigenvalues are Lipschitz in a; H +- sqrt(H^2 - K) would lose half the digits wherever the two are equal.
// k[0] >= k[1].
NESTI_QUADRIC_HD inline void quadric_curvatures(const double (&a)[kQuadricCoeffs], double (&k)[2]) {
  const double g0 = a[1], g1 = a[2];
  const double w = sqrt(1.0 + (g0 * g0 + g1 * g1));
  const double den = w * (1.0 + w);
  const double p00 = 1.0 - (g0 * g0) / den, p01 = 0.0 - (g0 * g1) / den, p11 = 1.0 - (g1 * g1) / den;
  const double h00 = 2.0 * a[3], h01 = a[4], h11 = 2.0 * a[5];
  // T = Hh P, Sm = P T / w
  const double t00 = h00 * p00 + h01 * p01, t01 = h00 * p01 + h01 * p11;
  const double t10 = h01 * p00 + h11 * p01, t11 = h01 * p01 + h11 * p11;
  const double s00 = (p00 * t00 + p01 * t10) / w, s01 = (p00 * t01 + p01 * t11) / w;
  const double s10 = (p01 * t00 + p11 * t10) / w, s11 = (p01 * t01 + p11 * t11) / w;
  const double mean = (s00 + s11) / 2.0, dif = (s00 - s11) / 2.0, q = (s01 + s10) / 2.0;
  const double rad = sqrt(dif * dif + q * q);
  k[0] = mean + rad;
  k[1] = mean - rad;
}

}  // namespace nesti
