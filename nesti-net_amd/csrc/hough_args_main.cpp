// Stand-alone driver of the Hough-transform entries' host side (hough.hip): every argument refusal of nesti_hough_normals_nbr and
// nesti_hough_normals_nbr_at -- those of the list fits, the ranges of T, B and R, and the rotation table's -- all of which return before
// any device call.  Built and run by `make asan-hough` against the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};            // never dereferenced: the checks come first
  void* p = dummy;
  const int32_t ks[4] = {8, 16, 32, 64}, ks_zero[4] = {0, 16, 32, 64}, ks_down[4] = {8, 32, 16, 64}, ks_big[4] = {8, 16, 32, K + 1};
  // eight rotations about z by 0.1 r: orthonormal to rounding, the first the identity
  double rot[NESTI_HOUGH_MAX_ROT * 9];
  for (int r = 0; r < NESTI_HOUGH_MAX_ROT; ++r) {
    const double c = cos(0.1 * r), s = sin(0.1 * r);
    const double m[9] = {c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0};
    memcpy(rot + r * 9, m, sizeof(m));
  }
  double rot_nan[NESTI_HOUGH_MAX_ROT * 9], rot_inf[NESTI_HOUGH_MAX_ROT * 9], rot_skew[NESTI_HOUGH_MAX_ROT * 9],
      rot_scaled[NESTI_HOUGH_MAX_ROT * 9], rot_tail[NESTI_HOUGH_MAX_ROT * 9];
  memcpy(rot_nan, rot, sizeof(rot));
  memcpy(rot_inf, rot, sizeof(rot));
  memcpy(rot_skew, rot, sizeof(rot));
  memcpy(rot_scaled, rot, sizeof(rot));
  memcpy(rot_tail, rot, sizeof(rot));
  rot_nan[2 * 9 + 4] = NAN;
  rot_inf[0] = INFINITY;
  rot_skew[1 * 9 + 1] += 1e-5;                      // max |rot rot^T - I| about 2e-5
  for (int k = 0; k < 9; ++k) rot_scaled[4 * 9 + k] *= 2.0;
  for (int k = 0; k < 9; ++k) rot_tail[7 * 9 + k] = NAN;   // beyond R = 5: never read

#define IDX(cloud, n, q, m, row0, nbr, k, kk, s, T, B, R, rt)                                                                       \
  nesti_hough_normals_nbr((const float*)(cloud), n, (const int32_t*)(q), m, row0, (const int32_t*)(nbr), k, kk, s, T, B, R, rt, 7u, \
                          (float*)p, (float*)p, (int32_t*)p, (float*)p, (int32_t*)p, NULL)
#define AT(cloud, n, q, m, row0, nbr, k, kk, s, T, B, R, rt)                                                                         \
  nesti_hough_normals_nbr_at((const float*)(cloud), n, (const float*)(q), m, row0, (const int32_t*)(nbr), k, kk, s, T, B, R, rt, 7u, \
                             (float*)p, (float*)p, (int32_t*)p, (float*)p, (int32_t*)p, NULL)
#define BOTH(word, what, ...)                       \
  refused(IDX(__VA_ARGS__), word, "index: " what);  \
  refused(AT(__VA_ARGS__), word, "positions: " what)
  // the refusals of the list fits
  BOTH("null", "null cloud", NULL, N, p, M, 0, p, K, ks, 4, 100, 16, 5, rot);
  BOTH("null", "null list", p, N, p, M, 0, NULL, K, ks, 4, 100, 16, 5, rot);
  BOTH("null", "null ks", p, N, p, M, 0, p, K, NULL, 4, 100, 16, 5, rot);
  BOTH("empty cloud", "N = 0", p, 0, p, M, 0, p, K, ks, 4, 100, 16, 5, rot);
  BOTH("K must be", "K = 0", p, N, p, M, 0, p, 0, ks, 4, 100, 16, 5, rot);
  BOTH("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, M, 0, p, NESTI_KNN_MAX_K + 1, ks, 4, 100, 16, 5, rot);
  BOTH("n_scales", "S = 0", p, N, p, M, 0, p, K, ks, 0, 100, 16, 5, rot);
  BOTH("n_scales", "S = NESTI_MAX_SCALES + 1", p, N, p, M, 0, p, K, ks, NESTI_MAX_SCALES + 1, 100, 16, 5, rot);
  BOTH("ks must be", "k_0 = 0", p, N, p, M, 0, p, K, ks_zero, 4, 100, 16, 5, rot);
  BOTH("ks must be", "ks not ascending", p, N, p, M, 0, p, K, ks_down, 4, 100, 16, 5, rot);
  BOTH("ks must be", "k_3 > K", p, N, p, M, 0, p, K, ks_big, 4, 100, 16, 5, rot);
  BOTH("M must be", "M < 0", p, N, p, -1, 0, p, K, ks, 4, 100, 16, 5, rot);
  BOTH("query_row0", "query_row0 < 0", p, N, p, M, -1, p, K, ks, 4, 100, 16, 5, rot);
  refused(IDX(p, N, NULL, M, N - M + 1, p, K, ks, 4, 100, 16, 5, rot), "exceed the cloud", "index: rows beyond the cloud");
  refused(AT(p, N, NULL, M, 0, p, K, ks, 4, 100, 16, 5, rot), "null query_xyz_dev", "positions: null positions");
  // the estimator's own
  BOTH("T (triplets)", "T = 0", p, N, p, M, 0, p, K, ks, 4, 0, 16, 5, rot);
  BOTH("T (triplets)", "T < 0", p, N, p, M, 0, p, K, ks, 4, -3, 16, 5, rot);
  BOTH("T (triplets)", "T = NESTI_HOUGH_MAX_T + 1", p, N, p, M, 0, p, K, ks, 4, NESTI_HOUGH_MAX_T + 1, 16, 5, rot);
  BOTH("B (bins per axis)", "B = 1", p, N, p, M, 0, p, K, ks, 4, 100, 1, 5, rot);
  BOTH("B (bins per axis)", "B = NESTI_HOUGH_MAX_BINS + 1", p, N, p, M, 0, p, K, ks, 4, 100, NESTI_HOUGH_MAX_BINS + 1, 5, rot);
  BOTH("R (rotations)", "R = 0", p, N, p, M, 0, p, K, ks, 4, 100, 16, 0, rot);
  BOTH("R (rotations)", "R = NESTI_HOUGH_MAX_ROT + 1", p, N, p, M, 0, p, K, ks, 4, 100, 16, NESTI_HOUGH_MAX_ROT + 1, rot);
  BOTH("null rot", "null rotation table", p, N, p, M, 0, p, K, ks, 4, 100, 16, 5, (const double*)NULL);
  BOTH("rotation 2 is not finite", "a NaN entry", p, N, p, M, 0, p, K, ks, 4, 100, 16, 5, rot_nan);
  BOTH("rotation 0 is not finite", "an infinite entry", p, N, p, M, 0, p, K, ks, 4, 100, 16, 5, rot_inf);
  BOTH("rotation 1 is not orthonormal", "a skewed rotation", p, N, p, M, 0, p, K, ks, 4, 100, 16, 5, rot_skew);
  BOTH("rotation 4 is not orthonormal", "a scaled rotation", p, N, p, M, 0, p, K, ks, 4, 100, 16, 5, rot_scaled);
  // M = 0 is a no-op (rotations beyond R are not read), and an argument error is still one; the largest parameters are accepted
  if (IDX(p, N, NULL, 0, 0, p, K, ks, 4, 100, 16, 5, rot_tail) != 0 || AT(p, N, NULL, 0, 0, p, K, ks, 4, 100, 16, 5, rot_tail) != 0 ||
      IDX(p, N, NULL, 0, 0, p, K, ks, 4, NESTI_HOUGH_MAX_T, NESTI_HOUGH_MAX_BINS, NESTI_HOUGH_MAX_ROT, rot) != 0 ||
      AT(p, N, NULL, 0, 0, p, K, ks, 1, 1, 2, 1, rot) != 0) {
    printf("FAIL M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  refused(IDX(p, N, NULL, 0, 0, p, K, ks, 4, 100, 16, 8, rot_tail), "rotation 7 is not finite", "index: M = 0 with a NaN rotation inside R");
  refused(AT(p, N, NULL, 0, 0, p, K, ks, 4, 0, 16, 5, rot), "T (triplets)", "positions: M = 0 with T = 0");
  return finish("hough_args");
}
