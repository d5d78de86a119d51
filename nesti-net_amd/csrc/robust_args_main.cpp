// Stand-alone driver of the robust plane fit's host side (robust.hip): every argument refusal of nesti_robust_normals_nbr and
// nesti_robust_normals_nbr_at -- those of the list fits and the ranges of iters, sigma, falloff and floor -- all of which return before
// any device call.  Built and run by `make asan-robust` against the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};            // never dereferenced: the checks come first
  void* p = dummy;
  const int32_t ks[4] = {8, 16, 32, 64}, ks_zero[4] = {0, 16, 32, 64}, ks_down[4] = {8, 32, 16, 64}, ks_big[4] = {8, 16, 32, K + 1};

#define OUTS (const float*)p, (float*)p, (float*)p, (float*)p, (int32_t*)p, (int32_t*)p, (double*)p, (float*)p, (int32_t*)p, NULL
#define IDX(cloud, n, q, m, row0, nbr, k, kk, s, it, sg, fo, fl) \
  nesti_robust_normals_nbr((const float*)(cloud), n, (const int32_t*)(q), m, row0, (const int32_t*)(nbr), k, kk, s, it, sg, fo, fl, OUTS)
#define AT(cloud, n, q, m, row0, nbr, k, kk, s, it, sg, fo, fl) \
  nesti_robust_normals_nbr_at((const float*)(cloud), n, (const float*)(q), m, (const int32_t*)(nbr), k, kk, s, it, sg, fo, fl, OUTS)
#define BOTH(word, what, ...)                       \
  refused(IDX(__VA_ARGS__), word, "index: " what);  \
  refused(AT(__VA_ARGS__), word, "positions: " what)
  // the refusals of the list fits
  BOTH("null", "null cloud", NULL, N, p, M, 0, p, K, ks, 4, 8, 2.0, 0.5, 0.01);
  BOTH("null", "null list", p, N, p, M, 0, NULL, K, ks, 4, 8, 2.0, 0.5, 0.01);
  BOTH("null", "null ks", p, N, p, M, 0, p, K, NULL, 4, 8, 2.0, 0.5, 0.01);
  BOTH("empty cloud", "N = 0", p, 0, p, M, 0, p, K, ks, 4, 8, 2.0, 0.5, 0.01);
  BOTH("K must be", "K = 0", p, N, p, M, 0, p, 0, ks, 4, 8, 2.0, 0.5, 0.01);
  BOTH("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, M, 0, p, NESTI_KNN_MAX_K + 1, ks, 4, 8, 2.0, 0.5, 0.01);
  BOTH("n_scales", "S = 0", p, N, p, M, 0, p, K, ks, 0, 8, 2.0, 0.5, 0.01);
  BOTH("n_scales", "S = NESTI_MAX_SCALES + 1", p, N, p, M, 0, p, K, ks, NESTI_MAX_SCALES + 1, 8, 2.0, 0.5, 0.01);
  BOTH("ks must be", "k_0 = 0", p, N, p, M, 0, p, K, ks_zero, 4, 8, 2.0, 0.5, 0.01);
  BOTH("ks must be", "ks not ascending", p, N, p, M, 0, p, K, ks_down, 4, 8, 2.0, 0.5, 0.01);
  BOTH("ks must be", "k_3 > K", p, N, p, M, 0, p, K, ks_big, 4, 8, 2.0, 0.5, 0.01);
  BOTH("M must be", "M < 0", p, N, p, -1, 0, p, K, ks, 4, 8, 2.0, 0.5, 0.01);
  refused(IDX(p, N, p, M, -1, p, K, ks, 4, 8, 2.0, 0.5, 0.01), "query_row0", "index: query_row0 < 0");
  refused(IDX(p, N, NULL, M, N - M + 1, p, K, ks, 4, 8, 2.0, 0.5, 0.01), "exceed the cloud", "index: rows beyond the cloud");
  refused(AT(p, N, NULL, M, 0, p, K, ks, 4, 8, 2.0, 0.5, 0.01), "null query_xyz_dev", "positions: null positions");
  // the estimator's own
  BOTH("iters must be", "iters < 0", p, N, p, M, 0, p, K, ks, 4, -1, 2.0, 0.5, 0.01);
  BOTH("iters must be", "iters = NESTI_ROBUST_MAX_ITERS + 1", p, N, p, M, 0, p, K, ks, 4, NESTI_ROBUST_MAX_ITERS + 1, 2.0, 0.5, 0.01);
  BOTH("sigma must be", "sigma = 0", p, N, p, M, 0, p, K, ks, 4, 8, 0.0, 0.5, 0.01);
  BOTH("sigma must be", "sigma < 0", p, N, p, M, 0, p, K, ks, 4, 8, -2.0, 0.5, 0.01);
  BOTH("sigma must be", "sigma > 1e6", p, N, p, M, 0, p, K, ks, 4, 8, 1.0000001e6, 0.5, 0.01);
  BOTH("sigma must be", "sigma NaN", p, N, p, M, 0, p, K, ks, 4, 8, (double)NAN, 0.5, 0.01);
  BOTH("sigma must be", "sigma inf", p, N, p, M, 0, p, K, ks, 4, 8, (double)INFINITY, 0.5, 0.01);
  BOTH("falloff must be", "falloff < 0", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, -0.001, 0.01);
  BOTH("falloff must be", "falloff > 1", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, 1.001, 0.01);
  BOTH("falloff must be", "falloff NaN", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, (double)NAN, 0.01);
  BOTH("floor must be", "floor = 0", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, 0.5, 0.0);
  BOTH("floor must be", "floor < 1e-6", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, 0.5, 0.9e-6);
  BOTH("floor must be", "floor > 1", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, 0.5, 1.5);
  BOTH("floor must be", "floor NaN", p, N, p, M, 0, p, K, ks, 4, 8, 2.0, 0.5, (double)NAN);
  // M = 0 is a no-op at both ends of every range, and an argument error is still one
  if (IDX(p, N, NULL, 0, 0, p, K, ks, 4, 0, 1e6, 0.0, 1e-6) != 0 || AT(p, N, NULL, 0, 0, p, K, ks, 4, 0, 1e6, 0.0, 1e-6) != 0 ||
      IDX(p, N, NULL, 0, 0, p, K, ks, 4, NESTI_ROBUST_MAX_ITERS, 1e-300, 1.0, 1.0) != 0 ||
      AT(p, N, NULL, 0, 0, p, K, ks, 1, NESTI_ROBUST_MAX_ITERS, 1e-300, 1.0, 1.0) != 0) {
    printf("FAIL M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  refused(IDX(p, N, NULL, 0, 0, p, K, ks, 4, 65, 2.0, 0.5, 0.01), "iters must be", "index: M = 0 with iters = 65");
  refused(AT(p, N, NULL, 0, 0, p, K, ks, 4, 8, 2.0, 0.5, 2.0), "floor must be", "positions: M = 0 with floor = 2");
  return finish("robust_args");
}
