// Stand-alone driver of the scale-selected plane fit's host side (select.hip): every argument refusal of nesti_pca_select_nbr and
// nesti_pca_select_nbr_at -- those of the list fits, the length of the ladder, a ladder that is not strictly ascending or leaves 1 .. K,
// a slack that is negative or not finite -- all of which return before any device call.  Built and run by `make asan-select` against
// the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};            // never dereferenced: the checks come first
  void* p = dummy;
  int32_t ks[NESTI_SELECT_MAX_L + 1], ks_full[NESTI_SELECT_MAX_L];
  for (int c = 0; c <= NESTI_SELECT_MAX_L; ++c) ks[c] = c + 1;                       // 1 .. 33: strictly ascending, within K
  for (int c = 0; c < NESTI_SELECT_MAX_L; ++c) ks_full[c] = NESTI_KNN_MAX_K - NESTI_SELECT_MAX_L + 1 + c;   // ends at NESTI_KNN_MAX_K
  const int32_t ks_zero[3] = {0, 16, 32}, ks_down[3] = {8, 32, 16}, ks_tie[3] = {8, 16, 16}, ks_big[3] = {8, 16, K + 1}, ks_neg[1] = {-4};

#define IDX(cloud, n, q, m, row0, nbr, k, kk, l, slack)                                                                             \
  nesti_pca_select_nbr((const float*)(cloud), n, (const int32_t*)(q), m, row0, (const int32_t*)(nbr), k, kk, l, slack, (float*)p,   \
                       (float*)p, (int32_t*)p, (int32_t*)p, (float*)p, (float*)p, (float*)p, (float*)p, (float*)p, (int32_t*)p, NULL)
#define AT(cloud, n, q, m, row0, nbr, k, kk, l, slack)                                                                              \
  nesti_pca_select_nbr_at((const float*)(cloud), n, (const float*)(q), m, (const int32_t*)(nbr), k, kk, l, slack, (float*)p,        \
                          (float*)p, (int32_t*)p, (int32_t*)p, (float*)p, (float*)p, (float*)p, (float*)p, (float*)p, (int32_t*)p, NULL)
#define BOTH(word, what, ...)                                                       \
  refused(IDX(__VA_ARGS__), word, "index: " what);                                  \
  refused(1, "nesti_pca_select_nbr:", "index: " what ": under the entry's name");   \
  refused(AT(__VA_ARGS__), word, "positions: " what);                               \
  refused(1, "nesti_pca_select_nbr_at:", "positions: " what ": under the entry's name")
  // the refusals of the list fits
  BOTH("null", "null cloud", NULL, N, p, M, 0, p, K, ks, 10, 0.0);
  BOTH("null", "null list", p, N, p, M, 0, NULL, K, ks, 10, 0.0);
  BOTH("null", "null ladder", p, N, p, M, 0, p, K, NULL, 10, 0.0);
  BOTH("empty cloud", "N = 0", p, 0, p, M, 0, p, K, ks, 10, 0.0);
  BOTH("empty cloud", "N < 0", p, -3, p, M, 0, p, K, ks, 10, 0.0);
  BOTH("K must be", "K = 0", p, N, p, M, 0, p, 0, ks, 10, 0.0);
  BOTH("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, M, 0, p, NESTI_KNN_MAX_K + 1, ks, 10, 0.0);
  BOTH("M must be", "M < 0", p, N, p, -1, 0, p, K, ks, 10, 0.0);
  refused(IDX(p, N, p, M, -1, p, K, ks, 10, 0.0), "query_row0", "index: query_row0 < 0");
  refused(IDX(p, N, NULL, M, N - M + 1, p, K, ks, 10, 0.0), "exceed the cloud", "index: rows beyond the cloud");
  refused(AT(p, N, NULL, M, 0, p, K, ks, 10, 0.0), "null query_xyz_dev", "positions: null positions");
  // the entry's own
  BOTH("L must be", "L = 0", p, N, p, M, 0, p, K, ks, 0, 0.0);
  BOTH("L must be", "L < 0", p, N, p, M, 0, p, K, ks, -1, 0.0);
  BOTH("L must be", "L = NESTI_SELECT_MAX_L + 1", p, N, p, M, 0, p, K, ks, NESTI_SELECT_MAX_L + 1, 0.0);
  BOTH("ladder must be", "k_0 = 0", p, N, p, M, 0, p, K, ks_zero, 3, 0.0);
  BOTH("ladder must be", "k_0 < 0", p, N, p, M, 0, p, K, ks_neg, 1, 0.0);
  BOTH("ladder must be", "a descending ladder", p, N, p, M, 0, p, K, ks_down, 3, 0.0);
  BOTH("ladder must be", "a repeated count", p, N, p, M, 0, p, K, ks_tie, 3, 0.0);
  BOTH("ladder must be", "the top above K", p, N, p, M, 0, p, K, ks_big, 3, 0.0);
  BOTH("slack", "slack < 0", p, N, p, M, 0, p, K, ks, 10, -1e-300);
  BOTH("slack", "slack NaN", p, N, p, M, 0, p, K, ks, 10, (double)NAN);
  BOTH("slack", "slack +inf", p, N, p, M, 0, p, K, ks, 10, (double)INFINITY);
  BOTH("slack", "slack -inf", p, N, p, M, 0, p, K, ks, 10, -(double)INFINITY);
  // M = 0 is a no-op (the ends of every range are accepted), and an argument error is still one
  if (IDX(p, N, NULL, 0, 0, p, K, ks, 1, 0.0) != 0 || AT(p, N, NULL, 0, 0, p, K, ks, NESTI_SELECT_MAX_L, 1e300) != 0 ||
      IDX(p, N, NULL, 0, N, p, NESTI_KNN_MAX_K, ks_full, NESTI_SELECT_MAX_L, 0.5) != 0) {
    printf("FAIL M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  BOTH("ladder must be", "M = 0 with a descending ladder", p, N, NULL, 0, 0, p, K, ks_down, 3, 0.0);
  BOTH("slack", "M = 0 with a NaN slack", p, N, NULL, 0, 0, p, K, ks, 10, (double)NAN);
  return finish("select_args");
}
