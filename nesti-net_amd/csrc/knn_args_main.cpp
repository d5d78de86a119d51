// Stand-alone driver of the k-nearest-neighbour entries' host side (knn.hip): every argument refusal of the search (nesti_knn,
// nesti_knn_at) and of the two fits over neighbour lists (nesti_pca_normals_nbr*, nesti_quadric_fit_nbr*), all of which return before any
// device call.  Built and run by `make asan-knn` against the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};            // never dereferenced: the checks come first
  void* p = dummy;
  const size_t gws = nesti_patches_workspace_bytes(N);

  // ---- the search --------------------------------------------------------------------------------------------------------------------
#define IDX(cloud, n, q, m, row0, k, nbr, g, gb) \
  nesti_knn((const float*)(cloud), n, (const int32_t*)(q), m, row0, k, (int32_t*)(nbr), (double*)p, (int32_t*)p, g, gb, NULL)
#define AT(cloud, n, q, m, row0, k, nbr, g, gb) \
  nesti_knn_at((const float*)(cloud), n, (const float*)(q), m, k, (int32_t*)(nbr), (double*)p, (int32_t*)p, g, gb, NULL)
#define BOTH(word, what, ...)                         \
  refused(IDX(__VA_ARGS__), word, "index: " what);    \
  refused(AT(__VA_ARGS__), word, "positions: " what)
  BOTH("null", "null cloud", NULL, N, p, M, 0, K, p, p, gws);
  BOTH("null", "null neighbour output", p, N, p, M, 0, K, NULL, p, gws);
  BOTH("null", "null grid workspace", p, N, p, M, 0, K, p, NULL, gws);
  BOTH("empty cloud", "N = 0", p, 0, p, M, 0, K, p, p, gws);
  BOTH("empty cloud", "N < 0", p, -5, p, M, 0, K, p, p, gws);
  BOTH("K must be", "K = 0", p, N, p, M, 0, 0, p, p, gws);
  BOTH("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, M, 0, NESTI_KNN_MAX_K + 1, p, p, gws);
  BOTH("M must be", "M < 0", p, N, p, -1, 0, K, p, p, gws);
  BOTH("workspace too small", "short grid workspace", p, N, p, M, 0, K, p, p, gws - 1);
  refused(IDX(p, N, p, M, -1, K, p, p, gws), "query_row0", "index: query_row0 < 0");
  refused(IDX(p, N, NULL, M, N - M + 1, K, p, p, gws), "exceed the cloud", "index: rows beyond the cloud");
  refused(AT(p, N, NULL, M, 0, K, p, p, gws), "null query_xyz_dev", "positions: null positions");
  // M = 0 is a no-op, and an argument error is still one
  if (IDX(p, N, NULL, 0, 0, K, p, p, gws) != 0 || AT(p, N, NULL, 0, 0, K, p, p, gws) != 0) {
    printf("FAIL search: M = 0 is a no-op\n");
    ++failures;
  }
  refused(IDX(p, N, NULL, 0, 0, 0, p, p, gws), "K must be", "index: M = 0 with K = 0");
#undef IDX
#undef AT

  // ---- the fits over neighbour lists ---------------------------------------------------------------------------------------------------
  const int32_t ks[4] = {8, 16, 32, 64}, ks_zero[4] = {0, 16, 32, 64}, ks_down[4] = {8, 32, 16, 64}, ks_big[4] = {8, 16, 32, K + 1};
#define PCA_IDX(cloud, n, q, m, row0, nbr, k, kk, s) \
  nesti_pca_normals_nbr((const float*)(cloud), n, (const int32_t*)(q), m, row0, (const int32_t*)(nbr), k, kk, s, (float*)p, (float*)p, \
                        (float*)p, (int32_t*)p, NULL)
#define PCA_AT(cloud, n, q, m, row0, nbr, k, kk, s) \
  nesti_pca_normals_nbr_at((const float*)(cloud), n, (const float*)(q), m, (const int32_t*)(nbr), k, kk, s, (float*)p, (float*)p, \
                           (float*)p, (int32_t*)p, NULL)
#define QUAD_IDX(cloud, n, q, m, row0, nbr, k, kk, s) \
  nesti_quadric_fit_nbr((const float*)(cloud), n, (const int32_t*)(q), m, row0, (const int32_t*)(nbr), k, kk, s, (float*)p, (float*)p, \
                        (float*)p, (float*)p, (int32_t*)p, NULL)
#define QUAD_AT(cloud, n, q, m, row0, nbr, k, kk, s) \
  nesti_quadric_fit_nbr_at((const float*)(cloud), n, (const float*)(q), m, (const int32_t*)(nbr), k, kk, s, (float*)p, (float*)p, \
                           (float*)p, (float*)p, (int32_t*)p, NULL)
#define ALL(word, what, ...)                                        \
  refused(PCA_IDX(__VA_ARGS__), word, "plane, index: " what);       \
  refused(PCA_AT(__VA_ARGS__), word, "plane, positions: " what);    \
  refused(QUAD_IDX(__VA_ARGS__), word, "quadric, index: " what);    \
  refused(QUAD_AT(__VA_ARGS__), word, "quadric, positions: " what)
  ALL("null", "null cloud", NULL, N, p, M, 0, p, K, ks, 4);
  ALL("null", "null list", p, N, p, M, 0, NULL, K, ks, 4);
  ALL("null", "null ks", p, N, p, M, 0, p, K, NULL, 4);
  ALL("empty cloud", "N = 0", p, 0, p, M, 0, p, K, ks, 4);
  ALL("K must be", "K = 0", p, N, p, M, 0, p, 0, ks, 4);
  ALL("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, M, 0, p, NESTI_KNN_MAX_K + 1, ks, 4);
  ALL("n_scales", "S = 0", p, N, p, M, 0, p, K, ks, 0);
  ALL("n_scales", "S = NESTI_MAX_SCALES + 1", p, N, p, M, 0, p, K, ks, NESTI_MAX_SCALES + 1);
  ALL("ks must be", "k_0 = 0", p, N, p, M, 0, p, K, ks_zero, 4);
  ALL("ks must be", "ks not ascending", p, N, p, M, 0, p, K, ks_down, 4);
  ALL("ks must be", "k_3 > K", p, N, p, M, 0, p, K, ks_big, 4);
  ALL("M must be", "M < 0", p, N, p, -1, 0, p, K, ks, 4);
  refused(PCA_IDX(p, N, p, M, -1, p, K, ks, 4), "query_row0", "plane, index: query_row0 < 0");
  refused(QUAD_IDX(p, N, p, M, -1, p, K, ks, 4), "query_row0", "quadric, index: query_row0 < 0");
  refused(PCA_IDX(p, N, NULL, M, N - M + 1, p, K, ks, 4), "exceed the cloud", "plane, index: rows beyond the cloud");
  refused(QUAD_IDX(p, N, NULL, M, N - M + 1, p, K, ks, 4), "exceed the cloud", "quadric, index: rows beyond the cloud");
  refused(PCA_AT(p, N, NULL, M, 0, p, K, ks, 4), "null query_xyz_dev", "plane, positions: null positions");
  refused(QUAD_AT(p, N, NULL, M, 0, p, K, ks, 4), "null query_xyz_dev", "quadric, positions: null positions");
  if (PCA_IDX(p, N, NULL, 0, 0, p, K, ks, 4) != 0 || PCA_AT(p, N, NULL, 0, 0, p, K, ks, 4) != 0 ||
      QUAD_IDX(p, N, NULL, 0, 0, p, K, ks, 4) != 0 || QUAD_AT(p, N, NULL, 0, 0, p, K, ks, 4) != 0) {
    printf("FAIL fits: M = 0 is a no-op\n");
    ++failures;
  }
  refused(PCA_IDX(p, N, NULL, 0, 0, p, K, ks_down, 4), "ks must be", "plane, index: M = 0 with descending ks");
  return finish("knn_args");
}
