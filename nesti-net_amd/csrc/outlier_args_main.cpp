// Stand-alone driver of the outlier filter's host side (outlier.hip): the workspace size and every argument refusal of
// nesti_outlier_scores_nbr, nesti_outlier_threshold, nesti_outlier_compact and nesti_debug_outlier_lanes, all of which return before
// any device call.  Built and run by `make asan-outlier` against the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  double dummy[4] = {0.0, 0.0, 0.0, 0.0};   // never dereferenced: the checks come first
  void* p = dummy;
  const size_t ws = nesti_outlier_workspace_bytes(N);

  // ---- the workspace size --------------------------------------------------------------------------------------------------------------
  if (nesti_outlier_workspace_bytes(0) != 0 || nesti_outlier_workspace_bytes(-5) != 0 || ws == 0 || ws % 256 != 0 ||
      nesti_outlier_workspace_bytes(1) == 0 || nesti_outlier_workspace_bytes(1 << 20) < nesti_outlier_workspace_bytes(1000) ||
      nesti_outlier_workspace_bytes(2147483647) < (size_t)2147483647 / 256 * 16) {
    printf("FAIL nesti_outlier_workspace_bytes\n");
    ++failures;
  }

  // ---- nesti_outlier_scores_nbr ----------------------------------------------------------------------------------------------------------
#define SCORES(cloud, n, row0, m, nbr, K_, k) \
  nesti_outlier_scores_nbr((const float*)(cloud), n, row0, m, (const int32_t*)(nbr), K_, k, (double*)p, (double*)p, (int32_t*)p, NULL)
  const char* name = "nesti_outlier_scores_nbr";
#define REFUSED(CALL, word, what, ...)      \
  refused(CALL(__VA_ARGS__), word, what);   \
  refused(1, name, what ": under the entry's name")
  REFUSED(SCORES, "null", "scores: null cloud", NULL, N, 0, M, p, K, 16);
  REFUSED(SCORES, "null", "scores: null list", p, N, 0, M, NULL, K, 16);
  REFUSED(SCORES, "empty cloud", "scores: N = 0", p, 0, 0, M, p, K, 16);
  REFUSED(SCORES, "empty cloud", "scores: N < 0", p, -3, 0, M, p, K, 16);
  REFUSED(SCORES, "K must be", "scores: K = 0", p, N, 0, M, p, 0, 16);
  REFUSED(SCORES, "K must be", "scores: K = NESTI_KNN_MAX_K + 1", p, N, 0, M, p, NESTI_KNN_MAX_K + 1, 16);
  REFUSED(SCORES, "k must be", "scores: k = 0", p, N, 0, M, p, K, 0);
  REFUSED(SCORES, "k must be", "scores: k < 0", p, N, 0, M, p, K, -1);
  REFUSED(SCORES, "k must be", "scores: k = K", p, N, 0, M, p, K, K);
  REFUSED(SCORES, "k must be", "scores: k = 1 at K = 1", p, N, 0, M, p, 1, 1);
  REFUSED(SCORES, "k must be", "scores: k = NESTI_KNN_MAX_K", p, N, 0, M, p, NESTI_KNN_MAX_K, NESTI_KNN_MAX_K);
  REFUSED(SCORES, "M must be", "scores: M < 0", p, N, 0, -1, p, K, 16);
  REFUSED(SCORES, "query_row0", "scores: query_row0 < 0", p, N, -1, M, p, K, 16);
  REFUSED(SCORES, "exceed the cloud", "scores: rows beyond the cloud", p, N, N - M + 1, M, p, K, 16);
  // M = 0 is a no-op (the ends of every range are accepted), and an argument error is still one
  if (SCORES(p, N, 0, 0, p, 2, 1) != 0 || SCORES(p, N, N, 0, p, NESTI_KNN_MAX_K, NESTI_KNN_MAX_K - 1) != 0) {
    printf("FAIL scores: M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  REFUSED(SCORES, "k must be", "scores: M = 0 with k = K", p, N, 0, 0, p, K, K);

  // ---- nesti_outlier_threshold -------------------------------------------------------------------------------------------------------------
#define THRESHOLD(scores, m, ratio, stats, ws_, bytes) \
  nesti_outlier_threshold((const double*)(scores), m, ratio, (double*)(stats), ws_, bytes, NULL)
  name = "nesti_outlier_threshold";
  REFUSED(THRESHOLD, "null", "threshold: null scores", NULL, M, 1.0, p, p, ws);
  REFUSED(THRESHOLD, "null", "threshold: null stats", p, M, 1.0, NULL, p, ws);
  REFUSED(THRESHOLD, "null", "threshold: null workspace", p, M, 1.0, p, NULL, ws);
  REFUSED(THRESHOLD, "M must be", "threshold: M < 0", p, -1, 1.0, p, p, ws);
  REFUSED(THRESHOLD, "std_ratio", "threshold: std_ratio < 0", p, M, -1e-9, p, p, ws);
  REFUSED(THRESHOLD, "std_ratio", "threshold: std_ratio NaN", p, M, (double)NAN, p, p, ws);
  REFUSED(THRESHOLD, "std_ratio", "threshold: std_ratio inf", p, M, (double)INFINITY, p, p, ws);
  REFUSED(THRESHOLD, "workspace too small", "threshold: short workspace", p, N, 1.0, p, p, ws - 1);
  REFUSED(THRESHOLD, "workspace too small", "threshold: no workspace bytes", p, 1, 1.0, p, p, (size_t)0);
  if (THRESHOLD(p, 0, 0.0, p, p, (size_t)0) != 0) {
    printf("FAIL threshold: M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  REFUSED(THRESHOLD, "std_ratio", "threshold: M = 0 with a NaN std_ratio", p, 0, (double)NAN, p, p, ws);

  // ---- nesti_outlier_compact ---------------------------------------------------------------------------------------------------------------
#define COMPACT(cloud, n, scores, thr_dev, thr, xyz, n_kept, ws_, bytes)                                                              \
  nesti_outlier_compact((const float*)(cloud), n, (const double*)(scores), (const double*)(thr_dev), thr, (float*)(xyz), (int32_t*)p, \
                        (int32_t*)p, (uint8_t*)p, (int32_t*)(n_kept), ws_, bytes, NULL)
  name = "nesti_outlier_compact";
  REFUSED(COMPACT, "null", "compact: null scores", p, N, NULL, NULL, 1.0, p, p, p, ws);
  REFUSED(COMPACT, "null", "compact: null n_kept", p, N, p, NULL, 1.0, p, NULL, p, ws);
  REFUSED(COMPACT, "null", "compact: null workspace", p, N, p, NULL, 1.0, p, p, NULL, ws);
  REFUSED(COMPACT, "null", "compact: points asked for without a cloud", NULL, N, p, NULL, 1.0, p, p, p, ws);
  REFUSED(COMPACT, "empty cloud", "compact: N = 0", p, 0, p, NULL, 1.0, p, p, p, ws);
  REFUSED(COMPACT, "empty cloud", "compact: N < 0", p, -1, p, NULL, 1.0, p, p, p, ws);
  REFUSED(COMPACT, "thr must be", "compact: host thr < 0", p, N, p, NULL, -1e-9, p, p, p, ws);
  REFUSED(COMPACT, "thr must be", "compact: host thr NaN", p, N, p, NULL, (double)NAN, p, p, p, ws);
  REFUSED(COMPACT, "thr must be", "compact: host thr inf", p, N, p, NULL, (double)INFINITY, p, p, p, ws);
  REFUSED(COMPACT, "workspace too small", "compact: short workspace", p, N, p, NULL, 1.0, p, p, p, ws - 1);
  // a device threshold makes the host value meaningless: it is not looked at (the short workspace is what is refused)
  REFUSED(COMPACT, "workspace too small", "compact: device thr, NaN host thr, short workspace", p, N, p, p, (double)NAN, p, p, p, ws - 1);

  // ---- nesti_debug_outlier_lanes -----------------------------------------------------------------------------------------------------------
  lane_switch_refusals(nesti_debug_outlier_lanes, "nesti_debug_outlier_lanes");
  return finish("outlier_args");
}
