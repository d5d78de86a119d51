// Stand-alone driver of the normal-smoothing entry's host side (smooth.hip): every argument refusal of nesti_smooth_normals_nbr --
// those of the list fits, the null input normals, the ranges of k, cos_t and falloff, and the output that is the input -- all of which
// return before any device call, and the lane switch.  Built and run by `make asan-smooth` against the AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f}, other[4] = {0.f, 0.f, 0.f, 0.f};   // never dereferenced: the checks come first
  void* p = dummy;
  void* o = other;

#define CALL(cloud, n, nin, q, m, row0, nbr, K_, k, ct, fo, nout)                                                                      \
  nesti_smooth_normals_nbr((const float*)(cloud), n, (const float*)(nin), (const int32_t*)(q), m, row0, (const int32_t*)(nbr), K_, k, ct, \
                           fo, (float*)(nout), (float*)o, (int32_t*)o, NULL)
  const char* name = "nesti_smooth_normals_nbr";
#define REFUSED(word, what, ...)            \
  refused(CALL(__VA_ARGS__), word, what);   \
  refused(1, name, what ": under the entry's name")
  // the refusals of the list fits
  REFUSED("null", "null cloud", NULL, N, p, p, M, 0, p, K, 16, 0.7, 0.75, o);
  REFUSED("null", "null list", p, N, p, p, M, 0, NULL, K, 16, 0.7, 0.75, o);
  REFUSED("empty cloud", "N = 0", p, 0, p, p, M, 0, p, K, 16, 0.7, 0.75, o);
  REFUSED("K must be", "K = 0", p, N, p, p, M, 0, p, 0, 16, 0.7, 0.75, o);
  REFUSED("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, p, M, 0, p, NESTI_KNN_MAX_K + 1, 16, 0.7, 0.75, o);
  REFUSED("M must be", "M < 0", p, N, p, p, -1, 0, p, K, 16, 0.7, 0.75, o);
  REFUSED("query_row0", "query_row0 < 0", p, N, p, p, M, -1, p, K, 16, 0.7, 0.75, o);
  REFUSED("exceed the cloud", "rows beyond the cloud", p, N, p, NULL, M, N - M + 1, p, K, 16, 0.7, 0.75, o);
  // the pass's own
  REFUSED("null normals_in_dev", "null input normals", p, N, NULL, p, M, 0, p, K, 16, 0.7, 0.75, o);
  REFUSED("k must be", "k = 0", p, N, p, p, M, 0, p, K, 0, 0.7, 0.75, o);
  REFUSED("k must be", "k < 0", p, N, p, p, M, 0, p, K, -2, 0.7, 0.75, o);
  REFUSED("k must be", "k = K + 1", p, N, p, p, M, 0, p, K, K + 1, 0.7, 0.75, o);
  REFUSED("cos_t", "cos_t < 0", p, N, p, p, M, 0, p, K, 16, -1e-9, 0.75, o);
  REFUSED("cos_t", "cos_t = 1", p, N, p, p, M, 0, p, K, 16, 1.0, 0.75, o);
  REFUSED("cos_t", "cos_t just above 0.999999", p, N, p, p, M, 0, p, K, 16, 0.9999991, 0.75, o);
  REFUSED("cos_t", "cos_t NaN", p, N, p, p, M, 0, p, K, 16, (double)NAN, 0.75, o);
  REFUSED("cos_t", "cos_t inf", p, N, p, p, M, 0, p, K, 16, (double)INFINITY, 0.75, o);
  REFUSED("falloff", "falloff < 0", p, N, p, p, M, 0, p, K, 16, 0.7, -0.01, o);
  REFUSED("falloff", "falloff > 1", p, N, p, p, M, 0, p, K, 16, 0.7, 1.01, o);
  REFUSED("falloff", "falloff NaN", p, N, p, p, M, 0, p, K, 16, 0.7, (double)NAN, o);
  REFUSED("falloff", "falloff -inf", p, N, p, p, M, 0, p, K, 16, 0.7, -(double)INFINITY, o);
  REFUSED("must not be normals_in_dev", "the output is the input", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, p);
  // M = 0 is a no-op (the ends of every range are accepted), and an argument error is still one
  if (CALL(p, N, p, NULL, 0, 0, p, K, 1, 0.0, 0.0, o) != 0 || CALL(p, N, p, NULL, 0, 0, p, K, K, 0.999999, 1.0, o) != 0 ||
      CALL(p, N, p, NULL, 0, N, p, NESTI_KNN_MAX_K, NESTI_KNN_MAX_K, 0.5, 0.5, NULL) != 0) {
    printf("FAIL M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  REFUSED("cos_t", "M = 0 with a NaN cos_t", p, N, p, NULL, 0, 0, p, K, 16, (double)NAN, 0.75, o);
  REFUSED("must not be normals_in_dev", "M = 0 with the output the input", p, N, p, NULL, 0, 0, p, K, 16, 0.7, 0.75, p);
  lane_switch_refusals(nesti_debug_smooth_lanes, "nesti_debug_smooth_lanes");
  return finish("smooth_args");
}
