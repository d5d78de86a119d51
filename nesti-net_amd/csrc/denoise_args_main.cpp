// Stand-alone driver of the point-denoising entry's host side (denoise.hip): every argument refusal of nesti_denoise_points_nbr --
// those of the list fits, the null input normals, the ranges of k, cos_t, falloff, sigma and step, and the output that lies inside the
// cloud -- all of which return before any device call, and the lane switch.  Built and run by `make asan-denoise` against the
// AddressSanitizer build of the library.
#include "args_main.h"

int main() {
  const int N = 1000, M = 100, K = 64;
  // never dereferenced: the checks come first.  One block, so that the cloud [N,3] and the outputs [M,3] are known not to meet
  static float block[3 * N + 3 * M + 8];
  void* p = block;                     // the cloud, and every other input
  void* o = block + 3 * N;             // the outputs: behind the cloud's last row

#define CALL(cloud, n, nin, q, m, row0, nbr, K_, k, ct, fo, sg, st, pout)                                                                 \
  nesti_denoise_points_nbr((const float*)(cloud), n, (const float*)(nin), (const int32_t*)(q), m, row0, (const int32_t*)(nbr), K_, k, ct, \
                           fo, sg, st, (float*)(pout), (float*)o, (float*)o, (int32_t*)o, NULL)
  const char* name = "nesti_denoise_points_nbr";
#define REFUSED(word, what, ...)            \
  refused(CALL(__VA_ARGS__), word, what);   \
  refused(1, name, what ": under the entry's name")
  // the refusals of the list fits
  REFUSED("null", "null cloud", NULL, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("null", "null list", p, N, p, p, M, 0, NULL, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("empty cloud", "N = 0", p, 0, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("K must be", "K = 0", p, N, p, p, M, 0, p, 0, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("K must be", "K = NESTI_KNN_MAX_K + 1", p, N, p, p, M, 0, p, NESTI_KNN_MAX_K + 1, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("M must be", "M < 0", p, N, p, p, -1, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("query_row0", "query_row0 < 0", p, N, p, p, M, -1, p, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("exceed the cloud", "rows beyond the cloud", p, N, p, NULL, M, N - M + 1, p, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  // the pass's own
  REFUSED("null normals_in_dev", "null input normals", p, N, NULL, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("k must be", "k = 0", p, N, p, p, M, 0, p, K, 0, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("k must be", "k < 0", p, N, p, p, M, 0, p, K, -2, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("k must be", "k = K + 1", p, N, p, p, M, 0, p, K, K + 1, 0.7, 0.75, 0.5, 1.0, o);
  REFUSED("cos_t", "cos_t < 0", p, N, p, p, M, 0, p, K, 16, -1e-9, 0.75, 0.5, 1.0, o);
  REFUSED("cos_t", "cos_t = 1", p, N, p, p, M, 0, p, K, 16, 1.0, 0.75, 0.5, 1.0, o);
  REFUSED("cos_t", "cos_t just above 0.999999", p, N, p, p, M, 0, p, K, 16, 0.9999991, 0.75, 0.5, 1.0, o);
  REFUSED("cos_t", "cos_t NaN", p, N, p, p, M, 0, p, K, 16, (double)NAN, 0.75, 0.5, 1.0, o);
  REFUSED("cos_t", "cos_t inf", p, N, p, p, M, 0, p, K, 16, (double)INFINITY, 0.75, 0.5, 1.0, o);
  REFUSED("falloff", "falloff < 0", p, N, p, p, M, 0, p, K, 16, 0.7, -0.01, 0.5, 1.0, o);
  REFUSED("falloff", "falloff > 1", p, N, p, p, M, 0, p, K, 16, 0.7, 1.01, 0.5, 1.0, o);
  REFUSED("falloff", "falloff NaN", p, N, p, p, M, 0, p, K, 16, 0.7, (double)NAN, 0.5, 1.0, o);
  REFUSED("falloff", "falloff -inf", p, N, p, p, M, 0, p, K, 16, 0.7, -(double)INFINITY, 0.5, 1.0, o);
  REFUSED("sigma", "sigma = 0", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.0, 1.0, o);
  REFUSED("sigma", "sigma < 0", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, -0.5, 1.0, o);
  REFUSED("sigma", "sigma just above 1e6", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 1000000.0000001, 1.0, o);
  REFUSED("sigma", "sigma NaN", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, (double)NAN, 1.0, o);
  REFUSED("sigma", "sigma inf", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, (double)INFINITY, 1.0, o);
  REFUSED("step", "step = 0", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 0.0, o);
  REFUSED("step", "step < 0", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, -0.5, o);
  REFUSED("step", "step just above 1", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0000000001, o);
  REFUSED("step", "step NaN", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, (double)NAN, o);
  REFUSED("step", "step -inf", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, -(double)INFINITY, o);
  // the output inside the cloud: the cloud itself, its last row, and a cloud that begins inside the output
  REFUSED("must not lie inside the cloud", "the output is the cloud", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, p);
  REFUSED("must not lie inside the cloud", "the output begins at the cloud's last row", p, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0,
          block + 3 * (N - 1));
  REFUSED("must not lie inside the cloud", "the cloud begins inside the output", block + 3, N, p, p, M, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, p);
  // M = 0 is a no-op (the ends of every range are accepted, the open ones from inside), and an argument error is still one
  if (CALL(p, N, p, NULL, 0, 0, p, K, 1, 0.0, 0.0, 1e-300, 1e-300, o) != 0 || CALL(p, N, p, NULL, 0, 0, p, K, K, 0.999999, 1.0, 1e6, 1.0, o) != 0 ||
      CALL(p, N, p, NULL, 0, N, p, NESTI_KNN_MAX_K, NESTI_KNN_MAX_K, 0.5, 0.5, 0.25, 0.5, NULL) != 0) {
    printf("FAIL M = 0 is a no-op: '%s'\n", nesti_last_error());
    ++failures;
  }
  REFUSED("sigma", "M = 0 with a NaN sigma", p, N, p, NULL, 0, 0, p, K, 16, 0.7, 0.75, (double)NAN, 1.0, o);
  REFUSED("must not lie inside the cloud", "M = 0 with the output the cloud", p, N, p, NULL, 0, 0, p, K, 16, 0.7, 0.75, 0.5, 1.0, p);
  lane_switch_refusals(nesti_debug_denoise_lanes, "nesti_debug_denoise_lanes");
  return finish("denoise_args");
}
