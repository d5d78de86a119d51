// Stand-alone driver of the plane-fit entries' host side (pca.hip): every argument refusal, all of which return before any device
// call, and the eigen-solver behind nesti_sym3_eig on a few matrices.  Built and run by `make asan-pca` against the AddressSanitizer
// build of the library.
#include <math.h>

#include "args_main.h"

// eigenvalues ascending, C v = w v and V^T V = I to a small multiple of 2^-53 ||C||
static void solved(const double (&c)[6], const char* what) {
  double w[3], v[9];
  if (nesti_sym3_eig(c, w, v) != 0) { printf("FAIL %s: refused\n", what); ++failures; return; }
  const double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double norm = 0.0;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) norm = fmax(norm, fabs(a[i][j]));
  const double tol = 64.0 * ldexp(1.0, -53);
  bool ok = w[0] <= w[1] && w[1] <= w[2];
  for (int k = 0; k < 3 && ok; ++k) {
    for (int i = 0; i < 3; ++i) {
      double r = -w[k] * v[3 * k + i];
      for (int j = 0; j < 3; ++j) r += a[i][j] * v[3 * k + j];
      ok = ok && fabs(r) <= tol * norm;
    }
    for (int l = 0; l < 3; ++l) {
      double d = 0.0;
      for (int i = 0; i < 3; ++i) d += v[3 * k + i] * v[3 * l + i];
      ok = ok && fabs(d - (k == l ? 1.0 : 0.0)) <= tol;
    }
  }
  if (!ok) {
    printf("FAIL %s: w = %.17g %.17g %.17g\n", what, w[0], w[1], w[2]);
    ++failures;
  }
}

int main() {
  const int N = 1000, M = 100;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};            // never dereferenced: the checks come first
  void* p = dummy;
  nesti_config_t cfg;
  nesti_default_config(&cfg);
  const size_t gws = nesti_patches_workspace_bytes(N);
  const double r[4] = {0.01, 0.03, 0.05, 0.07}, r_zero[4] = {0.01, 0.0, 0.05, 0.07}, r_neg[4] = {-0.01, 0.03, 0.05, 0.07},
               r_nan[4] = {0.01, 0.03, NAN, 0.07}, r_inf[4] = {INFINITY, 0.03, 0.05, 0.07};
#define IDX(c, cloud, n, q, m, rad, row0, g, gb) \
  nesti_pca_normals(c, (const float*)(cloud), n, (const int32_t*)(q), m, rad, row0, (float*)p, (float*)p, (int32_t*)p, g, gb, NULL)
#define AT(c, cloud, n, q, m, rad, row0, g, gb) \
  nesti_pca_normals_at(c, (const float*)(cloud), n, (const float*)(q), m, rad, row0, (float*)p, (float*)p, (int32_t*)p, g, gb, NULL)
#define BOTH(word, what, ...)                         \
  refused(IDX(__VA_ARGS__), word, "index: " what);    \
  refused(AT(__VA_ARGS__), word, "positions: " what)
  BOTH("null", "null config", NULL, p, N, p, M, r, 0, p, gws);
  BOTH("null", "null cloud", &cfg, NULL, N, p, M, r, 0, p, gws);
  BOTH("null", "null radii", &cfg, p, N, p, M, NULL, 0, p, gws);
  BOTH("null", "null grid workspace", &cfg, p, N, p, M, r, 0, NULL, gws);
  BOTH("empty cloud", "N = 0", &cfg, p, 0, p, M, r, 0, p, gws);
  BOTH("M must be", "M < 0", &cfg, p, N, p, -1, r, 0, p, gws);
  BOTH("workspace too small", "short grid workspace", &cfg, p, N, p, M, r, 0, p, gws - 1);
  BOTH("query_row0", "query_row0 < 0", &cfg, p, N, p, M, r, -1, p, gws);
  BOTH("radii", "radius 0", &cfg, p, N, p, M, r_zero, 0, p, gws);
  BOTH("radii", "radius < 0", &cfg, p, N, p, M, r_neg, 0, p, gws);
  BOTH("radii", "radius NaN", &cfg, p, N, p, M, r_nan, 0, p, gws);
  BOTH("radii", "radius inf", &cfg, p, N, p, M, r_inf, 0, p, gws);
  nesti_config_t bad = cfg;
  bad.n_scales = 0;
  BOTH("n_scales", "S = 0", &bad, p, N, p, M, r, 0, p, gws);
  bad.n_scales = NESTI_MAX_SCALES + 1;
  BOTH("n_scales", "S = NESTI_MAX_SCALES + 1", &bad, p, N, p, M, r, 0, p, gws);
  refused(IDX(&cfg, p, N, NULL, M, r, N - M + 1, p, gws), "exceed the cloud", "index: rows beyond the cloud");
  refused(AT(&cfg, p, N, NULL, M, r, 0, p, gws), "null query_xyz_dev", "positions: null positions");
  // M = 0 is a no-op, and an argument error is still one
  if (IDX(&cfg, p, N, NULL, 0, r, 0, p, gws) != 0 || AT(&cfg, p, N, NULL, 0, r, 0, p, gws) != 0) {
    printf("FAIL M = 0 is a no-op\n");
    ++failures;
  }
  refused(IDX(&cfg, p, N, NULL, 0, r_nan, 0, p, gws), "radii", "index: M = 0 with a NaN radius");

  double w[3], v[9];
  const double c_id[6] = {1, 0, 0, 1, 0, 1};
  refused(nesti_sym3_eig(NULL, w, v), "null", "sym3_eig: null matrix");
  refused(nesti_sym3_eig(c_id, NULL, v), "null", "sym3_eig: null eigenvalues");
  refused(nesti_sym3_eig(c_id, w, NULL), "null", "sym3_eig: null eigenvectors");
  const double c_diag[6] = {3, 0, 0, 1, 0, 2}, c_zero[6] = {0, 0, 0, 0, 0, 0}, c_rank1[6] = {1, 2, 3, 4, 6, 9},
               c_full[6] = {0.30, 0.01, -0.02, 0.25, 0.005, 1e-4}, c_two[6] = {2, 1, 1, 2, 1, 2},
               c_wide[6] = {1.0, 1e-6, 1e-12, 1e-6, 1e-9, 1e-12}, c_plane[6] = {0.2, 0.05, 0, 0.3, 0, 0};
  solved(c_id, "identity");
  solved(c_diag, "diagonal");
  solved(c_zero, "rank 0");
  solved(c_rank1, "rank 1");
  solved(c_full, "a covariance");
  solved(c_two, "two equal eigenvalues");
  solved(c_wide, "entries over twelve decades");
  solved(c_plane, "a plane");
  nesti_sym3_eig(c_plane, w, v);
  if (!(w[0] == 0.0 && v[0] == 0.0 && v[1] == 0.0 && v[2] == 1.0)) {       // a zero row is never rotated
    printf("FAIL plane: w0 = %g, v0 = %g %g %g\n", w[0], v[0], v[1], v[2]);
    ++failures;
  }
  nesti_sym3_eig(c_diag, w, v);
  if (!(w[0] == 1.0 && w[1] == 2.0 && w[2] == 3.0 && v[1] == 1.0 && v[5] == 1.0 && v[6] == 1.0)) {
    printf("FAIL diagonal: w = %g %g %g\n", w[0], w[1], w[2]);
    ++failures;
  }
  return finish("pca_args");
}
