// Stand-alone driver of the plane-fit entries' host side (pca.hip): every argument refusal, all of which return before any device
// call, and the eigen-solver behind nesti_sym3_eig on a few matrices.  Built and run by `make asan-pca` against the AddressSanitizer
// build of the library.
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
  float out[4];                                     // never dereferenced: the checks come first
  ball_fit_refusals(
      [&](const nesti_config_t* c, const float* cloud, int n, const int32_t* q, int m, const double* rad, int row0, const void* g, size_t gb) {
        return nesti_pca_normals(c, cloud, n, q, m, rad, row0, out, out, (int32_t*)out, g, gb, NULL);
      },
      [&](const nesti_config_t* c, const float* cloud, int n, const float* q, int m, const double* rad, int row0, const void* g, size_t gb) {
        return nesti_pca_normals_at(c, cloud, n, q, m, rad, row0, out, out, (int32_t*)out, g, gb, NULL);
      });

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
