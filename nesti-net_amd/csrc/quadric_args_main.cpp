// Stand-alone driver of the quadric-fit entries' host side (quadric.hip): every argument refusal, all of which return before any
// device call, and the solve behind nesti_quadric_solve on a well-posed, a rank-deficient and a NaN moment vector.  Built and run by
// `make asan-quadric` against the AddressSanitizer build of the library.
#include "args_main.h"

// the 21 moments of n points (u, v, h)
static void moments(const double (*p)[3], int n, double (&m)[21]) {
  for (int i = 0; i < 21; ++i) m[i] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double u = p[i][0], v = p[i][1], h = p[i][2];
    int k = 0;
    for (int deg = 0; deg <= 4; ++deg)
      for (int q = 0; q <= deg; ++q) m[k++] += pow(u, deg - q) * pow(v, q);
    const double phi[6] = {1.0, u, v, u * u, u * v, v * v};
    for (int j = 0; j < 6; ++j) m[15 + j] += h * phi[j];
  }
}

int main() {
  float out[4];                                     // never dereferenced: the checks come first
  ball_fit_refusals(
      [&](const nesti_config_t* c, const float* cloud, int n, const int32_t* q, int m, const double* rad, int row0, const void* g, size_t gb) {
        return nesti_quadric_fit(c, cloud, n, q, m, rad, row0, out, out, out, (int32_t*)out, g, gb, NULL);
      },
      [&](const nesti_config_t* c, const float* cloud, int n, const float* q, int m, const double* rad, int row0, const void* g, size_t gb) {
        return nesti_quadric_fit_at(c, cloud, n, q, m, rad, row0, out, out, out, (int32_t*)out, g, gb, NULL);
      });
  // the entries name themselves: the last refusal was the positions form's
  if (!strstr(nesti_last_error(), "nesti_quadric_fit_at")) { printf("FAIL the message does not name the entry\n"); ++failures; }

  double m[21], a[6], k[2];
  int ok = -1;
  // a well-posed fit: nine points of h = 0.1 + 0.2 u - 0.3 v + 0.4 u^2 + 0.5 u v - 0.6 v^2 on a 3 x 3 grid are fitted exactly
  const double want[6] = {0.1, 0.2, -0.3, 0.4, 0.5, -0.6};
  double pts[9][3];
  for (int i = 0; i < 9; ++i) {
    const double u = 0.5 * (i % 3 - 1), v = 0.4 * (i / 3 - 1) + 0.1;
    pts[i][0] = u; pts[i][1] = v;
    pts[i][2] = want[0] + want[1] * u + want[2] * v + want[3] * u * u + want[4] * u * v + want[5] * v * v;
  }
  moments(pts, 9, m);
  refused(nesti_quadric_solve(NULL, a, k, &ok), "null", "quadric_solve: null moments");
  refused(nesti_quadric_solve(m, NULL, k, &ok), "null", "quadric_solve: null coefficients");
  refused(nesti_quadric_solve(m, a, NULL, &ok), "null", "quadric_solve: null curvatures");
  refused(nesti_quadric_solve(m, a, k, NULL), "null", "quadric_solve: null flag");
  bool good = nesti_quadric_solve(m, a, k, &ok) == 0 && ok == 1 && k[0] >= k[1];
  for (int i = 0; i < 6 && good; ++i) good = fabs(a[i] - want[i]) <= 1e-12;
  if (!good) { printf("FAIL well-posed fit: ok %d, a = %g %g %g %g %g %g\n", ok, a[0], a[1], a[2], a[3], a[4], a[5]); ++failures; }
  // a paraboloid cap h = -(u^2 + v^2) / 2: both curvatures -1
  for (int i = 0; i < 9; ++i) pts[i][2] = -0.5 * (pts[i][0] * pts[i][0] + pts[i][1] * pts[i][1]);
  moments(pts, 9, m);
  if (nesti_quadric_solve(m, a, k, &ok) != 0 || ok != 1 || fabs(k[0] + 1.0) > 1e-12 || fabs(k[1] + 1.0) > 1e-12) {
    printf("FAIL paraboloid: ok %d, k = %.17g %.17g\n", ok, k[0], k[1]);
    ++failures;
  }
  // rank-deficient: all v = 0; and five points
  for (int i = 0; i < 9; ++i) { pts[i][0] = 0.1 * i - 0.4; pts[i][1] = 0.0; pts[i][2] = pts[i][0] * pts[i][0]; }
  moments(pts, 9, m);
  const auto failed = [&](const char* what) {
    ok = -1;
    bool z = nesti_quadric_solve(m, a, k, &ok) == 0 && ok == 0 && k[0] == 0.0 && k[1] == 0.0;
    for (int i = 0; i < 6; ++i) z = z && a[i] == 0.0;
    if (!z) { printf("FAIL %s: ok %d\n", what, ok); ++failures; }
  };
  failed("all v = 0");
  for (int i = 0; i < 5; ++i) { pts[i][0] = cos(1.3 * i); pts[i][1] = sin(1.3 * i); pts[i][2] = 0.1 * i; }
  moments(pts, 5, m);
  failed("five points");
  // NaN moments: a failed fit, finite outputs
  moments(pts, 9, m);
  m[7] = NAN;
  failed("a NaN moment");
  for (int i = 0; i < 21; ++i) m[i] = NAN;
  failed("all moments NaN");
  return finish("quadric_args");
}
