// Stand-alone driver of the orientation entries' host side (orient.hip): the workspace size and every argument refusal, all of which
// return before any device call.  Built and run by `make asan-orient` against the AddressSanitizer build of the library.
#include <math.h>

#include "args_main.h"

int main() {
  const int M = 1000, K = 8;
  const double R = 0.1;
  float dummy[4] = {0.f, 0.f, 0.f, 0.f};            // never dereferenced: the checks come first
  void* p = dummy;
  const size_t gws = nesti_patches_workspace_bytes(M), ows = nesti_orient_workspace_bytes(M, K);
  if (!(ows > 0 && nesti_orient_workspace_bytes(0, K) == 0 && nesti_orient_workspace_bytes(-3, K) == 0 &&
        nesti_orient_workspace_bytes(M + 1, K) >= ows && nesti_orient_workspace_bytes(M, K + 1) > ows)) {
    printf("FAIL workspace bytes\n");
    ++failures;
  }
  const double vp[3] = {0.0, 0.0, 5.0}, vp_nan[3] = {0.0, NAN, 1.0}, vp_inf[3] = {INFINITY, 0.0, 1.0};
#define GRAPH(xyz, m, n, r, k, g, gb, w, wb) \
  nesti_orient_graph((const float*)(xyz), m, (const float*)(n), r, k, g, gb, w, wb, NULL, NULL, NULL, NULL, NULL, NULL)
#define NORMALS(xyz, m, n, mode, r, k, v, g, gb, w, wb) \
  nesti_orient_normals((const float*)(xyz), m, (float*)(n), mode, r, k, v, g, gb, w, wb, NULL, NULL, NULL)
  refused(GRAPH(NULL, M, p, R, K, p, gws, p, ows), "null", "graph: null xyz");
  refused(GRAPH(p, M, NULL, R, K, p, gws, p, ows), "null", "graph: null normals");
  refused(GRAPH(p, M, p, R, K, NULL, gws, p, ows), "null", "graph: null grid workspace");
  refused(GRAPH(p, M, p, R, K, p, gws, NULL, ows), "null", "graph: null workspace");
  refused(GRAPH(p, M, p, R, 0, p, gws, p, ows), "K", "graph: K = 0");
  refused(GRAPH(p, M, p, R, 17, p, gws, p, ows), "K", "graph: K = 17");
  refused(GRAPH(p, M, p, 0.0, K, p, gws, p, ows), "radius", "graph: radius 0");
  refused(GRAPH(p, M, p, NAN, K, p, gws, p, ows), "radius", "graph: radius NaN");
  refused(GRAPH(p, M, p, INFINITY, K, p, gws, p, ows), "radius", "graph: radius inf");
  refused(GRAPH(p, M, p, R, K, p, gws - 1, p, ows), "grid workspace too small", "graph: short grid workspace");
  refused(GRAPH(p, M, p, R, K, p, gws, p, ows - 1), "workspace too small", "graph: short workspace");
  refused(GRAPH(p, 1 << 28, p, R, 16, p, (size_t)1 << 62, p, (size_t)1 << 62), "2^32", "graph: M K = 2^32");
  refused(NORMALS(NULL, M, p, 0, R, K, NULL, p, gws, p, ows), "null", "normals: null xyz");
  refused(NORMALS(p, M, NULL, 0, R, K, NULL, p, gws, p, ows), "null", "normals: null normals");
  refused(NORMALS(p, M, p, 0, R, K, NULL, NULL, gws, p, ows), "null", "normals: null grid workspace");
  refused(NORMALS(p, M, p, 0, R, K, NULL, p, gws, NULL, ows), "null", "normals: null workspace");
  refused(NORMALS(p, M, p, 0, R, 0, NULL, p, gws, p, ows), "K", "normals: K = 0");
  refused(NORMALS(p, M, p, 0, R, 17, NULL, p, gws, p, ows), "K", "normals: K = 17");
  refused(NORMALS(p, M, p, 0, -1.0, K, NULL, p, gws, p, ows), "radius", "normals: radius < 0");
  refused(NORMALS(p, M, p, 0, NAN, K, NULL, p, gws, p, ows), "radius", "normals: radius NaN");
  refused(NORMALS(p, M, p, 2, R, K, NULL, p, gws, p, ows), "unknown mode", "normals: mode 2");
  refused(NORMALS(p, M, p, NESTI_ORIENT_VIEWPOINT, R, K, NULL, p, gws, p, ows), "viewpoint", "normals: viewpoint mode without one");
  refused(NORMALS(p, M, p, NESTI_ORIENT_MST, R, K, vp_nan, p, gws, p, ows), "finite", "normals: NaN viewpoint");
  refused(NORMALS(p, M, p, NESTI_ORIENT_VIEWPOINT, R, K, vp_inf, p, gws, p, ows), "finite", "normals: inf viewpoint");
  refused(NORMALS(p, M, p, 0, R, K, vp, p, gws - 1, p, ows), "grid workspace too small", "normals: short grid workspace");
  refused(NORMALS(p, M, p, 0, R, K, vp, p, gws, p, ows - 1), "workspace too small", "normals: short workspace");
  refused(NORMALS(p, 1 << 28, p, 0, R, 16, NULL, p, (size_t)1 << 62, p, (size_t)1 << 62), "2^32", "normals: M K = 2^32");
  if (GRAPH(NULL, 0, NULL, R, K, NULL, 0, NULL, 0) != 0 || NORMALS(NULL, 0, NULL, 0, R, K, vp, NULL, 0, NULL, 0) != 0) {
    printf("FAIL M = 0 is a no-op\n");
    ++failures;
  }
  return finish("orient_args");
}
