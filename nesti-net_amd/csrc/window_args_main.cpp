// Stand-alone driver of the image-window search's host side (window.hip): every argument refusal of nesti_depth_window_knn and the
// M = 0 no-op, all of which return before any device call.  Built and run by `make asan-window` against the AddressSanitizer build of
// the library.
#include <math.h>

#include "args_main.h"

static nesti_camera_t good_camera(void) {
  nesti_camera_t c;
  memset(&c, 0, sizeof(c));
  c.fx = c.fy = 120.0;
  c.cx = 63.5;
  c.cy = 47.5;
  c.depth_scale = 1e-3;
  c.z_near = 0.0;
  c.z_far = INFINITY;
  return c;
}

int main() {
  const int N = 1000, M = 100, H = 96, W = 128, R = 3, K = 16;
  float dummy[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // device pointers are never dereferenced: the checks come first
  void* p = dummy;
  const nesti_camera_t cam = good_camera();
#define WINDOW(xyz, n, pix, rank, h, w, c, idx, m, row0, r, k, nbr) \
  nesti_depth_window_knn((const float*)(xyz), n, (const int32_t*)(pix), (const int32_t*)(rank), h, w, c, (const int32_t*)(idx), m, row0, r, \
                         k, (int32_t*)(nbr), (double*)p, (int32_t*)p, (int32_t*)p, NULL)
  refused(WINDOW(NULL, N, p, p, H, W, &cam, p, M, 0, R, K, p), "null", "null cloud");
  refused(WINDOW(p, N, NULL, p, H, W, &cam, p, M, 0, R, K, p), "null", "null pix");
  refused(WINDOW(p, N, p, NULL, H, W, &cam, p, M, 0, R, K, p), "null", "null rank");
  refused(WINDOW(p, N, p, p, H, W, NULL, p, M, 0, R, K, p), "null", "null camera");
  refused(WINDOW(p, N, p, p, H, W, &cam, p, M, 0, R, K, NULL), "null", "null nbr_out_dev");
  refused(WINDOW(p, 0, p, p, H, W, &cam, p, M, 0, R, K, p), "empty cloud", "N = 0");
  refused(WINDOW(p, -5, p, p, H, W, &cam, p, M, 0, R, K, p), "empty cloud", "N < 0");
  refused(WINDOW(p, N, p, p, 0, W, &cam, p, M, 0, R, K, p), "H and W", "H = 0");
  refused(WINDOW(p, N, p, p, H, -4, &cam, p, M, 0, R, K, p), "H and W", "W < 0");
  refused(WINDOW(p, N, p, p, 1 << 13, (1 << 13) + 1, &cam, p, M, 0, R, K, p), "2^26", "H W > 2^26");
  refused(WINDOW(p, N, p, p, H, W, &cam, p, M, 0, 0, K, p), "R must be", "R = 0");
  refused(WINDOW(p, N, p, p, H, W, &cam, p, M, 0, NESTI_WINDOW_MAX_R + 1, K, p), "R must be", "R = NESTI_WINDOW_MAX_R + 1");
  refused(WINDOW(p, N, p, p, H, W, &cam, p, M, 0, R, 0, p), "K must be", "K = 0");
  refused(WINDOW(p, N, p, p, H, W, &cam, p, M, 0, R, NESTI_KNN_MAX_K + 1, p), "K must be", "K = NESTI_KNN_MAX_K + 1");
  refused(WINDOW(p, N, p, p, H, W, &cam, p, -1, 0, R, K, p), "M must be", "M < 0");
  refused(WINDOW(p, N, p, p, H, W, &cam, NULL, M, -1, R, K, p), "query_row0", "query_row0 < 0");
  refused(WINDOW(p, N, p, p, H, W, &cam, NULL, M, N - M + 1, R, K, p), "exceed the cloud", "rows beyond the cloud");
  // the camera: each field the entry reads
  for (int k = 0; k < 8; ++k) {
    nesti_camera_t c = good_camera();
    const char* word = "";
    switch (k) {
      case 0: c.fx = 0.0; word = "fx"; break;
      case 1: c.fy = NAN; word = "fx"; break;
      case 2: c.fx = INFINITY; word = "fx"; break;
      case 3: c.fy = 0.0; word = "fx"; break;
      case 4: c.cx = NAN; word = "cx"; break;
      case 5: c.cy = -INFINITY; word = "cx"; break;
      case 6: c.has_pose = 1; c.pose[0] = c.pose[5] = c.pose[10] = 1.0; c.pose[7] = NAN; word = "pose"; break;
      case 7: c.has_pose = 1; c.pose[0] = c.pose[5] = c.pose[10] = 1.0; c.pose[3] = INFINITY; word = "pose"; break;
    }
    char what[64];
    snprintf(what, sizeof(what), "camera case %d", k);
    refused(WINDOW(p, N, p, p, H, W, &c, p, M, 0, R, K, p), word, what);
  }
  // M = 0 is a no-op, with and without an index list; an argument error is still one
  if (WINDOW(p, N, p, p, H, W, &cam, NULL, 0, 0, R, K, p) != 0 || WINDOW(p, N, p, p, H, W, &cam, p, 0, 0, R, K, p) != 0) {
    printf("FAIL M = 0 is a no-op\n");
    ++failures;
  }
  refused(WINDOW(p, N, p, p, H, W, &cam, NULL, 0, 0, 0, K, p), "R must be", "M = 0 with R = 0");
  // depth_scale, z_near and z_far are not read: a camera that nesti_depth_to_cloud refuses for them is served (M = 0: no device call)
  nesti_camera_t loose = good_camera();
  loose.depth_scale = 0.0;
  loose.z_near = NAN;
  if (WINDOW(p, N, p, p, H, W, &loose, NULL, 0, 0, R, K, p) != 0) {
    printf("FAIL depth_scale and the range are not read\n");
    ++failures;
  }
  return finish("window");
}
