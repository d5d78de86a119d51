// Stand-alone driver of the depth-image entries' host side (depth.hip): the workspace size and every argument refusal, all of which
// return before any device call.  Built and run by `make asan-depth` against the AddressSanitizer build of the library.
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
  const int H = 96, W = 128;
  float dummy[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // device pointers are never dereferenced: the checks come first
  void* p = dummy;
  const float fill[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const size_t ws = nesti_depth_workspace_bytes(H, W);
  if (!(ws > 0 && nesti_depth_workspace_bytes(0, W) == 0 && nesti_depth_workspace_bytes(H, -1) == 0 &&
        nesti_depth_workspace_bytes(1 << 13, (1 << 13) + 1) == 0 && nesti_depth_workspace_bytes(1 << 13, 1 << 13) > ws &&
        nesti_depth_workspace_bytes(H + 1, W) >= ws && nesti_depth_workspace_bytes(1, 1) > 0)) {
    printf("FAIL workspace bytes\n");
    ++failures;
  }
  const nesti_camera_t cam = good_camera();
#define CLOUD(d, type, h, w, c, s, xyz, pix, cnt, wsp, wsb) \
  nesti_depth_to_cloud(d, type, h, w, c, s, (float*)(xyz), (int32_t*)(pix), NULL, NULL, (int32_t*)(cnt), wsp, wsb, NULL)
#define SCATTER(rows, pix, m, ch, h, w, f, img) nesti_image_scatter(rows, (const int32_t*)(pix), m, ch, h, w, f, img, NULL)
#define PROJECT(xyz, val, m, ch, h, w, c, f, img, wsp, wsb) \
  nesti_project_to_image((const float*)(xyz), val, m, ch, h, w, c, f, img, NULL, wsp, wsb, NULL)
  refused(CLOUD(NULL, NESTI_DEPTH_U16, H, W, &cam, 1, p, p, p, p, ws), "null", "cloud: null depth");
  refused(CLOUD(p, NESTI_DEPTH_U16, H, W, &cam, 1, NULL, p, p, p, ws), "null", "cloud: null xyz");
  refused(CLOUD(p, NESTI_DEPTH_U16, H, W, &cam, 1, p, NULL, p, p, ws), "null", "cloud: null pix");
  refused(CLOUD(p, NESTI_DEPTH_U16, H, W, &cam, 1, p, p, NULL, p, ws), "null", "cloud: null counts");
  refused(CLOUD(p, NESTI_DEPTH_U16, H, W, &cam, 1, p, p, p, NULL, ws), "null", "cloud: null workspace");
  refused(CLOUD(p, NESTI_DEPTH_U16, H, W, NULL, 1, p, p, p, p, ws), "null", "cloud: null camera");
  refused(CLOUD(p, 2, H, W, &cam, 1, p, p, p, p, ws), "unknown depth type", "cloud: depth type 2");
  refused(CLOUD(p, -1, H, W, &cam, 1, p, p, p, p, ws), "unknown depth type", "cloud: depth type -1");
  refused(CLOUD(p, NESTI_DEPTH_F32, 0, W, &cam, 1, p, p, p, p, ws), "H and W", "cloud: H = 0");
  refused(CLOUD(p, NESTI_DEPTH_F32, H, -4, &cam, 1, p, p, p, p, ws), "H and W", "cloud: W < 0");
  refused(CLOUD(p, NESTI_DEPTH_F32, 1 << 13, (1 << 13) + 1, &cam, 1, p, p, p, p, (size_t)1 << 62), "2^26", "cloud: H W > 2^26");
  refused(CLOUD(p, NESTI_DEPTH_F32, H, W, &cam, 0, p, p, p, p, ws), "stride", "cloud: stride 0");
  refused(CLOUD(p, NESTI_DEPTH_F32, H, W, &cam, 1, p, p, p, p, ws - 1), "workspace too small", "cloud: short workspace");
  refused(PROJECT(p, p, 10, 3, H, W, &cam, fill, p, p, ws - 1), "workspace too small", "project: short workspace");
  refused(PROJECT(NULL, p, 10, 3, H, W, &cam, fill, p, p, ws), "null", "project: null xyz");
  refused(PROJECT(p, NULL, 10, 3, H, W, &cam, fill, p, p, ws), "null", "project: null values");
  refused(PROJECT(p, p, 10, 3, H, W, &cam, NULL, p, p, ws), "null", "project: null fill");
  refused(PROJECT(p, p, 10, 3, H, W, &cam, fill, NULL, p, ws), "null", "project: no output");
  refused(PROJECT(p, p, 10, 3, H, W, &cam, fill, p, NULL, ws), "null", "project: null workspace");
  refused(PROJECT(p, p, 10, 3, H, W, NULL, fill, p, p, ws), "null", "project: null camera");
  refused(PROJECT(p, p, -1, 3, H, W, &cam, fill, p, p, ws), "M", "project: M < 0");
  refused(PROJECT(p, p, 10, 0, H, W, &cam, fill, p, p, ws), "C must", "project: C = 0");
  refused(PROJECT(p, p, 10, 9, H, W, &cam, fill, p, p, ws), "C must", "project: C = 9");
  refused(PROJECT(p, p, 10, 3, 0, W, &cam, fill, p, p, ws), "H and W", "project: H = 0");
  refused(PROJECT(p, p, 10, 3, 1 << 13, (1 << 13) + 1, &cam, fill, p, p, (size_t)1 << 62), "2^26", "project: H W > 2^26");
  refused(SCATTER(NULL, p, 10, 3, H, W, fill, p), "null", "scatter: null rows");
  refused(SCATTER(p, NULL, 10, 3, H, W, fill, p), "null", "scatter: null pix");
  refused(SCATTER(p, p, 10, 3, H, W, NULL, p), "null", "scatter: null fill");
  refused(SCATTER(p, p, 10, 3, H, W, fill, NULL), "null", "scatter: null image");
  refused(SCATTER(p, p, -1, 3, H, W, fill, p), "M", "scatter: M < 0");
  refused(SCATTER(p, p, 10, 0, H, W, fill, p), "C must", "scatter: C = 0");
  refused(SCATTER(p, p, 10, 9, H, W, fill, p), "C must", "scatter: C = 9");
  refused(SCATTER(p, p, 10, 3, H, 0, fill, p), "H and W", "scatter: W = 0");
  refused(SCATTER(p, p, 10, 3, 1 << 13, (1 << 13) + 1, fill, p), "2^26", "scatter: H W > 2^26");
  // the camera: each field on both entries that read it
  for (int entry = 0; entry < 2; ++entry) {
    for (int k = 0; k < 14; ++k) {
      nesti_camera_t c = good_camera();
      const char* word = "";
      switch (k) {
        case 0: c.fx = 0.0; word = "fx"; break;
        case 1: c.fy = NAN; word = "fx"; break;
        case 2: c.fx = INFINITY; word = "fx"; break;
        case 3: c.fy = 0.0; word = "fx"; break;
        case 4: c.cx = NAN; word = "cx"; break;
        case 5: c.cy = -INFINITY; word = "cx"; break;
        case 6: c.depth_scale = 0.0; word = "depth_scale"; break;
        case 7: c.depth_scale = -1e-3; word = "depth_scale"; break;
        case 8: c.depth_scale = NAN; word = "depth_scale"; break;
        case 9: c.depth_scale = INFINITY; word = "depth_scale"; break;
        case 10: c.z_near = 2.0; c.z_far = 1.0; word = "z_near"; break;
        case 11: c.z_near = NAN; word = "z_near"; break;
        case 12: c.has_pose = 1; c.pose[0] = c.pose[5] = c.pose[10] = 1.0; c.pose[7] = NAN; word = "pose"; break;
        case 13: c.has_pose = 1; c.pose[0] = c.pose[5] = c.pose[10] = 1.0; c.pose[3] = INFINITY; word = "pose"; break;
      }
      char what[64];
      snprintf(what, sizeof(what), "%s: camera case %d", entry ? "project" : "cloud", k);
      refused(entry ? PROJECT(p, p, 10, 3, H, W, &c, fill, p, p, ws) : CLOUD(p, NESTI_DEPTH_U16, H, W, &c, 1, p, p, p, p, ws), word, what);
    }
  }
  // a non-finite pose entry is not read when has_pose is 0: nothing to refuse there, and nothing else is wrong with this camera --
  // but the call would reach the device, so it is not made here
  return finish("depth_args");
}
