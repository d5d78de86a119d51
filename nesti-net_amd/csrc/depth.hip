// Depth images in, normal images out ("Depth images"): the two ends of the reference's Kinect route, MATLAB/ScanNet_depth2xyz.m
// (depth + intrinsics + pose -> cloud) and MATLAB/ScanNet_world2cam_normals.m / export_visualizations_nyu.m:146-153 (per-point results
// -> image).  The conventions are the library's own:
//   - pixel coordinates are 0-BASED, u = column, v = row (the MATLAB files are 1-based: a caller with MATLAB-convention intrinsics
//     passes cx - 1, cy - 1);
//   - the pose is a proper rigid transform, translation included (ScanNet_depth2xyz.m:14 multiplies with a homogeneous coordinate of
//     0 and thereby drops it);
//   - where several rows project onto one pixel the NEAREST wins, among equals the smaller row (the reference: the last one).
//
//   nesti_depth_to_cloud    validity -> per-block counts (ballot / popcount in a wave, LDS across waves) -> ONE single-workgroup scan
//                           of the block counts -> scatter in pixel order.  The same three steps serve both predicates (valid; valid
//                           and on the stride).  No atomics, no workgroup waits on another, no look-back: the order is the pixel order.
//   nesti_image_scatter     fill, then rows to their pixels: plain vector stores.
//   nesti_project_to_image  64-bit atomicMin of (bits of (float)zc) << 32 | row into a key image, then a resolve launch.
//
// Nothing synchronises, nothing is read back; every argument error is reported before any device call.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"

// every product, quotient and sum below is rounded on its own: the CPU restatement (tests/_depth_fixture.py) predicts each bit
#pragma clang fp contract(off)

#include "compact_dev.h"   // kThreads, blocks_of (wave_dev.h); block_rank, compact_scan_kernel

namespace nesti {
namespace {

constexpr long long kMaxPixels = 1ll << 26;
constexpr unsigned long long kNoKey = ~0ull;

struct DepthLayout {
  size_t cnt_valid, cnt_query, rank, keys, total;
};
inline DepthLayout depth_layout(size_t n) {
  DepthLayout L;
  size_t o = 0;
  L.cnt_valid = o; o += align_up(blocks_of(n) * 4, 256);
  L.cnt_query = o; o += align_up(blocks_of(n) * 4, 256);
  L.rank = o; o += align_up(n * 4, 256);
  L.keys = o; o += align_up(n * 8, 256);
  L.total = o;
  return L;
}

// the camera as the kernels take it: by value
struct Cam {
  double fx, fy, cx, cy, scale, z_near, z_far;
  int has_pose;
  double T[12];
};

struct Frame {
  const void* depth;
  int type, H, W, n, stride;
};

using nesti::finite_bits;             // the float form (common.h); a declaration here alone would hide it
__device__ __forceinline__ bool finite_bits(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// z = (double)raw * depth_scale of pixel i; valid iff finite, > 0 and inside [z_near, z_far]
__device__ __forceinline__ bool pixel_z(const Frame& f, const Cam& c, int i, double* z_out) {
  double raw;
  if (f.type == NESTI_DEPTH_U16) {
    raw = (double)((const unsigned short*)f.depth)[i];
  } else {
    const float r = ((const float*)f.depth)[i];
    if (!finite_bits(r)) return false;
    raw = (double)r;
  }
  const double z = raw * c.scale;
  *z_out = z;
  return finite_bits(z) && z > 0.0 && z >= c.z_near && z <= c.z_far;
}

// ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]
__device__ __forceinline__ double rigid_row(const double* T, int r, double x, double y, double z) {
  const double s = T[4 * r] * x + T[4 * r + 1] * y;       // contraction is off in this file: two products, one sum
  const double t = s + T[4 * r + 2] * z;
  return t + T[4 * r + 3];
}

// ---- the two predicates and what each writes at its position ----------------------------------------------------------------------
struct CloudOut {
  float* xyz;
  int32_t* pix;
  int32_t* rank;       // [n]: the caller's, or the workspace's
};
struct QueryOut {
  int32_t* qidx;       // may be NULL: counts only
  const int32_t* rank;
};

struct ValidPixels {
  using Out = CloudOut;
  __device__ static bool test(const Frame& f, const Cam& c, int i, double* z) { return pixel_z(f, c, i, z); }
  __device__ static void emit(const Frame& f, const Cam& c, const Out& o, int i, bool pred, int pos, double z) {
    o.rank[i] = pred ? pos : -1;
    if (!pred) return;
    const int v = i / f.W, u = i - v * f.W;
    const double xn = ((double)u - c.cx) * z, yn = ((double)v - c.cy) * z;
    double x = xn / c.fx, y = yn / c.fy, zz = z;
    if (c.has_pose) {
      const double wx = rigid_row(c.T, 0, x, y, z), wy = rigid_row(c.T, 1, x, y, z), wz = rigid_row(c.T, 2, x, y, z);
      x = wx; y = wy; zz = wz;
    }
    o.xyz[(size_t)pos * 3] = (float)x;
    o.xyz[(size_t)pos * 3 + 1] = (float)y;
    o.xyz[(size_t)pos * 3 + 2] = (float)zz;
    o.pix[pos] = i;
  }
};
struct StridePixels {
  using Out = QueryOut;
  __device__ static bool test(const Frame& f, const Cam& c, int i, double* z) {
    const int v = i / f.W, u = i - v * f.W;
    return (v % f.stride) == 0 && (u % f.stride) == 0 && pixel_z(f, c, i, z);
  }
  __device__ static void emit(const Frame& f, const Cam& c, const Out& o, int i, bool pred, int pos, double) {
    if (pred) o.qidx[pos] = o.rank[i];
  }
};

// ---- ordered compaction: count per block, one scan (compact_scan_kernel), scatter; block_rank and the scan: compact_dev.h -------------
template <class P>
__global__ __launch_bounds__(kThreads) void compact_count_kernel(Frame f, Cam c, int32_t* __restrict__ block_count) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  double z = 0.0;
  const bool pred = i < f.n && P::test(f, c, (int)i, &z);
  int total;
  block_rank(pred, &total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

template <class P>
__global__ __launch_bounds__(kThreads) void compact_scatter_kernel(Frame f, Cam c, const int32_t* __restrict__ block_start, typename P::Out out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  double z = 0.0;
  const bool pred = i < f.n && P::test(f, c, (int)i, &z);
  int total;
  const int pos = block_start[blockIdx.x] + block_rank(pred, &total);
  if (i < f.n) P::emit(f, c, out, (int)i, pred, pos, z);
}

// ---- rows -> image -------------------------------------------------------------------------------------------------------------------
struct Fill {
  uint32_t v[8];
};

__global__ void image_fill_kernel(uint32_t* __restrict__ image, size_t total, int C, Fill fill) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total) image[e] = fill.v[e % (size_t)C];
}

// one thread per (row, channel); pix entries are distinct by construction, an entry outside [0, n) is skipped
__global__ void image_scatter_kernel(const uint32_t* __restrict__ rows, const int32_t* __restrict__ pix, size_t total, int C, int n,
                                     uint32_t* __restrict__ image) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const size_t m = e / (size_t)C;
  const int p = pix[m];
  if (p < 0 || p >= n) return;
  image[(size_t)p * C + (e - m * (size_t)C)] = rows[e];
}

// ---- cloud -> image (nearest wins) -----------------------------------------------------------------------------------------------------
__global__ void project_init_kernel(unsigned long long* __restrict__ keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = kNoKey;
}

__global__ void project_min_kernel(const float* __restrict__ xyz, int M, Cam c, int H, int W, unsigned long long* __restrict__ keys) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= M) return;
  const float px = xyz[(size_t)row * 3], py = xyz[(size_t)row * 3 + 1], pz = xyz[(size_t)row * 3 + 2];
  if (!(finite_bits(px) && finite_bits(py) && finite_bits(pz))) return;
  double x = (double)px, y = (double)py, z = (double)pz;
  if (c.has_pose) {
    const double wx = rigid_row(c.T, 0, x, y, z), wy = rigid_row(c.T, 1, x, y, z), wz = rigid_row(c.T, 2, x, y, z);
    x = wx; y = wy; z = wz;
  }
  if (!(finite_bits(x) && finite_bits(y) && finite_bits(z)) || !(z > 0.0)) return;
  const double xf = x * c.fx, yf = y * c.fy;
  const double uq = xf / z, vq = yf / z;
  const double uc = uq + c.cx, vc = vq + c.cy;
  const double uf = floor(uc + 0.5), vf = floor(vc + 0.5);
  if (!(finite_bits(uf) && finite_bits(vf))) return;
  if (!(uf >= 0.0 && uf < (double)W && vf >= 0.0 && vf < (double)H)) return;
  const int u = (int)uf, v = (int)vf;
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)z) << 32) | (unsigned long long)(unsigned)row;
  atomicMin(&keys[(size_t)v * W + u], key);
}

// one thread per pixel: the winner's values[row, 0:C] or the fill; the winning row or -1
__global__ void project_resolve_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ values, int n, int C,
                                       Fill fill, uint32_t* __restrict__ image, int32_t* __restrict__ index_image) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const bool hit = key != kNoKey;
  const size_t row = (size_t)(key & 0xffffffffull);
  if (image) {
    for (int ch = 0; ch < C; ++ch) image[(size_t)i * C + ch] = hit ? values[row * C + ch] : fill.v[ch];
  }
  if (index_image) index_image[i] = hit ? (int32_t)row : -1;
}

// ---- host: argument checks (before any device call) ------------------------------------------------------------------------------------
int check_image(const std::string& w, int H, int W) {
  if (H <= 0 || W <= 0) NESTI_FAIL(w + ": H and W must be > 0");
  if ((long long)H * (long long)W > kMaxPixels) NESTI_FAIL(w + ": H * W must not exceed 2^26");
  return 0;
}

int check_camera(const std::string& w, const nesti_camera_t* cam, Cam* out) {
  if (!cam) NESTI_FAIL(w + ": null camera");
  if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0)
    NESTI_FAIL(w + ": fx and fy must be finite and non-zero");
  if (!std::isfinite(cam->cx) || !std::isfinite(cam->cy)) NESTI_FAIL(w + ": cx and cy must be finite");
  if (!std::isfinite(cam->depth_scale) || !(cam->depth_scale > 0.0)) NESTI_FAIL(w + ": depth_scale must be finite and > 0");
  if (std::isnan(cam->z_near) || std::isnan(cam->z_far) || cam->z_near > cam->z_far) NESTI_FAIL(w + ": z_near must not exceed z_far");
  Cam c;
  memset(&c, 0, sizeof(c));
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
  c.scale = cam->depth_scale; c.z_near = cam->z_near; c.z_far = cam->z_far;
  c.has_pose = cam->has_pose ? 1 : 0;
  if (c.has_pose) {
    for (int k = 0; k < 12; ++k) {
      if (!std::isfinite(cam->pose[k])) NESTI_FAIL(w + ": the pose must be finite");
      c.T[k] = cam->pose[k];
    }
  }
  *out = c;
  return 0;
}

int check_fill(const std::string& w, int C, const void* fill, Fill* out) {
  if (C < 1 || C > 8) NESTI_FAIL(w + ": C must be in [1, 8]");
  if (!fill) NESTI_FAIL(w + ": null fill");
  memset(out, 0, sizeof(*out));
  memcpy(out->v, fill, (size_t)C * 4);
  return 0;
}

inline unsigned grid_for(size_t n) { return (unsigned)blocks_of(n); }

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

size_t nesti_depth_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (long long)H * (long long)W > kMaxPixels) return 0;
  return depth_layout((size_t)H * (size_t)W).total;
}

int nesti_depth_to_cloud(const void* depth_dev, int depth_type, int H, int W, const nesti_camera_t* camera, int stride,
                         float* xyz_dev, int32_t* pix_dev, int32_t* rank_dev, int32_t* qidx_dev, int32_t* counts_dev, void* ws_dev,
                         size_t ws_bytes, void* stream) {
  const std::string w("nesti_depth_to_cloud");
  if (depth_type != NESTI_DEPTH_U16 && depth_type != NESTI_DEPTH_F32) NESTI_FAIL(w + ": unknown depth type");
  if (check_image(w, H, W)) return 1;
  if (stride < 1) NESTI_FAIL(w + ": stride must be >= 1");
  Cam c;
  if (check_camera(w, camera, &c)) return 1;
  if (!depth_dev || !xyz_dev || !pix_dev || !counts_dev || !ws_dev) NESTI_FAIL(w + ": null argument");
  const size_t n = (size_t)H * (size_t)W;
  const DepthLayout L = depth_layout(n);
  if (ws_bytes < L.total) NESTI_FAIL(w + ": workspace too small (nesti_depth_workspace_bytes(H, W))");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  int32_t* cnt_valid = (int32_t*)(ws + L.cnt_valid);
  int32_t* cnt_query = (int32_t*)(ws + L.cnt_query);
  int32_t* rank = rank_dev ? rank_dev : (int32_t*)(ws + L.rank);
  Frame f;
  f.depth = depth_dev; f.type = depth_type; f.H = H; f.W = W; f.n = (int)n; f.stride = stride;
  const unsigned nb = grid_for(n);
  hipLaunchKernelGGL(compact_count_kernel<ValidPixels>, dim3(nb), dim3(kThreads), 0, st, f, c, cnt_valid);
  hipLaunchKernelGGL(compact_count_kernel<StridePixels>, dim3(nb), dim3(kThreads), 0, st, f, c, cnt_query);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, cnt_valid, (long long)nb, counts_dev);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, cnt_query, (long long)nb, counts_dev + 1);
  CloudOut co;
  co.xyz = xyz_dev; co.pix = pix_dev; co.rank = rank;
  hipLaunchKernelGGL(compact_scatter_kernel<ValidPixels>, dim3(nb), dim3(kThreads), 0, st, f, c, (const int32_t*)cnt_valid, co);
  if (qidx_dev) {
    QueryOut qo;
    qo.qidx = qidx_dev; qo.rank = rank;
    hipLaunchKernelGGL(compact_scatter_kernel<StridePixels>, dim3(nb), dim3(kThreads), 0, st, f, c, (const int32_t*)cnt_query, qo);
  }
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int nesti_image_scatter(const void* rows_dev, const int32_t* pix_dev, int M, int C, int H, int W, const void* fill, void* image_dev,
                        void* stream) {
  const std::string w("nesti_image_scatter");
  if (check_image(w, H, W)) return 1;
  Fill fl;
  if (check_fill(w, C, fill, &fl)) return 1;
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (!image_dev || (M > 0 && (!rows_dev || !pix_dev))) NESTI_FAIL(w + ": null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)H * (size_t)W, total = n * (size_t)C, rows = (size_t)M * (size_t)C;
  hipLaunchKernelGGL(image_fill_kernel, dim3(grid_for(total)), dim3(kThreads), 0, st, (uint32_t*)image_dev, total, C, fl);
  if (M > 0)
    hipLaunchKernelGGL(image_scatter_kernel, dim3(grid_for(rows)), dim3(kThreads), 0, st, (const uint32_t*)rows_dev, pix_dev, rows, C,
                       (int)n, (uint32_t*)image_dev);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int nesti_project_to_image(const float* xyz_dev, const void* values_dev, int M, int C, int H, int W, const nesti_camera_t* camera,
                           const void* fill, void* image_dev, int32_t* index_image_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  const std::string w("nesti_project_to_image");
  if (check_image(w, H, W)) return 1;
  Fill fl;
  if (check_fill(w, C, fill, &fl)) return 1;
  Cam c;
  if (check_camera(w, camera, &c)) return 1;
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (!ws_dev || (!image_dev && !index_image_dev) || (M > 0 && (!xyz_dev || (image_dev && !values_dev)))) NESTI_FAIL(w + ": null argument");
  const size_t n = (size_t)H * (size_t)W;
  const DepthLayout L = depth_layout(n);
  if (ws_bytes < L.total) NESTI_FAIL(w + ": workspace too small (nesti_depth_workspace_bytes(H, W))");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)((unsigned char*)ws_dev + L.keys);
  hipLaunchKernelGGL(project_init_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, keys, (int)n);
  if (M > 0) hipLaunchKernelGGL(project_min_kernel, dim3(grid_for((size_t)M)), dim3(kThreads), 0, st, xyz_dev, M, c, H, W, keys);
  hipLaunchKernelGGL(project_resolve_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, (const unsigned long long*)keys,
                     (const uint32_t*)values_dev, (int)n, C, fl, (uint32_t*)image_dev, index_image_dev);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
