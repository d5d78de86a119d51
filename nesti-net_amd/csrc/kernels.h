// Launchers and device helpers shared between the .hip files and the host-side tower runner (model.hip).  The parameter blocks the
// launchers take (ConvParams, PoolParams) and the constants the planner and the weight packer share with the kernels (kTileM,
// kRowBytes, kMaxTaps) are host.h's: plan.cpp fills the blocks without a HIP header.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace nesti {

constexpr unsigned kWalkGrid = 1024;   // workgroups of a walking launch (ConvParams::walk): a multiple of 8, so a workgroup's tiles stay
                                       // on its XCD (tile & 7 == blockIdx.x & 7); four per CU, enough to run a non-empty round

int launch_conv(const ConvParams& p, int dtype, int TN, hipStream_t stream);
// k^3 taps (k = 3, 5) on the 8^3 volume (conv8n.hip): a workgroup = 4 points x one z half x 64 columns; p.m_tiles = groups of 4
// points, p.n_tiles = 64-column pairs, p.n_chunks = 64-byte K chunks, weights packed [pair][chunk][tap][2 x 32 rows][64 B]
int launch_conv8n(const ConvParams& p, int dtype, int k, hipStream_t stream);
// k^3 taps (k = 2 .. 5) on the 4^3 volume (conv4n.hip): a workgroup = 16 points x 64 voxels x 64 columns, an MFMA tile = one voxel of
// 16 points; p.m_tiles = groups of 16 points, p.n_tiles = 64-column tiles, p.n_chunks = 64-byte K chunks, weights packed
// [n tile][chunk][tap][64 rows][64 B]
int launch_conv4n(const ConvParams& p, int dtype, int k, hipStream_t stream);
// conv8n_kernel reads the x padding from an LDS address beyond the workgroup's allocation and relies on the
// hardware returning zeros there (gfx950 does: scripts/lds_oob_probe.hip).  Checked once per device, at model creation:
// the device must be gfx950 and a probe kernel must read zeros; otherwise the model is refused (returns 1 with a message).
int conv8_selftest();

// ---- the wrapper and the launcher of the tile kernels (conv.hip, conv8n.hip, conv4n.hip) -----------------------------------------
// A tile kernel's grid is (row tiles, rounded up to whole groups of 8) x (workgroups per row tile): workgroup b works on row tile
// 8 * (its group) + (b & 7), so a row tile's column tiles stay on one XCD's L2.  On the host for the capacity, in a walking kernel
// for the live points
__host__ __device__ __forceinline__ unsigned tile_rows8(unsigned m_tiles) { return (m_tiles + 7) / 8 * 8; }
template <class Params>               // ConvParams, PoolParams
__device__ __forceinline__ int live_points(const Params& p) {
  int npts = p.npoints;
  if (p.npoints_ptr) npts = min(npts, *p.npoints_ptr);
  return npts;
}
// Workgroup `bid` of such a grid -> its row tile and which of that row tile's `per_m` workgroups it is (column tile; conv8n: z half too)
struct TileId {
  int sub, m_tile;
};
__device__ __forceinline__ TileId tile_id(const unsigned bid, const int per_m) {
  const int xcd = bid & 7, grp = bid >> 3;
  return {grp % per_m, (grp / per_m) * 8 + xcd};
}
// A walking launch (ConvParams::walk) is a kernel of its own, so that the one-tile-per-workgroup kernel keeps its register
// allocation: `for (bid = blockIdx.x; bid < live tiles; bid += gridDim.x) tile(p, bid, walk_trip(bid))`.  walk_trip returns the thread
// index for that trip, laundered, otherwise hipcc hoists every per-lane address out of the tile loop and spills.  (The loop itself
// stays in the kernels: moved into a helper, hipcc allocates the scalar registers of a dozen instantiations differently.)
__device__ __forceinline__ int walk_trip(const unsigned bid) {
  if (bid != blockIdx.x) __syncthreads();    // the previous tile's epilogue is done with the LDS
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  return tid;
}

// The k^3-tap kernels (conv8n.hip, conv4n.hip) run kTapThreads threads and pass their activated outputs, 32 columns at a time,
// through an fp32 LDS tile of 1024 rows (4 points x a z half of 8^3; 16 points x 4^3) on the way to memory
constexpr int kTapThreads = 512;
constexpr int kEpiStride = 144;   // bytes per row of the fp32 [1024][32] epilogue tile (+16 B pad)
// What the k^3-tap kernels (launch_conv8n, launch_conv4n) refuse alike; `who` names the launcher in the message
inline int check_tap_launch(const ConvParams& p, const char* who) {
  const std::string w(who);
  if (p.point_index) NESTI_FAIL(w + ": no input gather (k^3 layers never read the routed MuPS tensor)");
  if (p.pool_k > 1 || p.split_tile != p.n_tiles) NESTI_FAIL(w + ": no fused avg-pool / merged layers");
  if (p.mp_mode == 2) NESTI_FAIL(w + ": max-pool mode 2 is conv1's (a 1x1x1 layer)");
  if (p.mp_mode != 0 && !p.mp_out) NESTI_FAIL(w + ": fused max-pool needs an output");
  return 0;
}

// One launch of a tile kernel with `lds` bytes of dynamic LDS; the opt-in to that much LDS is a per-device function attribute: one
// flag per device and kernel instantiation, not per process
template <auto Kernel>
int launch_tile_kernel(const ConvParams& p, int lds, unsigned threads, unsigned grid, hipStream_t stream) {
  constexpr int kMaxDevices = 64;
  static bool attr_set[kMaxDevices] = {};
  int dev = 0;
  NESTI_CHECK_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices || !attr_set[dev]) {
    NESTI_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if (dev >= 0 && dev < kMaxDevices) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, stream, p);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}
// ... of its one-tile-per-workgroup instantiation over the capacity's n_blocks tiles or, when p.walk is set, of its walking
// instantiation on a small grid
template <auto Kernel, auto WalkKernel>
int launch_tiles(const ConvParams& p, int lds, unsigned threads, unsigned n_blocks, hipStream_t stream) {
  if (!p.walk) return launch_tile_kernel<Kernel>(p, lds, threads, n_blocks, stream);
  return launch_tile_kernel<WalkKernel>(p, lds, threads, std::min(n_blocks, p.walk > 1 ? (unsigned)p.walk : kWalkGrid), stream);
}
// f(std::integral_constant<int, DT>) for the element type a launch runs in
template <class F>
int with_elem_type(int dtype, const char* who, F&& f) {
  if (dtype == NESTI_BF16) return f(std::integral_constant<int, NESTI_BF16>{});
  if (dtype == NESTI_F16) return f(std::integral_constant<int, NESTI_F16>{});
  if (dtype == NESTI_F32) return f(std::integral_constant<int, NESTI_F32>{});
  NESTI_FAIL(std::string(who) + ": unsupported dtype");
}

int launch_maxpool2(const PoolParams& p, int dtype, hipStream_t stream);
// tf.nn.max_pool3d [3,3,3] stride 2 SAME on a 3^3 volume (models/experts_n_est.py:238): input rows in the 4^3-embedded
// layout (log2S = 2), output 2^3 (8 rows per point); output cell o covers input {o, o+1} per axis.
int launch_maxpool3s2(const PoolParams& p, int dtype, hipStream_t stream);

}  // namespace nesti
