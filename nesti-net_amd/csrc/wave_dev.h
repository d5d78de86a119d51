// The shape of a workgroup and the reductions of its lanes, shared by every unit whose kernels run four 64-lane waves per workgroup
// (pca_dev.h and all that stands on it, compact_dev.h, depth.hip, voxel.hip): the constants, the blocks a range needs and the xor
// butterflies of a group of G lanes.  One definition, so the butterfly of a group IS the tail of the wave's, offset for offset, and the
// bytes of a sum do not depend on the unit that forms it.
//
// For the including unit: after kernels.h and after `#pragma clang fp contract(off)` -- every sum below is rounded on its own.  Needs
// nothing of patches_dev.h.
#pragma once
#include "kernels.h"

namespace nesti {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kRowsPerBlock = kWaves;                         // of a kernel that serves one row per wave (wave_row, pca_dev.h)

// host side: the workgroups that hold n items at `per` items each
inline size_t blocks_of(size_t n, size_t per = kThreads) { return (n + per - 1) / per; }

// the reductions of a group of G lanes, G a power of two: xor offsets G / 2, ..., 1; every lane of the group ends up with the result
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off, kWave);
  return v;
}
template <int G>
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
template <int G>
__device__ __forceinline__ int group_min(int v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, kWave));
  return v;
}
template <int G>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
  return v;
}

// the wave's: the group of all 64 lanes (xor offsets 32, 16, ..., 1)
__device__ __forceinline__ double wave_sum(double v) { return group_sum<kWave>(v); }
__device__ __forceinline__ int wave_sum(int v) { return group_sum<kWave>(v); }
__device__ __forceinline__ int wave_min(int v) { return group_min<kWave>(v); }
__device__ __forceinline__ double wave_max(double v) { return group_max<kWave>(v); }

}  // namespace
}  // namespace nesti
