// What the list passes that serve a row by a GROUP of lanes share (smooth.hip, denoise.hip): the reductions of a group of G lanes,
// G = 16, 32 or 64, and the eligibility of a normal.  One definition, so a group's butterfly and the test on the bits are the same in
// both units.
//
// For the including unit: include patches_dev.h first, then `#pragma clang fp contract(off)`, then pca_dev.h and this header -- every
// sum below is rounded on its own.
#pragma once
#include "pca_dev.h"

namespace nesti {
namespace {

__device__ __forceinline__ bool nonzero_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) != 0u; }
// all three components finite and at least one non-zero, on the bits: orient.hip's rule
__device__ __forceinline__ bool eligible_normal(float x, float y, float z) {
  return finite_bits(x) && finite_bits(y) && finite_bits(z) && (nonzero_bits(x) || nonzero_bits(y) || nonzero_bits(z));
}

// the reductions of a group of G lanes (G = 64: wave_sum / wave_min / wave_max of pca_dev.h, offset for offset)
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

}  // namespace
}  // namespace nesti
