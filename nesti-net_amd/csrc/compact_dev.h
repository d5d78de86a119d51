// Ordered compaction, shared by depth.hip, outlier.hip and voxel.hip: a count per block of 256 items (block_rank), ONE single-workgroup
// exclusive scan of the block counts (compact_scan_kernel) and a scatter in item order (block_rank again, on top of the block's
// start).  No atomics, no workgroup waits on another, no look-back: the order of the output is the order of the input.  Each unit keeps
// its predicate and what it writes at a kept item's position; the rank and the scan are one definition.  All integer: prefix sums of
// counts do not depend on the form of the scan.
//
// For the including unit: after kernels.h; it holds no floating-point arithmetic, so the contraction setting does not matter.
#pragma once
#include "wave_dev.h"

namespace nesti {
namespace {

constexpr int kScanPer = 16;                        // entries per thread and trip of a scan
constexpr int kScanChunk = kThreads * kScanPer;     // entries per workgroup and trip

// Position of a thread's element among the block's true predicates, and the block's total.  Every thread of the block calls it.
__device__ __forceinline__ int block_rank(bool pred, int* total) {
  __shared__ int wave_count[kWaves];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(pred);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wave_count[wave] = __popcll(b);
  __syncthreads();
  int off = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = wave_count[w];
    if (w < wave) off += c;
    sum += c;
  }
  *total = sum;
  return off + before;
}

// The exclusive prefix sums of the kThreads * kScanPer values a workgroup holds, kScanPer consecutive ones per thread, in place; returns
// their total, the same in every thread.  Every thread of the block calls it; a second call needs a barrier first.
__device__ __forceinline__ int block_scan(int (&e)[kScanPer]) {
  __shared__ int wave_total[kWaves];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  int sum = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) sum += e[j];
  int incl = sum;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += o;
  }
  if (lane == kWave - 1) wave_total[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int s = wave_total[w];
    if (w < wave) off += s;
    tot += s;
  }
  int run = off + incl - sum;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    const int x = e[j];
    e[j] = run;
    run += x;
  }
  return tot;
}

// ONE workgroup: v[0 .. n) -> exclusive prefix sums in place, the grand total to *total_out (or nowhere).  kScanPer consecutive
// entries per thread and trip; the sums stay below 2^31 (they count rows).
__global__ __launch_bounds__(kThreads) void compact_scan_kernel(int32_t* __restrict__ v, long long n, int32_t* __restrict__ total_out) {
  int carry = 0;                                            // the same in every thread
  for (long long base = 0; base < n; base += kScanChunk) {
    const long long i0 = base + (long long)threadIdx.x * kScanPer;
    int e[kScanPer];
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) e[j] = i0 + j < n ? v[i0 + j] : 0;
    const int tot = block_scan(e);
#pragma unroll
    for (int j = 0; j < kScanPer; ++j)
      if (i0 + j < n) v[i0 + j] = carry + e[j];
    carry += tot;
    __syncthreads();                                        // block_scan's LDS is rewritten by the next trip
  }
  if (total_out && threadIdx.x == 0) *total_out = carry;
}

}  // namespace
}  // namespace nesti
