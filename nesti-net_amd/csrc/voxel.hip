// Voxel-grid downsampling before estimation (DESIGN.md 2 "Voxel downsampling"): the first step of the textbook pipeline -- one point per
// occupied cell of a regular grid -- as three entries: a key per row (nesti_voxel_keys), a stable device-wide radix sort of (key, row
// index) pairs (nesti_sort_pairs) and a reduction of the sorted runs (nesti_voxel_reduce: centroid, nearest row, count, key, the voxel
// of every row).  The conventions are the library's own, chosen so that a restatement in plain IEEE arithmetic
// (tests/_voxel_fixture.py) predicts every output bit: fp64 where there is arithmetic, every operation rounded on its own; only
// + - x /, floor, comparisons and integer arithmetic; no floating-point atomics and no global-memory atomics (the sort counts digits
// with integer LDS atomics, as hough.hip does); no workgroup waits on another.  No parity with any published code is claimed.
//
// KEYS.  Per axis a: d = (double)p - origin, t = d / voxel, i = (int64)floor(t); key = (i_z dims_y + i_y) dims_x + i_x.  A row with a
// non-finite coordinate (on the bits) or an i outside [0, dims) is LOST: its key is dims_x dims_y dims_z, one past the largest real
// key, so lost rows sort last.
//
// SORT.  Least-significant-digit radix sort, 8-bit digits, ceil(key_bits / 8) passes; the payload of row i is i; keys are carried
// whole and bits at and above key_bits take no part.  A pass is four launches over tiles of kSortTile consecutive positions:
//   1. histogram: a workgroup counts the digits of its tile, one 256-bin LDS histogram per wave, and writes column `block` of the
//      digit-major table [256, blocks];
//   2. scan, two levels (one workgroup looping over the whole table took 0.23 ms of a 0.26 ms pass at a million rows): every chunk of
//      kScanChunk table entries is scanned in place by a workgroup of its own, which leaves the chunk's total; ONE workgroup then turns
//      the totals into exclusive prefix sums; the scatter adds its chunk's;
//   3. scatter: a workgroup recomputes the stable rank of each of its keys among the keys of the same digit in its tile.  Wave w of
//      the four holds positions [256 w, 256 w + 256) of the tile, its item j the 64 consecutive positions from 64 j, one per lane: the
//      rank order -- wave, then item, then lane -- IS position order.  Per item the lanes of equal digit find each other with eight
//      64-bit ballots; the lowest of them takes the wave's running count of the digit (an integer LDS atomic on the wave's own
//      histogram) and hands it round; a lane's rank is that count plus the equal-digit lanes below it.  Equal keys never swap.
// The passes ping-pong between the caller's outputs and the workspace so that the last one lands in the outputs.  The result is
// np.argsort(keys & mask, kind="stable").
//
// REDUCE.  Heads: sorted position i starts a voxel when key[i] != key[i - 1] and key[i] != lost_key; ordered compaction by count / one
// single-workgroup scan / scatter (compact_dev.h, shared with outlier.hip and depth.hip) gives V, every voxel's first
// position, count and key, and voxel_of[idx[i]].  Centroid: the voxel's rows come in ascending index (stability); row number s adds
// d_a = (double)p_a - origin_a in lane s mod 64, a lane's slots ascending from +0.0, the lanes meet in the xor butterfly 32 .. 1 (the
// list fits' statement); c_a = origin_a + S_a / (double)count, rounded to f32 once.  An idle lane holds +0.0 and changes no bit, so a
// voxel is served by a GROUP of 16 lanes with four accumulators each, combined in the butterfly's order (a0 + a2) + (a1 + a3) -- the
// bytes of the 64-lane statement -- and a voxel of more than kGroupMax rows by its whole wave.  Representative: the row with the
// smallest (d2, index), e_a = d_a - S_a / count, d2 = (e_x e_x + e_y e_y) + e_z e_z.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "kernels.h"

// every product, quotient and sum below is rounded on its own: the CPU restatement (tests/_voxel_fixture.py) predicts every bit
#pragma clang fp contract(off)

#include "compact_dev.h"   // kThreads, kWave, kWaves, blocks_of, group_sum (wave_dev.h); block_rank, block_scan, compact_scan_kernel

namespace nesti {
namespace {

constexpr int kDigits = 256;
constexpr int kSortItems = 4;                       // keys per thread and pass
constexpr int kSortTile = kThreads * kSortItems;    // keys per workgroup and pass
constexpr int kGroup = 16;                          // lanes that serve a voxel of at most kGroupMax rows
constexpr int kGroupMax = 256;

struct VoxelLayout {
  size_t keys, idx, hist, chunk, block_cnt, first, total;
};
inline VoxelLayout voxel_layout(size_t n) {
  VoxelLayout L;
  size_t o = 0;
  L.keys = o; o += align_up(n * 8, 256);                                            // the sort's second (key, index) buffer
  L.idx = o; o += align_up(n * 4, 256);
  L.hist = o; o += align_up(blocks_of(n, kSortTile) * kDigits * 4, 256);            // [256, blocks] digit-major
  L.chunk = o; o += align_up(blocks_of(blocks_of(n, kSortTile) * kDigits, kScanChunk) * 4, 256);   // the table's chunk totals
  L.block_cnt = o; o += align_up(blocks_of(n) * 4, 256);                  // the reduce: heads per block
  L.first = o; o += align_up((n + 1) * 4, 256);                                     // the reduce: first sorted position of voxel v; [V] = the live rows
  L.total = o;
  return L;
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------
struct KeyParams {
  const float* cloud;
  int N;
  double origin[3], voxel[3];
  long long dims[3];
  unsigned long long lost;
  unsigned long long* keys_out;
};

// the cell of one coordinate, or -1: floor(t) outside [0, dims)
__device__ __forceinline__ long long cell_of(float p, double origin, double voxel, long long dims) {
  const double d = (double)p - origin;
  const double t = d / voxel;
  const double f = floor(t);
  if (!(f >= 0.0 && f < 9223372036854775808.0)) return -1;      // NaN too; below 2^63 the conversion is exact
  const long long i = (long long)f;
  return i < dims ? i : -1;
}

__global__ __launch_bounds__(kThreads) void voxel_keys_kernel(const KeyParams p) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.N) return;
  const float* c = p.cloud + (size_t)i * 3;
  const float x = c[0], y = c[1], z = c[2];
  unsigned long long key = p.lost;
  if (finite_bits(x) && finite_bits(y) && finite_bits(z)) {
    const long long ix = cell_of(x, p.origin[0], p.voxel[0], p.dims[0]);
    const long long iy = cell_of(y, p.origin[1], p.voxel[1], p.dims[1]);
    const long long iz = cell_of(z, p.origin[2], p.voxel[2], p.dims[2]);
    if (ix >= 0 && iy >= 0 && iz >= 0)
      key = ((unsigned long long)iz * (unsigned long long)p.dims[1] + (unsigned long long)iy) * (unsigned long long)p.dims[0] +
            (unsigned long long)ix;
  }
  p.keys_out[i] = key;
}

// ---- sort -----------------------------------------------------------------------------------------------------------------------------------
struct SortPass {
  const unsigned long long* keys_in;
  const int32_t* idx_in;              // NULL: the payload of position i is i (the first pass)
  unsigned long long* keys_out;
  int32_t* idx_out;
  int32_t* hist;                      // [256, nb]
  const int32_t* chunk;               // the scanned totals of the table's chunks of kScanChunk entries
  int N, nb, shift;
  unsigned mask;                      // of the pass's digit: 0xff, or fewer bits in the last pass
};

__device__ __forceinline__ unsigned digit_of(const SortPass& p, unsigned long long key) { return (unsigned)(key >> p.shift) & p.mask; }
// position of item j of this thread: wave w holds [256 w, 256 w + 256) of the tile, item j its 64 positions from 64 j
__device__ __forceinline__ long long sort_pos(int j) {
  return (long long)blockIdx.x * kSortTile + (threadIdx.x >> 6) * (kWave * kSortItems) + j * kWave + (threadIdx.x & (kWave - 1));
}

__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const SortPass p) {
  __shared__ int h[kWaves][kDigits];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) h[w][threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    const long long i = sort_pos(j);
    if (i < p.N) atomicAdd(&h[wave][digit_of(p, p.keys_in[i])], 1);
  }
  __syncthreads();
  int sum = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) sum += h[w][threadIdx.x];
  p.hist[(size_t)threadIdx.x * p.nb + blockIdx.x] = sum;
}

// The first level of the sort's scan, over block_scan (compact_dev.h): workgroup b scans entries [b kScanChunk, (b + 1) kScanChunk)
// of v[0 .. n) in place and leaves their total in chunk_total[b]
__global__ __launch_bounds__(kThreads) void sort_scan_chunks_kernel(int32_t* __restrict__ v, long long n, int32_t* __restrict__ chunk_total) {
  const long long i0 = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanPer;
  int e[kScanPer];
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) e[j] = i0 + j < n ? v[i0 + j] : 0;
  const int tot = block_scan(e);
#pragma unroll
  for (int j = 0; j < kScanPer; ++j)
    if (i0 + j < n) v[i0 + j] = e[j];
  if (threadIdx.x == 0) chunk_total[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(const SortPass p) {
  __shared__ int cnt[kWaves][kDigits];                     // a wave's running count per digit; then where its keys of the digit go
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) cnt[w][threadIdx.x] = 0;
  __syncthreads();
  unsigned long long key[kSortItems];
  int32_t pay[kSortItems];
  int rank[kSortItems];
  unsigned dig[kSortItems];
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    const long long i = sort_pos(j);
    const bool live = i < p.N;
    key[j] = live ? p.keys_in[i] : 0ull;
    pay[j] = live ? (p.idx_in ? p.idx_in[i] : (int32_t)i) : 0;
    dig[j] = digit_of(p, key[j]);
  }
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    const bool live = sort_pos(j) < p.N;
    // the live lanes of this item whose digit is mine
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dig[j] >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    int base = 0, leader = 0;
    if (live) {
      leader = __ffsll((long long)peers) - 1;              // peers holds this lane: never empty
      if (lane == leader) base = atomicAdd(&cnt[wave][dig[j]], __popcll(peers));
    }
    base = __shfl(base, leader, kWave);
    rank[j] = base + __popcll(peers & below);
  }
  __syncthreads();
  {                                                         // thread d: the tile's start for digit d, then wave by wave
    const size_t entry = (size_t)threadIdx.x * p.nb + blockIdx.x;
    int run = p.hist[entry] + p.chunk[entry / kScanChunk];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = cnt[w][threadIdx.x];
      cnt[w][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    if (sort_pos(j) >= p.N) continue;
    const long long dst = (long long)cnt[wave][dig[j]] + rank[j];
    if (dst < 0 || dst >= p.N) continue;                    // cannot happen: the table counts the same keys
    p.keys_out[dst] = key[j];
    p.idx_out[dst] = pay[j];
  }
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
struct ReduceParams {
  const float* cloud;
  const unsigned long long* keys;     // sorted
  const int32_t* idx;                 // the rows in sorted order
  int N;
  unsigned long long lost;
  double origin[3];
  float* centroid_out;
  int32_t* rep_out;
  int32_t* count_out;
  unsigned long long* key_out;
  int32_t* voxel_of_out;
  const int32_t* n_voxels;            // device: V, written by the scan
  int32_t* first;                     // [N + 1] workspace
};

__device__ __forceinline__ bool is_head(const ReduceParams& p, long long i) {
  if (i >= p.N) return false;
  const unsigned long long k = p.keys[i];
  return k != p.lost && (i == 0 || k != p.keys[i - 1]);
}

__global__ __launch_bounds__(kThreads) void voxel_count_kernel(const ReduceParams p, int32_t* __restrict__ block_count) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  int total;
  block_rank(is_head(p, i), &total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void voxel_heads_kernel(const ReduceParams p, const int32_t* __restrict__ block_start) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool head = is_head(p, i);
  int total;
  const int before = block_start[blockIdx.x] + block_rank(head, &total);   // the heads below position i: <= i
  if (i >= p.N) return;
  const unsigned long long k = p.keys[i];
  const bool lost = k == p.lost;
  if (head) {
    p.first[before] = (int32_t)i;
    if (p.key_out) p.key_out[before] = k;
  }
  // where the live rows end: the first lost position or, where there is none, N -- entry V of `first`
  if (lost && (i == 0 || p.keys[i - 1] != p.lost)) p.first[before] = (int32_t)i;
  if (!lost && i == p.N - 1) p.first[before + (head ? 1 : 0)] = p.N;
  if (p.voxel_of_out) {
    const int32_t row = p.idx[i];
    if ((unsigned)row < (unsigned)p.N) p.voxel_of_out[row] = lost ? -1 : before + (head ? 1 : 0) - 1;
  }
}

// One voxel by a group of G lanes (sl: the lane within it): G = 64 is the statement; G = 16 holds the four lanes sl, sl + 16, sl + 32,
// sl + 48 of the statement as accumulators and meets them in the butterfly's order.  Every lane of the group calls it.
template <int G>
__device__ __forceinline__ void reduce_voxel(const ReduceParams& p, int v, int begin, int count, int sl) {
  constexpr int A = kWave / G;
  const double ox = p.origin[0], oy = p.origin[1], oz = p.origin[2];
  double sx[A], sy[A], sz[A];
#pragma unroll
  for (int a = 0; a < A; ++a) sx[a] = sy[a] = sz[a] = 0.0;
  for (int base = 0; base < count; base += kWave) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
      const int s = base + a * G + sl;
      if (s < count) {
        const int32_t row = p.idx[begin + s];
        if ((unsigned)row < (unsigned)p.N) {
          const float* c = p.cloud + (size_t)row * 3;
          sx[a] = sx[a] + ((double)c[0] - ox);
          sy[a] = sy[a] + ((double)c[1] - oy);
          sz[a] = sz[a] + ((double)c[2] - oz);
        }
      }
    }
  }
  double Sx, Sy, Sz;
  if constexpr (A == 4) {                                   // offsets 32 and 16 of the butterfly
    Sx = (sx[0] + sx[2]) + (sx[1] + sx[3]);
    Sy = (sy[0] + sy[2]) + (sy[1] + sy[3]);
    Sz = (sz[0] + sz[2]) + (sz[1] + sz[3]);
  } else {
    static_assert(A == 1, "a group of 16 lanes or the wave");
    Sx = sx[0]; Sy = sy[0]; Sz = sz[0];
  }
  Sx = group_sum<G>(Sx);
  Sy = group_sum<G>(Sy);
  Sz = group_sum<G>(Sz);
  const double n = (double)count;
  const double mx = Sx / n, my = Sy / n, mz = Sz / n;
  if (sl == 0) {
    if (p.centroid_out) {
      const double cx = ox + mx, cy = oy + my, cz = oz + mz;
      float* dst = p.centroid_out + (size_t)v * 3;
      dst[0] = (float)cx; dst[1] = (float)cy; dst[2] = (float)cz;
    }
    if (p.count_out) p.count_out[v] = count;
  }
  if (!p.rep_out) return;
  // the row nearest the fp64 centroid: the smallest (d2, index); a lane's rows come in ascending index
  double best = (double)INFINITY;
  int best_row = 0x7fffffff;
  for (int s = sl; s < count; s += G) {
    const int32_t row = p.idx[begin + s];
    if ((unsigned)row >= (unsigned)p.N) continue;
    const float* c = p.cloud + (size_t)row * 3;
    const double ex = ((double)c[0] - ox) - mx, ey = ((double)c[1] - oy) - my, ez = ((double)c[2] - oz) - mz;
    const double d2 = (ex * ex + ey * ey) + ez * ez;
    if (d2 < best || (d2 == best && row < best_row)) {
      best = d2;
      best_row = row;
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const double ob = __shfl_xor(best, off, kWave);
    const int orow = __shfl_xor(best_row, off, kWave);
    if (ob < best || (ob == best && orow < best_row)) {
      best = ob;
      best_row = orow;
    }
  }
  if (sl == 0) p.rep_out[v] = best_row;
}

// A wave serves four consecutive voxels, one per group of 16 lanes; a voxel of more than kGroupMax rows is then served by the whole
// wave, 64 lanes, with the same bytes.
__global__ __launch_bounds__(kThreads) void voxel_reduce_kernel(const ReduceParams p) {
  const int lane = threadIdx.x & (kWave - 1);
  const int V = min(max(*p.n_voxels, 0), p.N);
  constexpr int kPerWave = kWave / kGroup;
  const long long v0 = ((long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kPerWave;
  if (v0 >= V) return;
  const long long v = v0 + lane / kGroup;
  int begin = 0, count = 0;
  if (v < V) {                                              // clamped: a table of a caller's unsorted keys must not lead outside
    begin = min(max(p.first[v], 0), p.N);
    count = min(max(p.first[v + 1], begin), p.N) - begin;
  }
  const bool big = count > kGroupMax;
  if (v < V && !big) reduce_voxel<kGroup>(p, (int)v, begin, count, lane & (kGroup - 1));
  const unsigned long long bigs = __ballot(big);
  for (int g = 0; g < kPerWave; ++g) {
    if (!((bigs >> (g * kGroup)) & 1ull)) continue;         // the same in every lane
    const int b = __shfl(begin, g * kGroup, kWave), c = __shfl(count, g * kGroup, kWave);
    reduce_voxel<kWave>(p, (int)(v0 + g), b, c, lane);
  }
}

bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

size_t nesti_voxel_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return voxel_layout((size_t)n).total;
}

int nesti_sort_tile_items(void) { return kSortTile; }

int nesti_voxel_keys(const float* cloud_dev, int N, const double* origin, const double* voxel, const int64_t* dims, uint64_t* keys_out_dev,
                     void* stream) {
  const std::string w("nesti_voxel_keys");
  if (!cloud_dev || !origin || !voxel || !dims || !keys_out_dev) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(voxel[a]) || !(voxel[a] > 0.0)) NESTI_FAIL(w + ": voxel sizes must be finite and > 0");
  if (!finite3(origin)) NESTI_FAIL(w + ": origin must be finite");
  unsigned long long cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) NESTI_FAIL(w + ": dims must be >= 1");
    if ((unsigned long long)dims[a] >= (1ull << 62) / cells + 1) NESTI_FAIL(w + ": dims: the number of cells must be below 2^62");
    cells *= (unsigned long long)dims[a];
  }
  if (cells >= (1ull << 62)) NESTI_FAIL(w + ": dims: the number of cells must be below 2^62");
  KeyParams p;
  p.cloud = cloud_dev; p.N = N; p.lost = cells; p.keys_out = (unsigned long long*)keys_out_dev;
  for (int a = 0; a < 3; ++a) {
    p.origin[a] = origin[a]; p.voxel[a] = voxel[a]; p.dims[a] = (long long)dims[a];
  }
  hipStream_t st = (hipStream_t)stream;
  const int tok = prof_begin(NESTI_PROF_PATCHES, st);
  hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)blocks_of((size_t)N)), dim3(kThreads), 0, st, p);
  prof_end(NESTI_PROF_PATCHES, tok, st);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int nesti_sort_pairs(const uint64_t* keys_in_dev, int N, int key_bits, uint64_t* keys_out_dev, int32_t* idx_out_dev, void* ws_dev,
                     size_t ws_bytes, void* stream) {
  const std::string w("nesti_sort_pairs");
  if (!keys_in_dev || !keys_out_dev || !idx_out_dev || !ws_dev) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": N must be > 0");
  if (key_bits < 1 || key_bits > 64) NESTI_FAIL(w + ": key_bits must be in 1 .. 64");
  const VoxelLayout L = voxel_layout((size_t)N);
  if (ws_bytes < L.total) NESTI_FAIL(w + ": workspace too small (nesti_voxel_workspace_bytes(N))");
  if (keys_out_dev == keys_in_dev) NESTI_FAIL(w + ": keys_out must not be keys_in (the passes ping-pong through it)");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  unsigned long long* keys_buf[2] = {(unsigned long long*)keys_out_dev, (unsigned long long*)(ws + L.keys)};
  int32_t* idx_buf[2] = {idx_out_dev, (int32_t*)(ws + L.idx)};
  const int passes = (key_bits + 7) / 8;
  const int nb = (int)blocks_of((size_t)N, kSortTile);
  SortPass p;
  p.hist = (int32_t*)(ws + L.hist);
  int32_t* chunk = (int32_t*)(ws + L.chunk);
  p.chunk = chunk;
  const long long entries = (long long)nb * kDigits;
  const int n_chunks = (int)blocks_of((size_t)entries, kScanChunk);
  p.N = N; p.nb = nb;
  p.keys_in = (const unsigned long long*)keys_in_dev;
  p.idx_in = nullptr;
  const int tok = prof_begin(NESTI_PROF_PATCHES, st);
  for (int pass = 0; pass < passes; ++pass) {
    const int to = (passes - 1 - pass) & 1;                 // the last pass writes the outputs (buffer 0)
    p.keys_out = keys_buf[to];
    p.idx_out = idx_buf[to];
    p.shift = 8 * pass;
    const int bits = std::min(8, key_bits - p.shift);
    p.mask = (1u << bits) - 1u;
    hipLaunchKernelGGL(sort_hist_kernel, dim3(nb), dim3(kThreads), 0, st, p);
    hipLaunchKernelGGL(sort_scan_chunks_kernel, dim3(n_chunks), dim3(kThreads), 0, st, p.hist, entries, chunk);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, chunk, (long long)n_chunks, (int32_t*)nullptr);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(nb), dim3(kThreads), 0, st, p);
    p.keys_in = p.keys_out;
    p.idx_in = p.idx_out;
  }
  prof_end(NESTI_PROF_PATCHES, tok, st);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

int nesti_voxel_reduce(const float* cloud_dev, int N, const uint64_t* sorted_keys_dev, const int32_t* sorted_idx_dev, uint64_t lost_key,
                       const double* origin, float* centroid_out_dev, int32_t* rep_out_dev, int32_t* count_out_dev, uint64_t* key_out_dev,
                       int32_t* voxel_of_out_dev, int32_t* n_voxels_out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  const std::string w("nesti_voxel_reduce");
  if (!cloud_dev || !sorted_keys_dev || !sorted_idx_dev || !origin || !n_voxels_out_dev || !ws_dev) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (!finite3(origin)) NESTI_FAIL(w + ": origin must be finite");
  const VoxelLayout L = voxel_layout((size_t)N);
  if (ws_bytes < L.total) NESTI_FAIL(w + ": workspace too small (nesti_voxel_workspace_bytes(N))");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  int32_t* block_cnt = (int32_t*)(ws + L.block_cnt);
  ReduceParams p;
  p.cloud = cloud_dev; p.keys = (const unsigned long long*)sorted_keys_dev; p.idx = sorted_idx_dev; p.N = N;
  p.lost = (unsigned long long)lost_key;
  for (int a = 0; a < 3; ++a) p.origin[a] = origin[a];
  p.centroid_out = centroid_out_dev; p.rep_out = rep_out_dev; p.count_out = count_out_dev;
  p.key_out = (unsigned long long*)key_out_dev; p.voxel_of_out = voxel_of_out_dev;
  p.n_voxels = n_voxels_out_dev; p.first = (int32_t*)(ws + L.first);
  const int nb = (int)blocks_of((size_t)N);
  const int tok = prof_begin(NESTI_PROF_PATCHES, st);
  hipLaunchKernelGGL(voxel_count_kernel, dim3(nb), dim3(kThreads), 0, st, p, block_cnt);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, block_cnt, (long long)nb, n_voxels_out_dev);
  hipLaunchKernelGGL(voxel_heads_kernel, dim3(nb), dim3(kThreads), 0, st, p, (const int32_t*)block_cnt);
  if (centroid_out_dev || rep_out_dev || count_out_dev) {
    // a voxel per group of 16 lanes, over the N voxels there may be; the groups beyond V leave at once
    const unsigned grid = (unsigned)blocks_of((size_t)N, (size_t)kWaves * (kWave / kGroup));
    hipLaunchKernelGGL(voxel_reduce_kernel, dim3(grid), dim3(kThreads), 0, st, p);
  }
  prof_end(NESTI_PROF_PATCHES, tok, st);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
