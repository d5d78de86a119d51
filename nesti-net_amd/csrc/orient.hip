// Consistent orientation of estimated normals ("Orientation"): Hoppe's spanning-tree propagation made unique, as a
// post-pass over [M] positions and their normals.  The reference has no such step (its loss is unoriented); the consumer is its
// "RMS oriented" figure (utils/evaluate.py:151).  The conventions below are the library's own.
//
//   grid (patches.hip, one scale of radius R)  ->  eligibility  ->  K nearest eligible neighbours inside R per row (fp64 distances,
//   dot3 below: five separately rounded operations, NOT the fused ball_d2 of patches_dev.h; one wave per row)  ->  one edge per
//   unordered neighbour pair with key (bits of 1 - cos^2) << 32 | id  ->  Boruvka's minimum spanning forest over a union-find whose
//   words carry the sign parity to the parent  ->  per tree the root (largest z, or nearest to the viewpoint) and its sign  ->  sign
//   flips.
//
// One kernel per step, fixed launch counts derived from M, integer atomics only: the result is a pure function of the inputs, no
// workgroup waits on another and the host neither synchronises nor reads anything back.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"

// every product and sum below is rounded on its own: the CPU restatement (tests/_orient_fixture.py) predicts each bit
#pragma clang fp contract(off)

namespace nesti {
namespace {

constexpr int kMaxK = 16;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kThreads / kWave;       // orient_knn_kernel: one wave per row
constexpr unsigned long long kNoKey = ~0ull;

// stats block of the workspace (int32 words): the four counters of nesti_orient_stats_t, then one "a component hooked" flag per
// Boruvka round
constexpr int kStatEligible = 0, kStatComponents = 1, kStatFlipped = 2, kStatEdges = 3, kStatRoundFlag = 8;
constexpr int kMaxRounds = 40;
constexpr size_t kStatBytes = 256;
static_assert((kStatRoundFlag + kMaxRounds) * 4 <= (int)kStatBytes, "stats block");

struct OrientLayout {
  size_t stats, elig, nbr, eu, ev, ekey, eflip, uf, comp, best, rootkey, rootidx, total;
};
inline OrientLayout orient_layout(int M, int K) {
  OrientLayout L;
  const size_t m = (size_t)M, mk = (size_t)M * (size_t)K;
  size_t o = 0;
  L.stats = o; o += kStatBytes;
  L.elig = o; o += align_up(m, 256);
  L.nbr = o; o += align_up(mk * 4, 256);
  L.eu = o; o += align_up(mk * 4, 256);
  L.ev = o; o += align_up(mk * 4, 256);
  L.ekey = o; o += align_up(mk * 8, 256);
  L.eflip = o; o += align_up(mk, 256);
  L.uf = o; o += align_up(m * 4, 256);
  L.comp = o; o += align_up(m * 4, 256);
  L.best = o; o += align_up(m * 8, 256);
  L.rootkey = o; o += align_up(m * 8, 256);
  L.rootidx = o; o += align_up(m * 4, 256);
  L.total = o;
  return L;
}

__device__ __forceinline__ bool nonzero_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) != 0u; }
// all three components finite and at least one non-zero, on the bits
__device__ __forceinline__ bool eligible_normal(const float* n) {
  return finite_bits(n[0]) && finite_bits(n[1]) && finite_bits(n[2]) && (nonzero_bits(n[0]) || nonzero_bits(n[1]) || nonzero_bits(n[2]));
}
// (ax bx + ay by) + az bz in fp64, each operation rounded on its own
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  const double s = ax * bx + ay * by;     // contraction is off in this file: two products, one sum
  return s + az * bz;
}
// adds a wave's number of true predicates to a counter with one atomic
__device__ __forceinline__ void count_wave(bool pred, int* counter) {
  const unsigned long long b = __ballot(pred);
  if (b && (int)(threadIdx.x & (kWave - 1)) == __ffsll((long long)b) - 1) atomicAdd(counter, __popcll(b));
}

__global__ void orient_eligible_kernel(const float* __restrict__ normals, int M, unsigned char* __restrict__ elig, int* stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool e = false;
  if (i < M) {
    e = eligible_normal(normals + (size_t)i * 3);
    elig[i] = e ? 1 : 0;
  }
  count_wave(e, stats + kStatEligible);
}

// ---- K nearest eligible neighbours inside the ball --------------------------------------------------------------------------------
struct Cand {
  double d2;
  int j;
};
__device__ __forceinline__ bool cand_less(const Cand& a, const Cand& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.j < b.j); }

// One wave per row.  The nine x-spans of the 3 x 3 x 3 cell block are block_span's (patches_dev.h), written out; every lane keeps the
// KC >= K smallest (d2, j) of the candidates it saw, sorted, in registers; K rounds of a wave-wide minimum over the lanes' heads then emit
// the list in order (the winner shifts its list down).  A candidate is seen by exactly one lane, so j identifies the winner.
template <int KC>
__global__ __launch_bounds__(kThreads) void orient_knn_kernel(const float* __restrict__ xyz, const unsigned char* __restrict__ elig,
                                                              const float4* __restrict__ sorted, const int* __restrict__ start,
                                                              const GridHeader* __restrict__ header, int M, int K, double r2,
                                                              int32_t* __restrict__ nbr) {
  const int lane = threadIdx.x & (kWave - 1);
  const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= M) return;                                    // whole waves leave: the shuffles below see full waves
  const float cf0 = xyz[(size_t)row * 3], cf1 = xyz[(size_t)row * 3 + 1], cf2 = xyz[(size_t)row * 3 + 2];
  const bool live = elig[row] && finite_bits(cf0) && finite_bits(cf1) && finite_bits(cf2);
  int b = 0, e = 0;
  if (live && lane < 9) {
    const GridHeader h = *header;
    int ix, iy, iz;
    cell_coords(h, cf0, cf1, cf2, &ix, &iy, &iz);
    const int zz = iz + lane / 3 - 1, yy = iy + lane % 3 - 1;
    if (zz >= 0 && zz < h.dims[2] && yy >= 0 && yy < h.dims[1]) {
      const int x0 = max(ix - 1, 0), x1 = min(ix + 1, h.dims[0] - 1);
      b = start[cell_flat(h, x0, yy, zz)];
      e = start[cell_flat(h, x1, yy, zz) + 1];
    }
  }
  Cand a[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) { a[s].d2 = INFINITY; a[s].j = 0x7fffffff; }
  const double cx = cf0, cy = cf1, cz = cf2;
  for (int sp = 0; sp < 9; ++sp) {
    const int sb = __shfl(b, sp, kWave), se = min(__shfl(e, sp, kWave), M);     // a span never leaves the cell-ordered copy
    for (int i = max(sb, 0) + lane; i < se; i += kWave) {
      const float4 c = sorted[i];
      const double dx = (double)c.x - cx, dy = (double)c.y - cy, dz = (double)c.z - cz;
      Cand n;
      n.d2 = dot3(dx, dy, dz, dx, dy, dz);
      n.j = __float_as_int(c.w);
      if (n.d2 <= r2 && cand_less(n, a[KC - 1]) && n.j != row && n.j >= 0 && n.j < M && elig[n.j]) {
        a[KC - 1] = n;
#pragma unroll
        for (int s = KC - 1; s > 0; --s) {
          if (cand_less(a[s], a[s - 1])) {
            const Cand t = a[s];
            a[s] = a[s - 1];
            a[s - 1] = t;
          }
        }
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    Cand m = a[0];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      Cand o;
      o.d2 = __shfl_xor(m.d2, off, kWave);
      o.j = __shfl_xor(m.j, off, kWave);
      if (cand_less(o, m)) m = o;
    }
    const bool found = m.j != 0x7fffffff;
    if (found && a[0].j == m.j) {                          // the winning lane: drop its head
#pragma unroll
      for (int s = 0; s + 1 < KC; ++s) a[s] = a[s + 1];
      a[KC - 1].d2 = INFINITY;
      a[KC - 1].j = 0x7fffffff;
    }
    if (lane == 0) nbr[(size_t)row * K + k] = found ? m.j : -1;
  }
}

// ---- edges ------------------------------------------------------------------------------------------------------------------------
// One thread per (i, slot).  The pair {a < b} lives in the slot of b in nbr(a) when b is in nbr(a), else in the slot of a in nbr(b):
// slot (i, s) holding j is that slot iff i < j, or i > j and i is not in nbr(j).
__global__ void orient_edges_kernel(const float* __restrict__ normals, const int32_t* __restrict__ nbr, int M, int K,
                                    int32_t* __restrict__ eu, int32_t* __restrict__ ev, unsigned long long* __restrict__ ekey,
                                    unsigned char* __restrict__ eflip, uint32_t* __restrict__ wbits_out, int* stats) {
  const unsigned id = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned total = (unsigned)M * (unsigned)K;
  bool valid = false;
  if (id < total) {
    const int i = (int)(id / (unsigned)K);
    const int j = nbr[id];
    valid = j >= 0;
    if (valid && i > j) {
      for (int s = 0; s < K; ++s)
        if (nbr[(size_t)j * K + s] == i) valid = false;
    }
    int u = -1, v = -1;
    unsigned wb = 0u;
    unsigned char f = 0;
    if (valid) {
      u = min(i, j);
      v = max(i, j);
      const float* na = normals + (size_t)u * 3;
      const float* nb = normals + (size_t)v * 3;
      const double ax = na[0], ay = na[1], az = na[2], bx = nb[0], by = nb[1], bz = nb[2];
      const double d = dot3(ax, ay, az, bx, by, bz);
      const double qa = dot3(ax, ay, az, ax, ay, az), qb = dot3(bx, by, bz, bx, by, bz);
      const double dd = d * d, qq = qa * qb;
      const double c2 = dd / qq;
      const double w = fmax(0.0, 1.0 - c2);
      wb = __float_as_uint((float)w);
      f = d < 0.0 ? 1 : 0;
    }
    eu[id] = u;
    ev[id] = v;
    ekey[id] = valid ? (((unsigned long long)wb << 32) | (unsigned long long)id) : kNoKey;
    eflip[id] = f;
    if (wbits_out) wbits_out[id] = wb;
  }
  count_wave(valid, stats + kStatEdges);
}

// ---- Boruvka over a parity-carrying union-find -------------------------------------------------------------------------------------
// word[x] = parent(x) << 1 | parity of x's sign relative to its parent.  Round r: comp[] = the flattened words (a snapshot the round's
// min and hook steps read while the hook writes uf[]), best[] = the smallest key leaving each component.  Rounds after one in which
// nothing hooked return at once (flag[r - 1] == 0).
__global__ void orient_uf_init_kernel(unsigned* __restrict__ uf, int M) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < M) uf[x] = (unsigned)x << 1;
}

__global__ void orient_round_reset_kernel(const unsigned* __restrict__ uf, unsigned* __restrict__ comp,
                                          unsigned long long* __restrict__ best, int M, const int* prev_flag) {
  if (prev_flag && *prev_flag == 0) return;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < M) {
    comp[x] = uf[x];
    best[x] = kNoKey;
  }
}

__global__ void orient_round_min_kernel(const int32_t* __restrict__ eu, const int32_t* __restrict__ ev,
                                        const unsigned long long* __restrict__ ekey, const unsigned* __restrict__ comp,
                                        unsigned long long* __restrict__ best, unsigned total, const int* prev_flag) {
  if (prev_flag && *prev_flag == 0) return;
  const unsigned id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const int u = eu[id];
  if (u < 0) return;
  const unsigned cu = comp[u] >> 1, cv = comp[ev[id]] >> 1;
  if (cu == cv) return;
  const unsigned long long key = ekey[id];
  atomicMin(&best[cu], key);
  atomicMin(&best[cv], key);
}

// component c with best edge (u in c, v in c'): parent[c] = c', parity P(u) ^ f ^ P(v) -- unless c' chose the same edge and c < c'
// (a mutual pair: the smaller stays root; keys are distinct, so mutual pairs are the only possible cycles)
__global__ void orient_round_hook_kernel(const int32_t* __restrict__ eu, const int32_t* __restrict__ ev,
                                         const unsigned char* __restrict__ eflip, const unsigned* __restrict__ comp,
                                         const unsigned long long* __restrict__ best, unsigned* __restrict__ uf, int M,
                                         unsigned char* __restrict__ tree_edge, const int* prev_flag, int* flag) {
  if (prev_flag && *prev_flag == 0) return;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= M) return;
  if ((comp[c] >> 1) != (unsigned)c) return;
  const unsigned long long key = best[c];
  if (key == kNoKey) return;
  const unsigned id = (unsigned)(key & 0xffffffffull);
  const unsigned wu = comp[eu[id]], wv = comp[ev[id]];
  const unsigned other = (wu >> 1) == (unsigned)c ? (wv >> 1) : (wu >> 1);
  if (best[other] == key && (unsigned)c < other) return;
  uf[c] = (other << 1) | ((wu ^ wv ^ (unsigned)eflip[id]) & 1u);
  if (tree_edge) tree_edge[id] = 1;
  *flag = 1;                                              // every writer stores the same value
}

// pointer jumping in place: p's word is a valid (ancestor, parity to it) pair whether read before or after p's own update
__global__ void orient_round_jump_kernel(unsigned* __restrict__ uf, int M, const int* flag) {
  if (*flag == 0) return;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= M) return;
  const unsigned w = __hip_atomic_load(&uf[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned p = w >> 1;
  if (p == (unsigned)x) return;
  const unsigned wp = __hip_atomic_load(&uf[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((wp >> 1) == p) return;                              // the parent is a root
  __hip_atomic_store(&uf[x], (wp & ~1u) | ((w ^ wp) & 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- roots and signs ----------------------------------------------------------------------------------------------------------------
struct View {
  int on;
  double v[3];
};
// n . (v - p) in fp64, the viewpoint test of both modes
__device__ __forceinline__ bool faces_away(const float* n, const float* p, const View& vw) {
  const double dx = vw.v[0] - (double)p[0], dy = vw.v[1] - (double)p[1], dz = vw.v[2] - (double)p[2];
  return dot3((double)n[0], (double)n[1], (double)n[2], dx, dy, dz) < 0.0;
}
// smaller = better root: the bits of the fp64 d2 to the viewpoint, or the inverted order-preserving word of z (-0 counts as +0)
__device__ __forceinline__ unsigned long long root_key(const float* p, const View& vw) {
  if (vw.on) {
    const double dx = vw.v[0] - (double)p[0], dy = vw.v[1] - (double)p[1], dz = vw.v[2] - (double)p[2];
    return (unsigned long long)__double_as_longlong(dot3(dx, dy, dz, dx, dy, dz));
  }
  unsigned u = __float_as_uint(p[2]);
  if ((u & 0x7fffffffu) == 0u) u = 0u;
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (unsigned long long)(~ord);
}

__global__ void orient_root_init_kernel(unsigned long long* __restrict__ rootkey, int32_t* __restrict__ rootidx, int M) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < M) {
    rootkey[x] = kNoKey;
    rootidx[x] = 0x7fffffff;
  }
}
// pass 0: the best key of each tree; pass 1: the smallest index that has it
__global__ void orient_root_kernel(const float* __restrict__ xyz, const unsigned char* __restrict__ elig,
                                   const unsigned* __restrict__ uf, int M, View vw, unsigned long long* __restrict__ rootkey,
                                   int32_t* __restrict__ rootidx, int pass) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= M || !elig[x]) return;
  const unsigned r = uf[x] >> 1;
  const unsigned long long key = root_key(xyz + (size_t)x * 3, vw);
  if (pass == 0) atomicMin(&rootkey[r], key);
  else if (rootkey[r] == key) atomicMin(&rootidx[r], x);
}

// Per tree (thread of its union-find root r): the flip of the tree's root t = rootidx[r] by the root rule, stored relative to r as
// cflip[r] = flip(t) ^ P(t), P = parity to r.  A kernel of its own: the rule reads t's normal, which orient_apply_kernel rewrites.
__global__ void orient_rootflip_kernel(const float* __restrict__ xyz, const float* __restrict__ normals,
                                       const unsigned char* __restrict__ elig, const unsigned* __restrict__ uf,
                                       const int32_t* __restrict__ rootidx, int M, View vw, unsigned* __restrict__ cflip, int* stats) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool is_root = r < M && elig[r] && (uf[r] >> 1) == (unsigned)r;
  if (is_root) {
    int t = rootidx[r];
    if (t < 0 || t >= M) t = r;                            // cannot happen: r's own key took part in both passes
    const float* nt = normals + (size_t)t * 3;
    bool g;
    if (vw.on) {
      g = faces_away(nt, xyz + (size_t)t * 3, vw);
    } else {                                               // the first non-zero of (n_z, n_y, n_x) becomes positive
      const float lead = nonzero_bits(nt[2]) ? nt[2] : nonzero_bits(nt[1]) ? nt[1] : nt[0];
      g = (__float_as_uint(lead) & 0x80000000u) != 0u;
    }
    cflip[r] = (g ? 1u : 0u) ^ (uf[t] & 1u);
  }
  count_wave(is_root, stats + kStatComponents);
}

// flip(x) = flip(tree root) ^ parity of the tree path root -> x = cflip[r] ^ P(x); a flip negates the three floats, sign bits only
__global__ void orient_apply_kernel(float* __restrict__ normals, const unsigned char* __restrict__ elig,
                                    const unsigned* __restrict__ uf, const unsigned* __restrict__ cflip, int M, int* stats) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  bool flip = false;
  if (x < M && elig[x]) {
    const unsigned w = uf[x];
    flip = ((cflip[w >> 1] ^ w) & 1u) != 0u;
  }
  if (flip) {
    unsigned* n = reinterpret_cast<unsigned*>(normals + (size_t)x * 3);
    n[0] ^= 0x80000000u;
    n[1] ^= 0x80000000u;
    n[2] ^= 0x80000000u;
  }
  count_wave(flip, stats + kStatFlipped);
}

// NESTI_ORIENT_VIEWPOINT: no graph
__global__ void orient_viewpoint_kernel(const float* __restrict__ xyz, float* __restrict__ normals, int M, View vw, int* stats) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  bool e = false, flip = false;
  if (x < M) {
    float* n = normals + (size_t)x * 3;
    e = eligible_normal(n);
    flip = e && faces_away(n, xyz + (size_t)x * 3, vw);
    if (flip) {
      unsigned* u = reinterpret_cast<unsigned*>(n);
      u[0] ^= 0x80000000u;
      u[1] ^= 0x80000000u;
      u[2] ^= 0x80000000u;
    }
  }
  count_wave(e, stats + kStatEligible);
  count_wave(flip, stats + kStatFlipped);
}

int ceil_log2(long long n) {
  int b = 0;
  while ((1ll << b) < n) ++b;
  return b;
}

// ---- host: argument checks (before any device call), then the launches ------------------------------------------------------------
int check_common(const std::string& w, const float* xyz_dev, int M, const float* normals_dev, double radius, int K,
                 const void* grid_ws_dev, size_t grid_ws_bytes, const void* ws_dev, size_t ws_bytes) {
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (K < 1 || K > kMaxK) NESTI_FAIL(w + ": K must be in [1, 16]");
  if (!std::isfinite(radius) || !(radius > 0.0)) NESTI_FAIL(w + ": radius must be finite and > 0");
  if ((unsigned long long)M * (unsigned long long)K >= (1ull << 32)) NESTI_FAIL(w + ": M * K must be below 2^32 (edge ids are 32-bit)");
  if (M == 0) return 0;
  if (!xyz_dev || !normals_dev || !grid_ws_dev || !ws_dev) NESTI_FAIL(w + ": null argument");
  if (grid_ws_bytes < patch_ws_layout(M).total) NESTI_FAIL(w + ": grid workspace too small (nesti_patches_workspace_bytes(M))");
  if (ws_bytes < orient_layout(M, K).total) NESTI_FAIL(w + ": workspace too small (nesti_orient_workspace_bytes(M, K))");
  return 0;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// grid, eligibility, neighbour lists and edges into the workspace
int build_graph(const float* xyz, int M, const float* normals, double radius, int K, void* grid_ws, size_t grid_ws_bytes,
                unsigned char* ws, const OrientLayout& L, uint32_t* wbits_out, hipStream_t st) {
  nesti_config_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.n_scales = 1;
  const double r_abs[1] = {radius};
  if (nesti_patches_grid(&cfg, xyz, M, r_abs, grid_ws, grid_ws_bytes, st)) return 1;
  const WsLayout G = patch_ws_layout(M);
  const unsigned char* gws = (const unsigned char*)grid_ws;
  int* stats = (int*)(ws + L.stats);
  unsigned char* elig = ws + L.elig;
  int32_t* nbr = (int32_t*)(ws + L.nbr);
  NESTI_CHECK_HIP(hipMemsetAsync(stats, 0, kStatBytes, st));
  hipLaunchKernelGGL(orient_eligible_kernel, dim3(blocks_for(M)), dim3(kThreads), 0, st, normals, M, elig, stats);
  const unsigned kb = (unsigned)(((size_t)M + kRowsPerBlock - 1) / kRowsPerBlock);
  const float4* sorted = (const float4*)(gws + G.sorted);
  const int* start = (const int*)(gws + G.start);
  const GridHeader* header = (const GridHeader*)(gws + G.header);
  const double r2 = radius * radius;
  if (K <= 8)
    hipLaunchKernelGGL(orient_knn_kernel<8>, dim3(kb), dim3(kThreads), 0, st, xyz, elig, sorted, start, header, M, K, r2, nbr);
  else
    hipLaunchKernelGGL(orient_knn_kernel<kMaxK>, dim3(kb), dim3(kThreads), 0, st, xyz, elig, sorted, start, header, M, K, r2, nbr);
  hipLaunchKernelGGL(orient_edges_kernel, dim3(blocks_for((size_t)M * K)), dim3(kThreads), 0, st, normals, nbr, M, K,
                     (int32_t*)(ws + L.eu), (int32_t*)(ws + L.ev), (unsigned long long*)(ws + L.ekey), ws + L.eflip, wbits_out, stats);
  NESTI_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

size_t nesti_orient_workspace_bytes(int M, int K) {
  if (M <= 0 || K < 1 || K > kMaxK) return 0;
  return orient_layout(M, K).total;
}

int nesti_orient_graph(const float* xyz_dev, int M, const float* normals_dev, double radius, int K, void* grid_ws_dev,
                       size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes, int32_t* nbr_out_dev, int32_t* edge_u_dev,
                       int32_t* edge_v_dev, uint32_t* edge_wbits_dev, uint8_t* edge_flip_dev, void* stream) {
  if (check_common("nesti_orient_graph", xyz_dev, M, normals_dev, radius, K, grid_ws_dev, grid_ws_bytes, ws_dev, ws_bytes)) return 1;
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  const OrientLayout L = orient_layout(M, K);
  if (build_graph(xyz_dev, M, normals_dev, radius, K, grid_ws_dev, grid_ws_bytes, ws, L, edge_wbits_dev, st)) return 1;
  const size_t mk = (size_t)M * K;
  if (nbr_out_dev) NESTI_CHECK_HIP(hipMemcpyAsync(nbr_out_dev, ws + L.nbr, mk * 4, hipMemcpyDeviceToDevice, st));
  if (edge_u_dev) NESTI_CHECK_HIP(hipMemcpyAsync(edge_u_dev, ws + L.eu, mk * 4, hipMemcpyDeviceToDevice, st));
  if (edge_v_dev) NESTI_CHECK_HIP(hipMemcpyAsync(edge_v_dev, ws + L.ev, mk * 4, hipMemcpyDeviceToDevice, st));
  if (edge_flip_dev) NESTI_CHECK_HIP(hipMemcpyAsync(edge_flip_dev, ws + L.eflip, mk, hipMemcpyDeviceToDevice, st));
  return 0;
}

int nesti_orient_normals(const float* xyz_dev, int M, float* normals_dev, int mode, double radius, int K, const double* viewpoint,
                         void* grid_ws_dev, size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes, uint8_t* tree_edge_out_dev,
                         nesti_orient_stats_t* stats_dev, void* stream) {
  const std::string w("nesti_orient_normals");
  if (mode != NESTI_ORIENT_MST && mode != NESTI_ORIENT_VIEWPOINT) NESTI_FAIL(w + ": unknown mode");
  if (mode == NESTI_ORIENT_VIEWPOINT && !viewpoint) NESTI_FAIL(w + ": NESTI_ORIENT_VIEWPOINT needs a viewpoint");
  View vw;
  memset(&vw, 0, sizeof(vw));
  if (viewpoint) {
    for (int c = 0; c < 3; ++c) {
      if (!std::isfinite(viewpoint[c])) NESTI_FAIL(w + ": the viewpoint must be finite");
      vw.v[c] = viewpoint[c];
    }
    vw.on = 1;
  }
  if (check_common(w, xyz_dev, M, normals_dev, radius, K, grid_ws_dev, grid_ws_bytes, ws_dev, ws_bytes)) return 1;
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)ws_dev;
  const OrientLayout L = orient_layout(M, K);
  int* stats = (int*)(ws + L.stats);
  const size_t mk = (size_t)M * K;
  const unsigned vb = blocks_for(M), eb = blocks_for(mk);
  if (tree_edge_out_dev) NESTI_CHECK_HIP(hipMemsetAsync(tree_edge_out_dev, 0, mk, st));
  if (mode == NESTI_ORIENT_VIEWPOINT) {
    NESTI_CHECK_HIP(hipMemsetAsync(stats, 0, kStatBytes, st));
    hipLaunchKernelGGL(orient_viewpoint_kernel, dim3(vb), dim3(kThreads), 0, st, xyz_dev, normals_dev, M, vw, stats);
  } else {
    if (build_graph(xyz_dev, M, normals_dev, radius, K, grid_ws_dev, grid_ws_bytes, ws, L, nullptr, st)) return 1;
    const int32_t* eu = (const int32_t*)(ws + L.eu);
    const int32_t* ev = (const int32_t*)(ws + L.ev);
    const unsigned long long* ekey = (const unsigned long long*)(ws + L.ekey);
    const unsigned char* elig = ws + L.elig;
    unsigned* uf = (unsigned*)(ws + L.uf);
    unsigned* comp = (unsigned*)(ws + L.comp);
    unsigned long long* best = (unsigned long long*)(ws + L.best);
    unsigned long long* rootkey = (unsigned long long*)(ws + L.rootkey);
    int32_t* rootidx = (int32_t*)(ws + L.rootidx);
    hipLaunchKernelGGL(orient_uf_init_kernel, dim3(vb), dim3(kThreads), 0, st, uf, M);
    // ceil(log2 M) + 1 rounds always suffice; in round r at most M >> r components hook, so the hooked chains are no deeper than
    // (M >> r) + 1 and ceil(log2) of that, plus one, pointer-jumping launches flatten them
    const int rounds = std::min(kMaxRounds, ceil_log2(M) + 1);
    for (int r = 0; r < rounds; ++r) {
      const int* prev = r ? stats + kStatRoundFlag + r - 1 : nullptr;
      int* flag = stats + kStatRoundFlag + r;
      hipLaunchKernelGGL(orient_round_reset_kernel, dim3(vb), dim3(kThreads), 0, st, uf, comp, best, M, prev);
      hipLaunchKernelGGL(orient_round_min_kernel, dim3(eb), dim3(kThreads), 0, st, eu, ev, ekey, comp, best, (unsigned)mk, prev);
      hipLaunchKernelGGL(orient_round_hook_kernel, dim3(vb), dim3(kThreads), 0, st, eu, ev, ws + L.eflip, comp, best, uf, M,
                         tree_edge_out_dev, prev, flag);
      const int jumps = ceil_log2(((long long)M >> r) + 2) + 1;
      for (int j = 0; j < jumps; ++j)
        hipLaunchKernelGGL(orient_round_jump_kernel, dim3(vb), dim3(kThreads), 0, st, uf, M, flag);
    }
    hipLaunchKernelGGL(orient_root_init_kernel, dim3(vb), dim3(kThreads), 0, st, rootkey, rootidx, M);
    hipLaunchKernelGGL(orient_root_kernel, dim3(vb), dim3(kThreads), 0, st, xyz_dev, elig, uf, M, vw, rootkey, rootidx, 0);
    hipLaunchKernelGGL(orient_root_kernel, dim3(vb), dim3(kThreads), 0, st, xyz_dev, elig, uf, M, vw, rootkey, rootidx, 1);
    hipLaunchKernelGGL(orient_rootflip_kernel, dim3(vb), dim3(kThreads), 0, st, xyz_dev, normals_dev, elig, uf, rootidx, M, vw, comp, stats);
    hipLaunchKernelGGL(orient_apply_kernel, dim3(vb), dim3(kThreads), 0, st, normals_dev, elig, uf, comp, M, stats);
  }
  NESTI_CHECK_HIP(hipGetLastError());
  if (stats_dev) NESTI_CHECK_HIP(hipMemcpyAsync(stats_dev, stats, sizeof(nesti_orient_stats_t), hipMemcpyDeviceToDevice, st));
  return 0;
}

}  // extern "C"
