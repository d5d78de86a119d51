// Device-side pieces of the multi-scale patch extraction (utils/pcpnet_dataset.py:286-343) shared by patches_kernel
// (patches.hip: materialises the patch tensors, the parity entry point) and patches_mups_kernel (mups.hip: feeds the
// selected neighbours straight into the MuPS sweep, the product path).  See patches.hip for the data structure.
#pragma once
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"

namespace nesti {
namespace {

constexpr int kMaxDim = 128;
constexpr int kMaxCells = kMaxDim * kMaxDim * kMaxDim;
constexpr int kPatchThreads = 256;
constexpr int kListCap = 1024;   // candidates kept for the final rank sort (>= 2P for P = 512)

struct GridHeader {
  double minv[3];
  double inv_cell;
  int dims[3];
  int ncells;
};

struct WsLayout {
  size_t header, bbox, count, start, cursor, sorted, total;
};
inline WsLayout patch_ws_layout(int N) {
  WsLayout L;
  size_t o = 0;
  L.header = o; o += 256;
  L.bbox = o; o += 256;
  L.count = o; o += align_up((size_t)(kMaxCells + 1) * 4, 256);
  L.start = o; o += align_up((size_t)(kMaxCells + 1) * 4, 256);
  L.cursor = o; o += align_up((size_t)(kMaxCells + 1) * 4, 256);
  L.sorted = o; o += align_up((size_t)N * 16, 256);
  L.total = o;
  return L;
}

// Cell of a coordinate, clamped to the grid IN DOUBLE before the integer conversion: a far-away coordinate gets a defined
// border cell instead of an undefined conversion.  For a cloud point the result is its cell.  A non-finite query centre never
// gets here: every kernel tests the BIT PATTERNS of the centre (centre_lost) and gives such a query empty spans -- mups.hip is
// built with -fno-honor-nans, under which neither fmax(NaN, 0) nor an ordered compare against NaN can be relied on.
// A query POSITION (PatchParams::query_xyz) may lie outside the bounding box: the cell edge is >= 1.0001 x the largest
// radius, so a centre whose true cell index is -1 or dims has its whole ball inside cells [-2, 0] resp. [dims - 1, dims + 1],
// of which only the border cell holds points, and the 3 x 3 x 3 block around the CLAMPED cell contains that border cell;
// a centre further out has an empty ball, which the distance test finds (no candidate passes it).
__device__ __forceinline__ int cell_axis(double v, double minv, double inv_cell, int dim) {
  return (int)fmin((double)(dim - 1), fmax(0.0, floor((v - minv) * inv_cell)));
}
__device__ __forceinline__ void cell_coords(const GridHeader& h, float x, float y, float z, int* ix, int* iy, int* iz) {
  *ix = cell_axis((double)x, h.minv[0], h.inv_cell, h.dims[0]);
  *iy = cell_axis((double)y, h.minv[1], h.inv_cell, h.dims[1]);
  *iz = cell_axis((double)z, h.minv[2], h.inv_cell, h.dims[2]);
}
__device__ __forceinline__ int cell_flat(const GridHeader& h, int ix, int iy, int iz) {
  return (iz * h.dims[1] + iy) * h.dims[0] + ix;   // x fastest: a row of cells is one contiguous span
}

// splitmix64 finaliser over (seed, query, scale, point): the documented subsample key
__device__ __forceinline__ unsigned subsample_hash(unsigned long long seed, unsigned q, unsigned s, unsigned idx) {
  unsigned long long z = seed ^ ((unsigned long long)q << 34) ^ ((unsigned long long)s << 32) ^ (unsigned long long)idx;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (unsigned)(z >> 32);
}

struct PatchParams {
  const float* cloud;
  const float4* sorted;
  const int* start;
  const GridHeader* header;
  const int32_t* query_idx;
  const float* query_xyz;          // [M,3] query POSITIONS (nesti_*_at): the centre is query_xyz[q], not a cloud point
  int M, N, S, P, row0;
  unsigned long long seed;
  double r2[NESTI_MAX_SCALES];     // r*r, like cKDTree's upper_bound for p = 2
  float rad_f[NESTI_MAX_SCALES];   // (float)r : torch divides the f32 patch by the scalar in f32
  float* points_out;
  int32_t* n_eff_out;
  int32_t* nbr_out;
  int32_t* n_ball_out;
};


// Shared-memory state of one query (one 256-thread workgroup)
struct PatchShared {
  int span_beg[9], span_end[9];
  int s_count[NESTI_MAX_SCALES];
  int s_cnt;
  unsigned long long keys[kListCap];
  int sel[kListCap];
};

// ---- the grid-neighbourhood walk the ball query kernels share -----------------------------------------------------------------
// centre -> 3 x 3 x 3 cell block as nine contiguous x-spans of the cell-ordered copy -> candidates streamed with a stride -> fp64
// d2 -> body.  Workgroup-per-query kernels (patch_select_scale, patches_ref_kernel) keep the spans in LDS and stride by the
// workgroup; the wave-per-row pca_kernel keeps span t in lane t and strides by the wave.  patch_query_setup and orient.hip's
// orient_knn_kernel keep the walk written out (profiles/refactor_isa_grid.txt: each measured slower through these functions).

// exponent all ones: +-inf or NaN, tested on the bits of a WAVE-UNIFORM value (a query centre: uniform per workgroup or per wave).
// The empty asm ties the word to a scalar register, which is only right for such a value, and makes it opaque: without it the
// compiler recognises the mask test as a floating-point class test of v and, under -fno-honor-nans, drops the NaN half of it
// (it became v_cmp_eq_f32 |v|, inf, which a NaN fails).  Per-lane values: finite_bits (common.h).
__device__ __forceinline__ bool non_finite_bits(float v) {
  unsigned u = __float_as_uint(v);
  asm volatile("" : "+s"(u));
  return (u & 0x7f800000u) == 0x7f800000u;
}
// a centre with an infinite or NaN coordinate has empty balls: it visits no cell, so no distance is ever formed from it
__device__ __forceinline__ bool centre_lost(float x, float y, float z) {
  return non_finite_bits(x) || non_finite_bits(y) || non_finite_bits(z);
}

// the centre of query q: a position, or the cloud point of a listed index or of row row0 + q ('full' sampler: patch row == point
// index); an index is clamped into the cloud
__device__ __forceinline__ const float* query_centre(const PatchParams& p, int q) {
  if (p.query_xyz) return p.query_xyz + (size_t)q * 3;        // uniform per launch; a position need not be in its own ball
  int qi = p.query_idx ? p.query_idx[q] : p.row0 + q;
  qi = min(max(qi, 0), p.N - 1);
  return p.cloud + (size_t)qi * 3;
}

// x-span t in [0, 9) of the cell block round the FINITE centre (x, y, z): rows (z, y) = (t / 3 - 1, t % 3 - 1) of the block, cells
// x - 1 .. x + 1 of each, as [b, e) in the cell-ordered copy of the N points; empty outside the grid.  Clamped into [0, N]: a span
// never leaves the cell-ordered copy, whatever a grid workspace that does not belong to the cloud holds.
struct Span {
  int b, e;
};
__device__ __forceinline__ Span block_span(const GridHeader& h, const int* start, int N, float x, float y, float z, int t) {
  int ix, iy, iz;
  cell_coords(h, x, y, z, &ix, &iy, &iz);
  const int zz = iz + t / 3 - 1, yy = iy + t % 3 - 1;
  Span s = {0, 0};
  if (zz >= 0 && zz < h.dims[2] && yy >= 0 && yy < h.dims[1]) {
    const int x0 = max(ix - 1, 0), x1 = min(ix + 1, h.dims[0] - 1);
    s.b = max(start[cell_flat(h, x0, yy, zz)], 0);
    s.e = min(start[cell_flat(h, x1, yy, zz) + 1], N);
  }
  return s;
}

// where a walk finds its nine spans: in LDS, or span t in lane t of the wave
struct LdsSpans {
  const int* b;
  const int* e;
  __device__ __forceinline__ Span operator[](int t) const { return {b[t], e[t]}; }
};
struct WaveSpans {
  int b, e;
  __device__ __forceinline__ Span operator[](int t) const { return {__shfl(b, t, 64), __shfl(e, t, 64)}; }
};

// The ball test's squared distance, (dx dx + dy dy) + dz dz in fp64 -- cKDTree's formula, in plain operators.
// WARNING for an includer: the bits depend on the contraction setting AT THE #include of this header.  patches.hip, mups.hip and
// pca.hip include it under the compiler's default, where hipcc forms d2 = fma(dz, dz, fma(dx, dx, dy dy)): cKDTree's value up to the
// two roundings the FMAs save, not bit for bit.  Included after `#pragma clang fp contract(off)` it would round all five operations.
// (__dmul_rn / __dadd_rn would not say more: they are inline functions of the HIP headers with plain operators inside, defined
// before any pragma of ours.)
__device__ __forceinline__ double ball_d2(double dx, double dy, double dz) {
  return (dx * dx + dy * dy) + dz * dz;
}

// body(candidate {x, y, z, index bits}, d2 to the centre) for candidates first, first + stride, ... of each of the nine spans.
// The candidate loop stays rolled and scalar: with its bounds in registers hipcc would otherwise unroll and vectorise it, eight
// times the code and, in the workgroup-per-query kernels, four times the registers for a loop of a few trips per lane.
template <class Spans, class Body>
__device__ __forceinline__ void walk_block(const float4* sorted, const Spans& spans, int first, int stride, double cx,
                                           double cy, double cz, Body&& body) {
  for (int sp = 0; sp < 9; ++sp) {
    const Span s = spans[sp];
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = s.b + first; i < s.e; i += stride) {
      const float4 c = sorted[i];
      body(c, ball_d2((double)c.x - cx, (double)c.y - cy, (double)c.z - cz));
    }
  }
}

// The query point, the 3 x 3 cell block as nine contiguous x-spans of the cell-ordered copy, and the ball sizes of every scale
// (pass A).  Ends with a barrier: sh.s_count[] is valid on return.  The spans and the candidate loop are written out here rather than
// through block_span and walk_block: with them patches_count_kernel, which is this function and little else, measured 2 % slower
// (profiles/refactor_isa_grid.txt); the spans are therefore not clamped here.
__device__ __forceinline__ void patch_query_setup(const PatchParams& p, PatchShared& sh, int q, int t, float (&cf)[3]) {
  const float* centre = query_centre(p, q);
  const GridHeader h = *p.header;
  cf[0] = centre[0]; cf[1] = centre[1]; cf[2] = centre[2];
  const double cx = cf[0], cy = cf[1], cz = cf[2];
  const bool lost = centre_lost(cf[0], cf[1], cf[2]);
  if (t < 9) {
    int b = 0, e = 0;
    if (!lost) {
      int ix, iy, iz;
      cell_coords(h, cf[0], cf[1], cf[2], &ix, &iy, &iz);
      const int zz = iz + t / 3 - 1, yy = iy + t % 3 - 1;
      if (zz >= 0 && zz < h.dims[2] && yy >= 0 && yy < h.dims[1]) {
        const int x0 = max(ix - 1, 0), x1 = min(ix + 1, h.dims[0] - 1);
        b = p.start[cell_flat(h, x0, yy, zz)];
        e = p.start[cell_flat(h, x1, yy, zz) + 1];
      }
    }
    sh.span_beg[t] = b;
    sh.span_end[t] = e;
  }
  if (t < NESTI_MAX_SCALES) sh.s_count[t] = 0;
  __syncthreads();
  // ---- pass A: ball sizes ------------------------------------------------------------------
  int local[NESTI_MAX_SCALES] = {0, 0, 0, 0};
  for (int sp = 0; sp < 9; ++sp) {
    for (int i = sh.span_beg[sp] + t; i < sh.span_end[sp]; i += kPatchThreads) {
      const float4 c = p.sorted[i];
      const double d2 = ball_d2((double)c.x - cx, (double)c.y - cy, (double)c.z - cz);
#pragma unroll
      for (int s = 0; s < NESTI_MAX_SCALES; ++s)
        if (s < p.S && d2 <= p.r2[s]) ++local[s];
    }
  }
#pragma unroll
  for (int s = 0; s < NESTI_MAX_SCALES; ++s)
    if (s < p.S && local[s]) atomicAdd(&sh.s_count[s], local[s]);
  __syncthreads();
}

// Scale s: the n_eff = min(ball, P) neighbours with the smallest (hash, index) keys, in key order, into sh.sel[]
// (pass B + rank sort).  Ends with a barrier: sh.sel[0 .. n_eff) is valid on return.  Returns n_eff.
__device__ __forceinline__ int patch_select_scale(const PatchParams& p, PatchShared& sh, int q, int t, int s, const float (&cf)[3]) {
  const int n_ball = sh.s_count[s];
  const int n_eff = min(n_ball, p.P);   // utils/pcpnet_dataset.py:310
  // ---- pass B: collect the hits whose key is <= T; T is bisected until P <= kept <= cap --
  unsigned lo = 0u, hi = 0xffffffffu, T = 0xffffffffu;
  if (n_ball > p.P) T = (unsigned)fmin(4294967295.0, 4294967296.0 * 1.25 * (double)p.P / (double)n_ball);
  int kept = 0;
  for (int iter = 0; iter < 40; ++iter) {
    __syncthreads();
    if (t == 0) sh.s_cnt = 0;
    __syncthreads();
    walk_block(p.sorted, LdsSpans{sh.span_beg, sh.span_end}, t, kPatchThreads, cf[0], cf[1], cf[2], [&](const float4& c, double d2) {
      if (d2 <= p.r2[s]) {
        const unsigned idx = (unsigned)__float_as_int(c.w);
        const unsigned hsh = subsample_hash(p.seed, (unsigned)(p.row0 + q), (unsigned)s, idx);
        if (hsh <= T) {
          const int pos = atomicAdd(&sh.s_cnt, 1);
          if (pos < kListCap) sh.keys[pos] = ((unsigned long long)hsh << 32) | idx;
        }
      }
    });
    __syncthreads();
    kept = sh.s_cnt;
    if (kept >= n_eff && kept <= kListCap) break;
    if (kept < n_eff) lo = T + 1u; else hi = T - 1u;
    T = lo + (hi - lo) / 2u;
  }
  kept = min(kept, kListCap);
  // ---- rank sort: position = number of smaller keys; keep the first n_eff -----------------
  for (int e = t; e < kept; e += kPatchThreads) {
    const unsigned long long my = sh.keys[e];
    int rank = 0;
    for (int j = 0; j < kept; ++j) rank += (sh.keys[j] < my) ? 1 : 0;
    if (rank < n_eff) sh.sel[rank] = (int)(unsigned)(my & 0xffffffffull);
  }
  __syncthreads();
  return n_eff;
}

// coordinate `axis` of neighbour idx relative to the query, scaled: (pts[idx] - pts[center]) / rad in f32 with IEEE
// subtraction and division (utils/pcpnet_dataset.py:330-343)
__device__ __forceinline__ float patch_coord(const PatchParams& p, int idx, int axis, float c, float rad) {
  return __fdiv_rn(__fsub_rn(p.cloud[(size_t)idx * 3 + axis], c), rad);
}

// host side: the view of the search grid inside its workspace (sorted, start, header); every entry that walks the grid fills it here
inline void patch_params_grid(PatchParams* p, int N, const void* grid_ws_dev) {
  const WsLayout L = patch_ws_layout(N);
  const unsigned char* ws = (const unsigned char*)grid_ws_dev;
  p->sorted = (const float4*)(ws + L.sorted);
  p->start = (const int*)(ws + L.start);
  p->header = (const GridHeader*)(ws + L.header);
}

// host side: fill the kernel parameter block from the C-ABI arguments (validated by the caller)
inline void patch_params_fill(PatchParams* p, const nesti_config_t* cfg, const float* cloud_dev, int N,
                              const int32_t* query_idx_dev, int M, const double* r_abs, uint64_t seed, int query_row0,
                              const void* grid_ws_dev) {
  memset(p, 0, sizeof(*p));
  patch_params_grid(p, N, grid_ws_dev);
  p->cloud = cloud_dev;
  p->query_idx = query_idx_dev;
  p->M = M; p->N = N; p->S = cfg->n_scales; p->P = cfg->points_per_scale; p->seed = seed; p->row0 = query_row0;
  for (int s = 0; s < cfg->n_scales; ++s) {
    p->r2[s] = r_abs[s] * r_abs[s];
    p->rad_f[s] = (float)r_abs[s];
  }
}

// host side: what every entry over a cloud and its grid workspace refuses first, under the entry's name `w`.  The radii come last
// and only where `radii_used`: an entry that returns early for M <= 0 "whatever the radii are" passes M > 0.  An infinite radius
// (one infinite coordinate makes the host's bounding-box diagonal infinite) would give header_kernel inv_cell = 0 and a NaN to convert.
inline int refuse_grid_cloud(const std::string& w, const nesti_config_t* cfg, const float* cloud_dev, int N, const double* r_abs,
                             const void* grid_ws_dev, size_t grid_ws_bytes, bool radii_used = true) {
  if (!cfg || !cloud_dev || !r_abs || !grid_ws_dev) NESTI_FAIL(w + ": null argument");
  if (N <= 0) NESTI_FAIL(w + ": empty cloud");
  if (cfg->n_scales < 1 || cfg->n_scales > NESTI_MAX_SCALES) NESTI_FAIL(w + ": bad n_scales");
  if (grid_ws_bytes < patch_ws_layout(N).total) NESTI_FAIL(w + ": grid workspace too small");
  for (int s = 0; radii_used && s < cfg->n_scales; ++s)
    if (!(r_abs[s] > 0.0) || !std::isfinite(r_abs[s])) NESTI_FAIL(w + ": radii must be positive and finite");
  return 0;
}
// ... and of its M queries.  rows_are_centres: the centres are the cloud rows [query_row0, query_row0 + M) -- no index list, no
// positions -- and must lie inside the cloud.  Listed indices live on the device: the host mirror (provider.CloudPatches) validates
// them once at upload and query_centre clamps, so a bad index yields a wrong patch, never an out-of-bounds read.  For positions
// query_row0 is only the subsample key's row; any position is served (cell_axis).
inline int refuse_query_rows(const std::string& w, int N, bool rows_are_centres, int M, int query_row0) {
  if (query_row0 < 0) NESTI_FAIL(w + ": query_row0 must be >= 0");
  if (rows_are_centres && M > 0 && (long long)query_row0 + M > (long long)N)
    NESTI_FAIL(w + ": query rows [query_row0, query_row0 + M) exceed the cloud (N points)");
  return 0;
}

}  // namespace
}  // namespace nesti
