// Kernel parameter blocks and launchers shared between the .hip files and the
// host-side graph executor (model.hip).  kRowBytes and kMaxTaps, which the weight packer shares, are host.h's.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace nesti {

constexpr int kTileM = 512;       // GEMM rows (voxels x points) per workgroup
constexpr unsigned kWalkGrid = 1024;   // workgroups of a walking launch (ConvParams::walk): a multiple of 8, so a workgroup's tiles stay
                                       // on its XCD (tile & 7 == blockIdx.x & 7); four per CU, enough to run a non-empty round

// One conv3d / fully-connected layer as an implicit GEMM:
//   out[r, n] = act( sum_{tap, c} in[shift(r, tap), c] * W[tap, c, n] + bias[n] )
// rows r = point * V + voxel (V = S^3, channels-last); a tap that leaves the S^3 volume
// contributes zero (TF 'SAME', utils/tf_util.py:298-300).
struct ConvParams {
  const void* in;      // [points * V, in_cstride] elements of the model dtype
  void* out;           // [points * V, out_cstride] (model dtype, or f32 if out_f32)
  const void* wpk;     // packed weights [n_tiles][n_chunks][n_taps][TN][128 B] (pre-swizzled)
  const float* bias;   // [n_tiles * TN] BN-folded bias
  const int32_t* npoints_ptr;   // optional device-side point count (top-1 routing); NULL -> npoints
  const int32_t* point_index;   // optional gather of INPUT points (routing); NULL -> identity
  int npoints;         // capacity (grid is sized for this)
  int in_cstride, in_coff;
  int in_chunk_bytes;  // plain (non-pair) K loop of conv_igemm_kernel: byte distance between consecutive 128-byte K chunks of an
                       // input row -- 128, or 256 when a plain-f16 layer reads the hi planes of a pair-layout tensor (model.hip)
  int in_pair;         // plain K loop of conv8n_kernel / conv4n_kernel: 1 = the input tensor has the pair layout and only its hi planes
                       // are read (64-byte chunk c = 32 channels sits at byte (c >> 1) * 256 + (c & 1) * 64 of a row); with
                       // `split` the outputs are written as pairs again -- a single-product layer inside a pair-mode tower
  int out_cstride, out_coff;
  int n_chunks, n_taps;
  int tap_k;           // kernel edge k when all k^3 taps are present in x-fastest order (conv4n_kernel derives the taps from counters)
  int log2S;           // S in {1,2,4,8}: the index space rows are laid out in
  int s_real;          // 0, or the real volume edge when it is smaller than S (3^3 Gaussian grid embedded in 4^3:
                       // voxels with a coordinate >= s_real are dead rows -- never read as neighbours, contents ignored)
  int relu, out_f32;
  int m_tiles, n_tiles;
  // merged inception conv1|conv4 launch: column tiles >= split_tile are conv4's; they write at
  // out_coff2 and average the pre-activation over the pool_k^3 SAME window (pool_k == 1: plain).
  int split_tile;      // == n_tiles for an ordinary layer
  int out_coff2;
  int pool_k;
  // fused tf.nn.max_pool3d 2^3 stride 2 (utils/tf_util.py:424-428) for the FIRST tile group: 1 = write only the pooled
  // tensor, 2 = write the full-resolution tensor and the pooled one
  void* mp_out;        // [points * V/8, mp_cstride], same channel offsets as `out`
  int mp_cstride;
  int mp_mode;
  int mp_mode2;        // 1: the conv4 half (fused avg-pool epilogue) writes ONLY its 2^3 / 2 max-pooled tensor, into mp_out at
                       // out_coff2 -- the block is followed by max_pool3d and nobody reads conv4 at full resolution
  // k^3-tap layers: 1 = the 16 32-row MFMA tiles of a workgroup are (8x,2y,2z) blocks (8^3) / x-lines of the
  // 8 points (4^3), dealt to the 4 SIMDs as a Latin square so that the tiles a padding tap skips are spread evenly
  // over the matrix pipes (conv.hip: tile_row).  0 = tile t holds rows [32t, 32t+32).  2 (2^3 volumes) = a tile is ONE voxel of
  // 32 points and the chunk sits in LDS in (voxel, point) order: padding skips whole tiles in all three axes.
  int remap;
  // A launch that is probably EMPTY (a later round of a routing / flag list walk, a widening pass of the two-stage gate: the row
  // count sits in device memory) is made with a small fixed grid whose workgroups WALK the tiles (tile = blockIdx.x, += gridDim.x,
  // bounded by the live row count): an empty launch then costs a few hundred workgroups instead of one per tile of the capacity
  // (a full-capacity grid of early-exiting workgroups costs ~1.1 ns each: 0.11 ms for 100k).  0 = one tile per workgroup; 1 = kWalkGrid
  // workgroups; > 1 = that many (a multiple of 8): the conditioning guard's towers see a few dozen rows and use 64.
  int walk;
  // NESTI_BF16X3 / NESTI_F16X3 (common.h): in_cstride / in_coff / out_cstride / mp_cstride and n_chunks are PHYSICAL (two planes per
  // 64-channel group); out_coff / out_coff2 stay logical and every 16-bit store goes through split_col + two planes.
  int split;
  int x2;              // 1x1x1 / FC layers of the NESTI_F16X3C filter pass (conv_igemm_kernel, KPIPE): PLAIN 16-bit activations times the
                       // pair-packed weights [W_hi | W_lo] -- hi * W_hi + hi * W_lo, i.e. the layer multiplies by its exact weights.  K chunks
                       // of 32 channels: 64-byte A rows, 128-byte B rows; n_chunks / acc_scale / wpk are the pair packing's.  These layers
                       // are fill-bound, so the second product is nearly free, and it removes the weight-rounding half of the filter's error
  int x3native;        // pair modes: the kernels' pair K loop (conv.hip / conv8n.hip: X3) -- K chunks [hi | lo] x [W_hi | W_lo], three MFMAs
                       // per fragment set; the packed weights follow (pack.h: PackMeta::x3n)
  // FP8 cross terms (NESTI_F16X8 / NESTI_F16X8C; conv8n.hip X8).  Producer side (a 1x1x1 layer, conv.hip): aux8_out != NULL makes the
  // FIRST tile group (conv1) also write the e4m3 planes of its activated outputs v = hi + lo into the side buffer -- per row and
  // 64-channel group [lo8 64 B | hi8 64 B] with lo8 = e4m3(lo 2^x8_sa), hi8 = e4m3(v 2^x8_sc), saturated at +-448; aux8_stride = bytes
  // per row.  Consumer side (conv8n_kernel): x8 = 1, aux8_in = that buffer, x8_scale_a / x8_scale_b = the E8M0 codes (127 - sa,
  // 127 - sb) of the block scales that undo the pre-scales of the activation and weight planes
  const void* aux8_in;
  void* aux8_out;
  int aux8_stride;
  int x8, x8_sa, x8_sc, x8_scale_a, x8_scale_b;
  // x8_fmt == 6: the block-scaled FP6 (e2m3) form of the same cross terms (conv8n.hip X6).  The side buffer keeps its geometry; the 32
  // bytes of a row's 16-channel chunk (16 where lo8 went, 16 where hi8 went) now hold 32 six-bit elements -- slot 2i = e2m3(lo_i 2^11 / s),
  // slot 2i + 1 = e2m3(hi_i / s) -- then the block's own scale s = 2^(E - 2), E = exponent of the chunk's largest |hi|, as an E8M0 byte
  // (byte 24), zeros after it; |lo_i 2^11| <= |hi_i| element by element, so one scale serves both halves.  The weight rows follow the
  // same pattern (pack.cpp: cross_rows, the 2^-11 folded into their scale byte); x8_sa / x8_sc / x8_scale_* are not used.
  int x8_fmt;
  float acc_scale;     // the accumulators are multiplied by this before the bias (1, or 2^-s when the layer's packed weights
                       // carry a 2^s scale: NESTI_F16X3 keeps the weight pairs in f16's normal range that way)
  int8_t tap[kMaxTaps][4];   // dz, dy, dx, -
};

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

struct PoolParams {
  const void* in;
  void* out;
  const int32_t* npoints_ptr;
  int npoints;
  int in_cstride, in_coff, out_cstride, out_coff;
  int C;               // channels to process (multiple of 8)
  int log2S;           // input S
  int split;           // pair modes: cstrides physical, in_coff / out_coff / C logical (split_col), values = hi + lo
};
int launch_maxpool2(const PoolParams& p, int dtype, hipStream_t stream);
// tf.nn.max_pool3d [3,3,3] stride 2 SAME on a 3^3 volume (models/experts_n_est.py:238): input rows in the 4^3-embedded
// layout (log2S = 2), output 2^3 (8 rows per point); output cell o covers input {o, o+1} per axis.
int launch_maxpool3s2(const PoolParams& p, int dtype, hipStream_t stream);

// softmax over the first E logits of each row + first-index arg-max
// (models/experts_n_est.py:177, test_n_est_w_experts.py:150); optional routing lists.
int launch_gate_finish(const float* logits, int lstride, int B, int E, float* probs,
                       int32_t* expert, int32_t* counts /*[E] or NULL*/,
                       int32_t* lists /*[E][B] or NULL*/, hipStream_t stream);
// NESTI_F16X3C, the two-stage gate (pool.hip): keep [B, NESTI_MAX_EXPERTS] f32 (the f16 pass's logits), flag_list [B],
// cstat = the model's device counters, fcounts = a 512-byte block of the call's workspace laid out as int32 words:
//   [0] rows flagged by the filter pass, [kRoundCountsOff + r] of them in recheck round r (cap rows per round),
//   [kTauEffOff] the call's threshold tau_eff as a float (raised to the upper end of every band a widening pass has covered),
//   [kWidenUpperOff] the upper end of the current widening pass's band (float, snapshotted when the pass starts),
//   [kWidenCountOff] rows flagged by the current widening pass, [kWidenRoundsOff + r] of them in its tower round r
constexpr int kMaxCascadeRounds = 24;
constexpr int kRoundCountsOff = 8, kTauEffOff = 40, kWidenUpperOff = 41, kWidenCountOff = 48, kWidenRoundsOff = 56;
static_assert(kRoundCountsOff + kMaxCascadeRounds <= kTauEffOff && kWidenRoundsOff + kMaxCascadeRounds <= 128, "fcounts layout");
int launch_gate_flag(const float* logits, int lstride, int B, int E, float tau, float widen, float* probs, int32_t* expert,
                     float* keep, int32_t* fcounts, int32_t* flag_list, int cap, int n_rounds, unsigned long long* cstat,
                     const unsigned long long* rstat, hipStream_t stream);
// after the recheck rounds, one widening pass: snapshot upper = widen * max_margin_err, flag list (storage reused) of the rows
// in [tau_eff, upper), its round counts, then tau_eff = max(tau_eff, upper)
int launch_gate_widen(const float* keep, int B, int E, float widen, int32_t* fcounts, int32_t* flag_list, int cap, int n_rounds,
                      unsigned long long* cstat, hipStream_t stream);
// rstat = the counter block of the reproducible mode (nesti_model_set_reproducible: [0] gate_violations, [1] guard_violations), null
// in the default mode: with it the call's threshold is tau itself and gate_recheck counts the rows whose widen x error exceeds
// fcounts[kTauEffOff] instead of anything acting on them
int launch_gate_recheck(const float* logits, int lstride, const int32_t* flag_list, const int32_t* count_ptr, int cap, int E,
                        const float* keep, float* probs, int32_t* expert, unsigned long long* cstat, const int32_t* fcounts,
                        float widen, unsigned long long* rstat, hipStream_t stream);
// a float maximum kept as bits in one counter word (cstat[3] max_margin_err, gstat[2] max_dn) <-> a device float (multi-GPU: every
// rank works with the largest value any rank has measured, nesti_model_gate_error_export / _import and the _guard_ twins)
int launch_stat_max_export(const unsigned long long* word, float* dst, hipStream_t stream);
int launch_stat_max_import(unsigned long long* word, const float* src, int n, hipStream_t stream);
// out[i * n_rounds + r] = clamp(counts[i] - r * cap, 0, cap): the rows of list i that round r of a `cap`-row tower covers
int launch_round_counts(const int32_t* counts, int n_lists, int cap, int n_rounds, int32_t* out, hipStream_t stream);
// ms_sw_n_est's switch (models/ms_sw_n_est.py:80-82): noise = logits[b*lstride]; expert = noise < threshold ? 0 : 1;
// probs[b] = noise (one column); optional routing lists over the 2 towers.
int launch_switch_finish(const float* logits, int lstride, int B, float threshold, float* probs,
                         int32_t* expert, int32_t* counts /*[2] or NULL*/, int32_t* lists /*[2][B] or NULL*/,
                         hipStream_t stream);
// the conditioning guard of the FP8 cross-term experts (pool.hip): band of |n| for this pass, flag expert e's rows inside it, replace
// them by their f16x3 re-evaluation and measure |dn|
int launch_x8_guard_begin(int pass, float thr, float scale, int B, unsigned long long* gstat, float* slot,
                          const unsigned long long* rstat, hipStream_t stream);
int launch_x8_guard_flag(const int32_t* list, const int32_t* count_ptr, int count_cap, const float* normals, const float* slot,
                         int32_t* glist, int32_t* gcount, int cap, unsigned long long* gstat, hipStream_t stream);
int launch_x8_guard_fix(const float* src, int sstride, const int32_t* glist, const int32_t* gcount, int cap, float* normals,
                        unsigned long long* gstat, float thr, float scale, unsigned long long* rstat, hipStream_t stream);
// position queries: rows whose n_eff is 0 at every scale get the sentinel normal (0,0,0), expert -1, probs 0 (expert / probs may be NULL)
int launch_mask_empty_queries(const int32_t* n_eff, int M, int S, float* normals, int32_t* expert, float* probs, int E,
                              hipStream_t stream);
// build routing lists from a caller-supplied expert assignment
int launch_route(const int32_t* expert, int B, int E, int32_t* counts, int32_t* lists,
                 hipStream_t stream);
// out[index[j]*3 + c] = src[j*sstride + c] for j < *count (or count_cap when count_ptr NULL)
int launch_scatter3(const float* src, int sstride, const int32_t* index, const int32_t* count_ptr,
                    int count_cap, float* out, hipStream_t stream);

}  // namespace nesti
