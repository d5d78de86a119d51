// What the host-only units of libnesti_hip.so (graph.cpp, pack.cpp, plan.cpp) share with the HIP files: the error slot, the dtype
// predicates, the layout constants the weight packer and the planner share with the kernels, the counter and workspace words of the
// deciding kernels, and the kernels' parameter blocks (ConvParams, PoolParams).  No HIP header: common.h includes this file, so host
// and device code see the same definitions.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "../../include/nesti_hip.h"

namespace nesti {

void set_error(const std::string& msg);   // model.hip: the message nesti_last_error returns on this thread

#define NESTI_FAIL(msg)           \
  do {                            \
    ::nesti::set_error(msg);      \
    return 1;                     \
  } while (0)

static inline size_t dtype_size(int dt) { return dt == NESTI_F32 ? 4 : 2; }
// NESTI_BF16X3: the kernels are the bf16 ones with the pair K loop (conv.hip / conv8n.hip: X3); an activation row holds, per
// group of 64 channels, the two 64-element planes [hi | lo] (128 elements), a packed weight row [W_hi | W_lo] per K chunk,
// and one set of fragment reads feeds hi*W_hi + lo*W_hi + hi*W_lo.  Writers emit the planes (common.h: split_col / split_pack2).
// NESTI_F16X3: the same with f16 pairs and the f16 kernels.
// NESTI_F16X3C is NESTI_F16X3 everywhere except in the gating net's first pass (model.hip: gate_cascade)
static inline int main_dtype(int dt) { return (dt == NESTI_F16X3C || dt == NESTI_F16X8 || dt == NESTI_F16X8C) ? NESTI_F16X3 : dt; }
static inline bool dtype_cascade(int dt) { return dt == NESTI_F16X3C || dt == NESTI_F16X8C; }
static inline bool dtype_x8(int dt) { return dt == NESTI_F16X8 || dt == NESTI_F16X8C; }
static inline int kernel_dtype(int dt) { return dt == NESTI_BF16X3 ? NESTI_BF16 : dt == NESTI_F16X3 ? NESTI_F16 : dt; }
constexpr int kPairPlanes = 2;    // hi, lo
static inline int act_planes(int dt) { return (dt == NESTI_BF16X3 || dt == NESTI_F16X3) ? kPairPlanes : 1; }
constexpr int kSplitGroup = 64;
constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr int kRowBytes = 128;    // bytes of one K-chunk row in LDS (64 x 16-bit or 32 x f32)
constexpr int kTileM = 512;       // GEMM rows (voxels x points) per workgroup
constexpr int kMaxTaps = 125;     // 5^3

// ---- the words the deciding kernels (decide.hip) share with their host readers (model.hip) and the planner (plan.cpp) ------------
#ifdef __HIP__
#define NESTI_HD __host__ __device__
#else
#define NESTI_HD
#endif
// A model's counter blocks: 64 bytes = eight 64-bit words each (include/nesti_hip.h: nesti_cascade_stats_t, nesti_x8_guard_stats_t,
// nesti_reproducible_stats_t).  cstat, the two-stage gate: queries; rechecked (rows decided by the f16x3 gate, widening rounds
// included); changed; the bits of max_margin_err; a double, the sum of the squared pair errors; the number of pairs in that sum; rows
// rechecked by a widening round; forward calls whose widening round was not empty
enum CStat { kCQueries, kCRechecked, kCChanged, kCMaxErrBits, kCSumSq, kCPairs, kCWidened, kCWidenEvents };
// cstat2, recheck stage 2 of NESTI_F16X8C (the gating net with its 8^3 tap layers in the FP6 form; decide.hip): rows that went through
// it; rows it decided; rows it passed on to stage 3, the f16x3 gate (the residual); the bits of its largest error on a logit
// difference, measured on the rows both stages decided; the sum of those errors squared and their number; rows the call's widening
// round passed on to stage 3 afterwards; rows that round could not hold
enum C2Stat { kC2Rows, kC2Decided, kC2Residual, kC2MaxErrBits, kC2SumSq, kC2Pairs, kC2Widened, kC2Dropped };
// gstat, the conditioning guard: queries; rows re-evaluated; the bits of the largest |dn|; rows dropped because a list was full
enum GStat { kGQueries, kGRechecked, kGMaxDnBits, kGDropped };
// rstat, the reproducible mode: rows whose error would have widened the gate's margin / the guard's band
enum RStat { kRGateViolations, kRGuardViolations };
// a float >= 0 kept as its bits in a counter word (it orders like its bit pattern, so atomicMax keeps the largest)
NESTI_HD inline float counter_float(unsigned long long word) {
  const uint32_t bits = (uint32_t)word;
  float f;
  __builtin_memcpy(&f, &bits, 4);
  return f;
}
// the threshold of a forward call of the two-stage gate (decide.hip: gate_begin_kernel; nesti_model_cascade_stats reports it)
NESTI_HD inline float gate_tau_eff(float tau, float widen, float max_margin_err) { return fmaxf(tau, widen * max_margin_err); }
// the conditioning guard's widen / theta, theta = sqrt(2 x bar): scale x |dn| is the |n| below which an output may tilt by more than the bar
inline float x8_guard_scale() { return NESTI_X8_GUARD_WIDEN / sqrtf(2.f * NESTI_X8_GUARD_BAR); }

// fcounts, a block of the call's workspace (plan.cpp: ws_layout), as int32 words:
//   [0] rows flagged by the filter pass, [kRoundCountsOff + r] of them in recheck round r (cap rows per round),
//   [kTauEffOff] the call's threshold tau_eff as a float (raised to the upper end of every band a widening pass has covered),
//   [kWidenUpperOff] the upper end of the current widening pass's band (float, snapshotted when the pass starts),
//   [kWidenCountOff] rows flagged by the current widening pass, [kWidenRoundsOff + r] of them in its tower round r
//   recheck stage 2: [kResCountOff] rows of the current residual list, [kTau2EffOff] the call's second threshold tau2_eff (float),
//   [kTau2UpperOff] the upper end of the band of the stage's widening round (float), [kRound2Off + r] the flagged rows in the stage's
//   round r (plan.h: Stage2Plan::cap rows per round)
constexpr int kFcountsBytes = 512;
constexpr int kMaxCascadeRounds = 24;
constexpr int kRoundCountsOff = 8, kTauEffOff = 40, kWidenUpperOff = 41, kWidenCountOff = 48, kWidenRoundsOff = 56;
constexpr int kResCountOff = 80, kTau2EffOff = 81, kTau2UpperOff = 82, kRound2Off = 88;
static_assert(kWidenRoundsOff + kMaxCascadeRounds <= kResCountOff && kTau2UpperOff < kRound2Off &&
              (kRound2Off + kMaxCascadeRounds) * 4 <= kFcountsBytes, "fcounts layout: stage 2");
static_assert(kRoundCountsOff + kMaxCascadeRounds <= kTauEffOff && (kWidenRoundsOff + kMaxCascadeRounds) * 4 <= kFcountsBytes, "fcounts layout");
// ecounts, the next block, as int32 words: [e * rounds + r] rows of expert e's round r from word 0 (plan.h: they end before the
// guard's words), [kGuardCountOff + e] the length of the guard's list for expert e, [kGuardSlotOff], [+ 1] the |n| band (floats)
constexpr int kEcountsBytes = 1024;
constexpr int kGuardCountOff = 128, kGuardSlotOff = 140;
static_assert(kGuardCountOff + NESTI_MAX_EXPERTS <= kGuardSlotOff && (kGuardSlotOff + 2) * 4 <= kEcountsBytes, "ecounts layout");

// host-side conversions used by the weight repacker (pack.cpp)
uint16_t host_f32_to_bf16(float f);
uint16_t host_f32_to_f16(float f);
float host_f16_to_f32(uint16_t h);

// ---- the parameter blocks of the conv and pool kernels: filled by the planner (plan.cpp), launched through kernels.h ------------
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
                       // input row -- 128, or 256 when a plain-f16 layer reads the hi planes of a pair-layout tensor (plan.cpp)
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

}  // namespace nesti
