// Batch-norm folding and weight repacking for the MFMA kernels (pack.h).  Host only: no HIP header, no HIP call; compiled as plain
// C++ by the same compiler as the HIP files, so the _Float16 conversions are the ones the kernels' tests were taken with.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <regex>

#include "pack.h"

namespace nesti {

// ------------------------------------------------------------------------------------------
// host number formats
// ------------------------------------------------------------------------------------------
uint16_t host_f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
uint16_t host_f32_to_f16(float f) {
  _Float16 h = (_Float16)f;   // clang host: IEEE RNE conversion
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}

float host_f16_to_f32(uint16_t b) {
  _Float16 h;
  memcpy(&h, &b, 2);
  return (float)h;
}

// OCP e4m3 (1-4-3, bias 7, no infinities, largest finite 448) of a float, round to nearest even, saturating; subnormals kept
static uint8_t host_f32_to_e4m3(float f) {
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  float a = fabsf(f);
  if (!(a == a)) return 0x7f;
  a = std::min(a, 448.f);
  if (a == 0.f) return sign;
  int e;
  (void)frexpf(a, &e);                       // a = m 2^e, m in [0.5, 1)
  e = std::max(e - 1, -6);                   // exponent of the leading bit, not below the smallest normal's
  const float quantum = ldexpf(1.f, e - 3);
  float q = nearbyintf(a / quantum);         // default rounding mode: to nearest, ties to even
  float v = q * quantum;
  if (v == 0.f) return sign;
  if (v < ldexpf(1.f, -6)) return (uint8_t)(sign | (uint8_t)nearbyintf(v / ldexpf(1.f, -9)));   // subnormal: exponent field 0
  int e2;
  (void)frexpf(v, &e2);
  e2 -= 1;
  const int mant = (int)nearbyintf(v / ldexpf(1.f, e2 - 3)) - 8;
  return (uint8_t)(sign | ((e2 + 7) << 3) | mant);
}

// e2m3 (1-2-3, bias 1, largest finite 7.5) code of a non-negative magnitude already divided by its block scale: round to nearest even,
// saturating.  The code is monotone in the value and the grid is piecewise uniform: [0, 1) step 1/8 (subnormals), [1, 2) 1/8, [2, 4) 1/4,
// [4, 7.5] 1/2; a value that rounds up to the next binade's first point gets that point's code.
static uint8_t host_mag_to_e2m3(float a) {
  if (!(a == a)) return 31;
  int code;
  if (a < 2.f) code = (int)nearbyintf(a * 8.f);                    // 0 .. 16 (16 = 2.0)
  else if (a < 4.f) code = 16 + (int)nearbyintf((a - 2.f) * 4.f);    // .. 24 (= 4.0)
  else code = 24 + (int)nearbyintf((std::min(a, 8.f) - 4.f) * 2.f);
  return (uint8_t)std::min(code, 31);
}
static uint8_t host_f32_to_e2m3(float f, float inv_scale) {
  return (uint8_t)(host_mag_to_e2m3(fabsf(f) * inv_scale) | (std::signbit(f) ? 32 : 0));
}

// ------------------------------------------------------------------------------------------
// TF tensors of a layer, batch-norm folding
// ------------------------------------------------------------------------------------------
static bool shape_is(const nesti_tensor_t* t, std::initializer_list<int64_t> dims) {
  if (!t || !t->data || t->ndim != (int)dims.size()) return false;
  int i = 0;
  for (int64_t d : dims) if (t->dims[i++] != d) return false;
  return true;
}

void layer_tensors(const LayerDesc& d, std::vector<std::pair<std::string, std::vector<int64_t>>>* out) {
  for (const std::string* sc : {&d.scope, &d.scope2}) {
    if (sc->empty()) continue;
    if (d.is_fc) out->push_back({*sc + "/weights", {d.cin, d.cout}});
    else out->push_back({*sc + "/weights", {d.k, d.k, d.k, d.cin, d.cout}});
    out->push_back({*sc + "/biases", {d.cout}});
    if (d.bn) {
      for (const char* n : {"beta", "gamma", "mean", "var"}) out->push_back({*sc + "/bn/" + n, {d.cout}});
    }
  }
}

// BN-folded weights/bias of one TF layer (utils/tf_util.py:298-311, 491-494)
struct Folded {
  const float* w = nullptr;        // [taps][cin][cout]
  std::vector<float> scale, bias;  // per real output channel
};
static int fold_layer(const LayerDesc& d, const std::string& scope, const TensorTable& tt, Folded* f) {
  const nesti_tensor_t* w = tt.get(scope + "/weights");
  const nesti_tensor_t* b = tt.get(scope + "/biases");
  const bool wok = d.is_fc ? shape_is(w, {d.cin, d.cout}) : shape_is(w, {d.k, d.k, d.k, d.cin, d.cout});
  if (!wok) NESTI_FAIL("missing or mis-shaped tensor " + scope + "/weights");
  if (!shape_is(b, {d.cout})) NESTI_FAIL("missing or mis-shaped tensor " + scope + "/biases");
  f->w = w->data;
  f->scale.assign(d.cout, 1.0f);
  f->bias.resize(d.cout);
  for (int n = 0; n < d.cout; ++n) f->bias[n] = b->data[n];
  if (d.bn) {
    const nesti_tensor_t* beta = tt.get(scope + "/bn/beta");
    const nesti_tensor_t* gamma = tt.get(scope + "/bn/gamma");
    const nesti_tensor_t* mean = tt.get(scope + "/bn/mean");
    const nesti_tensor_t* var = tt.get(scope + "/bn/var");
    if (!shape_is(beta, {d.cout}) || !shape_is(gamma, {d.cout}) || !shape_is(mean, {d.cout}) || !shape_is(var, {d.cout}))
      NESTI_FAIL("missing or mis-shaped batch-norm tensors under " + scope + "/bn/");
    for (int n = 0; n < d.cout; ++n) {
      // tf.nn.batch_normalization(x, mean, var, beta, gamma, 1e-3)  (utils/tf_util.py:494)
      const double inv = (double)gamma->data[n] / sqrt((double)var->data[n] + 1e-3);
      f->scale[n] = (float)inv;
      f->bias[n] = (float)(((double)b->data[n] - (double)mean->data[n]) * inv + (double)beta->data[n]);
    }
  }
  return 0;
}

bool use_conv8(const LayerDesc& d) {
  if (d.is_fc || d.log2S != 3 || d.s_real || !d.scope2.empty()) return false;
  return d.k == 5 || d.k == 3;
}
// ... and on conv4n_kernel (conv4n.hip): the k^3 taps (k = 2 .. 5) on the 4^3 volume (not the 3^3 grid embedded in 4^3)
static bool use_conv4(const LayerDesc& d, int dtype) {
  if (d.is_fc || d.log2S != 2 || d.s_real || !d.scope2.empty() || d.k < 2 || d.k > 5) return false;
  return act_planes(dtype) == 1 || !(d.k & 1);   // pair modes: the even kernels only (conv4n.hip: launch_conv4n_dt)
}
int layer_kind(const LayerDesc& d, int dtype) { return use_conv8(d) ? 2 : use_conv4(d, dtype) ? 3 : 0; }

// ------------------------------------------------------------------------------------------
// the packer's steps, each written once
// ------------------------------------------------------------------------------------------
namespace {

// The taps of a layer in x-fastest order (TF SAME, stride 1), without those that never land inside the volume: their offsets
// (PackMeta::tap, n_taps) and, per tap, the index of its [cin][cout] slab in the TF weight tensor (widx).  At 8^3 with k <= 5 every
// tap lands inside (|offset| <= 2 < 8), so the X8 / X6 form gets all k^3 of them.  layer_taps is the list's length.
int tap_list(const LayerDesc& d, PackMeta* pm, int* widx /*[kMaxTaps]*/) {
  if (d.k < 1 || d.k * d.k * d.k > kMaxTaps) NESTI_FAIL("internal: kernel edge outside 1 .. 5");
  const int S = d.s_real ? d.s_real : (1 << d.log2S), lo = (d.k - 1) / 2;
  pm->n_taps = 0;
  for (int a = 0; a < d.k; ++a)
    for (int bb = 0; bb < d.k; ++bb)
      for (int c = 0; c < d.k; ++c) {
        const int dz = a - lo, dy = bb - lo, dx = c - lo;
        if (abs(dz) >= S || abs(dy) >= S || abs(dx) >= S) continue;
        int8_t* tp = pm->tap[pm->n_taps];
        tp[0] = (int8_t)dz; tp[1] = (int8_t)dy; tp[2] = (int8_t)dx; tp[3] = 0;
        widx[pm->n_taps++] = (a * d.k + bb) * d.k + c;
      }
  return 0;
}

// NESTI_F16X3: one power-of-two scale per layer (over its one or two fused parts) brings the largest folded weight into
// [2^13, 2^14), so that the lo halves of the weight pairs (2^-12 of a weight) are normal f16 numbers; the epilogue multiplies the
// accumulators by 2^-e (exact).  Returns e.
int pair_scale_exponent(const LayerDesc& d, const Folded* parts, int n_parts, const int* widx, int n_taps) {
  float wmax = 0.f;
  for (int part = 0; part < n_parts; ++part) {
    const Folded& f = parts[part];
    for (int t = 0; t < n_taps; ++t) {
      const float* wt = f.w + (size_t)widx[t] * d.cin * d.cout;
      for (int c = 0; c < d.cin; ++c)
        for (int n = 0; n < d.cout; ++n) wmax = std::max(wmax, fabsf(wt[(size_t)c * d.cout + n] * f.scale[n]));
    }
  }
  int e = 0;
  if (wmax > 0.f && std::isfinite(wmax)) {
    (void)frexpf(wmax, &e);                  // wmax = m 2^e, m in [0.5, 1)
    e = std::min(24, std::max(-8, 14 - e));
  }
  return e;
}

// Byte offset, inside a weight tile, of 16-byte slot `slot` of row `row`: the kernels' LDS image, XOR-swizzled per kernel family
// (PackMeta::kind) -- conv_igemm_kernel: 128-byte rows, key (row >> 1) & 7; conv8n_kernel: 64-byte rows, key (row >> 2) & 3;
// conv4n_kernel: 64-byte rows, key {0, 2, 3, 1}[(row >> 2) & 3]
size_t weight_slot(int kind, int row, int slot) {
  if (kind == 0) return (size_t)row * kRowBytes + ((slot ^ ((row >> 1) & 7)) << 4);
  const int key = kind == 3 ? (0x78 >> (2 * ((row >> 2) & 3))) & 3 : (row >> 2) & 3;
  return (size_t)row * 64 + ((slot ^ key) << 4);
}

// The hi / lo split of a scaled weight in f16 or bf16: hi = round16(v), lo = round16(v - widen16(hi)) (v - hi is exact in fp32)
uint16_t round16(float v, bool b16) { return b16 ? host_f32_to_bf16(v) : host_f32_to_f16(v); }
float widen16(uint16_t h, bool b16) {
  if (!b16) return host_f16_to_f32(h);
  const uint32_t hb = (uint32_t)h << 16;
  float hf;
  memcpy(&hf, &hb, 4);
  return hf;
}

}  // namespace

int layer_taps(const LayerDesc& d) {
  PackMeta pm;
  int widx[kMaxTaps];
  return tap_list(d, &pm, widx) ? 0 : pm.n_taps;
}

// Error attribution in the pair modes (scripts/exp_attribution.py), ONLY in builds made with -DNESTI_ATTRIBUTION (the product
// library has no such switch): NESTI_X3_PLAIN = "regex,regex,..." -- a layer whose scope matches drops the hi * W_lo product
// (its W_lo weights are packed as zeros: the layer then sees its weights rounded to 16 bits).  Round 3's full sweep
// (profiles/r03_attribution_sweep.txt) also switched off lo * W_hi per layer; that needed the three-plane layout
// [hi | lo | hi] x [W_hi ; W_hi ; W_lo] of commit 6f246d7 and is not available in the two-plane layout.
#ifdef NESTI_ATTRIBUTION
static int x3_drop_mask(const LayerDesc& d) {
  const char* e = getenv("NESTI_X3_PLAIN");
  if (!e || !*e) return 0;
  std::string spec(e);
  size_t pos = 0;
  while (pos <= spec.size()) {
    size_t end = spec.find(',', pos);
    if (end == std::string::npos) end = spec.size();
    const std::string item = spec.substr(pos, end - pos);
    pos = end + 1;
    if (item.empty()) continue;
    try {
      const std::regex re(item);
      if (std::regex_search(d.scope, re) || (!d.scope2.empty() && std::regex_search(d.scope2, re))) {
        fprintf(stderr, "libnesti_hip (attribution build): layer %s packed WITHOUT its W_lo plane\n", d.scope.c_str());
        return 2;
      }
    } catch (const std::regex_error&) {
      fprintf(stderr, "libnesti_hip (attribution build): bad regex '%s' in NESTI_X3_PLAIN\n", item.c_str());
    }
  }
  return 0;
}
#else
static inline int x3_drop_mask(const LayerDesc&) { return 0; }
#endif

int x8_activation_exponent(const LayerDesc& d, const TensorTable& tt) {
  // A data-free bound from the layer's own batch-norm: hi8 = e4m3(v 2^sc) must stay below the format's 448.  After
  // tf.nn.batch_normalization the pre-activation of channel n is beta_n + gamma_n z with z ~ N(0, 1) on the data the statistics were
  // taken from, so |v| <= |beta_n| + 8 |gamma_n| but for 8-sigma events; 2^sc brings that bound into (128, 256].  A larger value
  // saturates and loses only its own cross terms.
  float amax = 16.f;
  const nesti_tensor_t* beta = tt.get(d.scope + "/bn/beta");
  const nesti_tensor_t* gamma = tt.get(d.scope + "/bn/gamma");
  if (d.bn && beta && gamma && beta->data && gamma->data) {
    amax = 0.f;
    for (int n = 0; n < d.cout; ++n) amax = std::max(amax, fabsf(beta->data[n]) + 8.f * fabsf(gamma->data[n]));
  }
  if (!(amax > 0.f) || !std::isfinite(amax)) amax = 16.f;
  int e;
  (void)frexpf(amax, &e);                        // amax = m 2^e, m in [0.5, 1): amax <= 2^e
  return std::min(20, std::max(-8, 8 - e));
}

// ------------------------------------------------------------------------------------------
// the packer
// ------------------------------------------------------------------------------------------
// The cross-term half of the X8 / X6 rows of one tile (conv8n.hip X8 / X6; NESTI_F16X8 / NESTI_F16X8C): such a row is the pair row
// [W_hi f16 k0..15 | W_lo f16 k0..15] of a k^3 tap layer at 8^3 with, where W_lo went, narrow codes of BOTH halves of the same scaled
// weights (W 2^e, |W| 2^e < 2^14); whi / wlo = W_hi and W - W_hi of the tile's 16 channels x 64 columns, zero on padding.
// fmt == 8: [W_hi8 k0..15 | W_lo8 k0..15], W_hi8 = e4m3(W_hi 2^sb), W_lo8 = e4m3((W - W_hi) 2^(sb + 11)) with sb = -6 (both below 256).
// fmt == 6: the block-scaled FP6 form (host.h: ConvParams::x8_fmt): the same 32 bytes hold 32 e2m3 elements -- slot 2i = W_hi[i] / s,
// slot 2i + 1 = W_lo[i] 2^11 / s of the chunk's 16 input channels (the order the producer's conversion instruction writes [lo | hi]
// activations in, so that slot products are lo W_hi and hi W_lo) -- and in byte 24 the E8M0 code of s 2^-11 (s = 2^(E - 2), E = exponent of
// the chunk's largest |W_hi|; the 2^-11 undoes BOTH 2^11 pre-scales, the activations' and the weights', since every product carries
// exactly one of them).
static int cross_rows(unsigned char* tile, const float (*whi)[64], const float (*wlo)[64], int fmt, int sb) {
  const float mul_hi8 = ldexpf(1.f, sb), mul_lo8 = ldexpf(1.f, sb + 11);
  for (int nl = 0; nl < 64; ++nl) {
    unsigned char blk[32] = {};
    if (fmt == 8) {
      for (int kc = 0; kc < 16; ++kc) {
        blk[kc] = host_f32_to_e4m3(whi[kc][nl] * mul_hi8);
        blk[16 + kc] = host_f32_to_e4m3(wlo[kc][nl] * mul_lo8);
      }
    } else {
      float amax = 0.f;
      for (int kc = 0; kc < 16; ++kc) amax = std::max(amax, fabsf(whi[kc][nl]));
      if (!(amax > 0.f) || !std::isfinite(amax)) continue;          // an all-zero (padding) block: codes 0, scale byte 0
      int ea;
      (void)frexpf(amax, &ea);                                       // amax = m 2^ea, m in [0.5, 1): leading exponent ea - 1
      const int sexp = ea - 1 - 2;                                   // s = 2^sexp: the largest element lands in [4, 8)
      const float inv_s = ldexpf(1.f, -sexp);
      for (int kc = 0; kc < 16; ++kc) {
        const unsigned c2[2] = {host_f32_to_e2m3(whi[kc][nl], inv_s), host_f32_to_e2m3(wlo[kc][nl] * 2048.f, inv_s)};
        for (int j = 0; j < 2; ++j) {
          const int pos = 6 * (2 * kc + j);
          const unsigned w = c2[j] << (pos & 7);
          blk[pos >> 3] |= (unsigned char)w;
          blk[(pos >> 3) + 1] |= (unsigned char)(w >> 8);
        }
      }
      const int sbyte = sexp - 11 + 127;
      if (sbyte < 1 || sbyte > 254) NESTI_FAIL("internal: FP6 weight block scale out of the E8M0 range");
      blk[24] = (unsigned char)sbyte;
    }
    memcpy(tile + weight_slot(2, nl, 2), blk, 16);
    memcpy(tile + weight_slot(2, nl, 3), blk + 16, 16);
  }
  return 0;
}

// The packing of any layer, one or two fused parts, for the kernels of `dtype`: plain (f32 / f16 / bf16) or pair (NESTI_BF16X3 /
// NESTI_F16X3); x8_fmt = 8 or 6: the X8 / X6 form of the NESTI_F16X3 rows of a k^3 tap layer at 8^3 (cross_rows), 0: none
static int pack_layer(const LayerDesc& d, const TensorTable& tt, int dtype, int x8_fmt, PackedImage* pl) {
  if (x8_fmt && !use_conv8(d)) NESTI_FAIL("internal: the X8 / X6 packing is for the k^3 tap layers at 8^3");
  const int n_parts = d.scope2.empty() ? 1 : 2;
  Folded parts[2];
  if (fold_layer(d, d.scope, tt, &parts[0])) return 1;
  if (n_parts == 2 && fold_layer(d, d.scope2, tt, &parts[1])) return 1;
  const int part_p = d.Cout_p / n_parts;   // padded width of one part
  int widx[kMaxTaps];
  if (tap_list(d, pl, widx)) return 1;
  const size_t esz = dtype_size(dtype);
  // NESTI_BF16X3 / NESTI_F16X3 (host.h): a K chunk of a packed weight row is [W_hi | W_lo] for half as many channels as the
  // plain chunk holds (the kernels' pair K loop multiplies hi*W_hi + lo*W_hi + hi*W_lo from it: conv.hip / conv8n.hip, X3)
  const int planes = act_planes(dtype);
  const int drop = planes > 1 && !x8_fmt ? x3_drop_mask(d) : 0;
  pl->kind = layer_kind(d, dtype);
  if (pl->kind >= 2 && d.Cout_p % 64) NESTI_FAIL("internal: conv8n_kernel / conv4n_kernel need 64-column tiles");
  pl->x3n = planes > 1 && !x8_fmt;
  pl->x8_sb = x8_fmt ? -6 : 0;
  const int K_phys = d.Cin_p * planes;
  const int row_bytes = pl->kind >= 1 ? 64 : kRowBytes;   // bytes of one K chunk of one row
  const int KC = row_bytes / (int)esz;
  const int chunk_ch = KC / planes;                       // input channels per K chunk
  pl->TN = pl->kind >= 2 ? 64 : (part_p % 128 == 0) ? 128 : 64;   // a tile never straddles the two parts
  pl->n_tiles = d.Cout_p / pl->TN;
  pl->split_tile = n_parts == 1 ? pl->n_tiles : part_p / pl->TN;
  pl->n_chunks = K_phys / KC;
  if (K_phys % KC || d.Cin_p % kSplitGroup) NESTI_FAIL("internal: Cin_p not a multiple of the K chunk");
  if (n_parts == 2 && pl->n_taps != 1) NESTI_FAIL("internal: fused layers must be 1x1x1");
  const int e = dtype == NESTI_F16X3 ? pair_scale_exponent(d, parts, n_parts, widx, pl->n_taps) : 0;
  const float wmul = ldexpf(1.0f, e);
  pl->acc_scale = ldexpf(1.0f, -e);
  std::vector<int> inv(d.Cin_p, -1);   // padded input channel -> real input channel (-1: padding)
  for (int c = 0; c < d.cin; ++c) inv[d.in_pos[c]] = c;
  const size_t tile_bytes = (size_t)pl->TN * row_bytes;
  pl->w.assign((size_t)pl->n_tiles * pl->n_chunks * pl->n_taps * tile_bytes, 0);
  const int per_slot = 16 / (int)esz;
  const bool b16 = kernel_dtype(dtype) == NESTI_BF16;
  float whi[16][64], wlo[16][64];      // X8 / X6: W_hi and W - W_hi of a tile, which take the place of its W_lo half (cross_rows)
  for (int nt = 0; nt < pl->n_tiles; ++nt) {
    const int part = (nt * pl->TN) / part_p;
    const int n_base = nt * pl->TN - part * part_p;    // first real channel of this tile within its part
    const Folded& f = parts[part];
    for (int ch = 0; ch < pl->n_chunks; ++ch)
      for (int t = 0; t < pl->n_taps; ++t) {
        unsigned char* tile = pl->w.data() + (((size_t)nt * pl->n_chunks + ch) * pl->n_taps + t) * tile_bytes;
        const float* wt = f.w + (size_t)widx[t] * d.cin * d.cout;
        if (x8_fmt) { memset(whi, 0, sizeof(whi)); memset(wlo, 0, sizeof(wlo)); }
        for (int kc = 0; kc < (x8_fmt ? chunk_ch : KC); ++kc) {
          // which half of the row this K position is (0: W_hi, 1: W_lo) and the padded input channel it multiplies
          const int plane = kc / chunk_ch;
          const int cr = inv[ch * chunk_ch + kc % chunk_ch];
          if (cr < 0) continue;
          if (plane == 1 && (drop & 2)) continue;
          const float* wrow = wt + (size_t)cr * d.cout;
          for (int nl = 0; nl < pl->TN; ++nl) {
            const int n = n_base + nl;
            if (n >= d.cout) break;
            const float v = wrow[n] * f.scale[n] * wmul;
            unsigned char* dst = tile + weight_slot(pl->kind, nl, kc / per_slot) + (kc % per_slot) * esz;
            if (dtype == NESTI_F32) { memcpy(dst, &v, 4); continue; }
            uint16_t h = round16(v, b16);
            if (plane == 1 || x8_fmt) {
              const float hf = widen16(h, b16);
              if (x8_fmt) { whi[kc][nl] = hf; wlo[kc][nl] = v - hf; }   // the W_hi slot keeps h
              else h = round16(v - hf, b16);                            // W_lo = rne(W - W_hi)
            }
            memcpy(dst, &h, 2);
          }
        }
        if (x8_fmt && cross_rows(tile, whi, wlo, x8_fmt, pl->x8_sb)) return 1;
      }
  }
  pl->bias.assign((size_t)d.Cout_p, 0.f);   // the folded biases of the parts, each zero-padded to its share of the columns
  for (int part = 0; part < n_parts; ++part)
    for (int n = 0; n < d.cout; ++n) pl->bias[(size_t)part * part_p + n] = parts[part].bias[n];
  return 0;
}

int pack_form(const LayerDesc& d, const TensorTable& tt, int form, int mdt, PackedImage* img) {
  switch (form) {
    case NESTI_DEBUG_FORM_X8: return pack_layer(d, tt, NESTI_F16X3, 8, img);
    case NESTI_DEBUG_FORM_X6: return pack_layer(d, tt, NESTI_F16X3, 6, img);
    case kFormMix: return pack_layer(d, tt, kernel_dtype(mdt), 0, img);
    case NESTI_DEBUG_FORM_PLAIN: return pack_layer(d, tt, act_planes(mdt) > 1 ? NESTI_F16 : mdt, 0, img);   // pair models: the filter pass
    default: return pack_layer(d, tt, mdt, 0, img);
  }
}

}  // namespace nesti

// include/nesti_hip.h: the FP6 weight encoder, exposed for tests/test_abi.py
extern "C" int nesti_f32_to_e2m3(float value, float inv_scale) { return (int)nesti::host_f32_to_e2m3(value, inv_scale); }

// include/nesti_hip.h: the packer without a device (tests/test_pack.py)
extern "C" int nesti_debug_pack_layer(const nesti_config_t* cfg, const nesti_tensor_t* tensors, int n_tensors, int dtype, int form,
                                      int layer, nesti_debug_pack_t* info, void* w, size_t max_w, float* bias, size_t max_bias) {
  using namespace nesti;
  if (!cfg || !tensors || !info) NESTI_FAIL("nesti_debug_pack_layer: null argument");
  if (dtype < NESTI_F32 || dtype > NESTI_F16X8C) NESTI_FAIL("nesti_debug_pack_layer: bad dtype");
  Graph g;
  if (build_graph(cfg, &g, dtype_x8(dtype))) return 1;
  if (layer < 0 || layer >= (int)g.layers.size()) NESTI_FAIL("nesti_debug_pack_layer: layer index outside the model");
  const LayerDesc& d = g.layers[layer];
  const int mdt = main_dtype(dtype), packing = form_packing(form);
  const bool x8 = packing == NESTI_DEBUG_FORM_X8 || packing == NESTI_DEBUG_FORM_X6;
  if (packing != NESTI_DEBUG_FORM_PLAIN && packing != NESTI_DEBUG_FORM_PAIR && !x8) NESTI_FAIL("nesti_debug_pack_layer: form is NESTI_DEBUG_FORM_*");
  if (packing == NESTI_DEBUG_FORM_PAIR && act_planes(mdt) == 1)
    NESTI_FAIL("nesti_debug_pack_layer: the pair packing is for the pair dtypes (NESTI_BF16X3, NESTI_F16X3 and the modes built on it)");
  if (x8 && !(g.x8 && use_conv8(d)))
    NESTI_FAIL("nesti_debug_pack_layer: the X8 / X6 packings are for the k^3 tap layers at 8^3 of NESTI_F16X8 / NESTI_F16X8C models; " + d.scope +
               " is not one");
  const TensorTable tt = tensor_table(tensors, n_tensors);
  PackedImage img;
  if (pack_form(d, tt, packing, mdt, &img)) return 1;
  memset(info, 0, sizeof(*info));
  info->kind = img.kind; info->TN = img.TN; info->n_tiles = img.n_tiles; info->split_tile = img.split_tile;
  info->n_chunks = img.n_chunks; info->n_taps = img.n_taps; info->x3n = img.x3n ? 1 : 0; info->acc_scale = img.acc_scale;
  info->x8_sb = img.x8_sb; info->x8_sc = x8_activation_exponent(d, tt);
  info->w_bytes = (int64_t)img.w.size(); info->n_bias = (int64_t)img.bias.size();
  memcpy(info->tap, img.tap, sizeof(info->tap));
  if ((w && max_w < img.w.size()) || (bias && max_bias < img.bias.size())) NESTI_FAIL("nesti_debug_pack_layer: output arrays too small");
  if (w) memcpy(w, img.w.data(), img.w.size());
  if (bias) memcpy(bias, img.bias.data(), img.bias.size() * sizeof(float));
  return 0;
}
