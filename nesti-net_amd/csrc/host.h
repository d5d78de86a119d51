// What the host-only units of libnesti_hip.so (graph.cpp, pack.cpp) share with the HIP files: the error slot, the dtype
// predicates and the layout constants the weight packer shares with the kernels.  No HIP header: common.h includes this file,
// so host and device code see the same definitions.
#pragma once
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
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr int kRowBytes = 128;    // bytes of one K-chunk row in LDS (64 x 16-bit or 32 x f32)
constexpr int kMaxTaps = 125;     // 5^3

// host-side conversions used by the weight repacker (pack.cpp)
uint16_t host_f32_to_bf16(float f);
uint16_t host_f32_to_f16(float f);
float host_f16_to_f32(uint16_t h);

}  // namespace nesti
