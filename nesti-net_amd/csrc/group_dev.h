// What the list passes that serve a row by a GROUP of lanes share (smooth.hip, denoise.hip, outlier.hip) beyond the group's row and
// list (group_row, group_centre_lost, group_nbr_row: nbr_dev.h) and its reductions (wave_dev.h): the eligibility of a normal, the
// cone weight of smoothing and denoising, and on the host the choice of the group, its launch and the switch behind the
// nesti_debug_*_lanes entries.  One definition, so the test on the bits and the weight are the same values in both units.
//
// For the including unit: include patches_dev.h first, then `#pragma clang fp contract(off)`, then pca_dev.h, nbr_dev.h and this
// header -- every product and sum below is rounded on its own.
#pragma once
#include <atomic>

#include "nbr_dev.h"

namespace nesti {
namespace {

__device__ __forceinline__ bool nonzero_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) != 0u; }
// all three components finite and at least one non-zero, on the bits: orient.hip's rule
__device__ __forceinline__ bool eligible_normal(float x, float y, float z) {
  return finite_bits(x) && finite_bits(y) && finite_bits(z) && (nonzero_bits(x) || nonzero_bits(y) || nonzero_bits(z));
}

// The cone weight of a slot (smooth.hip step 3, denoise.hip step 4): the neighbour's normal (f0, f1, f2) against the centre's
// (ncx, ncy, ncz), q_c = knn_d2 of it, span = 1 - cos_t.  counts: the normal is eligible and t > 0 (false for NaN); then
// n = (double)n_j, qj = q_j, dd = n_c . n_j and tt = min(t, 1).
struct ConeWeight {
  bool counts;
  double nx, ny, nz, qj, dd, tt;
};
__device__ __forceinline__ ConeWeight cone_weight(double ncx, double ncy, double ncz, double qc, float f0, float f1, float f2,
                                                  double cos_t, double span) {
  ConeWeight c = {false, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (eligible_normal(f0, f1, f2)) {
    c.nx = f0; c.ny = f1; c.nz = f2;
    c.qj = knn_d2(c.nx, c.ny, c.nz);
    c.dd = (ncx * c.nx + ncy * c.ny) + ncz * c.nz;
    const double ca = fabs(c.dd) / sqrt(qc * c.qj);
    const double tt = (ca - cos_t) / span;
    c.counts = tt > 0.0;                                      // false for NaN: the slot adds nothing
    c.tt = tt < 1.0 ? tt : 1.0;
  }
  return c;
}
// the falloff with distance that goes with it: u = 1 - (falloff d2) / r2, or 1 where the neighbourhood has no extent
__device__ __forceinline__ double cone_falloff(double falloff, double d2, double r2) { return r2 > 0.0 ? 1.0 - (falloff * d2) / r2 : 1.0; }

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, G>) for the lane group G of a launch: the smallest of 16, 32 and 64 that holds `need` slots, or a
// wider one asked for (the unit's nesti_debug_*_lanes switch; 0: none), like with_scales (pca_dev.h)
template <class F>
int with_lane_group(int need, int asked, F&& f) {
  const int G = std::max(asked, need <= 16 ? 16 : need <= 32 ? 32 : kWave);
  if (G == 16) return f(std::integral_constant<int, 16>{});
  if (G == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, kWave>{});
}
// one launch of a kernel that serves M > 0 rows by groups of G lanes (group_row): waves of 64 / G rows each
template <int G, class Params>
int launch_group_rows(void (*kernel)(Params), const Params& params, int M, void* stream) {
  constexpr int kPerWave = kWave / G;
  return launch_wave_rows(kernel, params, (M + kPerWave - 1) / kPerWave, stream);
}
// the body of a nesti_debug_*_lanes entry: each unit has a switch of its own, so one never moves another's kernels
inline int set_lane_group(const char* entry, std::atomic<int>& lanes_switch, int lanes) {
  if (lanes != 0 && lanes != 16 && lanes != 32 && lanes != kWave) NESTI_FAIL(std::string(entry) + ": lanes must be 0, 16, 32 or 64");
  lanes_switch.store(lanes, std::memory_order_relaxed);
  return 0;
}

}  // namespace
}  // namespace nesti
