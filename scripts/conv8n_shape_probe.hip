// Does conv8n_kernel's plain tap loop (MODE 0) run faster on v_mfma_f32_16x16x32_f16 than on v_mfma_f32_32x32x16_f16?
// The instruction issues the same FLOP per cycle in both shapes, but the clock the chip holds under load depends on the shape
// (the microarchitecture notes measured 1.12-1.14x FLOP/s for 16x16x32 on random data with LDS-fed operands).  This probe runs
// the loop's skeleton in both shapes on random f16 data at 2 waves per SIMD:
//   * 512 threads, 8 waves, 4 x-line tiles x 2 column tiles (64 columns) per wave, the 6 staged planes of a z half (k = 5);
//   * every fragment read unconditional, only the MFMAs of dead tiles skipped -- conv8n's 5^3 skip pattern (Latin square of
//     tiles over the waves, 72 % live);
//   * per (tile, tap) 4 x 32x32x16 (SHAPE 0) or 8 x 16x16x32 (SHAPE 1: row half x column quarter) from the SAME two A and four
//     B ds_read_b128 per tap, with the kernel's per-lane addresses and swizzles (SHAPE 1: the K-slot order {0, 3, 1, 2});
//   * the 3-slot weight-row ring: one 20-KiB row of taps streams in by LDS-DMA two rows ahead, one s_barrier per row.
// A timing skeleton, not a reference for conv8n's addressing: its source-run offsets (base_of) only approximate the kernel's -- for
// wave 0 and dz < 2 they point below the input region (into the weight slots) and for the last runs past the 160-KiB allocation
// (reads there return zeros on gfx950); on random data the reads cost the same, and the values are never checked.
// Second part, the price of the same change in the experts' FP6 loop (MODE 3): a register-only loop of block-scaled e2m3 MFMAs
// (random sextets, scale 2^0), v_mfma_scale_f32_32x32x64_f8f6f4 against v_mfma_scale_f32_16x16x128_f8f6f4 at equal FLOP per trip.
// Each shape runs >= 2 s back-to-back before its timed launches.  Built with -DPROBE_STAMPS (a diagnostic build) wave 0 of every
// workgroup also stamps s_memtime / s_memrealtime around its loop into a buffer of its own: the in-kernel clock (median over
// workgroups) and the loop's cycles.
//   hipcc -O3 --offload-arch=gfx950 scripts/conv8n_shape_probe.hip -o scripts/conv8n_shape_probe
//   hipcc -O3 --offload-arch=gfx950 -DPROBE_STAMPS scripts/conv8n_shape_probe.hip -o scripts/conv8n_shape_stamps_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) u32x4_t* lds_u32x4_ptr;
__device__ __forceinline__ uint4 lds128(unsigned addr) {
  const u32x4_t v = *(lds_u32x4_ptr)(size_t)addr;
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void glds16(const unsigned char* src, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}

constexpr int kTile = 2048, kBTile = 4096, kAOff = 65536, kSlot = 5 * kBTile, kNZ = 6, kLds = 163840;
constexpr unsigned kOob = 0x40000u;
constexpr int kGrid = 2048;

template <int SHAPE>
__global__ __launch_bounds__(512) void k(const unsigned char* in, float* out, int chunks, unsigned long long* stamps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  for (int i = tid; i < kLds / 16; i += 512) reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(in)[i];
  __syncthreads();
  constexpr bool M16 = SHAPE == 1;
  const int l31 = lane & 31, khalf = lane >> 5;
  const int lr = M16 ? (lane & 15) : l31;
  const int ks = M16 ? (0x9C >> (2 * (lane >> 4))) & 3 : khalf;
  const int pt = lr >> 3, rx = lr & 7;
  const int a_sw = (ks ^ pt) & 3, b_sw = (ks ^ (lr >> 2)) & 3;
  const unsigned a_lane = lds0 + kAOff + (unsigned)(lr * 64 + (a_sw << 4));
  const unsigned b_lane = lds0 + (unsigned)(lr * 64 + (b_sw << 4));
  const unsigned a_d1 = (M16 ? 1024u : 0u) + ((a_sw & 2) ? (unsigned)-32 : 32u);
  const unsigned b_d1 = M16 ? 1024u : (b_sw & 2) ? (unsigned)-32 : 32u;
  unsigned pa[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) pa[d] = ((unsigned)(rx + d - 2) < 8u) ? a_lane + (unsigned)((d - 2) * 64) : kOob;
  unsigned ym = 0u, zm = 0u;                    // z half 0: tile j is (y = (wave - j) & 7, z = j)
#pragma unroll
  for (int d = 0; d < 5; ++d)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((unsigned)(((wave - j) & 7) + d - 2) < 8u) ym |= 1u << (4 * d + j);
      if ((unsigned)(j + d - 2) < 8u) zm |= 1u << (4 * d + j);
    }
  f32x16 acc[4][2];
  f32x4 acc4[4][2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][n][r] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc4[j][n][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  uint4 a[4][2], b[2][2][2];
  auto load_b = [&](uint4 (&dst)[2][2], unsigned src) __attribute__((always_inline)) {
#pragma unroll
    for (int n = 0; n < 2; ++n) { dst[n][0] = lds128(src + n * kTile); dst[n][1] = lds128(src + n * kTile + b_d1); }
  };
  auto tile_mma = [&](int j, const uint4 (&bc)[2][2]) __attribute__((always_inline)) {
    if constexpr (M16) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc4[j][h][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[j][h]), __builtin_bit_cast(f16x8, bc[q >> 1][q & 1]), acc4[j][h][q], 0, 0, 0);
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[j][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[j][s]), __builtin_bit_cast(f16x8, bc[n][s]), acc[j][n], 0, 0, 0);
    }
  };
  // approximate source-run offsets (see the header): timing only
  auto base_of = [&](int g) -> int { const int dz = g / 5, dy = g % 5; return (((wave + dy + dz - 4) & 7) * kNZ + dz - 2) * kTile; };
  auto mask_of = [&](int g) -> unsigned { const int dz = g / 5, dy = g % 5; return (zm >> (4 * dz)) & (ym >> (4 * dy)) & 0xfu; };
  auto stage = [&](int row, int slot) {
    const unsigned char* src = in + (size_t)(row & 7) * kSlot;
    for (int pid = wave; pid < kSlot / 1024; pid += 8) glds16(src + pid * 1024 + lane * 16, lds0 + slot * kSlot + pid * 1024);
  };
#ifdef PROBE_STAMPS
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (int c = 0; c < chunks; ++c) {
    stage(0, 0);
    stage(1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    load_b(b[1], b_lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j][0] = lds128(pa[0] + base_of(0) + j * kTile); a[j][1] = lds128(pa[0] + base_of(0) + a_d1 + j * kTile); }
    for (int g = 0; g < 25; ++g) {
      if (g + 2 < 25) stage(g + 2, (g + 2) % 3);
      const bool more = g + 1 < 25;
      unsigned mask_g = mask_of(g), mask_n = more ? mask_of(g + 1) : 0u;
      const int base_g = base_of(g), base_n = more ? base_of(g + 1) : 0;
      const unsigned boff = (unsigned)((g % 3) * kSlot), boff_n = (unsigned)(((g + 1) % 3) * kSlot);
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const bool last_u = u == 4;
        unsigned m_mm = mask_g;
        asm volatile("" : "+s"(m_mm));
        const unsigned nb0 = pa[last_u ? 0 : u + 1] + (unsigned)(last_u ? base_n : base_g);
        const unsigned bsrc = b_lane + (last_u ? boff_n : boff + (unsigned)((u + 1) * kBTile));
        if (u == 0) {
#pragma unroll
          for (int n = 0; n < 2; ++n) { b[0][n][0] = b[1][n][0]; b[0][n][1] = b[1][n][1]; }
        }
        load_b(b[(u + 1) & 1], bsrc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (m_mm & (1u << j)) tile_mma(j, b[u & 1]);
          a[j][0] = lds128(nb0 + j * kTile);
          a[j][1] = lds128(nb0 + a_d1 + j * kTile);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __syncthreads();
  }
#ifdef PROBE_STAMPS
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
#endif
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s += acc[j][n][r];
#pragma unroll
      for (int q = 0; q < 4; ++q) s += acc4[j][n][q][0] + acc4[j][n][q][1] + acc4[j][n][q][2] + acc4[j][n][q][3];
    }
  out[blockIdx.x * 512 + tid] = s;
}

typedef int i32x8 __attribute__((ext_vector_type(8)));
template <int SHAPE>   // 0: 4 x 32x32x64 per trip, 1: 8 x 16x16x128 per trip (e2m3 x e2m3, the upper 2 of 8 operand registers unused)
__global__ __launch_bounds__(512) void kx6(const unsigned char* in, float* out, int iters, unsigned long long* stamps) {
  const int tid = threadIdx.x;
  i32x8 a[2], b[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a[i] = reinterpret_cast<const i32x8*>(in)[(tid * 4 + i) & 4095];
    b[i] = reinterpret_cast<const i32x8*>(in)[(tid * 4 + 2 + i) & 4095];
  }
  int sa = 0x7f, sb = 0x7f;
  asm volatile("" : "+v"(sa), "+v"(sb));
  f32x16 acc[4];
  f32x4 acc4[8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#ifdef PROBE_STAMPS
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (int it = 0; it < iters; ++it) {
    if constexpr (SHAPE == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i & 1], b[i >> 1], acc[i], 2, 2, 0, sa, 0, sb);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc4[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i & 1], b[(i >> 1) & 1], acc4[i], 2, 2, 0, sa, 0, sb);
    }
  }
#ifdef PROBE_STAMPS
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
#endif
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[i][r];
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc4[i][0] + acc4[i][1] + acc4[i][2] + acc4[i][3];
  out[blockIdx.x * 512 + tid] = s;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

// launch(): one launch of the kernel under test; flop_wg: the FLOP one workgroup issues per launch
template <typename F>
void run(const char* name, F launch, double flop_wg, unsigned long long* stamps) {
  const int timed = 20;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  float ms = 0.f, warm = 0.f;
  while (warm < 2000.f) {                                // >= 2 s back-to-back before the timed launches
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < 20; ++i) launch();
    CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    warm += ms;
  }
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < timed; ++i) launch();
  CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  ms /= timed;
  printf("%-22s %8.3f ms/launch  %7.1f TFLOP/s issued", name, ms, flop_wg * kGrid / (ms * 1e-3) / 1e12);
#ifdef PROBE_STAMPS
  std::vector<unsigned long long> h(2 * kGrid);
  CHECK(hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> clk(kGrid), cyc(kGrid);
  for (int i = 0; i < kGrid; ++i) { cyc[i] = (double)h[2 * i]; clk[i] = h[2 * i + 1] ? (double)h[2 * i] / (double)h[2 * i + 1] * 100.0 : 0.0; }
  std::sort(clk.begin(), clk.end()); std::sort(cyc.begin(), cyc.end());
  printf("  | in-kernel clock %5.0f MHz, loop %.4g cycles per workgroup (medians), %.1f cycles per MFLOP issued",
         clk[kGrid / 2], cyc[kGrid / 2], cyc[kGrid / 2] / flop_wg * 1e6);
#endif
  printf("\n");
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

int main() {
  unsigned char* in; float* out; unsigned long long* stamps;
  CHECK(hipMalloc(&in, 1 << 20)); CHECK(hipMalloc(&out, (size_t)kGrid * 512 * 4)); CHECK(hipMalloc(&stamps, (size_t)kGrid * 16));
  CHECK(hipMemset(stamps, 0, (size_t)kGrid * 16));
  std::vector<uint16_t> h(1 << 19);
  srand(1);
  for (auto& v : h) v = (uint16_t)(((rand() & 1) << 15) | ((11 + rand() % 4) << 10) | (rand() & 1023));   // random f16 in about [-1, 1]
  CHECK(hipMemcpy(in, h.data(), 1 << 20, hipMemcpyHostToDevice));
  double live = 0;                                       // conv8n's 5^3 pattern on z half 0 (half 1 is its mirror image)
  for (int w = 0; w < 8; ++w)
    for (int j = 0; j < 4; ++j)
      for (int dz = -2; dz <= 2; ++dz)
        for (int dy = -2; dy <= 2; ++dy) {
          const int y = (w - j) & 7, z = j;
          if ((unsigned)(y + dy) < 8u && (unsigned)(z + dz) < 8u) live += 5;
        }
  live /= 8 * 4 * 125.0;
  printf("random data, 2 waves per SIMD; live fraction of the 5^3 skip pattern %.4f\n", live);
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k<0>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&kx6<0>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&kx6<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  // tap loop: per workgroup and chunk 8 waves x 125 taps x 4 tiles x live x (32 x 64 x 32 x 2 FLOP); 40 chunks per launch
  const int chunks = 40;
  const double flop_tap = (double)chunks * 8 * 125 * 4 * live * 32 * 64 * 32 * 2;
  for (int rep = 0; rep < 2; ++rep) {                    // interleaved
    run("tap loop 32x32x16", [&] { hipLaunchKernelGGL(k<0>, dim3(kGrid), dim3(512), kLds, 0, in, out, chunks, stamps); }, flop_tap, stamps);
    run("tap loop 16x16x32", [&] { hipLaunchKernelGGL(k<1>, dim3(kGrid), dim3(512), kLds, 0, in, out, chunks, stamps); }, flop_tap, stamps);
  }
  // register-only e2m3: 8 waves x iters x (4 x 32 x 32 x 64 x 2 FLOP); the 160-KiB LDS allocation holds it at 2 waves per SIMD
  const int iters = 16000;
  const double flop_x6 = 8.0 * iters * 4 * 32 * 32 * 64 * 2;
  for (int rep = 0; rep < 2; ++rep) {
    run("e2m3 regs 32x32x64", [&] { hipLaunchKernelGGL(kx6<0>, dim3(kGrid), dim3(512), kLds, 0, in, out, iters, stamps); }, flop_x6, stamps);
    run("e2m3 regs 16x16x128", [&] { hipLaunchKernelGGL(kx6<1>, dim3(kGrid), dim3(512), kLds, 0, in, out, iters, stamps); }, flop_x6, stamps);
  }
  return 0;
}
