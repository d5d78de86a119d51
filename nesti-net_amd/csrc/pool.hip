// The max pools of the CNN towers that stand alone: 2^3 stride 2, and 3^3 stride 2 on the 3^3 volume, on channels-last activations
// (the average pool and most max pools are fused into conv epilogues, conv.hip).  Memory-bound.
#include "kernels.h"

namespace nesti {
namespace {

constexpr int kThreads = 256;

template <int DT> struct Vec16;   // 16-byte vector of elements <-> floats
template <> struct Vec16<NESTI_F32> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  }
};
template <int DT> struct Vec16_16 {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = Elem<DT>::to_f32((uint16_t)(w[i] & 0xffffu));
      f[2 * i + 1] = Elem<DT>::to_f32((uint16_t)(w[i] >> 16));
    }
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] = (uint32_t)Elem<DT>::from_f32(f[2 * i]) | ((uint32_t)Elem<DT>::from_f32(f[2 * i + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct Vec16<NESTI_BF16> : Vec16_16<NESTI_BF16> {};
template <> struct Vec16<NESTI_F16> : Vec16_16<NESTI_F16> {};

// Pair-mode activations (NESTI_BF16X3 / NESTI_F16X3, common.h): eight logical channels = the hi vector at split_col(col)
// and the lo vector one 64-element plane further; the value is hi + lo.  Stores emit both planes.
template <int DT>
__device__ __forceinline__ void load_vec(const unsigned char* base, long long row_elems, int coff, int cv, int split, float* f) {
  using V = Vec16<DT>;
  constexpr int kEsz = (DT == NESTI_F32) ? 4 : 2;
  if constexpr (DT != NESTI_F32) {
    if (split) {
      const unsigned char* s0 = base + (row_elems + split_col(coff + cv * 8)) * 2;
      float h[8], l[8];
      V::unpack(*reinterpret_cast<const uint4*>(s0), h);
      V::unpack(*reinterpret_cast<const uint4*>(s0 + 2 * kSplitGroup), l);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = h[e] + l[e];
      return;
    }
  }
  V::unpack(*reinterpret_cast<const uint4*>(base + (row_elems + coff) * kEsz + cv * 16), f);
}
template <int DT>
__device__ __forceinline__ void store_vec(unsigned char* base, long long row_elems, int coff, int cv, int split, const float* m) {
  using V = Vec16<DT>;
  constexpr int kEsz = (DT == NESTI_F32) ? 4 : 2;
  if constexpr (DT != NESTI_F32) {
    if (split) {
      store_act8<Elem<DT>>(base, row_elems, coff + cv * 8, make_float4(m[0], m[1], m[2], m[3]), make_float4(m[4], m[5], m[6], m[7]), 1);
      return;
    }
  }
  *reinterpret_cast<uint4*>(base + (row_elems + coff) * kEsz + cv * 16) = V::pack(m);
}

// tf.nn.max_pool3d 2^3 stride 2 SAME on an even volume (utils/tf_util.py:424-428)
template <int DT>
__global__ __launch_bounds__(kThreads) void maxpool2_kernel(const PoolParams p) {
  using V = Vec16<DT>;
  const int npts = live_points(p);
  const int log2S = p.log2S, log2V = 3 * log2S;
  const int log2So = log2S - 1, So = 1 << log2So, log2Vo = 3 * log2So;
  const int vecs = p.C / V::N;
  const long long total = ((long long)npts << log2Vo) * vecs;
  const unsigned char* in_b = reinterpret_cast<const unsigned char*>(p.in);
  unsigned char* out_b = reinterpret_cast<unsigned char*>(p.out);
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int cv = (int)(i % vecs);
    const long long orow = i / vecs;
    const long long pt = orow >> log2Vo;
    const int vox = (int)(orow & ((1 << log2Vo) - 1));
    const int z = vox >> (2 * log2So), y = (vox >> log2So) & (So - 1), x = vox & (So - 1);
    float m[V::N];
#pragma unroll
    for (int e = 0; e < V::N; ++e) m[e] = -INFINITY;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const int zz = 2 * z + (a >> 2), yy = 2 * y + ((a >> 1) & 1), xx = 2 * x + (a & 1);
      const long long srow = (pt << log2V) + (((zz << log2S) + yy) << log2S) + xx;
      float f[V::N];
      load_vec<DT>(in_b, srow * p.in_cstride, p.in_coff, cv, p.split, f);
#pragma unroll
      for (int e = 0; e < V::N; ++e) m[e] = fmaxf(m[e], f[e]);
    }
    store_vec<DT>(out_b, orow * p.out_cstride, p.out_coff, cv, p.split, m);
  }
}

// tf.nn.max_pool3d(k=[3,3,3], stride 2, SAME) on a 3^3 volume (conv_net_3g, models/experts_n_est.py:238): TF pads one
// voxel in front, so output cell o reads input {2o-1, 2o, 2o+1} clipped to [0,2] = {o, o+1} per axis.  Input rows live
// in the 4^3 index space (row 16 z + 4 y + x), output is a dense 2^3.
template <int DT>
__global__ __launch_bounds__(kThreads) void maxpool3s2_kernel(const PoolParams p) {
  using V = Vec16<DT>;
  const int npts = live_points(p);
  const int nv = p.C / V::N;
  const long long total = (long long)npts * 8 * nv;
  const unsigned char* in_b = reinterpret_cast<const unsigned char*>(p.in);
  unsigned char* out_b = reinterpret_cast<unsigned char*>(p.out);
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % nv);
    const long long orow = idx / nv;
    const long long pt = orow >> 3;
    const int cell = (int)(orow & 7);
    const int z = cell >> 2, y = (cell >> 1) & 1, x = cell & 1;
    float m[V::N];
#pragma unroll
    for (int e = 0; e < V::N; ++e) m[e] = -INFINITY;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const int zz = z + (a >> 2), yy = y + ((a >> 1) & 1), xx = x + (a & 1);
      const long long srow = pt * 64 + zz * 16 + yy * 4 + xx;
      float f[V::N];
      load_vec<DT>(in_b, srow * p.in_cstride, p.in_coff, cv, p.split, f);
#pragma unroll
      for (int e = 0; e < V::N; ++e) m[e] = fmaxf(m[e], f[e]);
    }
    store_vec<DT>(out_b, orow * p.out_cstride, p.out_coff, cv, p.split, m);
  }
}

int grid_for(long long work) {
  long long g = (work + kThreads - 1) / kThreads;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

int launch_maxpool2(const PoolParams& p, int dtype, hipStream_t stream) {
  if (p.npoints <= 0) return 0;
  if (p.log2S < 1) NESTI_FAIL("maxpool2: input volume must be >= 2^3");
  const int n = (dtype == NESTI_F32) ? 4 : 8;
  if (p.C % n) NESTI_FAIL("maxpool2: C must be a multiple of the 16-byte vector");
  const long long work = ((long long)p.npoints << (3 * (p.log2S - 1))) * (p.C / n);
  return with_elem_type(dtype, "launch_maxpool2", [&](auto dt) {
    hipLaunchKernelGGL(maxpool2_kernel<decltype(dt)::value>, dim3(grid_for(work)), dim3(kThreads), 0, stream, p);
    NESTI_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

int launch_maxpool3s2(const PoolParams& p, int dtype, hipStream_t stream) {
  if (p.npoints <= 0) return 0;
  const int n = (dtype == NESTI_F32) ? 4 : 8;
  if (p.C % n) NESTI_FAIL("maxpool3s2: C must be a multiple of the 16-byte vector");
  const long long work = (long long)p.npoints * 8 * (p.C / n);
  return with_elem_type(dtype, "launch_maxpool3s2", [&](auto dt) {
    hipLaunchKernelGGL(maxpool3s2_kernel<decltype(dt)::value>, dim3(grid_for(work)), dim3(kThreads), 0, stream, p);
    NESTI_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // namespace nesti
