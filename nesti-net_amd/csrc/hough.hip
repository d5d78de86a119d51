// Hough-transform normals over neighbour lists (DESIGN.md 2 "Hough-transform normals"): the sharp-feature estimator after Boulch and
// Marlet, "Fast and Robust Normal Estimation for Point Clouds with Sharp Features" (SGP 2012) -- planes through random triplets of a
// neighbourhood vote for their normal in an accumulator over the hemisphere, and the fullest bin names the normal -- with conventions
// of the library's own, chosen so that a restatement in plain IEEE arithmetic (tests/_hough_fixture.py) predicts every output bit:
// fp64 throughout, every operation rounded on its own; only + - x / sqrt, comparisons and integer arithmetic, so their (phi, theta)
// accumulator is a hemi-octahedral one, their random triplets are hashed ones and their random rotations a caller-supplied table.  No
// model, no weights.  No parity with their code is claimed.
//
// THE ESTIMATOR (nesti_hough_normals_nbr / nesti_hough_normals_nbr_at).  Centres, the list nbr_dev [M, K], ks [S], the valid prefix,
// n_s = min(ks[s], valid prefix), d = (double)p - (double)c and r2_s are exactly as for nesti_pca_normals_nbr (nbr_dev.h): the list is
// untrusted, the prefix ends at the first entry outside [0, N), a non-finite centre has an empty prefix.  Parameters: T triplets
// (1 .. 4096), B bins per axis (2 .. 16), R rotations (1 .. 8), rot [R, 9] fp64 row-major on the HOST, seed, query_row0.  Per row i with
// key row q = query_row0 + i, per scale s with n = n_s and slots d_0 .. d_{n-1}:
//  1 TRIPLET t = 0 .. T-1:  h_c = subsample_hash(seed, q, 0, 3 t + c), c = 0, 1, 2 (the scale argument is 0 on purpose: scale s of ks
//    equals the single scale of a run with ks = {ks[s]}).  Indices from 64-bit products, not %:  i0 = (h0 n) >> 32;
//    j = (h1 (n - 1)) >> 32, i1 = j + (j >= i0);  lo, hi = min, max(i0, i1);  j = (h2 (n - 2)) >> 32, j += (j >= lo), i2 = j + (j >= hi).
//    Distinct for n >= 3.
//  2 PLANE:  e1 = d_i1 - d_i0, e2 = d_i2 - d_i0;  v = e1 x e2, each component two products and one difference;
//    l1 = (e1x^2 + e1y^2) + e1z^2, l2 and qq (the same sum for v) likewise.  The triplet is VALID iff qq > 2^-20 (l1 l2): false for
//    NaN, for coincident points and for near-collinear ones (sin < 2^-10).  u = v / sqrt(qq), three divisions.
//  3 VOTE, for each rotation rho:  w_k = (rot[rho][3k] u_x + rot[rho][3k+1] u_y) + rot[rho][3k+2] u_z;  sigma = -1 if the first
//    non-zero of (w_z, w_y, w_x) is negative, else +1;  w <- sigma w;  m = (|w_x| + |w_y|) + w_z, a = w_x / m, b = w_y / m;
//    bi = clamp((int)floor(((a + b) + 1) (B / 2.0)), 0, B - 1), bj the same with a - b;  bin = bi B + bj;  count[rho][bin] += 1 (integer).
//  4 WINNER:  per rho the bin with the largest count, among equals the smaller bin; rho* the rotation whose winner has the largest
//    count, among equals the smaller rho (together: the smallest flat index rho B^2 + bin among the largest counts).  win = that count,
//    valid = the number of valid triplets.
//  5 NORMAL:  over the valid triplets whose bin under rho* is the winner, the sum of sigma_t u_t (sigma_t under rho*, u_t unrotated):
//    lane l adds its triplets t = l, l + 64, ... in ascending order into three fp64 partial sums, the lanes meet in wave_sum (pca_dev.h:
//    xor offsets 32, 16, ..., 1).  nn = (X^2 + Y^2) + Z^2; if nn > 0 and finite the normal is (X, Y, Z) / sqrt(nn), rounded to f32
//    once, then signed on the f32 values so that the first non-zero of (n_z, n_y, n_x) is positive; zeros are +0.
//  6 OUTPUTS (device; any may be NULL):  normals_out_dev [M,S,3] f32;  conf_out_dev [M,S] f32 = (float)((double)win / (double)valid);
//    votes_out_dev [M,S,2] int32 = (win, valid);  radius_out_dev [M,S] f32 and count_out_dev [M,S] int32 as the other list entries
//    write them ((float)sqrt(r2_s), n_s).
//  7 SENTINEL:  n < 3, valid == 0 or a failed step 5 gives normal 0 0 0, confidence 0 and votes (0, valid); radius and count are still
//    written.  No output is NaN or infinite for finite input.
// DETERMINISM.  No floating-point atomics; the votes are integer additions, whose order cannot change a count.  A row's bits are a
// pure function of (cloud, centre, list prefix, T, B, R, rot, seed, key row): independent of batching, streams and the grid.
//
// THE KERNEL.  One wave per query, four per workgroup, like pca_nbr_kernel; waves never meet and whole waves leave for q >= M.  The row's
// neighbour coordinates are staged once in LDS as f32 (3 KiB per wave at K = 256) and the centre is subtracted on the fly with the same
// arithmetic, so the 3 T random gathers of a scale hit LDS, not HBM.  The R B^2 int32 counters live in LDS (at most 8 KiB per wave),
// cleared per scale and voted with integer LDS atomics; the arg-max is a wave reduction on one int key (count, -flat bin); pass 2
// recomputes every triplet under rho* only.  Scales run one after the other.  44 KiB of LDS per workgroup: three workgroups per CU.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
#include "patches_dev.h"   // query_centre, centre_lost, subsample_hash; its ball_d2 is not used here

// every product and sum below is rounded on its own: the CPU restatement (tests/_hough_fixture.py) predicts every bit
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "nbr_dev.h"

namespace nesti {
namespace {

constexpr int kMaxBins2 = NESTI_HOUGH_MAX_BINS * NESTI_HOUGH_MAX_BINS;
constexpr int kMaxCounters = NESTI_HOUGH_MAX_ROT * kMaxBins2;
static_assert(NESTI_HOUGH_MAX_T < (1 << 15) && kMaxCounters <= (1 << 16), "the arg-max key holds (count, 65535 - flat bin) in one int");

struct HoughParams {
  NbrParams np;                       // np.p.seed: the hash seed; np.p.row0: the key row of row 0
  int T, B, R;
  double rot[NESTI_HOUGH_MAX_ROT * 9];
  float* normals_out;                 // [M, S, 3] or NULL
  float* conf_out;                    // [M, S] or NULL
  int32_t* votes_out;                 // [M, S, 2] or NULL
};

struct HoughShared {
  float xyz[kRowsPerBlock][3][NESTI_KNN_MAX_K];
  int count[kRowsPerBlock][kMaxCounters];
};

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
  return v;
}

// steps 1 and 2: the unit normal u of triplet t's plane over the n >= 3 staged slots; false where the triplet is not valid
__device__ __forceinline__ bool hough_triplet(const float (&xyz)[3][NESTI_KNN_MAX_K], int n, unsigned long long seed, unsigned key, int t,
                                              double cx, double cy, double cz, double (&u)[3]) {
  const unsigned long long h0 = subsample_hash(seed, key, 0u, 3u * (unsigned)t);
  const unsigned long long h1 = subsample_hash(seed, key, 0u, 3u * (unsigned)t + 1u);
  const unsigned long long h2 = subsample_hash(seed, key, 0u, 3u * (unsigned)t + 2u);
  const int i0 = (int)((h0 * (unsigned long long)n) >> 32);
  int j = (int)((h1 * (unsigned long long)(n - 1)) >> 32);
  const int i1 = j + (j >= i0 ? 1 : 0);
  const int lo = min(i0, i1), hi = max(i0, i1);
  j = (int)((h2 * (unsigned long long)(n - 2)) >> 32);
  j += (j >= lo ? 1 : 0);
  const int i2 = j + (j >= hi ? 1 : 0);
  const double ax = (double)xyz[0][i0] - cx, ay = (double)xyz[1][i0] - cy, az = (double)xyz[2][i0] - cz;
  const double bx = (double)xyz[0][i1] - cx, by = (double)xyz[1][i1] - cy, bz = (double)xyz[2][i1] - cz;
  const double gx = (double)xyz[0][i2] - cx, gy = (double)xyz[1][i2] - cy, gz = (double)xyz[2][i2] - cz;
  const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
  const double e2x = gx - ax, e2y = gy - ay, e2z = gz - az;
  const double vx = e1y * e2z - e1z * e2y, vy = e1z * e2x - e1x * e2z, vz = e1x * e2y - e1y * e2x;
  const double l1 = knn_d2(e1x, e1y, e1z), l2 = knn_d2(e2x, e2y, e2z), qq = knn_d2(vx, vy, vz);
  const bool valid = qq > 0x1p-20 * (l1 * l2);
  const double len = sqrt(qq);
  u[0] = vx / len; u[1] = vy / len; u[2] = vz / len;
  return valid;
}

// step 3 under one rotation (nine fp64, uniform): the bin of u in the B x B hemi-octahedral accumulator, and the sign that took the
// rotated vector to the upper hemisphere
__device__ __forceinline__ int hough_bin(const double* rot, const double (&u)[3], int B, double& sigma) {
  double wx = (rot[0] * u[0] + rot[1] * u[1]) + rot[2] * u[2];
  double wy = (rot[3] * u[0] + rot[4] * u[1]) + rot[5] * u[2];
  double wz = (rot[6] * u[0] + rot[7] * u[1]) + rot[8] * u[2];
  const double lead = wz != 0.0 ? wz : (wy != 0.0 ? wy : wx);
  sigma = lead < 0.0 ? -1.0 : 1.0;
  wx = sigma * wx; wy = sigma * wy; wz = sigma * wz;
  const double m = (fabs(wx) + fabs(wy)) + wz;
  const double a = wx / m, b = wy / m;
  const double half = (double)B / 2.0;
  const int bi = min(max((int)floor(((a + b) + 1.0) * half), 0), B - 1);
  const int bj = min(max((int)floor(((a - b) + 1.0) * half), 0), B - 1);
  return bi * B + bj;
}

__global__ __launch_bounds__(kThreads) void hough_nbr_kernel(const HoughParams hp) {
  __shared__ HoughShared sh;
  constexpr int S = NESTI_MAX_SCALES;                         // ks[] is padded with its last entry: one kernel for every number of scales
  const NbrParams& np = hp.np;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= np.p.M) return;                                    // whole waves leave: the shuffles below see full waves
  float (&xyz)[3][NESTI_KNN_MAX_K] = sh.xyz[threadIdx.x >> 6];
  int* count = sh.count[threadIdx.x >> 6];
  const float* centre = query_centre(np.p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const double cx = cf0, cy = cf1, cz = cf2;
  int j[kNbrTrips], ns[S];
  nbr_row<S>(np, q, lane, centre_lost(cf0, cf1, cf2), j, ns);
  // ---- the radius of every scale, as plane_fit_nbr forms it, and the coordinates into LDS -------------------------------------------
  double r2s[S];
#pragma unroll
  for (int s = 0; s < S; ++s) r2s[s] = 0.0;
  walk_list(np.p.cloud, j, ns[S - 1], lane, cx, cy, cz, [&](int i, double, double, double, double d2) {
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (i < ns[s]) r2s[s] = fmax(r2s[s], d2);
  });
#pragma unroll
  for (int t = 0; t < kNbrTrips; ++t) {
    const int i = lane + t * kWave;                           // i < n <= NESTI_KNN_MAX_K, and j[t] lies in [0, N): nbr_row
    if (i < ns[S - 1]) {
      const float* pt = np.p.cloud + (size_t)j[t] * 3;
      xyz[0][i] = pt[0]; xyz[1][i] = pt[1]; xyz[2][i] = pt[2];
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) r2s[s] = wave_max(r2s[s]);
  const int n_scales = np.p.S, T = hp.T, B = hp.B;
  const int bins = B * B, counters = hp.R * bins;             // <= kMaxCounters: checked on the host
  const unsigned key = (unsigned)(np.p.row0 + q);
  const unsigned long long seed = np.p.seed;
#pragma unroll 1
  for (int s = 0; s < n_scales; ++s) {
    int n = ns[0];
    double r2 = r2s[0];
#pragma unroll
    for (int k = 1; k < S; ++k)
      if (k == s) { n = ns[k]; r2 = r2s[k]; }
    n = uniform(n);
    int win = 0, valid = 0;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (n >= 3) {
      for (int i = lane; i < counters; i += kWave) count[i] = 0;
      wave_lds_fence();                                       // the coordinates (first scale) and the cleared counters
      // ---- pass 1: every triplet votes once per rotation ------------------------------------------------------------------------------
      int nvalid = 0;
#pragma unroll 1
      for (int t = lane; t < T; t += kWave) {
        double u[3], sigma;
        if (hough_triplet(xyz, n, seed, key, t, cx, cy, cz, u)) {
          ++nvalid;
#pragma unroll 1
          for (int rho = 0; rho < hp.R; ++rho) atomicAdd(&count[rho * bins + hough_bin(hp.rot + rho * 9, u, B, sigma)], 1);
        }
      }
      valid = wave_sum(nvalid);
      wave_lds_fence();
      // ---- the winner: the largest count, among equals the smallest flat index rho B^2 + bin ------------------------------------------
      int best = 0;
      for (int i = lane; i < counters; i += kWave) best = max(best, (count[i] << 16) | (0xffff - i));
      best = uniform(wave_max(best));
      win = best >> 16;
      const int flat = 0xffff - (best & 0xffff);
      const int rho = uniform(flat / bins), bin = flat - rho * bins;
      wave_lds_fence();                                       // the counters are read before the next scale clears them
      // ---- pass 2: the winner's triplets under rho* ------------------------------------------------------------------------------------
      double X = 0.0, Y = 0.0, Z = 0.0;
      if (win > 0) {
#pragma unroll 1
        for (int t = lane; t < T; t += kWave) {
          double u[3], sigma;
          if (hough_triplet(xyz, n, seed, key, t, cx, cy, cz, u) && hough_bin(hp.rot + rho * 9, u, B, sigma) == bin) {
            X = X + sigma * u[0]; Y = Y + sigma * u[1]; Z = Z + sigma * u[2];
          }
        }
      }
      X = wave_sum(X); Y = wave_sum(Y); Z = wave_sum(Z);
      const double nn = (X * X + Y * Y) + Z * Z;
      if (win > 0 && nn > 0.0 && nn < INFINITY) {
        const double len = sqrt(nn);
        fx = (float)(X / len); fy = (float)(Y / len); fz = (float)(Z / len);
        const float lead = fz != 0.f ? fz : (fy != 0.f ? fy : fx);
        if (lead < 0.f) { fx = -fx; fy = -fy; fz = -fz; }
        fx = fx + 0.f; fy = fy + 0.f; fz = fz + 0.f;          // -0 + +0 = +0: no negative zero leaves
      } else {
        win = 0;
      }
    }
    if (lane == 0) {
      const size_t o = (size_t)q * n_scales + s;
      if (hp.normals_out) { hp.normals_out[o * 3] = fx; hp.normals_out[o * 3 + 1] = fy; hp.normals_out[o * 3 + 2] = fz; }
      if (hp.conf_out) hp.conf_out[o] = win > 0 ? (float)((double)win / (double)valid) : 0.f;
      if (hp.votes_out) { hp.votes_out[o * 2] = win; hp.votes_out[o * 2 + 1] = valid; }
      if (np.radius_out) np.radius_out[o] = (float)sqrt(r2);
      if (np.count_out) np.count_out[o] = n;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

// nesti_hough_normals_nbr and nesti_hough_normals_nbr_at: one body
int hough_nbr_impl(const char* who, bool at, const float* cloud_dev, int N, const int32_t* query_idx_dev, const float* query_xyz_dev,
                   int M, int query_row0, const int32_t* nbr_dev, int K, const int32_t* ks, int S, int T, int B, int R, const double* rot,
                   uint64_t seed, float* normals_out_dev, float* conf_out_dev, int32_t* votes_out_dev, float* radius_out_dev,
                   int32_t* count_out_dev, void* stream) {
  const std::string w(who);
  HoughParams hp;
  if (nbr_params_fill(w, at, &hp.np, cloud_dev, N, query_idx_dev, query_xyz_dev, M, query_row0, nbr_dev, K, ks, S, radius_out_dev,
                      count_out_dev))
    return 1;
  if (T < 1 || T > NESTI_HOUGH_MAX_T) NESTI_FAIL(w + ": T (triplets) must be in 1 .. " + std::to_string(NESTI_HOUGH_MAX_T));
  if (B < 2 || B > NESTI_HOUGH_MAX_BINS) NESTI_FAIL(w + ": B (bins per axis) must be in 2 .. " + std::to_string(NESTI_HOUGH_MAX_BINS));
  if (R < 1 || R > NESTI_HOUGH_MAX_ROT) NESTI_FAIL(w + ": R (rotations) must be in 1 .. " + std::to_string(NESTI_HOUGH_MAX_ROT));
  if (!rot) NESTI_FAIL(w + ": null rot");
  for (int r = 0; r < R; ++r) {
    const double* m = rot + r * 9;
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(m[k])) NESTI_FAIL(w + ": rotation " + std::to_string(r) + " is not finite");
    double err = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double dot = m[a * 3] * m[b * 3] + m[a * 3 + 1] * m[b * 3 + 1] + m[a * 3 + 2] * m[b * 3 + 2];
        err = std::fmax(err, std::fabs(dot - (a == b ? 1.0 : 0.0)));
      }
    if (!(err <= 1e-6)) NESTI_FAIL(w + ": rotation " + std::to_string(r) + " is not orthonormal (max |rot rot^T - I| > 1e-6)");
  }
  if (M == 0) return 0;
  hp.np.p.seed = seed;
  hp.T = T; hp.B = B; hp.R = R;
  memset(hp.rot, 0, sizeof(hp.rot));
  memcpy(hp.rot, rot, sizeof(double) * 9 * (size_t)R);
  hp.normals_out = normals_out_dev;
  hp.conf_out = conf_out_dev;
  hp.votes_out = votes_out_dev;
  return launch_wave_rows(hough_nbr_kernel, hp, M, stream);
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_hough_normals_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                            int K, const int32_t* ks, int S, int T, int B, int R, const double* rot, uint64_t seed,
                            float* normals_out_dev, float* conf_out_dev, int32_t* votes_out_dev, float* radius_out_dev,
                            int32_t* count_out_dev, void* stream) {
  return hough_nbr_impl("nesti_hough_normals_nbr", false, cloud_dev, N, query_idx_dev, nullptr, M, query_row0, nbr_dev, K, ks, S, T, B, R,
                        rot, seed, normals_out_dev, conf_out_dev, votes_out_dev, radius_out_dev, count_out_dev, stream);
}

int nesti_hough_normals_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, int query_row0, const int32_t* nbr_dev,
                               int K, const int32_t* ks, int S, int T, int B, int R, const double* rot, uint64_t seed,
                               float* normals_out_dev, float* conf_out_dev, int32_t* votes_out_dev, float* radius_out_dev,
                               int32_t* count_out_dev, void* stream) {
  return hough_nbr_impl("nesti_hough_normals_nbr_at", true, cloud_dev, N, nullptr, query_xyz_dev, M, query_row0, nbr_dev, K, ks, S, T, B,
                        R, rot, seed, normals_out_dev, conf_out_dev, votes_out_dev, radius_out_dev, count_out_dev, stream);
}

}  // extern "C"
