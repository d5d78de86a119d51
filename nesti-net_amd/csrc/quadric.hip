// Quadric-fit normals and principal curvatures at every patch scale (DESIGN.md 2 "Quadric fit"): the osculating-jet estimator of
// Cazals and Pouget at degree 2, the second row of the paper's comparison tables, and the source of the per-point principal curvatures
// the reference's data layer reads from <shape>.curv (utils/pcpnet_dataset.py:260-263, 349-352, 410-413).  No model, no weights.
//
// Per query centre c and scale s (radius r), over the FULL ball of nesti_pca_normals (fp64 ball_d2 <= r^2, not capped, not subsampled),
// with d = (double)p - (double)c and n the ball size:
//   1  n0 = the plane-fit normal of that ball exactly as nesti_pca_normals returns it (pca_dev.h: rounded to f32, signed), taken back
//      to fp64 and not renormalised; it is an output too (plane_out)
//   2  frame from n0 alone: j = the index of the smallest |n0_j| (ties: x, y, z), t1 = (n0 x e_j) / |n0 x e_j|, t2 = n0 x t1
//   3  (u, v, h) = ((t . d) / r) for t = t1, t2, n0, the dot product bracketed (tx dx + ty dy) + tz dz; phi = (1, u, v, u^2, u v, v^2)
//   4  the moments m[0..14] = sum u^p v^q (p + q <= 4), m[15..20] = sum h phi_i, m[0] = n.  The monomials are formed as
//      u2 = u u, uv = u v, v2 = v v, u3 = u2 u, u2v = u2 v, uv2 = u v2, v3 = v2 v, u4 = u2 u2, u3v = u3 v, u2v2 = u2 v2, uv3 = u v3,
//      v4 = v2 v2, and h u, h v, h u2, h uv, h v2
//   5  N a = b by Cholesky with a pivot threshold (quadric_solve.h); the fit FAILS if n < 6, if n0 is the zero row, if a pivot fails
//      or if a coefficient is not finite
//   6  nu = (n0 - a1 t1) - a2 t2, normalised in fp64, rounded to f32 once, zeros +0.  nu . n0 > 0; no second sign rule
//   7  curvatures from the shape operator in an orthonormal tangent basis (quadric_solve.h), divided by r: absolute units, k_max >= k_min,
//      positive where the surface bends toward nu
//   8  a failed fit writes nu = 0 0 0 and k = 0 0 (so does one whose nu or k would not be finite, which takes an overflow);
//      plane_out and n_ball are written as nesti_pca_normals writes them
//
// One wave per query, four queries per workgroup, like pca_kernel.  Pass 1 is pca_kernel's (pca_dev.h).  Lane s then holds n0 of scale
// s; it is read from there into scalar registers and every lane builds the same frame.  Pass 2 walks the same spans again and adds the
// 20 fp64 sums of every scale whose ball holds the candidate; the totals come from the fixed xor-butterfly and lane s solves scale s.
//
// DETERMINISM, as in pca.hip: no floating-point atomics, no LDS; candidate i of a span goes to lane (i - span begin) mod 64 and the
// lanes meet in a fixed tree, so for ONE prepared grid a row's bits do not depend on batching, streams or partition.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
// before the pragma below, like pca.hip: the ball is the plane fit's ball (ball_d2, patches_dev.h)
#include "patches_dev.h"

// every product and sum below -- the plane fit of pca_dev.h and the solve of quadric_solve.h included -- is rounded on its own, on the
// host (nesti_quadric_solve) as on the device: the CPU restatement (tests/_quadric_fixture.py) bounds each step
#pragma clang fp contract(off)

#include "pca_dev.h"
#include "quadric_dev.h"  // the frames, the per-candidate body, the totals and the solve, shared with the neighbour-list kernel of knn.hip

namespace nesti {
namespace {

struct QuadricParams {
  PatchParams p;                      // points_out / n_eff_out / nbr_out unused; n_ball_out optional
  double r[NESTI_MAX_SCALES];         // the radii themselves: (t . d) / r
  float* normals_out;                 // [M, S, 3] or NULL
  float* curv_out;                    // [M, S, 2] or NULL
  float* plane_out;                   // [M, S, 3] or NULL
};

template <int S>
__global__ __launch_bounds__(kThreads) void quadric_kernel(const QuadricParams qp) {
  const PatchParams& p = qp.p;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= p.M) return;                                       // whole waves leave: the shuffles below see full waves
  const float* centre = query_centre(p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const WaveSpans spans = wave_spans(p, lane, cf0, cf1, cf2);
  const double cx = cf0, cy = cf1, cz = cf2;
  // ---- pass 1: the plane fit; lane s solves scale s ---------------------------------------------------------------------------------
  int n;
  float nrm[3], ev[3];
  {
    double sum[kSums], r2;
    plane_sums<S>(p, spans, lane, cx, cy, cz, sum, n, r2);
    plane_solve(sum, lane < S ? n : 0, r2, nrm, ev);
  }
  // ---- the frame of every scale, the same in every lane.  A scale that cannot be fitted (n < 6, or no plane normal) gets a ball
  // nothing is inside of, so pass 2 adds nothing for it
  double fr[S][9], r2live[S], rad[S];
  bool live[S];
  quadric_frames<S>(nrm, n, fr, live);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    r2live[s] = live[s] ? p.r2[s] : -1.0;
    rad[s] = qp.r[s];
  }
  // ---- pass 2: the moments ------------------------------------------------------------------------------------------------------------
  double acc[S][kQSums];
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int k = 0; k < kQSums; ++k) acc[s][k] = 0.0;
  }
  walk_block(p.sorted, spans, lane, kWave, cx, cy, cz, [&](const float4& c, double d2) {
    const double dx = (double)c.x - cx, dy = (double)c.y - cy, dz = (double)c.z - cz;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (d2 <= r2live[s]) quadric_add(acc[s], fr[s], rad[s], dx, dy, dz);
    }
  });
  // every lane ends up with every total; lane s keeps those, the frame and the radius of scale s
  double m[kQuadricMoments], f[9], r = 1.0;
#pragma unroll
  for (int k = 0; k < kQuadricMoments; ++k) m[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) quadric_totals(acc[s], fr[s], rad[s], lane == s, m, f, r);
  if (lane >= S) return;
  // ---- lane s: solve, normal, curvatures ------------------------------------------------------------------------------------------------
  quadric_solve_write(m, f, r, n, nrm, (size_t)q * S + lane, QuadricOut{qp.normals_out, qp.curv_out, qp.plane_out, p.n_ball_out});
}

// nesti_quadric_fit (centres = cloud points, by index or row) and nesti_quadric_fit_at (centres = positions): one body
int quadric_impl(const char* who, bool at, const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev,
                 const float* query_xyz_dev, int M, const double* r_abs, int query_row0, float* normals_out_dev, float* curv_out_dev,
                 float* plane_out_dev, int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  const std::string w(who);
  if (refuse_grid_cloud(w, cfg, cloud_dev, N, r_abs, grid_ws_dev, grid_ws_bytes)) return 1;
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (refuse_query_rows(w, N, !at && !query_idx_dev, M, query_row0)) return 1;
  if (M == 0) return 0;
  if (at && !query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev");
  QuadricParams qp;
  patch_params_fill(&qp.p, cfg, cloud_dev, N, query_idx_dev, M, r_abs, 0, query_row0, grid_ws_dev);
  qp.p.query_xyz = at ? query_xyz_dev : nullptr;
  qp.p.n_ball_out = n_ball_out_dev;
  for (int s = 0; s < NESTI_MAX_SCALES; ++s) qp.r[s] = s < cfg->n_scales ? r_abs[s] : 1.0;
  qp.normals_out = normals_out_dev;
  qp.curv_out = curv_out_dev;
  qp.plane_out = plane_out_dev;
  return with_scales(cfg->n_scales, [&](auto s) { return launch_wave_rows(quadric_kernel<decltype(s)::value>, qp, M, stream); });
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_quadric_fit(const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                      const double* r_abs, int query_row0, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                      int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  return quadric_impl("nesti_quadric_fit", false, cfg, cloud_dev, N, query_idx_dev, nullptr, M, r_abs, query_row0, normals_out_dev,
                      curv_out_dev, plane_out_dev, n_ball_out_dev, grid_ws_dev, grid_ws_bytes, stream);
}

int nesti_quadric_fit_at(const nesti_config_t* cfg, const float* cloud_dev, int N, const float* query_xyz_dev, int M,
                         const double* r_abs, int query_row0, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                         int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  return quadric_impl("nesti_quadric_fit_at", true, cfg, cloud_dev, N, nullptr, query_xyz_dev, M, r_abs, query_row0, normals_out_dev,
                      curv_out_dev, plane_out_dev, n_ball_out_dev, grid_ws_dev, grid_ws_bytes, stream);
}

int nesti_quadric_solve(const double m[21], double a[6], double k[2], int* ok) {
  if (!m || !a || !k || !ok) NESTI_FAIL("nesti_quadric_solve: null argument");
  double mm[kQuadricMoments], aa[kQuadricCoeffs], kk[2] = {0.0, 0.0};
  for (int i = 0; i < kQuadricMoments; ++i) mm[i] = m[i];
  bool fitted = quadric_solve(mm, aa);
  if (fitted) {
    quadric_curvatures(aa, kk);
    if (!std::isfinite(kk[0]) || !std::isfinite(kk[1])) {     // an overflow: a failed fit like any other
      fitted = false;
      kk[0] = kk[1] = 0.0;
      for (int i = 0; i < kQuadricCoeffs; ++i) aa[i] = 0.0;
    }
  }
  for (int i = 0; i < kQuadricCoeffs; ++i) a[i] = aa[i];
  k[0] = kk[0];
  k[1] = kk[1];
  *ok = fitted ? 1 : 0;
  return 0;
}

}  // extern "C"
