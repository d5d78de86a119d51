// Plane-fit (PCA) normals and surface variation at every patch scale ("Plane-fit normals"): the classical estimator, the
// first row of the paper's comparison tables and the frame of the reference dataset's use_pca step (utils/pcpnet_dataset.py:357-377,
// which the test path never takes).  It needs no model and no weights.
//
// Per query and scale s, over the FULL ball B_s = {p : d2(p, c) <= r_s^2} of the search grid (patches.hip; the fp64 ball test
// ball_d2 of patches_dev.h, not capped at P and not subsampled), with d = (double)p - (double)c:
//     n = |B_s|,  m = (sum d) / n,  C = ((sum d d^T) / n - m m^T) / r_s^2          (units of r^2: eigenvalues are scale-free, <= 1)
//     (w, V) = sym3_eig(C)  (pca_eig.h: cyclic Jacobi, fp64, fixed sweeps),  w ascending
//     normal  = V[0] normalised in fp64, rounded to f32 once, then signed ON THE F32 VALUES so that the first non-zero of
//               (n_z, n_y, n_x) is positive (the rule orient.hip uses for a tree root); zeros are written as +0
//     eig     = (float)max(0, w_k)
// A scale with n < 3 writes normal 0 0 0 and eigenvalues 0 0 0 (the count is still written): an empty ball, a lone point, and every
// scale of a query whose position is not finite (it visits no cell, so n = 0).
//
// One wave per query, four queries per workgroup (the candidates of a query are a few thousand float4: ~50 trips per lane; no LDS, no
// barrier; the nine fp64 sums and the count of a scale are each reduced by one fixed xor-butterfly of wave shuffles).  A candidate is tested once for all
// scales: the six products of d are formed once and added to the sums of every scale whose ball holds it.  Lane s then solves scale s.
//
// DETERMINISM.  No floating-point atomics and no dependence on which workgroup runs first: candidate i of a span goes to lane
// (i - span begin) mod 64 and the lanes meet in a fixed tree, so for ONE prepared grid a row's outputs are identical bits however the
// rows are batched.  The cell-ordered copy of the cloud is filled through an atomic cursor (patches.hip: fill_kernel): the order inside
// a cell, and with it the last bits of an fp64 sum, may differ between two grid builds.  Across grid builds the outputs agree to the
// bounds of tests/test_gpu_pca.py (counts exactly), no more is promised.
#include <string.h>

#include <cmath>
#include <string>

#include "kernels.h"
// before the pragma below, like patches.hip and mups.hip: the ball of a scale is then the patch kernels' ball, whose d2 hipcc forms
// with two FMAs (ball_d2, patches_dev.h)
#include "patches_dev.h"

// every product and sum below -- the solver of pca_eig.h included -- is rounded on its own, on the host (nesti_sym3_eig) as on the
// device: the CPU restatement (tests/_pca_fixture.py) bounds each step
#pragma clang fp contract(off)

#include "pca_dev.h"     // the fit itself, shared with pass 1 of quadric.hip

namespace nesti {
namespace {

struct PcaParams {
  PatchParams p;                      // points_out / n_eff_out / nbr_out unused; n_ball_out optional
  float* normals_out;                 // [M, S, 3] or NULL
  float* eig_out;                     // [M, S, 3] or NULL
};

template <int S>
__global__ __launch_bounds__(kThreads) void pca_kernel(const PcaParams pp) {
  const PatchParams& p = pp.p;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = wave_row();
  if (q >= p.M) return;                                       // whole waves leave: the shuffles below see full waves
  const float* centre = query_centre(p, q);
  const float cf0 = centre[0], cf1 = centre[1], cf2 = centre[2];
  const WaveSpans spans = wave_spans(p, lane, cf0, cf1, cf2);
  double sum[kSums];
  int n;
  double r2;
  plane_sums<S>(p, spans, lane, (double)cf0, (double)cf1, (double)cf2, sum, n, r2);
  if (lane >= S) return;                                      // lane s solves scale s
  float nrm[3], ev[3];
  plane_solve(sum, n, r2, nrm, ev);
  const size_t o = (size_t)q * S + lane;
  if (pp.normals_out) { pp.normals_out[o * 3] = nrm[0]; pp.normals_out[o * 3 + 1] = nrm[1]; pp.normals_out[o * 3 + 2] = nrm[2]; }
  if (pp.eig_out) { pp.eig_out[o * 3] = ev[0]; pp.eig_out[o * 3 + 1] = ev[1]; pp.eig_out[o * 3 + 2] = ev[2]; }
  if (p.n_ball_out) p.n_ball_out[o] = n;
}

// nesti_pca_normals (centres = cloud points, by index or row) and nesti_pca_normals_at (centres = positions): one body
int pca_impl(const char* who, bool at, const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev,
             const float* query_xyz_dev, int M, const double* r_abs, int query_row0, float* normals_out_dev, float* eig_out_dev,
             int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  const std::string w(who);
  if (refuse_grid_cloud(w, cfg, cloud_dev, N, r_abs, grid_ws_dev, grid_ws_bytes)) return 1;
  if (M < 0) NESTI_FAIL(w + ": M must be >= 0");
  if (refuse_query_rows(w, N, !at && !query_idx_dev, M, query_row0)) return 1;
  if (M == 0) return 0;
  if (at && !query_xyz_dev) NESTI_FAIL(w + ": null query_xyz_dev");
  PcaParams pp;
  patch_params_fill(&pp.p, cfg, cloud_dev, N, query_idx_dev, M, r_abs, 0, query_row0, grid_ws_dev);
  pp.p.query_xyz = at ? query_xyz_dev : nullptr;
  pp.p.n_ball_out = n_ball_out_dev;
  pp.normals_out = normals_out_dev;
  pp.eig_out = eig_out_dev;
  return with_scales(cfg->n_scales, [&](auto s) { return launch_wave_rows(pca_kernel<decltype(s)::value>, pp, M, stream); });
}

}  // namespace
}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_pca_normals(const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                      const double* r_abs, int query_row0, float* normals_out_dev, float* eig_out_dev, int32_t* n_ball_out_dev,
                      const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  return pca_impl("nesti_pca_normals", false, cfg, cloud_dev, N, query_idx_dev, nullptr, M, r_abs, query_row0, normals_out_dev,
                  eig_out_dev, n_ball_out_dev, grid_ws_dev, grid_ws_bytes, stream);
}

int nesti_pca_normals_at(const nesti_config_t* cfg, const float* cloud_dev, int N, const float* query_xyz_dev, int M,
                         const double* r_abs, int query_row0, float* normals_out_dev, float* eig_out_dev, int32_t* n_ball_out_dev,
                         const void* grid_ws_dev, size_t grid_ws_bytes, void* stream) {
  return pca_impl("nesti_pca_normals_at", true, cfg, cloud_dev, N, nullptr, query_xyz_dev, M, r_abs, query_row0, normals_out_dev,
                  eig_out_dev, n_ball_out_dev, grid_ws_dev, grid_ws_bytes, stream);
}

int nesti_sym3_eig(const double c[6], double w[3], double v[9]) {
  if (!c || !w || !v) NESTI_FAIL("nesti_sym3_eig: null argument");
  const double cc[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
  double ww[3], vec[3][3];
  sym3_eig(cc, ww, vec);
  for (int k = 0; k < 3; ++k) {
    w[k] = ww[k];
    for (int i = 0; i < 3; ++i) v[3 * k + i] = vec[k][i];
  }
  return 0;
}

}  // extern "C"
