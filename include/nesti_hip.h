/*
 * nesti_hip.h -- C-ABI of libnesti_hip.so: the MI355X (gfx950) implementation of
 * Nesti-Net's per-point inference hot path.
 *
 * The reference (sitzikbs/Nesti-Net, Python 2.7 + TF 1.12) has no FFI or operator
 * registry; its seams are Python call sites.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - every `*_dev` pointer is a caller-owned DEVICE pointer (e.g. torch tensor
 *     .data_ptr()); the library never allocates outputs or frees inputs;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     launches are asynchronous on it and no call synchronises the device
 *     unless stated;
 *   - return value 0 = ok, non-zero = error; nesti_last_error() returns a
 *     thread-local message for the last failing call on this thread;
 *   - model handles are immutable after creation (except the NESTI_F16X3C gate margin, which must not be changed while
 *     forward calls are in flight, and its device-side counters, which forward calls update atomically): concurrent
 *     forward calls on different streams are safe provided they use different workspaces.  In the default mode those
 *     counters also DECIDE: the gate margin and the conditioning guard's threshold follow what a model has measured, so the
 *     outputs of a NESTI_F16X3C / NESTI_F16X8 / NESTI_F16X8C model depend on the calls it has seen since its counters were
 *     reset.  nesti_model_set_reproducible (below) freezes both thresholds: the counters then only measure, and a query's
 *     outputs are a function of the weights, the thresholds, the cloud, the seed and its patch row.
 */
#ifndef NESTI_HIP_H
#define NESTI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NESTI_MAX_SCALES 4
#define NESTI_KNN_MAX_K 256   /* the largest K of nesti_knn and of a neighbour list (nesti_*_nbr) */
#define NESTI_HOUGH_MAX_T 4096   /* nesti_hough_normals_nbr: the most triplets per row and scale, */
#define NESTI_HOUGH_MAX_BINS 16  /* ... bins per axis of the accumulator */
#define NESTI_HOUGH_MAX_ROT 8    /* ... and rotations of it */
#define NESTI_SELECT_MAX_L 32    /* nesti_pca_select_nbr: the most neighbour counts of a ladder */
#define NESTI_ROBUST_MAX_ITERS 64 /* nesti_robust_normals_nbr: the most re-weighting iterations of a call */
#define NESTI_MAX_EXPERTS 8
#define NESTI_MUPS_CH 20 /* channels per scale: utils/tf_util.py:711-720 */

/* element types for activations / weights.  NESTI_BF16X3 / NESTI_F16X3 are MODEL dtypes only (nesti_model_create):
 * activations and weights are kept as a 16-bit (hi, lo) pair, v ~ hi + lo, and every multiply is the three 16-bit MFMA
 * products hi*hi + lo*hi + hi*lo accumulated in fp32 -- a third of the 16-bit rate instead of the fp32 MFMA rate.
 * bf16 pairs hold 2^-17 relative; f16 pairs hold max(2^-23 relative, 3e-8 absolute) with the weights of each layer scaled
 * by a power of two into f16's normal range (undone in the epilogue): the mode that keeps test_n_est_w_experts.py's outputs
 * within the 1e-5 cosine / arg-max tolerance with two orders of magnitude to spare. */
enum { NESTI_F32 = 0, NESTI_BF16 = 1, NESTI_F16 = 2, NESTI_BF16X3 = 3, NESTI_F16X3 = 4, NESTI_F16X3C = 5, NESTI_F16X8 = 6, NESTI_F16X8C = 7 };
/* NESTI_F16X3C ("cascade", MODEL dtype only, gated models): everything that reaches the outputs is computed as in
 * NESTI_F16X3 -- the experts, and the gating net for every query whose decision could depend on it -- but the gating net
 * first runs in plain f16 as a FILTER (plain f16 activations and tap layers; its 1x1x1 / FC layers, which are fill-bound, multiply
 * by the exact pair-packed weights -- two products -- which halves the filter's error variance for a third more time in those
 * layers): a query whose top-2 logit margin in that pass is at least the gate margin tau keeps its arg-max (a flip would need a
 * filter error of tau), every other query is decided again by the f16x3 gating net.
 * expert_out / normals_out are then those of NESTI_F16X3 as long as the f16 gate's error on a logit difference stays below
 * the margin, which every call re-measures on the queries it decides twice and widens by itself when the measured error
 * comes within a factor NESTI_GATE_WIDEN of it (nesti_model_cascade_stats); probs_out carries the filter pass's probabilities
 * (within ~0.013 of NESTI_F16X3's) for the queries that were not re-decided. */

/* NESTI_F16X8 / NESTI_F16X8C (round 6; MODEL dtypes only, experts_n_est on the 8^3 grid): NESTI_F16X3 / NESTI_F16X3C with the two
 * CROSS terms of the pair scheme -- lo * W_hi + hi * W_lo, 2^-11 of a layer's result -- of the EXPERT towers' tap layers at 8^3
 * (models/experts_n_est.py:258-262: conv2 (3^3) and conv3 (5^3) of inception1 / inception2, 86 % of an expert's multiply-accumulates)
 * computed by one block-scaled MFMA of a narrow format (K = 64, fp32 accumulate into the same accumulator: FP6 e2m3 x e2m3 with one scale
 * per 16-channel block by default, or FP8 e4m3 x e4m3 with one scale per layer -- nesti_model_set_x8_format) instead of four f16 MFMAs;
 * hi * W_hi stays an exact f16 product.  The gating net -- filter AND recheck -- is untouched, so expert_out is NESTI_F16X3C's bit for
 * bit.  The normals differ from NESTI_F16X3's by a residual 28x below single-product f16 (1 - cos p50 6e-10, p99 2e-8), and the
 * queries on which that residual could matter -- expert outputs of very small norm -- are evaluated again in f16x3 proper by the
 * conditioning guard (nesti_model_set_x8_guard below): measured over 2.38 M queries of 32 clouds, max 1 - cos 5.8e-7 against f16x3,
 * none above 2.5e-6, 0.21 % of the outputs re-evaluated (profiles/r06_stream32_check.json), against the 1e-5 tolerance.  The e4m3
 * planes' power-of-two pre-scales come from the producing layer's folded batch-norm (|beta| + 8 |gamma|: a data-free bound on its
 * activations; larger values saturate at the format's 448 and lose only their own cross terms).
 * nesti_model_set_x8_layers picks the layers: bit 0 / 1 = inception1 conv2 (3^3) / conv3 (5^3), bit 2 / 3 = inception2 conv2 / conv3;
 * the default is 0b1111 (all four), 0b1010 keeps to the 5^3 layers, 0 is NESTI_F16X3 proper.  Must not be changed while forward calls
 * are in flight (declared below: nesti_model_set_x8_layers). */

/* which graph nesti_model_create builds */
enum {
  NESTI_ARCH_EXPERTS = 0, /* models/experts_n_est.py:40-108  (MoE, the hot path)    */
  NESTI_ARCH_SINGLE = 1,  /* models/ss_norm_est.py:35-92     (BASELINE config 0)    */
  NESTI_ARCH_MULTI = 2,   /* models/ms_norm_est.py:45-140    (multi-scale ablation) */
  NESTI_ARCH_SWITCH = 3   /* models/ms_sw_n_est.py:41-89     (noise-switched two-scale ablation):
                           * 2 scales; gate = noise_est_net on scale 1, tower 0 = 'small' (scale 0),
                           * tower 1 = 'large' (scale 1); n_experts / expert_scale_* are ignored      */
};

/* Hyper-parameters the reference reads from parameters.p / gmm.p
 * (test_n_est_w_experts.py:46-54, :201). */
typedef struct {
  int arch;                                /* NESTI_ARCH_*                                      */
  int n_scales;                            /* len(patch_radius)                                 */
  int points_per_scale;                    /* num_point (P)                                     */
  int grid_n;                              /* Gaussians per axis: 8, or 3 (experts_n_est only)  */
  double variance;                         /* gmm covariance (0.0156)                           */
  int n_experts;                           /* E                                                 */
  int expert_scale_lo[NESTI_MAX_EXPERTS];  /* min(expert_dict[i])   models/experts_n_est.py:100 */
  int expert_scale_cnt[NESTI_MAX_EXPERTS]; /* len(expert_dict[i])   models/experts_n_est.py:101 */
} nesti_config_t;

/* One named float32 host tensor in TF variable layout
 * (conv [kd,kh,kw,Cin,Cout] utils/tf_util.py:289; fc [In,Out] utils/tf_util.py:334). */
typedef struct {
  const char* name;
  const float* data; /* host pointer; may be NULL in nesti_model_describe output */
  int ndim;
  int64_t dims[5];
} nesti_tensor_t;

typedef struct nesti_model nesti_model_t;

const char* nesti_last_error(void);
const char* nesti_version(void);

/* Fill cfg with the published Nesti-Net configuration (3 radii, 8^3 Gaussians, variance 0.0156, 7 experts with the
 * expert_dict of train_n_est_w_experts.py:62) -- not the argparse defaults of that script (3^3 Gaussians). */
void nesti_default_config(nesti_config_t* cfg);

/* utils/utils.py:70-95 get_3d_grid_gmm: host arrays w[n^3], mu[n^3*3], sigma[n^3*3]
 * (sigma = sqrt(covariances_), as fed at test_n_est_w_experts.py:146). */
int nesti_gmm_grid(int n, double variance, float* w, float* mu, float* sigma);

/* utils/tf_util.py:655-753 get_3dmfv_n_est + models/experts_n_est.py:66-76 (MuPS
 * assembly) with the exact TF placeholder contract (models/experts_n_est.py:26-35):
 *   points_dev [B, S*P, 3] f32, n_eff_dev [B, S] int32
 *   out_dev    [B, R, R, R, out_cstride] of out_dtype; channel 20*s+c holds
 *              scale s, statistic c; channels >= 20*S are written as zero.
 * Rows whose n_eff is 0 (the zero-padded tail of the reference's last batch,
 * test_n_est_w_experts.py:134-140) are written as zeros instead of NaN.
 * out_dtype NESTI_BF16X3 / NESTI_F16X3: out_cstride is a multiple of 128 16-bit elements and channel c is stored as the planes
 * hi at 128*(c/64) + c%64 and lo 64 elements further (value = hi + lo).
 * INPUT DOMAIN.  Rows 0 .. min(n_eff, P-1) of a scale are read and must hold finite coordinates; rows beyond n_eff are never
 * read and may hold anything (NaN and infinities included).  The posterior is evaluated per axis, q_i = e_i / sum_i e_i with
 * e_i = expf(-((x - mu_i) / sigma)^2 / 2), so one axis of one point stays defined while at least one e_i is non-zero: the
 * float32 expf is 0 below about -103.97 (-87.34 where subnormal results are flushed), i.e. once the NEAREST centre is further
 * than sigma sqrt(2 x 87.34) = 13.2 sigma away.  With the outermost centre at 1 - 1/n that is
 *     8^3 grid, variance 0.0156 (sigma 0.125):  |x| > 0.875 + 13.2 x 0.125 = 2.52   (2.68 with subnormals)
 *     3^3 grid, variance 0.111  (sigma 0.333):  |x| > 0.667 + 13.2 x 0.333 = 5.07   (5.47 with subnormals)
 * The outputs are finite, and within the bound tests/_mups_fixture.py derives, for every coordinate in [-2, 2] on both grids
 * (the `outside` case of tests/test_gpu_mups_cases.py); the transcription of the reference's three-axis form in float32
 * (oracle/mups_ref.mups_literal) already gives NaN at the corners of that cube on the 8^3 grid.  The product path stays far inside:
 * the ball query keeps a patch coordinate (p - c) / r at norm <= 1 (up to its float32 rounding).  Beyond the figures above an
 * axis is 0 / 0 and the channels of that (row, scale) are not finite (this file is built without NaN semantics: unspecified). */
int nesti_mups_forward(const nesti_config_t* cfg, const float* points_dev,
                       const int32_t* n_eff_dev, int B, void* out_dev, int out_dtype,
                       int out_cstride, void* stream);

/* utils/pcpnet_dataset.py:286-343 __getitem__ (center='point', use_pca=False,
 * point_tuple=1) for M query points of one cloud, on the GPU:
 *   cloud_dev [N,3] f32; query_idx_dev [M] int32 (NULL = points query_row0..query_row0+M-1,
 *   the 'full' sampler utils/pcpnet_dataset.py:41-55); r_abs[S] = bbdiag*rad as double
 *   (utils/pcpnet_dataset.py:282), each positive and finite -- every entry below refuses another
 *   value with "radii must be positive and finite"; query_row0 = patch row of the first query within
 *   its shape (so the subsample below does not depend on how rows are batched).
 * Ball membership is the fp64 test scipy's cKDTree applies (:304).  When a ball
 * holds more than P points the P kept are those with the smallest
 * (hash(seed, query_row0+i, scale, index), index) keys -- a uniform P-subset like :320-321
 * but reproducible; see DESIGN.md.  Outputs (any may be NULL):
 *   points_out_dev [M,S*P,3] f32, n_eff_out_dev [M,S] int32,
 *   nbr_idx_out_dev [M,S*P] int32 (-1 padded), n_ball_out_dev [M,S] int32 (uncapped).
 * grid_ws_dev / grid_ws_bytes: scratch from nesti_patches_workspace_bytes(N). */
size_t nesti_patches_workspace_bytes(int N);
/* Step 1 (once per cloud; replaces the cKDTree build, utils/pcpnet_dataset.py:37): bounding
 * box, cell counts, scan and cell-ordered copy of the cloud into grid_ws_dev. */
int nesti_patches_grid(const nesti_config_t* cfg, const float* cloud_dev, int N,
                       const double* r_abs, void* grid_ws_dev, size_t grid_ws_bytes,
                       void* stream);
/* Step 2 (per batch of queries; replaces __getitem__, utils/pcpnet_dataset.py:286-343). */
int nesti_patches_query(const nesti_config_t* cfg, const float* cloud_dev, int N,
                        const int32_t* query_idx_dev, int M, const double* r_abs,
                        uint64_t seed, int query_row0, float* points_out_dev,
                        int32_t* n_eff_out_dev, int32_t* nbr_idx_out_dev,
                        int32_t* n_ball_out_dev, const void* grid_ws_dev,
                        size_t grid_ws_bytes, void* stream);
/* Step 2 for query POSITIONS: generalises utils/pcpnet_dataset.py:304, where the reference hands cKDTree.query_ball_point the
 * cloud point pts[center_point_ind] although the tree answers for any position.  Like nesti_patches_query with
 * query_xyz_dev [M,3] f32 (device) in place of query_idx_dev: query i's centre is query_xyz_dev[i], which need not be a cloud
 * point, may lie outside the cloud's bounding box and may be non-finite (its balls are then empty).  Everything else is
 * unchanged: the fp64 ball test, the f32 (p - c) / r, the subsample key hash(seed, query_row0 + i, scale, index) -- the patch
 * ROW, not the position, so results do not depend on batching -- and the key order.  query_row0 >= 0 is only that row.
 * EMPTY BALLS (the library's convention; the reference divides by zero there): a scale whose ball is empty has n_eff = 0
 * and all-zero patch rows, and contributes zero MuPS channels (as nesti_mups_forward writes for n_eff = 0); a query whose
 * balls are empty at EVERY scale has no neighbourhood, see nesti_mask_empty_queries. */
int nesti_patches_query_at(const nesti_config_t* cfg, const float* cloud_dev, int N,
                           const float* query_xyz_dev, int M, const double* r_abs,
                           uint64_t seed, int query_row0, float* points_out_dev,
                           int32_t* n_eff_out_dev, int32_t* nbr_idx_out_dev,
                           int32_t* n_ball_out_dev, const void* grid_ws_dev,
                           size_t grid_ws_bytes, void* stream);
/* Steps 1 + 2 in one call. */
int nesti_patches_build(const nesti_config_t* cfg, const float* cloud_dev, int N,
                        const int32_t* query_idx_dev, int M, const double* r_abs,
                        uint64_t seed, int query_row0, float* points_out_dev,
                        int32_t* n_eff_out_dev, int32_t* nbr_idx_out_dev,
                        int32_t* n_ball_out_dev, void* grid_ws_dev, size_t grid_ws_bytes,
                        void* stream);

/* ---- the reference's own subsample ORDER on the GPU (utils/pcpnet_dataset.py:304, 320-321) ----------------------------------
 * When a ball holds n > P points the reference keeps ball[rng.choice(n, P, replace=False)] of cKDTree's traversal-ordered ball.
 * query_ball_point returns a ball in ascending position in tree.indices, so the order is a sort key and the random stream only
 * needs the ball sizes:
 *   nesti_patches_count      n_ball_out_dev[M, S] = ball sizes of the queries (the count pass; nothing else is written);
 *   nesti_refstream_picks    (host, below) replays the shared RandomState over those sizes in visiting order -> pick table;
 *   nesti_patches_query_ref  the patch tensors exactly as PointcloudPatchDataset.__getitem__ builds them: per query the points
 *                            inside the largest ball are sorted in LDS by tree_rank_dev[i] (= position of point i in
 *                            tree.indices; tree_order_dev = tree.indices itself, both int32 [N], built on the host with
 *                            scipy.spatial.cKDTree(pts, 10) like utils/pcpnet_dataset.py:37), each scale's ball is taken in
 *                            that order, n <= P: as it is, rows beyond n zero; n > P: ball[picks] with the P uint16 picks at
 *                            picks_dev[pick_offsets_dev[q * S + s]] (offset -1: the ball holds <= P points).
 * A ball of more than nesti_patches_ref_max_ball() points does not fit the LDS sort: its n_eff comes back as -1 and its rows
 * zero -- callers hold the counts and must refuse such a shape before the launch (provider.CloudPatches does). */
int nesti_patches_count(const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                        const double* r_abs, int query_row0, int32_t* n_ball_out_dev, const void* grid_ws_dev,
                        size_t grid_ws_bytes, void* stream);
int nesti_patches_ref_max_ball(void);
int nesti_patches_query_ref(const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                            const double* r_abs, int query_row0, const int32_t* tree_rank_dev, const int32_t* tree_order_dev,
                            const uint16_t* picks_dev, const int64_t* pick_offsets_dev, float* points_out_dev,
                            int32_t* n_eff_out_dev, int32_t* nbr_idx_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes,
                            void* stream);

/* Enumerate the variables the graph for cfg expects (names follow the reference's
 * scopes, models/experts_n_est.py:155-314).  Call with infos=NULL to get the count. */
int nesti_model_describe(const nesti_config_t* cfg, int* n_tensors, nesti_tensor_t* infos,
                         int max_infos);

/* tf.train.Saver().restore equivalent (test_n_est_w_experts.py:98-105): takes the
 * float32 variables, folds the inference-mode batch norm (utils/tf_util.py:491-494)
 * into weights+bias, repacks for the MFMA kernels in `dtype` (any of the four element types) and uploads.
 * This call allocates device memory owned by the handle and synchronises. */
int nesti_model_create(const nesti_config_t* cfg, const nesti_tensor_t* tensors,
                       int n_tensors, int dtype, nesti_model_t** out);
void nesti_model_destroy(nesti_model_t* m);

/* ---- NESTI_F16X3C: the gate margin and the running statistics of the two-stage gate ---------------------------------
 * tau is in units of the gating net's last-layer outputs (the values softmax sees, models/experts_n_est.py:174-177).
 * The margin protects itself: a forward call filters with
 *     tau_eff = max(tau, NESTI_GATE_WIDEN x max_margin_err measured since the last reset)
 * and, after its own recheck rounds, re-decides the rows whose f16 margin lies between that threshold and NESTI_GATE_WIDEN x
 * the (possibly larger) error it has just measured -- up to NESTI_GATE_WIDEN_PASSES further, normally empty passes on the
 * device (each takes a snapshot of the largest error when it starts and covers the band up to NESTI_GATE_WIDEN x that, so an
 * error first seen inside a widening pass is covered by the next pass of the same call), no host synchronisation.  A row
 * keeps the f16 arg-max only while its margin is at least NESTI_GATE_WIDEN x the largest error the f16 gate has shown on any
 * row decided twice up to the start of the call's last widening pass.  The guarantee is per call: calls in flight on other
 * streams share the counters, and what they measure after this call's last snapshot protects this stream from its next
 * call on.
 * nesti_model_cascade_stats synchronises `stream`, copies the counters accumulated by every forward call since the last
 * reset and optionally resets them:
 *   queries        rows that went through the gate,
 *   rechecked      rows decided by the f16x3 gate (f16 top-2 margin below tau_eff, or caught by a widening round),
 *   changed        rechecked rows whose arg-max differs between the two gates,
 *   max_margin_err largest |(l_a - l_k)_f16 - (l_a - l_k)_f16x3| over the rechecked rows and all experts k, a = the f16
 *                  arg-max: the f16 gate's error on exactly the quantity tau guards,
 *   sum_sq_pair_err / pairs: the same errors squared and summed over all (rechecked row, k != a) pairs, and their count --
 *                  exactly the pairs summed: a pair with a non-finite logit on either side measures nothing and enters neither
 *                  max_margin_err nor the sum nor the count (a row with such a logit is always rechecked) --:
 *                  sqrt(sum / pairs) is the standard deviation sigma of the f16 pass's error on one logit difference (the
 *                  errors are rounding noise: zero-mean, independent of the margin); tau is chosen as a multiple of it,
 *   widened        rows re-decided by a widening pass, widen_events: widening passes that were not empty,
 *   tau_eff        the threshold the next forward call starts from. */
#define NESTI_GATE_WIDEN 1.5f
#define NESTI_GATE_WIDEN_PASSES 3
typedef struct {
  uint64_t queries, rechecked, changed;
  float max_margin_err;
  float tau;
  double sum_sq_pair_err;
  uint64_t pairs;
  uint64_t widened, widen_events;
  float tau_eff;
  /* recheck stage 2 (NESTI_F16X8C, below); all zero for NESTI_F16X3C */
  int stage2;                       /* 1: forward calls run it (format 6, not switched off) */
  uint64_t stage2_rows, stage2_decided, stage2_residual;
  float max_margin_err2, tau2, tau2_eff;
  double sum_sq_pair_err2;
  uint64_t pairs2;
  uint64_t stage2_widened, stage2_dropped;
} nesti_cascade_stats_t;
int nesti_model_set_gate_margin(nesti_model_t* m, float tau);
int nesti_model_cascade_stats(const nesti_model_t* m, nesti_cascade_stats_t* out, int reset, void* stream);
/* ---- NESTI_F16X8C: recheck stage 2 ------------------------------------------------------------------------------------
 * The rows the filter flags (`rechecked` above) are first decided by the gating net with its six k^3 tap layers at 8^3 in the
 * block-scaled FP6 cross-term form the experts' tap layers run (NESTI_DEBUG_FORM_X6; the planes come from the blocks' 1x1x1
 * launches) -- every other layer keeps the f16x3 form.  A row whose stage-2 top-2 logit margin is at least
 *     tau2_eff = max(tau2, NESTI_GATE_WIDEN x max_margin_err2 measured since the last reset)
 * is final; the others, and every row with a stage-2 logit that is not finite, are the RESIDUAL and go through the f16x3 gate
 * (stage 3) as before.  The residual rows are decided by both stages and measure the stage-2 error on a logit difference
 * against the stage-2 arg-max -- max_margin_err2, sum_sq_pair_err2 / pairs2 like their filter twins -- and after its rounds a
 * call passes the rows stage 2 decided inside [tau2_eff, NESTI_GATE_WIDEN x the error known by then) on to stage 3 as well
 * (stage2_widened; stage2_dropped: rows that round could not hold, 0 unless tau2 is absurd).  Every row's arg-max is therefore
 * decided by a pass whose measured error leaves a NESTI_GATE_WIDEN margin; the probabilities of a row stage 2 decides carry
 * that pass's error.  The filter's own error is measured on every rechecked row against the pass that decides it.
 * stage2_rows = stage2_decided + stage2_residual.  The reproducible mode freezes tau2 like tau, enqueues no widening round and
 * counts a residual row whose error would have widened the margin in gate_violations.
 * The stage runs once a second margin has been set (nesti_model_set_gate_margin2: calibrate.calibrate_gate_margin does it together
 * with tau; there is no default tau2 -- until one is set every flagged row is decided by the f16x3 gate, as without the stage) and
 * while the model's cross-term format is 6 (nesti_model_set_x8_format); nesti_model_set_gate_stage2(m, 0) switches it off -- forward
 * calls are then those of a model without it, launch by launch.  tau2 = +inf sends every flagged row
 * through both stages (what the calibration does to measure the error), tau2 = 0 lets stage 2 decide every row with finite logits.
 * The stage takes no workspace of its own: its rounds run inside the tower arena of the forward workspace, which the filter pass
 * over the whole batch (batches above 4096) or the f16x3 gate of a round sizes.  A round holds as many flagged rows as fit there
 * together with the block of FP6 planes, the residual list, its logits and the margins (nesti_debug_gate_stage2_plan): the
 * recheck's own round above 4096 rows, about 7/8 of the batch below; a batch too small for any round runs without the stage.
 * nesti_model_gate_error2_export / _import are the multi-GPU twins of the _gate_error_ pair below for max_margin_err2. */
typedef struct {
  int cap, rounds;        /* flagged rows per stage-2 round and rounds for a full flag list; cap 0: the stage does not run at this batch */
  int64_t tower_bytes;    /* the stage-2 gating net at `cap` rows (nesti_debug_tower_ops, tower -1, x8_mask 0x3F), at offset 0 of the arena */
  int64_t residual, logits2, margin2, end;   /* arena offsets of the residual list, its logits, the margins; end of the block */
  int64_t arena_offset, arena_bytes;          /* the tower arena inside the forward workspace */
} nesti_debug_stage2_t;
/* Where recheck stage 2 lives for a forward call of capacity `batch`; needs no device.  dtype without the stage: cap 0. */
int nesti_debug_gate_stage2_plan(const nesti_config_t* cfg, int dtype, int batch, nesti_debug_stage2_t* out);
int nesti_model_set_gate_margin2(nesti_model_t* m, float tau2);
int nesti_model_set_gate_stage2(nesti_model_t* m, int on);
int nesti_model_gate_error2_export(const nesti_model_t* m, float* dst_dev, void* stream);
int nesti_model_gate_error2_import(nesti_model_t* m, const float* src_dev, int n, void* stream);
/* Multi-GPU (no reference counterpart): every rank should filter with the largest error ANY rank has
 * measured.  _export writes this model's max_margin_err to dst_dev[0]; _import raises it to the largest finite value of
 * src_dev[0..n).  Both are one tiny kernel on `stream`, no host synchronisation: the value rides in a spare row of the
 * per-step all-gather (nesti-net_amd/dist.py) instead of a collective of its own. */
int nesti_model_gate_error_export(const nesti_model_t* m, float* dst_dev, void* stream);
int nesti_model_gate_error_import(nesti_model_t* m, const float* src_dev, int n, void* stream);

/* ---- REPRODUCIBLE MODE (off by default; no reference counterpart) ------------------------------------------------------------
 * on != 0 freezes the two thresholds that otherwise follow the model's measurements:
 *   - the two-stage gate filters with exactly tau (nothing folds max_margin_err in) and enqueues no widening pass;
 *   - the conditioning guard re-evaluates exactly the rows with |n| in [0, thr) and enqueues no further pass (thr < 0 still
 *     switches it off, +inf still re-evaluates everything).
 * Everything that MEASURES keeps running -- max_margin_err, the squared-pair sums, max_dn, the counts, the _import calls -- but no
 * decision reads a counter, so the three outputs of a query no longer depend on the batch, the stream, the lane, a captured graph
 * or the calls that came before.  tau_eff / thr_eff of the stats structs then report tau / thr.  What the default mode would have
 * ACTED on is counted instead, in a 64-byte device block of its own:
 *   gate_violations   rows decided twice whose NESTI_GATE_WIDEN x error exceeds the call's tau,
 *   guard_violations  rows re-evaluated whose NESTI_X8_GUARD_WIDEN x |dn| / sqrt(2 x NESTI_X8_GUARD_BAR) exceeds thr,
 * and a caller that wants today's 1.5 x guarantee raises tau / thr from the reported maxima and runs the WHOLE range again
 * (nesti-net_amd/pipeline.py: NormalEstimator.run_verified) -- each pass is then a function of (thresholds, query set).
 * Accepted on every model (a no-op without two-stage gate and guard); the frozen path has fewer launches than the default one and
 * stays capturable into a hipGraph (a captured graph keeps the mode and the thresholds it was captured with).  Must not be changed
 * while forward calls are in flight.
 * nesti_model_reproducible_stats synchronises `stream` and reads the counters; reset != 0 clears this block TOGETHER with the
 * gate's and the guard's (nesti_model_cascade_stats / nesti_model_x8_guard_stats).  tau = 0 without a two-stage gate, thr = -1
 * without a guard. */
typedef struct {
  int on;
  uint64_t gate_violations, guard_violations, guard_dropped;
  float max_margin_err, max_dn, tau, thr;
} nesti_reproducible_stats_t;
int nesti_model_set_reproducible(nesti_model_t* m, int on);
int nesti_model_reproducible_stats(const nesti_model_t* m, nesti_reproducible_stats_t* out, int reset, void* stream);

/* EXPERIMENT (pair-mode experts_n_est models, 8^3 grid, created after nesti_experiment_mix_enable(1); no reference counterpart): which of the experts' k^3 tap layers run ONE
 * 16-bit product (hi * W_hi, reading only the hi planes of their pair-layout input, writing pairs again) instead of three.
 * Bits: 0 / 1 = inception1 conv2 (3^3) / conv3 (5^3), 2 / 3 = inception2 conv2 / conv3, 4 / 5 = inception4 conv2 (2^3) / conv3 (4^3).
 * 0 (the default) is NESTI_F16X3 proper.  Any other value does NOT hold the 1e-5 cosine tolerance on every query
 * (profiles/r05_expert_mix.txt); it exists to measure that.  Must not be changed while forward calls are in flight. */
int nesti_experiment_mix_enable(int on); /* process-wide, BEFORE nesti_model_create: pack the extra single-product copies (default off) */
int nesti_model_set_expert_mix(nesti_model_t* m, int mask);
/* The same switch for the gating net of a NESTI_F16X3 / NESTI_BF16X3 model (non-cascade nesti_gate_forward / nesti_forward):
 * on != 0 runs ALL its k^3 tap layers at 8^3 / 4^3 single-product, the 1x1x1 / FC layers stay three-product ("medium" gate);
 * on == 2 additionally rounds every layer's output to 16 bits (lo plane = 0): the numerics of a plain-f16 gate whose 1x1x1 / FC
 * layers multiply by the exact weights (hi * W_hi + hi * W_lo) -- the "exact-weight filter" of profiles/r05_gate_medium.txt; mode 2
 * exists only in measurement builds (EXTRA_CXXFLAGS=-DNESTI_EXPERIMENT_XW), the product library refuses it. */
int nesti_model_set_gate_mix(nesti_model_t* m, int on);
/* NESTI_F16X8 / NESTI_F16X8C models: which expert tap layers at 8^3 take their cross terms through FP8 (see the dtype's comment above;
 * default 0b1111, 0 = NESTI_F16X3 proper). */
int nesti_model_set_x8_layers(nesti_model_t* m, int mask);
/* ... and in which format: 8 = OCP e4m3 with one power-of-two scale per layer and operand (above), 6 = OCP e2m3 (FP6) with one scale per
 * 16-channel block of a row, taken from the block's largest |hi| and stored beside the elements (the instruction runs FP6 at twice the
 * FP8 rate; |lo 2^11| <= |hi| element by element, so one scale serves a block's lo and hi halves; the residual is ~1.2x e4m3's and
 * the conditioning guard below bounds its effect exactly as it does for e4m3).  The model holds both packings; must not be changed
 * while forward calls are in flight; recalibrate the guard after a change. */
int nesti_model_set_x8_format(nesti_model_t* m, int bits);
/* The CONDITIONING GUARD of those models (top-1 routed calls: nesti_forward, nesti_estimate_normals[_multi], nesti_experts_forward
 * with an expert assignment).  The FP8 residual moves an expert's raw output n by |dn| -- ~5e-5, at most 2e-4 on 100 000 queries, and
 * independent of |n| -- and 1 - cos against the three-product result is (|dn| / |n|)^2 / 2: only outputs of very small norm can be
 * tilted by more than the bar.  Every query whose |n| is below
 *     thr_eff = max(thr, NESTI_X8_GUARD_WIDEN x largest |dn| measured so far / sqrt(2 x NESTI_X8_GUARD_BAR))
 * is evaluated again by its expert in f16x3 proper and that result replaces the FP8 one (a fraction of a per cent of the queries);
 * the rows decided twice measure |dn|, so the threshold follows the measurement like the two-stage gate's margin does, and a call
 * whose own measurement opens a wider band re-evaluates the rows in between in NESTI_X8_GUARD_WIDEN_PASSES further passes.  An
 * un-re-evaluated query therefore differs from f16x3 by 1 - cos <= NESTI_X8_GUARD_BAR / NESTI_X8_GUARD_WIDEN^2 as long as |dn| stays
 * below the largest value measured.  nesti_model_set_x8_guard: thr >= 0 (default NESTI_X8_GUARD_DEFAULT; calibrate it like the gate
 * margin: calibrate.calibrate_x8_guard), thr < 0 switches the guard off, +inf re-evaluates everything (calibration).  Must not be
 * changed while forward calls are in flight.  Because thr_eff follows what the model has measured so far, WHICH rows are re-evaluated
 * (hence the last bits of a few normals near the threshold, never the expert index) depends on the order and partition of the batches
 * a model has seen since its counters were last reset (nesti_model_x8_guard_stats with reset = 1) -- in the default mode.  With
 * nesti_model_set_reproducible on, thr_eff IS thr: the rows re-evaluated are those with |n| < thr, whatever has been measured, and a
 * |dn| that would have raised the threshold is counted in guard_violations (nesti_model_reproducible_stats).
 * nesti_model_guard_error_export / _import are the twins of the gate pair above for max_dn: one tiny kernel each on `stream`. */
#define NESTI_X8_GUARD_BAR 2.5e-6f
#define NESTI_X8_GUARD_WIDEN 1.5f
#ifndef NESTI_X8_GUARD_WIDEN_PASSES
#define NESTI_X8_GUARD_WIDEN_PASSES 1
#endif
#define NESTI_X8_GUARD_DEFAULT 0.25f
typedef struct {
  uint64_t queries;    /* routed queries seen since the last reset                                      */
  uint64_t rechecked;  /* ... of them re-evaluated in f16x3                                              */
  uint64_t dropped;    /* flagged rows NOT re-evaluated because an expert's guard list was full (0 unless the threshold is absurd) */
  float max_dn;        /* largest |n_x8 - n_f16x3| measured on the re-evaluated rows                     */
  float thr, thr_eff;  /* the configured threshold and the one the next call starts from                 */
} nesti_x8_guard_stats_t;
int nesti_model_set_x8_guard(nesti_model_t* m, float thr);
int nesti_model_x8_guard_stats(const nesti_model_t* m, nesti_x8_guard_stats_t* out, int reset, void* stream);
int nesti_model_guard_error_export(const nesti_model_t* m, float* dst_dev, void* stream);
int nesti_model_guard_error_import(nesti_model_t* m, const float* src_dev, int n, void* stream);

/* Workspace of ONE tower for `batch` queries, from the configuration alone (no device needed): tower = -1 the gating
 * net, 0..E-1 an expert.  dtype as nesti_model_create (NESTI_F16X3C: the gate figure is the f16 filter's). */
size_t nesti_tower_workspace_bytes(const nesti_config_t* cfg, int dtype, int tower, int batch);

/* Scratch size for forward calls of up to max_batch points. */
size_t nesti_workspace_bytes(const nesti_model_t* m, int max_batch);
int nesti_model_mups_cstride(const nesti_model_t* m); /* channel stride of the internal MuPS tensor, in elements
                                                       * (NESTI_BF16X3 / NESTI_F16X3: 2 x the padded channel count) */
int nesti_model_mups_rows(const nesti_model_t* m);    /* rows per point of the internal MuPS tensor: 512 (8^3 grid)
                                                       * or 64 (3^3 grid: row 16i+4j+k of a 4^3 index space, rows with
                                                       * a coordinate of 3 are zero) */
/* MuPS (utils/tf_util.py:655-753 + models/experts_n_est.py:66-76) of a batch in the layout and dtype
 * nesti_gate_forward / nesti_experts_forward read: mups_out_dev is [B, nesti_model_mups_rows, nesti_model_mups_cstride].
 * Every element of it is written (pad channels and, on the 3^3 grid, the dead rows as zeros).  Input domain: as
 * nesti_mups_forward -- finite coordinates in the rows up to n_eff, |x| <= 2 tested, 0 / 0 on an axis from |x| > 2.52 (8^3)
 * or 5.07 (3^3); nesti_forward and the call of a model take caller-supplied points under the same domain. */
int nesti_model_mups(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev, int B,
                     void* mups_out_dev, void* stream);

/* scale_manager_net + arg-max (models/experts_n_est.py:155-179,
 * test_n_est_w_experts.py:150): mups_dev is [B,R^3,cstride] in the model dtype.
 * probs_out_dev [B,E] f32 (row-major, i.e. the transpose done at :151),
 * expert_out_dev [B] int32 (first index on ties, like np.argmax).
 * NESTI_ARCH_SWITCH: probs_out_dev is [B,1] = noise_est (models/ms_sw_n_est.py:75) and
 * expert_out_dev[b] = noise_est < 0.015 ? 0 (small) : 1 (large) (:80-82). */
int nesti_gate_forward(const nesti_model_t* m, const void* mups_dev, int B, void* ws_dev,
                       size_t ws_bytes, float* probs_out_dev, int32_t* expert_out_dev,
                       void* stream);

/* normal_est_net for every expert (models/experts_n_est.py:99-105, 243-291).
 * expert_dev == NULL : evaluate all experts, normals_out_dev is [E,B,3] (what the
 *                      reference's sess.run returns, test_n_est_w_experts.py:148);
 * expert_dev != NULL : top-1 routing -- only expert_dev[b] is evaluated for point b
 *                      and normals_out_dev is [B,3] (== n_est[e*,b,:], :152). */
int nesti_experts_forward(const nesti_model_t* m, const void* mups_dev, const int32_t* expert_dev,
                          int B, void* ws_dev, size_t ws_bytes, float* normals_out_dev,
                          void* stream);

/* One sess.run([n_pred, experts_prob]) + arg-max/select
 * (test_n_est_w_experts.py:142-152) with top-1 routing:
 *   points_dev [B,S*P,3] f32, n_eff_dev [B,S] int32 ->
 *   normals_out_dev [B,3] f32, expert_out_dev [B] int32, probs_out_dev [B,E] f32.
 * For NESTI_ARCH_SINGLE / NESTI_ARCH_MULTI only normals are produced (expert/probs may be NULL).
 * For NESTI_ARCH_SWITCH (one sess.run of test_n_est_w_switching.py:136) probs_out_dev is [B,1] =
 * noise_est and expert_out_dev the tower chosen by the 0.015 threshold. */
int nesti_forward(const nesti_model_t* m, const float* points_dev, const int32_t* n_eff_dev,
                  int B, void* ws_dev, size_t ws_bytes, float* normals_out_dev,
                  int32_t* expert_out_dev, float* probs_out_dev, void* stream);

/* The body of the reference's predict loop for ONE shape in one call (test_n_est_w_experts.py:129-152 with
 * utils/pcpnet_dataset.py:286-343 behind the data loader): search grid (when build_grid != 0; replaces the cKDTree of
 * utils/pcpnet_dataset.py:37) + ball query + MuPS + gating + routed expert for patch rows
 * [query_row0, query_row0 + M) of the cloud (query_idx_dev / r_abs / seed / grid_ws_dev as in nesti_patches_query),
 * `batch` queries at a time.  The patch tensors only ever live in ws_dev
 * (nesti_estimate_workspace_bytes(m, batch) bytes).  Outputs as nesti_forward: [M,3], [M], [M,E]. */
size_t nesti_estimate_workspace_bytes(const nesti_model_t* m, int batch);
/* The same figure from the configuration alone (no model, no device): what a caller needs to size batches against free memory
 * before anything is created (nesti-net_amd/cli.py: fit_batch).  dtype as nesti_model_create. */
size_t nesti_estimate_workspace_bytes_for_config(const nesti_config_t* cfg, int dtype, int batch);
int nesti_estimate_normals(const nesti_model_t* m, const float* cloud_dev, int N,
                           const int32_t* query_idx_dev, int M, const double* r_abs, uint64_t seed,
                           int query_row0, int batch, int build_grid, void* grid_ws_dev,
                           size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes,
                           float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev,
                           void* stream);

/* nesti_estimate_normals for query POSITIONS (generalises utils/pcpnet_dataset.py:304: the ball query's centre is any
 * position, see nesti_patches_query_at): query_xyz_dev [M,3] f32 in place of query_idx_dev; query_row0 >= 0 is the patch row of
 * the first query (the subsample key).  Both Gaussian grids.  n_ball_out_dev (optional) [M,S] int32: the uncapped ball sizes.
 * Rows without a neighbourhood carry the sentinel of nesti_mask_empty_queries on return. */
int nesti_estimate_normals_at(const nesti_model_t* m, const float* cloud_dev, int N,
                              const float* query_xyz_dev, int M, const double* r_abs, uint64_t seed,
                              int query_row0, int batch, int build_grid, void* grid_ws_dev,
                              size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes,
                              float* normals_out_dev, int32_t* expert_out_dev, float* probs_out_dev,
                              int32_t* n_ball_out_dev, void* stream);
/* The sentinel alone, for callers of the unfused path (nesti_patches_query_at -> nesti_forward; the reference has no such
 * rows: utils/pcpnet_dataset.py:304 always finds the centre itself): every row i of [0, M) whose n_eff_dev[i, 0..S) is 0 at
 * every scale gets normal (0, 0, 0), expert -1 and probabilities 0 (E columns); other rows are untouched.  expert_dev and
 * probs_dev may be NULL.  Enqueue it after everything that writes the rows (nesti_forward ends ordered on its stream). */
int nesti_mask_empty_queries(const int32_t* n_eff_dev, int M, int S, float* normals_dev, int32_t* expert_dev,
                             float* probs_dev, int E, void* stream);

/* ---- consistent orientation of estimated normals (orient.hip; DESIGN.md 2 "Orientation") ------------------------------------
 * No reference call site: Nesti-Net is trained with an unoriented loss and its .normals are lines, not vectors.  The consumer is
 * the reference's "RMS oriented" figure (utils/evaluate.py:151); the conventions below are the library's own.
 * Hoppe's propagation made unique, as a post-pass over positions xyz_dev [M,3] f32 and their normals [M,3] f32:
 *   eligible rows: all three normal components finite and one non-zero (tested on the bits); other rows are left untouched and
 *     are nobody's neighbour.  PRECONDITION: the positions of eligible rows are finite.
 *   nbr(i): the eligible j != i with fp64 d2 = (dx dx + dy dy) + dz dz <= radius^2, the K (1 .. 16) smallest by (d2, j), in order.
 *   edge {a < b}: b in nbr(a) or a in nbr(b); id = a K + slot of b in nbr(a) if b in nbr(a), else b K + slot of a in nbr(b).
 *     In fp64, every operation rounded on its own: d = (na.x nb.x + na.y nb.y) + na.z nb.z, q_i = |n_i|^2, flip bit f = d < 0,
 *     weight w = (float)max(0, 1 - (d d) / (q_a q_b)); key = (bits of w) << 32 | id.  Keys are distinct, so the minimum spanning
 *     forest under this order is unique.
 *   root of each tree: the vertex with the largest z (ties: smaller index), signed so that the first non-zero of (n_z, n_y, n_x)
 *     is positive; with a viewpoint v the vertex with the smallest fp64 d2 to v, flipped iff the fp64 n . (v - p) < 0.
 *   vertex x is flipped iff (root flipped) xor (xor of f over the tree path root -> x).  A flip negates the three floats: sign
 *     bits only, nothing is normalised.
 * NESTI_ORIENT_VIEWPOINT: no graph; every eligible row is flipped iff the fp64 n . (v - p) < 0 (viewpoint required).
 * Each tree is oriented on its own: a graph that falls apart (tiny radius, K = 1) gives trees whose root rule may pick the inner
 * side; n_components tells.  grid_ws_dev: nesti_patches_workspace_bytes(M) bytes (the call builds the search grid over xyz_dev);
 * ws_dev: nesti_orient_workspace_bytes(M, K) bytes.  M = 0 is a no-op.  Argument errors (null pointers, K outside 1 .. 16, a
 * radius that is not finite or <= 0, an unknown mode, NESTI_ORIENT_VIEWPOINT without a viewpoint, a non-finite viewpoint, a
 * short workspace, M K >= 2^32) are reported before any device call.  The calls enqueue on `stream` and neither synchronise nor
 * read anything back; the result is a pure function of the inputs. */
enum { NESTI_ORIENT_MST = 0, NESTI_ORIENT_VIEWPOINT = 1 };
typedef struct {
  int32_t n_eligible, n_components, n_flipped, n_edges;   /* NESTI_ORIENT_VIEWPOINT: n_components = n_edges = 0 */
} nesti_orient_stats_t;
/* host only; 0 for M <= 0 (and for K outside 1 .. 16) */
size_t nesti_orient_workspace_bytes(int M, int K);
/* The parity entry: neighbour lists and edges only.  Any output may be NULL: nbr_out_dev [M,K] int32, -1 padded; edge_u_dev /
 * edge_v_dev [M K] int32 indexed by edge id, -1 = no edge in this slot; edge_wbits_dev [M K] the bits of w; edge_flip_dev [M K] f. */
int nesti_orient_graph(const float* xyz_dev, int M, const float* normals_dev, double radius, int K,
                       void* grid_ws_dev, size_t grid_ws_bytes, void* ws_dev, size_t ws_bytes,
                       int32_t* nbr_out_dev, int32_t* edge_u_dev, int32_t* edge_v_dev,
                       uint32_t* edge_wbits_dev, uint8_t* edge_flip_dev, void* stream);
/* Orients normals_dev in place.  viewpoint: 3 doubles on the HOST, or NULL.  tree_edge_out_dev (optional) [M K] uint8: 1 for the
 * edge ids of the spanning forest.  stats_dev (optional): on the DEVICE, written on the stream. */
int nesti_orient_normals(const float* xyz_dev, int M, float* normals_dev, int mode, double radius, int K,
                         const double* viewpoint, void* grid_ws_dev, size_t grid_ws_bytes,
                         void* ws_dev, size_t ws_bytes, uint8_t* tree_edge_out_dev,
                         nesti_orient_stats_t* stats_dev, void* stream);

/* ---- plane-fit (PCA) normals and surface variation at every patch scale (pca.hip; DESIGN.md 2 "Plane-fit normals") -------------
 * The classical estimator: the first row of the paper's comparison tables and the frame of the reference dataset's use_pca step
 * (utils/pcpnet_dataset.py:357-377, which the test path never takes; the per-scale estimator itself has no reference call site).
 * No model, no weights.  Queries, radii, grid workspace and query_row0 as for nesti_patches_count / nesti_patches_query_at
 * (query_idx_dev NULL: row i is cloud point query_row0 + i; positions may lie anywhere and may be non-finite).  Per query and scale s,
 * over the FULL ball B = {p : fp64 d2(p, c) <= r_s^2} -- the ball test of nesti_patches_query, NOT capped at points_per_scale and not
 * subsampled -- with d = (double)p - (double)c:
 *     n = |B|,  m = (sum d) / n,  C = ((sum d d^T) / n - m m^T) / r_s^2     (units of r^2: eigenvalues are scale-free and <= 1)
 *     eigen-decomposition of C in fp64 (cyclic Jacobi, a fixed number of sweeps: nesti_sym3_eig), eigenvalues w0 <= w1 <= w2.
 * Outputs (device; any may be NULL):
 *     normals_out_dev [M,S,3] f32  the eigenvector of w0, normalised in fp64 and rounded to f32 once; then, on the f32 values, signed
 *                                  so that the first non-zero of (n_z, n_y, n_x) is positive (the root rule of nesti_orient_normals);
 *                                  zeros are +0
 *     eig_out_dev     [M,S,3] f32  max(0, w_k), ascending; surface variation = w0 / (w0 + w1 + w2)
 *     n_ball_out_dev  [M,S] int32  n (what nesti_patches_count writes)
 * SENTINEL: a scale with n < 3 -- an empty ball, and every scale of a non-finite position -- gets normal 0 0 0 and eigenvalues
 * 0 0 0; its count is still written.
 * DETERMINISM: no floating-point atomics; for ONE grid (one nesti_patches_grid call) a row's outputs are identical bits however the
 * rows are split over calls and streams.  The grid's cell-ordered copy is filled through an atomic cursor, so the order of the points
 * inside a cell, and with it the last bits of an fp64 sum, may differ between two grid builds: across builds the counts are equal,
 * eigenvalues agree to ~2^-23 relative + 8 n 2^-53 and directions to 2^-22 + 16 n 2^-53 / (w1 - w0) (tests/test_gpu_pca.py).
 * Argument errors (null cfg / cloud / radii / workspace, M < 0, a short workspace, n_scales outside 1 .. NESTI_MAX_SCALES, a radius
 * that is not finite or <= 0, rows beyond the cloud) are reported before any device call; M = 0 is a no-op.  The calls enqueue one
 * kernel on `stream`, neither synchronise nor read anything back, and can be captured into a graph. */
int nesti_pca_normals(const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                      const double* r_abs, int query_row0, float* normals_out_dev, float* eig_out_dev,
                      int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream);
int nesti_pca_normals_at(const nesti_config_t* cfg, const float* cloud_dev, int N, const float* query_xyz_dev, int M,
                         const double* r_abs, int query_row0, float* normals_out_dev, float* eig_out_dev,
                         int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream);
/* Host only: the solver of the two entries above, the same arithmetic on the CPU (csrc/pca_eig.h).  c = {xx, xy, xz, yy, yz, zz};
 * w[3]: eigenvalues ascending (not clamped); v[9]: v[3 k + i] = component i of the unit eigenvector of w[k].  Only + - x / sqrt,
 * every operation rounded on its own.  Returns 1 for a null pointer. */
int nesti_sym3_eig(const double c[6], double w[3], double v[9]);

/* ---- quadric-fit normals and principal curvatures at every patch scale (quadric.hip; DESIGN.md 2 "Quadric fit") ------------------
 * The osculating-jet estimator of Cazals and Pouget at degree 2: the second row of the paper's comparison tables, and the source of
 * the principal curvatures the reference's data layer reads from <shape>.curv (utils/pcpnet_dataset.py:260-263, 349-352, 410-413).
 * No model, no weights.  Queries, radii, grid workspace and query_row0 as for nesti_pca_normals.  Per query centre c and scale s
 * (radius r), over the FULL ball of nesti_pca_normals (fp64 d2(p, c) <= r^2, not capped at points_per_scale, not subsampled), with
 * d = (double)p - (double)c and n the ball size; fp64, every operation rounded on its own:
 *   1 plane normal  n0 = the normal nesti_pca_normals returns for that ball on the same grid (f32, signed), taken back to fp64, not
 *                   renormalised
 *   2 frame         j = the index of the smallest |n0_j| (ties: the first of x, y, z); t1 = (n0 x e_j) / |n0 x e_j|; t2 = n0 x t1,
 *                   not renormalised.  (The fitted surface does not depend on the rotation inside the tangent plane.)
 *   3 coordinates   (u, v, h) = ((t . d) / r) for t = t1, t2, n0, the dot product bracketed (t_x d_x + t_y d_y) + t_z d_z;
 *                   phi = (1, u, v, u^2, u v, v^2)
 *   4 moments       m[0..14] = sum u^p v^q for (p, q) = (0,0) (1,0) (0,1) (2,0) (1,1) (0,2) (3,0) (2,1) (1,2) (0,3) (4,0) (3,1) (2,2)
 *                   (1,3) (0,4); m[15..20] = sum h phi_i; m[0] = n
 *   5 solve         N a = b, N_ij = sum phi_i phi_j read from m, b = m[15..20]: Cholesky without pivoting in a fixed operation order
 *                   (csrc/quadric_solve.h).  The fit FAILS if n < 6, if n0 is the zero row, or if a pivot
 *                   s_j = N_jj - sum_k L_jk^2 is not > 2^-44 N_jj (a zero, negative or NaN pivot included), or if a coefficient
 *                   comes out non-finite (a NaN among the h moments, which no pivot sees)
 *   6 normal        nu = (n0 - a1 t1) - a2 t2, normalised in fp64, rounded to f32 once; zeros are +0.  nu . n0 > 0: it lies on
 *                   n0's side, and no second sign rule is applied, because the curvature signs refer to this side
 *   7 curvatures    the eigenvalues of the shape operator in an orthonormal tangent basis: g = (a1, a2), w = sqrt(1 + g.g),
 *                   Hh = [[2 a3, a4], [a4, 2 a5]], P = I - g g^T / (w (1 + w)), Sm = P Hh P / w, mean = (Sm00 + Sm11) / 2,
 *                   dif = (Sm00 - Sm11) / 2, q = (Sm01 + Sm10) / 2, rad = sqrt(dif^2 + q^2); k_max = (mean + rad) / r,
 *                   k_min = (mean - rad) / r, as f32.  ABSOLUTE units (1 / length), those of a PCPNet .curv file.  Positive where
 *                   the surface bends toward nu: a sphere of radius R with outward normals has k_max = k_min = -1 / R
 *   8 failed fit    nu = 0 0 0 and k = 0 0 (also where nu or k would not be finite, which takes an overflow); plane_out and n_ball
 *                   are written as nesti_pca_normals writes them.  No output is NaN or infinite for finite input; a non-finite
 *                   position has n = 0 at every scale.
 * FLIP: replacing n0 by -n0 gives t1 -> -t1, t2 -> t2, (u, v, h) -> (-u, v, -h), a -> (-a0, a1, -a2, -a3, a4, -a5), nu -> -nu
 * and (k_max, k_min) -> (-k_min, -k_max), all exactly.  Orienting a row is therefore: where the sign bits of nu were flipped, its
 * curvatures become (-k_min, -k_max).
 * Outputs (device; any may be NULL): normals_out_dev [M,S,3] f32 nu; curv_out_dev [M,S,2] f32 (k_max, k_min); plane_out_dev [M,S,3]
 * f32 n0, the bits of nesti_pca_normals' normals_out_dev; n_ball_out_dev [M,S] int32.
 * DETERMINISM as for nesti_pca_normals: no floating-point atomics; for ONE grid a row's outputs are identical bits however the rows
 * are split over calls and streams.  The argument errors of nesti_pca_normals are reported before any device call; M = 0 is a no-op.
 * The calls enqueue one kernel on `stream`, neither synchronise nor read anything back, and can be captured into a graph. */
int nesti_quadric_fit(const nesti_config_t* cfg, const float* cloud_dev, int N, const int32_t* query_idx_dev, int M,
                      const double* r_abs, int query_row0, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                      int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream);
int nesti_quadric_fit_at(const nesti_config_t* cfg, const float* cloud_dev, int N, const float* query_xyz_dev, int M,
                         const double* r_abs, int query_row0, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                         int32_t* n_ball_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream);
/* Host only: steps 5 and 7 on the CPU, the arithmetic of the two entries above (csrc/quadric_solve.h), in the scaled units of the fit
 * (k is not divided by r).  m[21] as in step 4; a[6] the coefficients; k[2] = (k_max, k_min); *ok = 1 if the fit succeeded, else 0
 * with a = 0 and k = 0 (m[0] < 6, or a pivot failed: rank-deficient or NaN moments).  Returns 1 for a null pointer. */
int nesti_quadric_solve(const double m[21], double a[6], double k[2], int* ok);

/* ---- k-nearest-neighbour neighbourhoods (knn.hip; DESIGN.md 2 "k-nearest neighbourhoods") -----------------------------------------
 * An exact k-NN search on the uniform grid of nesti_patches_grid, and the plane fit and the quadric fit over neighbour lists instead of
 * balls: a neighbourhood that adapts to the density where a fixed radius starves the sparse part of a cloud.  No model, no weights.
 *
 * SEARCH.  For a centre c -- cloud point query_idx_dev[i], or cloud row query_row0 + i where query_idx_dev is NULL (an index is clamped
 * into the cloud), or the position query_xyz_dev[i] -- over ALL N cloud points j, in fp64:
 *     d = (double)p_j - (double)c,   d2_j = (dx dx + dy dy) + dz dz, each of the five operations rounded on its own
 * (not the fused d2 of the ball test: a restatement in plain IEEE arithmetic predicts every bit).  The result is the K smallest pairs
 * (d2_j, j) in lexicographic order, ascending:
 *     nbr_out_dev   [M, K] int32   j
 *     d2_out_dev    [M, K] fp64    d2_j                (may be NULL)
 *     count_out_dev [M]    int32   min(K, N)           (may be NULL)
 * Slots beyond the count hold -1 and +inf.  A centre with a non-finite coordinate (tested on the bits) has count 0.  A cloud point
 * queried by index is its own neighbour (d2 = 0), as a ball contains its centre; duplicates tie on d2 and are ordered by index.  There
 * is no radius bound: a query far from everything still gets its K nearest.  1 <= K <= NESTI_KNN_MAX_K.
 * A cloud point with a NaN coordinate has a NaN d2 and is never a neighbour: the count of a query then falls below min(K, N) where
 * fewer than K other points exist.  Under nesti_profile_enable the search and the list fits are booked in the patches category, like
 * nesti_pca_normals and nesti_quadric_fit.
 * GRID.  grid_ws_dev is any workspace prepared by nesti_patches_grid over this cloud (any config, any radii); the result does not
 * depend on which one, nor on the order the build left inside a cell -- only the time does (aim at the order of K points in a
 * 3 x 3 x 3 cell block).  The search starts at the centre's (clamped) cell and grows the visited block shell by shell until it holds K
 * candidates and the K-th d2 is STRICTLY below the square of the distance from the centre to the nearest face of the block that still
 * has grid beyond it (less a margin of 2^-50 of the magnitudes involved, which covers the rounding of the cell assignment:
 * csrc/knn.hip), or the block covers the grid.  A position outside the bounding box starts from the clamped border cell.
 * One wave per query; candidates are compacted by ballot into an LDS buffer that is cut back to the K smallest pairs whenever it
 * fills: no floating-point atomics, no dependence on which workgroup runs first, and no limit on the points of one cell.
 * Argument errors (null cloud / workspace / nbr_out_dev, N <= 0, K outside 1 .. NESTI_KNN_MAX_K, M < 0, a short workspace, rows
 * beyond the cloud, null positions) are reported before any device call; M = 0 is a no-op.  The calls enqueue one kernel on `stream`,
 * neither synchronise nor read anything back, and can be captured into a graph. */
int nesti_knn(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, int K, int32_t* nbr_out_dev,
              double* d2_out_dev, int32_t* count_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream);
int nesti_knn_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, int K, int32_t* nbr_out_dev, double* d2_out_dev,
                 int32_t* count_out_dev, const void* grid_ws_dev, size_t grid_ws_bytes, void* stream);
/* FITS OVER NEIGHBOUR LISTS.  Centres as for nesti_knn; nbr_dev [M, K] int32 (device) is the list of every row, 1 <= K <=
 * NESTI_KNN_MAX_K; ks [S] (HOST) are the neighbour counts of the scales, 1 <= S <= NESTI_MAX_SCALES, 1 <= ks[0] <= ... <= ks[S-1]
 * <= K.  No grid is needed.  The list is untrusted: the valid prefix of a row ends at its first entry outside [0, N) (the -1 padding
 * of nesti_knn, a bad index), so a bad entry never causes an out-of-bounds read; a centre with a non-finite coordinate has an empty
 * prefix.  Lists need not be sorted and need not come from nesti_knn.  Per row and scale s: n_s = min(ks[s], valid prefix), the points
 * are the first n_s entries, d and d2 as for nesti_knn, and r2_s = the largest d2 among them (the last one of a sorted list).
 *   plane fit    nesti_pca_normals' estimator with the prefix in place of the ball and r2_s in place of r^2: the same nine sums by
 *                the same operations (slot i is added in lane i mod 64, a lane's slots in ascending order, the lanes meet in the same
 *                xor-butterfly), the same solve, rounding and sign rule.  Eigenvalues are in units of the neighbourhood's own radius
 *                squared.  n_s < 3 or r2_s == 0: normal 0 0 0, eigenvalues 0 0 0.
 *   quadric fit  steps 1 - 8 of nesti_quadric_fit with the prefix in place of the ball, r = sqrt(r2_s) (fp64) in place of the radius,
 *                pass 1 = the plane fit above bit for bit (plane_out_dev).  The failure rule is that entry's, plus r2_s == 0.
 *   outputs      (device; any may be NULL) normals / eig / curv / plane as for the ball entries, [M,S,..];
 *                radius_out_dev [M,S] f32 = (float)sqrt(r2_s); count_out_dev [M,S] int32 = n_s.
 * DETERMINISM: no floating-point atomics, and the summation order is fixed by the list.  With the list of nesti_knn a row's output
 * bits are a pure function of (cloud, centre, ks): independent of batching, of streams, of the grid and of the grid BUILD -- more
 * than the ball entries promise, whose sums follow the order inside a cell.  Scale s of ks equals the single scale of a run with
 * ks = {ks[s]}.
 * Argument errors (null cloud / list / ks, N <= 0, K outside 1 .. NESTI_KNN_MAX_K, S outside 1 .. NESTI_MAX_SCALES, ks not ascending
 * or outside 1 .. K, M < 0, rows beyond the cloud, null positions) are reported before any device call; M = 0 is a no-op. */
int nesti_pca_normals_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                          int K, const int32_t* ks, int S, float* normals_out_dev, float* eig_out_dev, float* radius_out_dev,
                          int32_t* count_out_dev, void* stream);
int nesti_pca_normals_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                             const int32_t* ks, int S, float* normals_out_dev, float* eig_out_dev, float* radius_out_dev,
                             int32_t* count_out_dev, void* stream);
int nesti_quadric_fit_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                          int K, const int32_t* ks, int S, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                          float* radius_out_dev, int32_t* count_out_dev, void* stream);
int nesti_quadric_fit_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                             const int32_t* ks, int S, float* normals_out_dev, float* curv_out_dev, float* plane_out_dev,
                             float* radius_out_dev, int32_t* count_out_dev, void* stream);

/* ---- scale-selected plane fit over neighbour lists (select.hip; DESIGN.md 2 "Scale-selected plane fit") ----------------------------
 * The plane fit of nesti_pca_normals_nbr at every neighbour count of a LADDER, and per row the choice of one of them: the candidate of
 * smallest surface variation e0 / (e0 + e1 + e2) -- Pauly, Keiser and Gross's multi-scale surface variation (2003) read as a selector,
 * standing in for the bias / variance trade of Mitra and Nguyen (2003).  The conventions are the library's own (no parity with any
 * published selector is claimed): the score uses only + - x / and comparisons, on the f32 eigenvalues AS WRITTEN, so a caller can
 * recompute every choice from the outputs.  No model, no weights, no grid.
 *
 * Centres, nbr_dev [M, K] (1 <= K <= NESTI_KNN_MAX_K), the valid prefix and the untrusted-list rule are exactly as for
 * nesti_pca_normals_nbr: the prefix ends at the first entry outside [0, N), a non-finite centre has an empty prefix, lists need not be
 * sorted.  ks [L] (HOST) is the ladder: 1 <= L <= NESTI_SELECT_MAX_L, 1 <= ks[0] < ks[1] < ... < ks[L-1] <= K (strictly ascending).
 * slack: fp64 on the host, finite and >= 0.
 *  1 CANDIDATE c = 0 .. L-1.  n_c = min(ks[c], valid prefix); d and d2 per slot as for nesti_knn; r2_c = the largest d2 among the
 *    first n_c slots (a prefix maximum: the last slot only where the list is sorted).  A short prefix gives several candidates the
 *    same n_c: they are the same fit.
 *  2 FIT.  The plane fit of candidate c is the output of nesti_pca_normals_nbr with ks = {ks[c]}, bit for bit: slot i is added in lane
 *    i mod 64, a lane adds its slots in ascending order from +0.0, each of the nine totals goes through the same xor-butterfly
 *    (offsets 32, 16, ..., 1), the same solve, rounding and sign rule.  n_c < 3 or r2_c == 0: normal 0 0 0, eigenvalues 0 0 0.
 *  3 SCORE, from the f32 eigenvalues e0 <= e1 <= e2 of step 2:  den = ((double)e0 + (double)e1) + (double)e2;  v_c = (double)e0 / den.
 *    Candidate c is ELIGIBLE iff n_c >= 3, r2_c > 0 and den > 0.
 *  4 SELECTION.  v_min = the smallest v_c over the eligible candidates;  thr = v_min + v_min slack (a product, then a sum, each
 *    rounded; +inf where it overflows);  sel = the LARGEST eligible c with v_c <= thr.  slack = 0: the arg-min, ties to the larger
 *    count.  No eligible candidate: sel = -1 and every selected output is 0.
 *  5 OUTPUTS (device; any may be NULL).  Selected:
 *      normals_out_dev [M,3] f32    the normal of candidate sel
 *      eig_out_dev     [M,3] f32    its eigenvalues, in units of r2_sel
 *      sel_out_dev     [M]   int32  sel
 *      k_out_dev       [M]   int32  n_sel
 *      radius_out_dev  [M]   f32    (float)sqrt(r2_sel)
 *    Per candidate:
 *      variation_all_out_dev [M,L]   f32    (float)v_c, 0 where the candidate is not eligible
 *      normals_all_out_dev   [M,L,3] f32    as nesti_pca_normals_nbr writes them
 *      eig_all_out_dev       [M,L,3] f32
 *      radius_all_out_dev    [M,L]   f32    (float)sqrt(r2_c)
 *      count_all_out_dev     [M,L]   int32  n_c
 * DETERMINISM: no atomics.  A row's bits are a pure function of (cloud, centre, list prefix, ladder, slack): independent of batching,
 * of streams and of the grid the list came from.
 * Argument errors -- those of nesti_pca_normals_nbr (null cloud / list / ks, N <= 0, K outside 1 .. NESTI_KNN_MAX_K, M < 0, rows
 * beyond the cloud, null positions); L outside 1 .. NESTI_SELECT_MAX_L; a ladder that is not strictly ascending or lies outside
 * 1 .. K; slack not finite or negative -- are reported under the entry's name before any device call; M = 0 is a no-op.  Each call
 * enqueues one kernel on `stream`, neither synchronises nor reads anything back, and can be captured into a graph.  Under
 * nesti_profile_enable the launch is booked in the patches category, like the other list fits. */
int nesti_pca_select_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                         int K, const int32_t* ks, int L, double slack, float* normals_out_dev, float* eig_out_dev, int32_t* sel_out_dev,
                         int32_t* k_out_dev, float* radius_out_dev, float* variation_all_out_dev, float* normals_all_out_dev,
                         float* eig_all_out_dev, float* radius_all_out_dev, int32_t* count_all_out_dev, void* stream);
int nesti_pca_select_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                            const int32_t* ks, int L, double slack, float* normals_out_dev, float* eig_out_dev, int32_t* sel_out_dev,
                            int32_t* k_out_dev, float* radius_out_dev, float* variation_all_out_dev, float* normals_all_out_dev,
                            float* eig_all_out_dev, float* radius_all_out_dev, int32_t* count_all_out_dev, void* stream);

/* ---- Hough-transform normals over neighbour lists (hough.hip; DESIGN.md 2 "Hough-transform normals") ------------------------------
 * The sharp-feature estimator after Boulch and Marlet (SGP 2012): planes through hashed triplets of a neighbourhood vote for their
 * normal in an accumulator over the hemisphere; the fullest bin names the normal.  Where the plane fit and the quadric fit average
 * across a crease, the vote picks one of its faces.  The conventions are the library's own (no parity with the authors' code): fp64
 * throughout, every operation rounded on its own, only + - x / sqrt, comparisons and integer arithmetic -- a restatement in plain IEEE
 * arithmetic predicts every output bit.  No model, no weights, and no ball variant: the estimator exists over lists only.
 *
 * Centres, nbr_dev [M, K], ks [S], the valid prefix, n_s = min(ks[s], valid prefix), d = (double)p - (double)c and r2_s are exactly as
 * for nesti_pca_normals_nbr: the list is untrusted, the prefix ends at the first entry outside [0, N), and a non-finite centre has an
 * empty prefix.  T triplets, 1 .. NESTI_HOUGH_MAX_T; B bins per axis, 2 .. NESTI_HOUGH_MAX_BINS; R rotations, 1 ..
 * NESTI_HOUGH_MAX_ROT; rot [R, 9] fp64 row-major on the HOST; seed; query_row0 (both entries: the key row of row i is query_row0 + i).
 * Per row i with key row q = query_row0 + i, per scale s with n = n_s and slots d_0 .. d_{n-1}:
 *  1 TRIPLET t = 0 .. T-1.  h_c = the subsample hash (splitmix64 finaliser) of (seed, q, 0, 3 t + c) for c = 0, 1, 2 -- the
 *    scale argument is 0 on purpose: scale s of ks equals the single scale of a run with ks = {ks[s]}.  Indices from 64-bit products:
 *      i0 = (h0 n) >> 32;   j = (h1 (n - 1)) >> 32, i1 = j + (j >= i0);   lo, hi = min, max(i0, i1);
 *      j = (h2 (n - 2)) >> 32, j += (j >= lo), i2 = j + (j >= hi).          The three are distinct for n >= 3.
 *  2 PLANE.  e1 = d_i1 - d_i0, e2 = d_i2 - d_i0; v = e1 x e2, each component two products and one difference;
 *    l1 = (e1x^2 + e1y^2) + e1z^2, l2 and qq (the same sum for v) likewise.  The triplet is VALID iff qq > 2^-20 (l1 l2): false for NaN,
 *    for coincident points and for near-collinear ones (sine below 2^-10).  u = v / sqrt(qq), three divisions.
 *  3 VOTE, for each rotation rho.  w_k = (rot[rho][3k] u_x + rot[rho][3k+1] u_y) + rot[rho][3k+2] u_z; sigma = -1 if the first non-zero
 *    of (w_z, w_y, w_x) is negative, else +1; w <- sigma w; m = (|w_x| + |w_y|) + w_z, a = w_x / m, b = w_y / m (the hemi-octahedral
 *    map of the upper hemisphere onto a square); bi = clamp((int)floor(((a + b) + 1) (B / 2.0)), 0, B - 1), bj the same with a - b;
 *    bin = bi B + bj; count[rho][bin] += 1, an integer.
 *  4 WINNER.  Per rho the bin with the largest count, among equals the smaller bin; rho* = the rotation whose winner has the largest
 *    count, among equals the smaller rho.  win = that count; valid = the number of valid triplets.
 *  5 NORMAL.  Over the valid triplets whose bin under rho* is the winner, the sum of sigma_t u_t (sigma_t: the sign of step 3 under
 *    rho*; u_t: the unrotated vector).  Lane l of a 64-lane wave adds its triplets t = l, l + 64, ... in ascending order into three fp64
 *    partial sums; the lanes meet in an xor-butterfly (offsets 32, 16, ..., 1).  nn = (X^2 + Y^2) + Z^2; if nn > 0 and finite the
 *    normal is (X, Y, Z) / sqrt(nn), rounded to f32 once, then signed on the f32 values so that the first non-zero of (n_z, n_y, n_x)
 *    is positive; zeros are +0.
 *  6 OUTPUTS (device; any may be NULL):
 *      normals_out_dev [M,S,3] f32    the normal of step 5
 *      conf_out_dev    [M,S]   f32    (float)((double)win / (double)valid)
 *      votes_out_dev   [M,S,2] int32  (win, valid)
 *      radius_out_dev  [M,S]   f32    (float)sqrt(r2_s), as the other list entries write it
 *      count_out_dev   [M,S]   int32  n_s, likewise
 *  7 SENTINEL.  n < 3, valid == 0 or a failed step 5 gives normal 0 0 0, confidence 0 and votes (0, valid); radius and count are still
 *    written.  No output is NaN or infinite for finite input.
 * DETERMINISM: no floating-point atomics (the votes are integer additions).  A row's bits are a pure function of (cloud, centre, list
 * prefix, T, B, R, rot, seed, key row): independent of batching, of streams and of the grid.
 * Argument errors -- those of nesti_pca_normals_nbr; T, B or R out of range; null rot; a rotation with a non-finite entry or with
 * max |rot rot^T - I| > 1e-6; query_row0 < 0 (both entries) -- are reported before any device call; M = 0 is a no-op.  Each call
 * enqueues one kernel on `stream`, neither synchronises nor reads anything back, and can be captured into a graph.  Under
 * nesti_profile_enable the launch is booked in the patches category, like the other list fits. */
int nesti_hough_normals_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                            int K, const int32_t* ks, int S, int T, int B, int R, const double* rot, uint64_t seed,
                            float* normals_out_dev, float* conf_out_dev, int32_t* votes_out_dev, float* radius_out_dev,
                            int32_t* count_out_dev, void* stream);
int nesti_hough_normals_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, int query_row0, const int32_t* nbr_dev,
                               int K, const int32_t* ks, int S, int T, int B, int R, const double* rot, uint64_t seed,
                               float* normals_out_dev, float* conf_out_dev, int32_t* votes_out_dev, float* radius_out_dev,
                               int32_t* count_out_dev, void* stream);

/* ---- robust plane-fit normals over neighbour lists (robust.hip; DESIGN.md 2 "Robust plane fit") ------------------------------------
 * An M-estimator of the plane through a neighbourhood, solved by iteratively re-weighted least squares (IRLS) -- after Mederos et al.
 * (2003), Fleishman et al. (2005) and the RIMLS of Oztireli et al. (2009): residuals to the current plane down-weight the points of the
 * other face of a crease, so the fit leans to one face where the plane fit averages both, and the normal stays continuous (no bins, no
 * triplets).  With a start normal the same entry REFINES any other estimator's normals against the points.  The conventions are the
 * library's own (no parity with any published code is claimed): fp64 throughout, every operation rounded on its own, only + - x /
 * sqrt, comparisons and integer arithmetic -- a restatement in plain IEEE arithmetic predicts every output bit.  No model, no weights,
 * no grid, and no ball variant.
 *
 * Centres, nbr_dev [M, K], ks [S], the valid prefix, n_s = min(ks[s], valid prefix), d = (double)p - (double)c, d2 and r2_s are exactly
 * as for nesti_pca_normals_nbr: the list is untrusted, the prefix ends at the first entry outside [0, N), and a non-finite centre has an
 * empty prefix.  On the HOST: iters in 0 .. NESTI_ROBUST_MAX_ITERS; sigma finite, in (0, 1e6]; falloff in [0, 1]; floor in [1e-6, 1].
 * init_normals_dev [M,S,3] f32 (device) or NULL: the start normals, indexed like the outputs.  Per row, per scale s with n = n_s:
 *  0 START.  plane = the normal nesti_pca_normals_nbr writes for the scale, bit for bit; it is always computed.  g = the init row where
 *    an init is given, else plane.  The row is SKIPPED -- normal 0 0 0, iters_done 0, support 0, inliers 0, moments 0 -- if n < 3, if
 *    r2_s == 0, if a d2 among the first n slots is not finite, or if g is 0 0 0 or has a non-finite component.  Otherwise g is put under
 *    the sign rule on its f32 values (negated if the first non-zero of (g_z, g_y, g_x) is negative, zeros +0): the caller's sign never
 *    reaches a bit of the result.
 *  ONE ITERATION, from the f32 normal g:
 *  1 v = (double)g / sqrt((g_x g_x + g_y g_y) + g_z g_z), the products of the converted values.
 *  2 h_i = (v_x dx_i + v_y dy_i) + v_z dz_i;  c = the element of 0-based rank n / 2 (integer division) of the h_i in ascending order --
 *    an element, never an average;  res_i = h_i - c.
 *  3 med = the element of rank n / 2 of the |res_i|;  sig = max(sigma med, floor sqrt(r2_s)).
 *  4 x_i = res_i / sig;  t_i = 1 / (1 + x_i x_i);  u_i = 1 - falloff (d2_i / r2_s);  a_i = u_i t_i;  w_i = a_i a_i  (Geman-McClure on
 *    the residual times the u^2 of nesti_smooth_normals_nbr on the distance).
 *  5 TEN SUMS.  sw = sum w_i, then sum w_i T for the nine terms T of the plane fit in its order: dx dy dz, then the products xx xy xz
 *    yy yz zz of d, each rounded BEFORE it meets w_i.  Slot i is added in lane i mod 64 of a 64-lane wave, a lane adds its slots in
 *    ascending order from +0.0, each total goes through the xor-butterfly of the plane fit (offsets 32, 16, ..., 1).
 *  6 m = (sum w d) / sw;  C = ((sum w d d^T) / sw - m m^T) / r2_s;  then the plane fit's eigen-solve (the arithmetic of
 *    nesti_sym3_eig), normalisation in fp64, one rounding to f32 and the sign rule: its solve with sw in the place of the count.
 *  7 The iteration FAILS if not sw > 0, if fewer than 3 slots have w_i > 0, or if the new normal is 0 0 0 or has a non-finite
 *    component.  After a failure g stays as it was and the row stops.  Otherwise g = the new normal.
 *  The state between iterations is the f32 normal alone: iters = T equals T chained calls of iters = 1 through init_normals_dev, bit for
 *  bit.  The result is g after the last iteration -- after a failure in the first one therefore the start normal under the sign rule,
 *  as given (not renormalised).  iters = 0: (float)v of step 1, put under the sign rule once more (a component may round to zero).
 *  8 OUTPUTS (device; any may be NULL, which leaves the others unchanged):
 *      normals_out_dev [M,S,3]  f32    the robust normal
 *      plane_out_dev   [M,S,3]  f32    plane of step 0
 *      support_out_dev [M,S]    f32    (float)sw of the last successful iteration, 0 if none
 *      inliers_out_dev [M,S]    int32  the slots with |res_i| <= sig in that iteration
 *      iters_out_dev   [M,S]    int32  the successful iterations
 *      moments_out_dev [M,S,10] fp64   the ten sums of that iteration in the order of step 5; zeros if none
 *      radius_out_dev  [M,S]    f32    (float)sqrt(r2_s), as the other list entries write it, skipped rows included
 *      count_out_dev   [M,S]    int32  n_s, likewise
 * DETERMINISM: no atomics.  A row's bits are a pure function of (cloud, centre, list prefix, ks, iters, sigma, falloff, floor, its
 * init row): independent of batching, of streams and of the grid the list came from.
 * Argument errors -- those of nesti_pca_normals_nbr; iters, sigma, falloff or floor outside the ranges above (NaN included) -- are
 * reported under the entry's name before any device call; M = 0 is a no-op.  Each call enqueues one kernel on `stream`, neither
 * synchronises nor reads anything back, and can be captured into a graph.  Under nesti_profile_enable the launch is booked in the
 * patches category, like the other list fits. */
int nesti_robust_normals_nbr(const float* cloud_dev, int N, const int32_t* query_idx_dev, int M, int query_row0, const int32_t* nbr_dev,
                             int K, const int32_t* ks, int S, int iters, double sigma, double falloff, double floor,
                             const float* init_normals_dev, float* normals_out_dev, float* plane_out_dev, float* support_out_dev,
                             int32_t* inliers_out_dev, int32_t* iters_out_dev, double* moments_out_dev, float* radius_out_dev,
                             int32_t* count_out_dev, void* stream);
int nesti_robust_normals_nbr_at(const float* cloud_dev, int N, const float* query_xyz_dev, int M, const int32_t* nbr_dev, int K,
                                const int32_t* ks, int S, int iters, double sigma, double falloff, double floor,
                                const float* init_normals_dev, float* normals_out_dev, float* plane_out_dev, float* support_out_dev,
                                int32_t* inliers_out_dev, int32_t* iters_out_dev, double* moments_out_dev, float* radius_out_dev,
                                int32_t* count_out_dev, void* stream);

/* ---- feature-preserving normal smoothing over neighbour lists (smooth.hip; DESIGN.md 2 "Normal smoothing") ------------------------
 * One pass of a bilateral filter of normals (Jones et al. 2004, Sun et al. 2007, the anisotropic normal smoothing of Huang et al.
 * 2013): a row's normal becomes the weighted mean of its neighbours' normals, the weight falling to zero where a neighbour's normal
 * leaves a cone round the row's own -- rows agree along a face, not across a crease.  It runs after any estimator; positions never
 * move.  The conventions are the library's own: fp64 throughout, every operation rounded on its own, only + - x / sqrt, comparisons
 * and integer arithmetic -- a restatement in plain IEEE arithmetic predicts every output bit.
 *
 * Centres (query_idx_dev / query_row0, M rows), nbr_dev [M, K] with row stride K (1 <= K <= NESTI_KNN_MAX_K) and the valid prefix are
 * exactly as for nesti_pca_normals_nbr: the list is untrusted, the prefix ends at the first entry outside [0, N), and a non-finite
 * centre position has an empty prefix.  normals_in_dev [N, 3] f32 holds a normal for every cloud point and is indexed like the cloud.
 * k in 1 .. K: the number of leading entries used.  cos_t and falloff: fp64 on the host.  There is no _at entry: a position has no
 * normal of its own to compare with.
 *  1 ELIGIBILITY.  A normal is eligible iff its three components are finite and one is non-zero, tested on the bits (the rule of
 *    nesti_orient_normals).  c = the centre's cloud index, n_c = normals_in[c], q_c = (x x + y y) + z z of n_c in fp64.  A row whose
 *    n_c is not eligible, or whose prefix is empty, gets the three floats of normals_in[c] copied bit for bit, support 0 and count 0.
 *  2 PREFIX.  n = min(k, valid prefix); d = (double)p - (double)c and d2 = (dx dx + dy dy) + dz dz per slot; r2 = the largest d2 of
 *    the prefix.
 *  3 SLOT i < n with neighbour j, n_j = normals_in[j] eligible (an ineligible neighbour adds nothing), q_j like q_c:
 *      d = (n_c.x n_j.x + n_c.y n_j.y) + n_c.z n_j.z;   ca = |d| / sqrt(q_c q_j);   t = (ca - cos_t) / (1 - cos_t);
 *      if not t > 0 the slot adds nothing (this also catches NaN);   t = min(t, 1);
 *      u = 1 - (falloff d2) / r2 if r2 > 0, else u = 1;   W = (u u) (t t);
 *      g = W / sqrt(q_j), negated if d < 0 -- the unoriented alignment: a neighbour counts on the centre's side;
 *      X += g n_j.x, Y += g n_j.y, Z += g n_j.z;   Wsum += W;   cnt += 1, an integer.
 *  4 ORDER.  Lane l of a 64-lane wave adds its slots l, l + 64, ... in ascending order into partial sums that start at +0.0; the lanes
 *    meet in an xor-butterfly (offsets 32, 16, ..., 1): the order of the other list fits.
 *  5 RESULT.  nn = (X X + Y Y) + Z Z; if nn > 0 and finite the output is (X, Y, Z) / sqrt(nn), rounded to f32 once, zeros written as
 *    +0; otherwise the input row is copied bit for bit (support and count are still those of step 3).  No sign rule is applied:
 *    every term lies in the centre's closed half-space, so an oriented field stays oriented and an unoriented one keeps each row's
 *    side.
 *  6 OUTPUTS (device; any may be NULL):
 *      normals_out_dev [M,3] f32
 *      support_out_dev [M]   f32    (float)Wsum
 *      count_out_dev   [M]   int32  cnt
 * DETERMINISM: no atomics.  A row's bits are a pure function of (cloud, centre, list prefix, the normals it reads, k, cos_t, falloff).
 * Argument errors -- those of nesti_pca_normals_nbr; a null normals_in_dev; k outside 1 .. K; cos_t not finite or outside
 * [0, 0.999999]; falloff not finite or outside [0, 1]; normals_out_dev == normals_in_dev (the pass is a Jacobi step: rows read their
 * neighbours' input) -- are reported before any device call; M = 0 is a no-op.  Each call enqueues one kernel on `stream`, neither
 * synchronises nor reads anything back, and can be captured into a graph.  Under nesti_profile_enable the launch is booked in the
 * patches category, like the other list fits. */
int nesti_smooth_normals_nbr(const float* cloud_dev, int N, const float* normals_in_dev, const int32_t* query_idx_dev, int M,
                             int query_row0, const int32_t* nbr_dev, int K, int k, double cos_t, double falloff, float* normals_out_dev,
                             float* support_out_dev, int32_t* count_out_dev, void* stream);
/* Measurement and tests only: the lane group that serves a row of nesti_smooth_normals_nbr in this process.  0 (the default): the
 * smallest of 16, 32 and 64 lanes that holds k; 16, 32 or 64: at least that many (a group smaller than k is widened to hold it), so 64
 * forces the one-wave-per-row form.  The choice moves the time of a pass, never a byte of its result.  Any other value is refused. */
int nesti_debug_smooth_lanes(int lanes);

/* ---- point denoising over neighbour lists (denoise.hip; DESIGN.md 2 "Point denoising") -----------------------------------------------
 * One pass of the bilateral point filter (Fleishman, Drori and Cohen-Or 2003; Digne and de Franchis 2017; the projection step of Huang
 * et al. 2013): a row's point moves along its own normal by the weighted mean of its neighbours' heights over its tangent plane.  The
 * weight is smoothing's cone weight on the normals times a distance falloff times a Geman-McClure weight on the height, so a face is
 * flattened and a crease is not rounded off.  It runs between outlier removal and estimation; normals are read, never written.  The
 * conventions are the library's own: fp64 throughout, every operation rounded on its own, only + - x / sqrt, comparisons and integer
 * arithmetic -- a restatement in plain IEEE arithmetic predicts every output bit.
 *
 * Centres (query_idx_dev / query_row0, M rows), nbr_dev [M, K] with row stride K (1 <= K <= NESTI_KNN_MAX_K) and the valid prefix are
 * exactly as for nesti_smooth_normals_nbr.  normals_in_dev [N, 3] f32 holds a normal for every cloud point and is indexed like the
 * cloud.  k in 1 .. K: the number of leading entries used.  cos_t in [0, 0.999999], falloff in [0, 1], sigma in (0, 1e6] (the height
 * scale in neighbourhood radii; at 1e6 the height weight is 1 to rounding) and step in (0, 1]: fp64 on the host.  There is no _at
 * entry: a position that is not a cloud point has nothing to move.
 *  1 ELIGIBILITY.  As for nesti_smooth_normals_nbr, on the bits.  c = the centre's cloud index, p_c = cloud[c], n_c = normals_in[c],
 *    q_c = (x x + y y) + z z of n_c in fp64.  A row whose n_c is not eligible, whose prefix is empty or whose centre is not finite
 *    moves nothing: the three floats of p_c are copied bit for bit, delta, support and count are 0.
 *  2 PREFIX.  n = min(k, valid prefix); d = (double)p - (double)c and d2 = (dx dx + dy dy) + dz dz per slot; r2 = the largest d2 of
 *    the prefix; rad = sqrt(r2).
 *  3 CENTRE NORMAL.  v = (double)n_c / sqrt(q_c), component by component.
 *  4 SLOT i < n with neighbour j, n_j = normals_in[j] eligible (an ineligible neighbour adds nothing), q_j like q_c:
 *      t as in step 3 of nesti_smooth_normals_nbr: dd = (n_c.x n_j.x + n_c.y n_j.y) + n_c.z n_j.z;   ca = |dd| / sqrt(q_c q_j);
 *      t = (ca - cos_t) / (1 - cos_t);   if not t > 0 the slot adds nothing (this also catches NaN);   t = min(t, 1);
 *      u = 1 - (falloff d2) / r2 if r2 > 0, else u = 1;
 *      h = (v.x dx + v.y dy) + v.z dz;   x = h / (sigma rad) if r2 > 0, else x = 0;   g = 1 / (1 + x x);
 *      a = (u t) g;   W = a a;   H += W h;   Wsum += W;   cnt += 1, an integer.
 *  5 ORDER.  That of nesti_smooth_normals_nbr: lane l of a 64-lane wave adds its slots l, l + 64, ... in ascending order into partial
 *    sums that start at +0.0; the lanes meet in an xor-butterfly (offsets 32, 16, ..., 1).
 *  6 RESULT.  If Wsum > 0 and delta = step (H / Wsum) is finite, the output is (float)((double)p_c + delta v) per component, the
 *    product and the sum rounded separately; otherwise the input row is copied bit for bit and delta is 0 (support and count are
 *    still those of step 4).
 *  7 OUTPUTS (device; any may be NULL):
 *      points_out_dev  [M,3] f32
 *      delta_out_dev   [M]   f32    (float)delta, the signed displacement along the centre's normal
 *      support_out_dev [M]   f32    (float)Wsum
 *      count_out_dev   [M]   int32  cnt
 * DETERMINISM: no atomics.  A row's bits are a pure function of (cloud, centre, list prefix, the normals it reads, k, cos_t, falloff,
 * sigma, step).  The output position does not depend on the sign of any input normal; delta takes the sign of the centre's.
 * Argument errors -- those of nesti_smooth_normals_nbr; sigma not finite or outside (0, 1e6]; step not finite or outside (0, 1];
 * points_out_dev [M,3] overlapping the cloud [N,3], equal base pointers included (the pass is a Jacobi step: rows read their
 * neighbours' input positions) -- are reported before any device call; M = 0 is a no-op.  Each call enqueues one kernel on `stream`,
 * neither synchronises nor reads anything back, and can be captured into a graph.  Under nesti_profile_enable the launch is booked in
 * the patches category, like the other list fits. */
int nesti_denoise_points_nbr(const float* cloud_dev, int N, const float* normals_in_dev, const int32_t* query_idx_dev, int M,
                             int query_row0, const int32_t* nbr_dev, int K, int k, double cos_t, double falloff, double sigma,
                             double step, float* points_out_dev, float* delta_out_dev, float* support_out_dev, int32_t* count_out_dev,
                             void* stream);
/* Measurement and tests only: the lane group that serves a row of nesti_denoise_points_nbr in this process, as
 * nesti_debug_smooth_lanes: 0 (the default) the smallest of 16, 32 and 64 lanes that holds k; 16, 32 or 64: at least that many.  The
 * choice moves the time of a pass, never a byte of its result.  Any other value is refused. */
int nesti_debug_denoise_lanes(int lanes);

/* ---- outlier removal before estimation (outlier.hip; DESIGN.md 2 "Outlier removal") --------------------------------------------------
 * The statistical and the radius outlier filter of a point cloud as three passes over the sorted lists nesti_knn returns: a score per
 * row, the statistics of a score array, an ordered compaction.  The conventions are the library's own: fp64 throughout, every
 * operation rounded on its own, only + - x / sqrt, comparisons and integer arithmetic, no atomics -- a restatement in plain IEEE
 * arithmetic predicts every output bit, and the kept set is a pure function of (cloud, parameters): independent of batching, streams,
 * the grid and the grid build.  No parity with any published code is claimed.
 *
 * nesti_outlier_scores_nbr: row q of M is cloud point c = query_row0 + q; nbr_dev [M, K] with row stride K (2 <= K <= NESTI_KNN_MAX_K)
 * is untrusted, as for nesti_pca_normals_nbr; 1 <= k < K.  P = min(k + 1, valid prefix), the prefix ending at the first entry outside
 * [0, N); d = (double)p - (double)c and d2 = (dx dx + dy dy) + dz dz per slot, as nesti_knn forms them.  Of the slots below P the first
 * whose INDEX is c is skipped (the index, not d2 == 0: duplicates tie and sort by index); where none is, the slots below min(k, P) are
 * used.  n_other = the number of slots used.
 *      mean_out_dev    [M] f64    (the sum of sqrt(d2) over the used slots) / n_other;  +inf where n_other == 0
 *      kth_d2_out_dev  [M] f64    the largest d2 used where n_other == k, else +inf
 *      n_other_out_dev [M] int32
 *  ORDER: slot i is added in lane i mod 64, a lane's slots in ascending order from +0.0; the lanes meet in an xor-butterfly (offsets 32,
 *  16, ..., 1): the order of the list fits.  A used slot whose d2 is NaN makes mean and kth_d2 the quiet NaN 0x7ff8000000000000; a centre
 *  with a non-finite coordinate has that mean and kth_d2 and n_other = 0.  Any output may be NULL.  One kernel.
 *
 * nesti_outlier_threshold: the statistics of ANY fp64 score array scores_dev [M] on the device.  A non-finite score (on the bits) is
 * absent: value +0, count 0.  Blocks of 256 consecutive rows are reduced by stride halving (v[t] = v[t] + v[t + s], s = 128, 64, ..., 1);
 * one workgroup of 256 reduces the block partials: thread t adds partials t, t + 256, ... in ascending order to +0.0, then the same
 * stride halving.  Pass 1: S and n, mean = S / n.  Pass 2: Q = the sum of (s - mean)(s - mean) by the same tree.
 *      stats_out_dev [4] f64:  n,  mean,  std = sqrt(Q / (n - 1)) for n >= 2 else 0,  thr = mean + std_ratio std
 *  n == 0: mean = std = 0 and thr = +inf.  ws_dev: nesti_outlier_workspace_bytes(M) bytes.  Four kernels.
 *
 * nesti_outlier_compact: row i of the N is KEPT iff scores_dev[i] is finite and <= the threshold -- *thr_dev (device; a threshold of
 * nesti_outlier_threshold, say &stats[3]) or, where thr_dev is NULL, the host value thr.  A tie is kept; NaN and the infinities leave.
 * Per-block counts, one single-workgroup scan, a scatter in row order (the scheme of nesti_depth_to_cloud).  Outputs (device; any but
 * n_kept_out_dev may be NULL; the caller sizes them for N rows):
 *      xyz_out_dev        [n_kept,3] f32    the kept rows of cloud_dev, copied bit for bit (cloud_dev may be NULL without it)
 *      kept_idx_out_dev   [n_kept]   int32  their indices, ascending
 *      new_of_old_out_dev [N]        int32  the new index of every row, -1 for a removed one
 *      keep_out_dev       [N]        uint8  1 / 0
 *      n_kept_out_dev     [1]        int32
 *  ws_dev: nesti_outlier_workspace_bytes(N) bytes.  Three kernels.  The radius filter is this entry over kth_d2 with
 *  thr = radius * radius and k = min_neighbours: it keeps the rows with at least that many other points within the radius.
 *
 * Argument errors -- a null pointer; N <= 0; K outside 1 .. NESTI_KNN_MAX_K or k outside 1 .. K - 1; M < 0; query_row0 < 0 or rows
 * beyond the cloud; a short workspace; a std_ratio or a host thr that is not finite or negative -- are reported before any device call.
 * M = 0 is a no-op for the scores and the statistics.  No entry synchronises or reads anything back; each can be captured into a
 * graph.  Under nesti_profile_enable the launches are booked in the patches category. */
size_t nesti_outlier_workspace_bytes(int n);
int nesti_outlier_scores_nbr(const float* cloud_dev, int N, int query_row0, int M, const int32_t* nbr_dev, int K, int k,
                             double* mean_out_dev, double* kth_d2_out_dev, int32_t* n_other_out_dev, void* stream);
int nesti_outlier_threshold(const double* scores_dev, int M, double std_ratio, double* stats_out_dev, void* ws_dev, size_t ws_bytes,
                            void* stream);
int nesti_outlier_compact(const float* cloud_dev, int N, const double* scores_dev, const double* thr_dev, double thr, float* xyz_out_dev,
                          int32_t* kept_idx_out_dev, int32_t* new_of_old_out_dev, uint8_t* keep_out_dev, int32_t* n_kept_out_dev,
                          void* ws_dev, size_t ws_bytes, void* stream);
/* Measurement and tests only: the lane group that serves a row of nesti_outlier_scores_nbr in this process.  0 (the default): the
 * smallest of 16, 32 and 64 lanes that holds k + 1; 16, 32 or 64: at least that many.  The choice moves the time of a pass, never a byte
 * of its result.  Any other value is refused. */
int nesti_debug_outlier_lanes(int lanes);

/* ---- voxel-grid downsampling before estimation (voxel.hip; DESIGN.md 2 "Voxel downsampling") ---------------------------------------
 * One point per occupied cell of a regular grid, as three entries: a key per row, a stable device-wide radix sort of (key, row index)
 * pairs, a reduction of the sorted runs.  The conventions are the library's own: fp64 where there is arithmetic, every operation
 * rounded on its own, only + - x /, floor, comparisons and integer arithmetic, no floating-point atomics and no global-memory atomics,
 * no workgroup waits on another -- a restatement in plain IEEE arithmetic predicts every output bit, and every output is a pure
 * function of its inputs: independent of streams and of timing.  No parity with any published code is claimed.
 *
 * nesti_voxel_workspace_bytes: the one size that serves nesti_sort_pairs and nesti_voxel_reduce over n rows; a multiple of 256; 0 for
 * n <= 0.  nesti_sort_tile_items: the keys one workgroup handles per pass of the sort, a constant (tests place their sizes around it).
 *
 * nesti_voxel_keys: origin [3] and voxel [3] are HOST doubles, dims [3] HOST int64; keys_out_dev [N] uint64.  Per axis a:
 *      d_a = (double)p_a - origin_a,  t_a = d_a / voxel_a,  i_a = (int64)floor(t_a);   key = (i_z dims_y + i_y) dims_x + i_x
 *  A row with a non-finite coordinate (tested on the bits) or with an i_a outside [0, dims_a) is LOST: its key is dims_x dims_y dims_z,
 *  one past the largest real key, so lost rows sort last.  One kernel.
 *
 * nesti_sort_pairs: keys_out_dev [N] uint64 and idx_out_dev [N] int32 = the keys of keys_in_dev [N] in ascending order of their low
 * key_bits (1 .. 64) bits and the row each came from; rows of equal low bits keep their order (STABLE): the result is
 * argsort(keys & mask, stable).  Keys are carried whole; bits at and above key_bits take no part in the order.  Least-significant-digit
 * radix sort, 8-bit digits, ceil(key_bits / 8) passes that ping-pong between the outputs and the workspace; a pass is a per-workgroup
 * digit histogram of a tile (one 256-bin LDS histogram per wave), a two-level scan of the digit-major table [256, blocks] (chunks of
 * 4096 entries by a workgroup each, their totals by ONE workgroup) and a scatter in which a workgroup recomputes the stable rank of
 * each of its keys among the keys of the same digit in its tile with 64-bit ballots: four kernels per pass.  keys_out_dev must not be keys_in_dev (keys_in_dev is left as it is).  ws_dev: nesti_voxel_workspace_bytes(N) bytes.
 *
 * nesti_voxel_reduce: sorted_keys_dev / sorted_idx_dev [N] as nesti_sort_pairs returns them for the keys of nesti_voxel_keys (row
 * indices outside [0, N) are skipped, never followed); lost_key = dims_x dims_y dims_z; origin as for the keys.  Sorted position i
 * starts a voxel when key[i] != key[i - 1] and key[i] != lost_key; ordered compaction by per-block counts, one single-workgroup scan
 * and a scatter (the scheme of nesti_outlier_compact).  Voxels come in ascending key order (z-major).  Outputs (device; any but
 * n_voxels_out_dev may be NULL; the per-voxel ones are sized for N rows by the caller, the first V are written):
 *      centroid_out_dev [V,3] f32    c_a = origin_a + S_a / (double)count, rounded to f32 once
 *      rep_out_dev      [V]   int32  the row nearest the fp64 centroid: the smallest (d2, index), e_a = d_a - S_a / count,
 *                                    d2 = (e_x e_x + e_y e_y) + e_z e_z
 *      count_out_dev    [V]   int32
 *      key_out_dev      [V]   uint64
 *      voxel_of_out_dev [N]   int32  the voxel of every row, -1 for a lost one
 *      n_voxels_out_dev [1]   int32  V
 *  ORDER of S_a: a voxel's rows come in ascending index (the sort is stable); row number s of the voxel adds d_a = (double)p_a - origin_a
 *  in lane s mod 64, a lane's slots in ascending order from +0.0; the lanes meet in an xor-butterfly (offsets 32, 16, ..., 1): the order
 *  of the list fits.  An idle lane holds +0.0 and changes no bit, so a voxel of up to 256 rows is served by 16 lanes with four
 *  accumulators each, met as (a0 + a2) + (a1 + a3), and a larger one by a whole wave: the same bytes.  ws_dev:
 *  nesti_voxel_workspace_bytes(N) bytes.  Four kernels (three where centroid, rep and count are all NULL).
 *
 * Argument errors -- a null pointer; N <= 0; a voxel size that is not finite or not > 0; a non-finite origin; a dims entry < 1 or a
 * product of the dims >= 2^62; key_bits outside 1 .. 64; keys_out_dev == keys_in_dev; a short workspace -- are reported before any
 * device call.  No entry synchronises or reads anything back; each can be captured into a graph.  Under nesti_profile_enable the
 * launches are booked in the patches category. */
size_t nesti_voxel_workspace_bytes(int n);
int nesti_sort_tile_items(void);
int nesti_voxel_keys(const float* cloud_dev, int N, const double* origin, const double* voxel, const int64_t* dims, uint64_t* keys_out_dev,
                     void* stream);
int nesti_sort_pairs(const uint64_t* keys_in_dev, int N, int key_bits, uint64_t* keys_out_dev, int32_t* idx_out_dev, void* ws_dev,
                     size_t ws_bytes, void* stream);
int nesti_voxel_reduce(const float* cloud_dev, int N, const uint64_t* sorted_keys_dev, const int32_t* sorted_idx_dev, uint64_t lost_key,
                       const double* origin, float* centroid_out_dev, int32_t* rep_out_dev, int32_t* count_out_dev, uint64_t* key_out_dev,
                       int32_t* voxel_of_out_dev, int32_t* n_voxels_out_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- depth images in, normal images out (depth.hip; DESIGN.md 2 "Depth images") --------------------------------------------------
 * The two ends of the reference's Kinect route: MATLAB/ScanNet_depth2xyz.m (depth + intrinsics + pose -> cloud) before
 * test_n_est_w_experts.py, and MATLAB/ScanNet_world2cam_normals.m / MATLAB/export_visualizations_nyu.m:146-153 (per-point results
 * -> image) after it.  The conventions are the library's own, because the reference's are MATLAB's:
 *   - pixel coordinates are 0-BASED, u = column, v = row.  The MATLAB files are 1-based: a caller with MATLAB-convention intrinsics
 *     passes cx - 1, cy - 1;
 *   - the pose is applied as a proper rigid transform, translation included.  ScanNet_depth2xyz.m:14 multiplies with a homogeneous
 *     coordinate of 0 and thereby drops the translation; that is not reproduced;
 *   - where several rows project onto one pixel the NEAREST wins and among equals the smaller row index (the reference lets the last
 *     row win).
 * nesti_camera_t lives on the HOST.  pose: row-major 3 x 4 [R | t], read only when has_pose != 0 -- camera -> world for
 * nesti_depth_to_cloud, world -> camera (the caller inverts) for nesti_project_to_image.  z_near / z_far: 0 and +inf keep everything.
 *
 * nesti_depth_to_cloud: depth_dev [H,W] uint16 or float32 (NESTI_DEPTH_*).  A pixel is VALID iff z = (double)raw * depth_scale is
 * finite (a float's finiteness is tested on its bits), > 0 and inside [z_near, z_far].  In fp64, every operation rounded on its own:
 *     xc = ((u - cx) * z) / fx,  yc = ((v - cy) * z) / fy,  zc = z,
 *     with a pose X_r = ((T[r][0] * xc + T[r][1] * yc) + T[r][2] * zc) + T[r][3],
 * then ONE rounding to float32.  Outputs, all in row-major pixel order (the order of the reference's loop):
 *   xyz_dev [n_valid,3] f32 and pix_dev [n_valid] int32 (pixel index v W + u): the caller provides room for H W rows;
 *   rank_dev [H W] int32 (optional): the cloud row of a pixel, or -1;
 *   qidx_dev (optional; room for ceil(H / stride) ceil(W / stride) entries): the cloud rows of the valid pixels with v % stride == 0
 *     and u % stride == 0, in pixel order -- what nesti_estimate_normals takes as query_idx_dev;
 *   counts_dev [2] int32 = {n_valid, n_queries}, on the DEVICE.
 * The compaction is deterministic and atomic-free: per-block counts, one single-workgroup scan over them, a scatter; no workgroup
 * waits on another.
 *
 * nesti_image_scatter: rows_dev [M,C] of 4-byte elements (f32 or int32) are written to image_dev [H,W,C] at the pixels pix_dev [M];
 * every other element is fill[C] (HOST, 4-byte elements).  pix entries must be distinct (they are by construction); an entry outside
 * [0, H W) is skipped.  M = 0 gives an all-fill image.
 *
 * nesti_project_to_image: for a cloud that did not come from nesti_depth_to_cloud.  Per row, in fp64, every operation rounded on its
 * own: camera coordinates (through `pose` as above if has_pose), u = floor(((xc * fx) / zc + cx) + 0.5), v likewise with fy, cy.  A
 * row lands iff its three floats and zc are finite, zc > 0 and 0 <= u < W, 0 <= v < H.  Per pixel the smallest key
 * (bits of (float)zc) << 32 | row wins (64-bit atomicMin); image_dev [H,W,C] gets the winner's values_dev[row, 0:C] (4-byte elements)
 * or fill[C]; index_image_dev [H,W] int32 (optional) the winning row or -1.  image_dev may be NULL when only the index is wanted.
 * depth_scale, z_near and z_far are checked but not used.
 *
 * ws_dev: nesti_depth_workspace_bytes(H, W) bytes (nesti_depth_to_cloud, nesti_project_to_image).  Argument errors -- null pointers,
 * H or W <= 0, H W > 2^26, stride < 1, fx or fy zero or not finite, cx / cy / depth_scale / pose not finite, depth_scale <= 0,
 * z_near > z_far, C outside 1 .. 8, M < 0, a short workspace, an unknown depth type -- are reported before any device call.  The calls
 * enqueue on `stream` and neither synchronise nor read anything back. */
enum { NESTI_DEPTH_U16 = 0, NESTI_DEPTH_F32 = 1 };
typedef struct {
  double fx, fy, cx, cy;
  double depth_scale;      /* metres (or any unit) per raw depth value: 1e-3 for uint16 millimetres */
  double z_near, z_far;
  int has_pose;
  double pose[12];
} nesti_camera_t;
/* host only; 0 for H or W <= 0 and for H W > 2^26 */
size_t nesti_depth_workspace_bytes(int H, int W);
int nesti_depth_to_cloud(const void* depth_dev, int depth_type, int H, int W, const nesti_camera_t* camera, int stride,
                         float* xyz_dev, int32_t* pix_dev, int32_t* rank_dev, int32_t* qidx_dev, int32_t* counts_dev,
                         void* ws_dev, size_t ws_bytes, void* stream);
int nesti_image_scatter(const void* rows_dev, const int32_t* pix_dev, int M, int C, int H, int W, const void* fill,
                        void* image_dev, void* stream);
int nesti_project_to_image(const float* xyz_dev, const void* values_dev, int M, int C, int H, int W,
                           const nesti_camera_t* camera, const void* fill, void* image_dev, int32_t* index_image_dev,
                           void* ws_dev, size_t ws_bytes, void* stream);

/* ---- image-window neighbour lists (window.hip; DESIGN.md 2 "Image-window neighbourhoods") ------------------------------------------
 * A depth frame is an organized cloud: the neighbours of a pixel's point are, almost always, points of nearby pixels, and rank_dev of
 * nesti_depth_to_cloud is the search structure.  nesti_depth_window_knn returns, per row, the K nearest among the points of a
 * (2 R + 1) x (2 R + 1) pixel window -- lists every nesti_*_nbr entry takes -- and PROVES where that list is the exact list of nesti_knn.
 * Everything is fp64, every operation rounded on its own, only + - * / sqrt, fabs and comparisons: a restatement in plain IEEE
 * arithmetic predicts every bit.
 * CENTRE.  Cloud row i = query_idx_dev[q] (clamped into the cloud, as for nesti_knn), or query_row0 + q where query_idx_dev is NULL.
 * Its pixel is p = pix_dev[i], v0 = p / W, u0 = p % W.  A p outside [0, H W), or a centre with a non-finite coordinate (tested on the
 * bits), gives count 0 and proven 0.
 * CANDIDATES.  One per pixel of [u0 - R, u0 + R] x [v0 - R, v0 + R], clipped to the image, whose rank_dev entry j lies in [0, N).
 * rank_dev [H W] and pix_dev [N] are untrusted: no entry causes an out-of-bounds read.
 * LIST.  d2_j as nesti_knn computes it from the f32 rows (d = (double)p_j - (double)c, d2 = (dx dx + dy dy) + dz dz; a NaN d2 is never
 * a neighbour).  The result is the K smallest pairs (d2_j, j), ascending:
 *     nbr_out_dev    [M, K] int32   j
 *     d2_out_dev     [M, K] fp64    d2_j                                  (may be NULL)
 *     count_out_dev  [M]    int32   min(K, candidates)                    (may be NULL)
 *     proven_out_dev [M]    int32   1: the list is nesti_knn's, bit for bit (may be NULL)
 * Slots beyond the count hold -1 and +inf.  1 <= K <= NESTI_KNN_MAX_K, 1 <= R <= NESTI_WINDOW_MAX_R.
 * PROOF.  A valid pixel outside the window lies, in the camera frame, beyond one of the four planes through the camera centre and
 * the window's edges; the distance from the centre to the nearest of them is a lower bound on the distance to every point outside.
 * A side has image beyond it when u0 - R > 0 (left), u0 + R < W - 1 (right), likewise top and bottom in v.  For such a side:
 *     e    = (u0 - R) - 0.5, resp. (u0 + R) + 0.5 (likewise in v): the edge coordinate
 *     a    = (e - cx) / fx                       (cy, fy for top and bottom)
 *     m_r  = T[r][axis] - a * T[r][2],  rel_r = c_r - T[r][3]   (axis 0 for left / right, 1 for top / bottom; T the pose, the
 *                                                                identity without one)
 *     s    = (m_0 rel_0 + m_1 rel_1) + m_2 rel_2,   dist = fabs(s) / sqrt(1 + a a)
 * bound is the smallest dist over those sides.  With no such side the window covers the image and proven = 1.  Otherwise
 *     b = max(0, bound (1 - 2^-21) - 2^-21 ((|c_0| + |c_1|) + |c_2|)),   proven = (count == K) && d2[K - 1] < b b   (strictly).
 * The margin covers the one f32 rounding of every stored point (8 x the bound derived in csrc/window.hip); the half pixel between the
 * edge and the first pixel centre outside covers the fp64 noise of nesti_depth_to_cloud.  The proof presumes that xyz_dev, pix_dev,
 * rank_dev and camera come from ONE nesti_depth_to_cloud call, that the points have not moved since, and that the pose is rigid.
 * Otherwise the lists are still as defined and proven means nothing.  depth_scale, z_near and z_far are not read.
 * One wave per row; the window's pairs go to an LDS buffer by ballot compaction and are sorted once: no atomics, no dependence on
 * which workgroup runs first.  Argument errors (null cloud / pix / rank / camera / nbr_out_dev, N <= 0, H or W <= 0, H W > 2^26, fx or
 * fy zero or not finite, cx / cy / pose not finite, R or K out of range, M < 0, rows beyond the cloud) are reported before any device
 * call; M = 0 is a no-op.  The call enqueues one kernel on `stream`, neither synchronises nor reads anything back, and is booked in
 * the patches category under nesti_profile_enable. */
#define NESTI_WINDOW_MAX_R 15   /* (2 R + 1)^2 = 961 candidates at most: one fill of the search's pair buffer */
int nesti_depth_window_knn(const float* xyz_dev, int N, const int32_t* pix_dev /*[N]*/, const int32_t* rank_dev /*[H W]*/,
                           int H, int W, const nesti_camera_t* camera, const int32_t* query_idx_dev, int M, int query_row0,
                           int R, int K, int32_t* nbr_out_dev, double* d2_out_dev, int32_t* count_out_dev,
                           int32_t* proven_out_dev, void* stream);

/* Several shapes in flight (BASELINE config 4; also every rank of a multi-GPU job, which holds a block of rows of
 * every shape): the queries of all items are processed as ONE stream of `batch`-sized batches, so small shapes / small
 * shards share the gate and expert launches instead of each paying for its own partially filled rounds.  Item i
 * contributes n_queries rows (as nesti_estimate_normals would for that shape, search grid already built); outputs are the
 * items' rows concatenated in order: [sum n_queries, 3], [sum], [sum, E].  8^3 Gaussian grid. */
typedef struct {
  const float* cloud_dev;        /* [n_points, 3] f32 */
  int n_points;
  const int32_t* query_idx_dev;  /* [n_queries] or NULL = rows query_row0 .. query_row0 + n_queries - 1 */
  int n_queries;
  double r_abs[NESTI_MAX_SCALES];
  uint64_t seed;
  int query_row0;
  const void* grid_ws_dev;       /* from nesti_patches_grid on this shape */
  size_t grid_ws_bytes;
} nesti_shape_queries_t;
int nesti_estimate_normals_multi(const nesti_model_t* m, const nesti_shape_queries_t* items, int n_items, int batch,
                                 void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev,
                                 float* probs_out_dev, void* stream);

/* nesti_estimate_normals_multi for query POSITIONS (generalises utils/pcpnet_dataset.py:304, see nesti_patches_query_at): what
 * sharded and multi-shape runs call.  Rows without a neighbourhood carry the sentinel of nesti_mask_empty_queries. */
typedef struct {
  const float* cloud_dev;        /* [n_points, 3] f32 */
  int n_points;
  const float* query_xyz_dev;    /* [n_queries, 3] f32 */
  int n_queries;
  double r_abs[NESTI_MAX_SCALES];
  uint64_t seed;
  int query_row0;                /* patch row of the item's first query: the subsample key */
  const void* grid_ws_dev;       /* from nesti_patches_grid on this shape */
  size_t grid_ws_bytes;
} nesti_shape_positions_t;
int nesti_estimate_normals_multi_at(const nesti_model_t* m, const nesti_shape_positions_t* items, int n_items, int batch,
                                    void* ws_dev, size_t ws_bytes, float* normals_out_dev, int32_t* expert_out_dev,
                                    float* probs_out_dev, void* stream);

/* ---- the reference's own subsample stream, replayed on the host (refreplay.cpp) ----------
 * utils/pcpnet_dataset.py:237-240, 320-321: ONE numpy RandomState(seed) shared by every patch and scale of every shape, one
 * rng.choice(n, P, replace=False) per ball that holds n > P points, in visiting order (patch-major, scale-minor).  The stream
 * object holds the MT19937 state between calls.  nesti_refstream_picks walks `n_balls` ball sizes in visiting order and writes,
 * for every over-full ball, the P positions choice() returns (positions in cKDTree's traversal-ordered ball, uint16: balls of
 * more than 65535 points are refused) at picks_out[offsets_out[b] .. + P); offsets_out[b] = -1 for a ball with n <= P (it draws
 * nothing).  A call that fails leaves the stream untouched.  Host only; bit-identical to numpy (tests/test_refreplay.py). */
typedef struct nesti_refstream nesti_refstream_t;
nesti_refstream_t* nesti_refstream_create(uint32_t seed);
void nesti_refstream_destroy(nesti_refstream_t* s);
int nesti_refstream_picks(nesti_refstream_t* s, const int32_t* sizes, int64_t n_balls, int P, uint16_t* picks_out,
                          int64_t picks_capacity, int64_t* offsets_out, int64_t* n_over_out);

/* ---- text I/O of the file seam (host only) ------------------------------------------------
 * Reading stays np.loadtxt (utils/pcpnet_dataset.py:250): numpy 2's parser is faster than a strtod loop, and the
 * .npy cache the reference writes next to the file makes it a one-off.  The writers are native: np.savetxt's
 * '%.18e' formatting dominates the wall time of a shape once the compute takes a second. */
/* np.savetxt(path, a) with the default '%.18e' format (test_n_est_w_experts.py:182-183, 187-188). */
int nesti_write_text_f32(const char* path, const float* data, int64_t rows, int cols);
/* np.savetxt(path, a.astype(int), fmt='%i') (test_n_est_w_experts.py:185-186). */
int nesti_write_text_i32(const char* path, const int32_t* data, int64_t rows);

/* CRC-32C of n host bytes continuing from `crc` (0 to start): the checksum of TensorFlow's tensor bundle, verified on
 * restore (test_n_est_w_experts.py:98-105 -> tf_ckpt.read_bundle).  Stored masked: ((crc >> 15) | (crc << 17)) + 0xa282ead8. */
uint32_t nesti_crc32c(const void* data, size_t n, uint32_t crc);

/* The OCP FP6 e2m3 code (sign bit 5, exponent bits 4-3 with bias 1, mantissa bits 2-0; grid 0, 0.125 .. 7.5) of value * inv_scale, rounded to
 * nearest even and saturating -- the host-side encoder of the FP6 weight packing (nesti_model_set_x8_format), exposed so that it can be
 * checked against the instruction's own decoding without a device (tests/test_abi.py; scripts/fp6_probe.hip holds the device side). */
int nesti_f32_to_e2m3(float value, float inv_scale);

/* ---- test hooks: one tower, launch by launch (no reference counterpart) -------------------------------------------
 * The per-layer conformance tests (tests/test_gpu_layers.py) check every conv and pool launch against an fp64 evaluation of
 * the same layer on the launch's own input.  nesti_debug_tower_ops describes a tower's buffers and launches from the
 * configuration alone (no device): where run_tower places every buffer in the tower workspace for `batch` queries, and what
 * every launch reads, computes and writes.  nesti_debug_tower_step runs launch `op` of that tower ALONE, on a caller
 * workspace laid out as described; steps 0 .. n_ops - 1 in order are exactly the product's tower pass. */
enum { NESTI_DEBUG_OP_CONV = 0, NESTI_DEBUG_OP_MAX = 1 /* max_pool3d 2^3 stride 2 */, NESTI_DEBUG_OP_MAX3 = 2 /* 3^3 stride 2 SAME, 3^3 grid */ };
enum { NESTI_DEBUG_FORM_PLAIN = 0, /* one product of f32 / f16 / bf16 elements                                          */
       NESTI_DEBUG_FORM_PAIR = 1,  /* hi W_hi + lo W_hi + hi W_lo (NESTI_F16X3 / NESTI_BF16X3; lo W_lo is dropped)         */
       NESTI_DEBUG_FORM_X2 = 2,    /* plain 16-bit activations times the pair-packed weights: hi (W_hi + W_lo) (filter pass) */
       NESTI_DEBUG_FORM_X8 = 3,    /* hi W_hi in f16 + the cross terms as e4m3 products (NESTI_F16X8 experts, format 8)     */
       NESTI_DEBUG_FORM_X6 = 4 };  /* ... as block-scaled e2m3 products (format 6)                                          */
typedef struct {
  int fast;     /* 1: the two-stage gate's plain-f16 filter pass (gating net of NESTI_F16X3C / NESTI_F16X8C models)          */
  int x8_mask;  /* (tower -1 of NESTI_F16X8C models: six bits, the gating net's 8^3 tap layers -- the form of recheck stage 2, format 6)
                   expert towers of NESTI_F16X8 / NESTI_F16X8C models: the tap layers that take the narrow cross terms
                 * (nesti_model_set_x8_layers; 0 = f16x3 proper)                                                           */
  int x8_fmt;   /* 8 or 6 (nesti_model_set_x8_format); 0 = 6.  nesti_debug_tower_step refuses a format the model does not run */
} nesti_debug_pass_t;
typedef struct {
  int64_t offset;  /* byte offset in the tower workspace; -1 for buffer 0, the caller's MuPS tensor                     */
  int64_t bytes;   /* bytes reserved for it (0: buffer 0, or a buffer this tower never uses)                            */
  int log2S;       /* rows per query: 2^(3 log2S), row = query * 2^(3 log2S) + voxel, channels last                     */
  int C;           /* logical channels of a row (zero-padded to 64)                                                     */
  int f32, aux8;   /* f32: a tower output in f32; aux8: a side buffer of cross-term codes, 2 bytes per channel          */
  int planes;      /* 2: pair layout (per 64-channel group [hi 64 | lo 64]); else 1                                     */
  int elem;        /* NESTI_F32 / NESTI_F16 / NESTI_BF16; -1 for aux8                                                    */
  int first, last; /* lifetime: the first op that writes it, the last op that reads it (n_ops: the tower's output)       */
} nesti_debug_buf_t;
typedef struct {
  int kind;             /* NESTI_DEBUG_OP_*                                                                          */
  int family;           /* conv: 0 conv_igemm_kernel, 2 conv8n_kernel, 3 conv4n_kernel; pools: -1                     */
  int form;             /* NESTI_DEBUG_FORM_* (pools: PLAIN or PAIR, the layout of their values)                      */
  int elem, planes;     /* element type and planes of the op's 16-bit / f32 activations                              */
  int layer;            /* conv: index of the layer in the model                                                     */
  const char* scope;    /* conv: TF scope; valid until the next call on this thread                                  */
  const char* scope2;   /* conv: "" or the fused 1x1x1 layer whose columns start at out_coff2 (conv4 of an inception) */
  int k, log2S, s_real, is_fc, bn, relu, pool_k, n_taps;
  int cin, cout, Cin_p, Cout_p;
  int in_pos_off;       /* conv: in_pos[in_pos_off + c] = padded input channel (relative to in_coff) of real channel c */
  int in_buf, in_coff, in_cstride, in_planes;   /* in_cstride: logical channels of an input row (a flattened view for fc1) */
  int out_buf, out_coff, out_coff2, out_f32;
  int mp_buf, mp_mode, mp_mode2;   /* fused 2^3 max-pool epilogue (kernels.h: ConvParams::mp_mode / mp_mode2)          */
  int aux_in_buf, aux_layer;       /* X8 / X6: the side buffer read and the layer that wrote it (else -1)              */
  int aux_out_buf;                 /* a producer in this pass: the side buffer it writes (else -1)                     */
  int C;                /* pools: channels                                                                           */
} nesti_debug_op_t;
/* tower -1 = gating net, 0..E-1 an expert; dtype as nesti_model_create; pass NULL = the model's main pass.  Array arguments
 * may be NULL (counts only); *ws_bytes = the tower workspace run_tower needs.  Host only. */
int nesti_debug_tower_ops(const nesti_config_t* cfg, int dtype, int tower, int batch, const nesti_debug_pass_t* pass,
                          nesti_debug_buf_t* bufs, int max_bufs, int* n_bufs, nesti_debug_op_t* ops, int max_ops, int* n_ops,
                          int32_t* in_pos, int max_in_pos, int* n_in_pos, size_t* ws_bytes);
/* Launch `op` of the tower on ws_dev (laid out for capacity `batch`), reading the MuPS tensor mups_dev.  The routed form
 * (experts): point_index_dev gathers the MuPS rows, npoints_dev holds the live count (both NULL: rows 0 .. batch - 1).
 * walk: 0, 1 (the default walking grid) or a multiple of 8 workgroups (kernels.h: ConvParams::walk). */
int nesti_debug_tower_step(const nesti_model_t* m, int tower, const nesti_debug_pass_t* pass, int op, const void* mups_dev, int batch,
                           const int32_t* point_index_dev, const int32_t* npoints_dev, int walk, void* ws_dev, size_t ws_bytes,
                           void* stream);

/* ---- test hook: one launcher of the deciding kernels alone (tests/test_gpu_decisions.py; no reference counterpart) ------
 * The two-stage gate, the conditioning guard, the gate's softmax and the routing helpers (csrc/decide.h, csrc/decide.hip), each
 * run on CALLER buffers: no model, the counter blocks (cstat, gstat, rstat: 8 x uint64 each) and the 512-byte fcounts block
 * are the caller's too.  op names the launcher; the struct carries its arguments under the launcher's own names, the few
 * launchers whose names differ say so below.  Forwards and nothing else; before any device call it refuses an unknown op, a
 * null pointer the launcher dereferences, E outside 1 .. NESTI_MAX_EXPERTS and n_rounds above the 24 the fcounts block holds. */
enum { NESTI_DECISION_GATE_FINISH = 0,     /* logits lstride B E probs? expert? counts? lists (with counts)                      */
       NESTI_DECISION_GATE_FLAG = 1,       /* logits lstride B E tau widen probs? expert keep fcounts flag_list cap n_rounds cstat rstat? */
       NESTI_DECISION_GATE_WIDEN = 2,      /* keep B E widen fcounts flag_list cap n_rounds cstat                                 */
       NESTI_DECISION_GATE_RECHECK = 3,    /* logits (compact rows) lstride flag_list count_ptr cap E keep probs? expert cstat
                                            * widen rstat? fcounts (with rstat)                                                   */
       NESTI_DECISION_ROUND_COUNTS = 4,    /* counts n_lists cap n_rounds round_out                                               */
       NESTI_DECISION_SWITCH_FINISH = 5,   /* logits lstride B thr (the threshold) probs? expert? counts? lists (with counts)     */
       NESTI_DECISION_X8_GUARD_BEGIN = 6,  /* pass thr scale B gstat slot rstat?                                                  */
       NESTI_DECISION_X8_GUARD_FLAG = 7,   /* lists (ONE list) count_ptr B (count_cap) normals slot glist gcount cap gstat        */
       NESTI_DECISION_X8_GUARD_FIX = 8,    /* src sstride glist gcount cap normals gstat thr scale rstat?                         */
       NESTI_DECISION_ROUTE = 9,           /* expert B E counts lists                                                             */
       NESTI_DECISION_SCATTER3 = 10,       /* src sstride index? count_ptr? cap (count_cap) normals (the destination)             */
       NESTI_DECISION_STAT_MAX_EXPORT = 11,/* word dst                                                                            */
       NESTI_DECISION_STAT_MAX_IMPORT = 12,/* word src B (the number of floats)                                                   */
       NESTI_DECISION_OPS = 13 };
typedef struct {
  const float* logits;
  int lstride, B, E, n_lists, cap, n_rounds, pass, sstride;
  float tau, widen, thr, scale;
  float* probs;
  int32_t* expert;
  float* keep;
  int32_t* fcounts;
  int32_t* flag_list;
  const int32_t* count_ptr;
  int32_t* counts;
  int32_t* lists;
  int32_t* round_out;
  uint64_t* cstat;
  uint64_t* gstat;
  uint64_t* rstat;
  uint64_t* word;
  float* slot;
  float* normals;
  const float* src;
  const int32_t* index;
  int32_t* glist;
  int32_t* gcount;
  float* dst;
} nesti_debug_decision_t;
int nesti_debug_decision_step(int op, const nesti_debug_decision_t* a, void* stream);

/* The weight packer without a device (tests/test_pack.py): builds the graph and packs ONE layer (index `layer` of the model, as
 * nesti_debug_op_t::layer) on the host, with the very code nesti_model_create uploads from.  form: the packing of a launch form --
 * NESTI_DEBUG_FORM_PLAIN, _PAIR, _X8 or _X6; _X2 runs on the pair packing and means _PAIR.  A form the layer or the dtype cannot
 * take is refused with a message.  info is always filled; w / bias may be NULL (sizes only: info->w_bytes, info->n_bias), max_w is
 * in bytes and max_bias in floats. */
typedef struct {
  int kind;            /* kernel family the bytes are laid out for: 0 conv_igemm_kernel, 2 conv8n_kernel, 3 conv4n_kernel   */
  int TN, n_tiles, split_tile, n_chunks, n_taps;   /* image = [n_tiles][n_chunks][n_taps][TN rows][128 or 64 bytes]            */
  int x3n;             /* rows are [W_hi | W_lo] K chunks                                                                    */
  float acc_scale;     /* 2^-s when the weights carry a 2^s scale                                                            */
  int x8_sb;           /* X8 / X6: power-of-two pre-scale of the e4m3 weight planes                                          */
  int x8_sc;           /* the pre-scale of the activation planes this layer would write as an X8 / X6 producer              */
  int64_t w_bytes, n_bias;
  int8_t tap[125][4];  /* dz, dy, dx, 0 of the n_taps kept taps                                                              */
} nesti_debug_pack_t;
int nesti_debug_pack_layer(const nesti_config_t* cfg, const nesti_tensor_t* tensors, int n_tensors, int dtype, int form, int layer,
                           nesti_debug_pack_t* info, void* w, size_t max_w, float* bias, size_t max_bias);

/* ---- measurement support (bench.py's roofline leg; no reference counterpart) ------------
 * nesti_profile_enable(1) makes every kernel launch of the forward path record a pair of
 * hipEvents on its stream; nesti_profile_read() synchronises on them and returns, per
 * (phase, category), the summed kernel time in ms and the number of launches since enable:
 * arrays of NESTI_PROF_PHASES * NESTI_PROF_CATEGORIES entries, index = phase * NESTI_PROF_CATEGORIES + category.
 * Categories are kernels (the four conv categories are the layer classes of DESIGN.md 4.3 / 4.4); phases say which part
 * of the forward pass launched them (NESTI_F16X3C: the gate's f16 filter pass counts as GATE, its f16x3 pass as RECHECK).
 * Not thread-safe; leave it off outside measurements. */
enum { NESTI_PROF_CONV8_K5 = 0,   /* conv8n_kernel, 5^3 taps at 8^3                                 */
       NESTI_PROF_CONV8_K3 = 1,   /* conv8n_kernel, 3^3 taps at 8^3                                 */
       NESTI_PROF_TAPS = 2,       /* conv4n_kernel: k^3 taps at 4^3; conv_igemm_kernel: taps at 2^3
                                   * and on the 3^3 grid embedded in 4^3                            */
       NESTI_PROF_ONE_BY_ONE = 3, /* conv_igemm_kernel, 1x1x1 layers (+ fused avg-pool) and FC      */
       NESTI_PROF_MUPS = 4, NESTI_PROF_POOL = 5, NESTI_PROF_PATCHES = 6, NESTI_PROF_CATEGORIES = 7 };
enum { NESTI_PHASE_INPUT = 0,     /* search grid, ball query, MuPS                                  */
       NESTI_PHASE_GATE = 1, NESTI_PHASE_RECHECK = 2, NESTI_PHASE_EXPERTS = 3,
       NESTI_PHASE_GUARD = 4,     /* the conditioning guard's f16x3 re-evaluations (NESTI_F16X8 / NESTI_F16X8C); its first pass overlaps
                                   * the experts on an auxiliary stream, so its launch durations are not wall time                  */
       NESTI_PROF_PHASES = 5 };
int nesti_profile_enable(int on);
int nesti_profile_read(double* ms /*[NESTI_PROF_PHASES * NESTI_PROF_CATEGORIES]*/,
                       long long* launches /*[NESTI_PROF_PHASES * NESTI_PROF_CATEGORIES]*/);
/* Multiply-accumulates per point of one tower (tower = -1: gating net, 0..E-1: expert), over the layers of conv
 * category `kind` (NESTI_PROF_CONV8_K5 .. NESTI_PROF_ONE_BY_ONE; -1: all of them):
 *   nominal = dense conv as TensorFlow executes it (zero-padding taps included),
 *   useful  = taps that land inside the volume only (the algorithmic figure),
 *   issued  = what the MFMA kernels issue for ONE 16-bit product: channel padding included, padding taps included except
 *             the MFMA tiles the kernels skip (x-lines whose y + dy or z + dz leaves the volume, at 8^3 and 4^3); the
 *             pair modes issue three such products per multiply. */
int nesti_model_macs(const nesti_model_t* m, int tower, int kind, double* nominal, double* useful,
                     double* issued);

#ifdef __cplusplus
}
#endif
#endif /* NESTI_HIP_H */
