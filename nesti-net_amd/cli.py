"""Command-line drop-in for the reference's ``test_n_est_w_experts.py``: same flags
(``:19-29``), same inputs (``<dataset_path>/<testset>`` shape list, ``<shape>.xyz``, optional
``<shape>.pidx``; ``--query_positions 1``: ``<shape>.qxyz``, the positions to estimate at) and same outputs (``<results_path>/<dataset_name>_results/<shape>.normals``,
``.experts``, ``.experts_probs`` written with ``np.savetxt`` like ``:182-188``, plus ``log.txt``).  ``--depth_images 1``: the inputs are
depth frames (``<name>.depth.npy``, ``<name>.camera``, optional ``<name>.cam2world``), the outputs one row per estimated pixel plus
``<name>.pix``, ``<name>.normal_map.npy`` and ``<name>.expert_map.npy`` (the reference's MATLAB route, DESIGN.md 2 "Depth images").

The trained-model directory holds either ``model.nstw`` (variables + hyper-parameters, see
:mod:`.weights`) or the reference's own ``parameters.p`` / ``gmm.p`` / ``model.ckpt.*`` (read by
:mod:`.tf_ckpt` without TensorFlow); ``--synthetic_weights`` substitutes seeded random weights (no
checkpoint ships with the reference).  ``--estimator pca`` needs none of them: the plane-fit normals of :mod:`.pca`, written as
``<shape>.normals`` (one scale), ``<shape>.pca_eig`` and ``<shape>.pca_count`` (every scale); nor does ``--estimator quadric``: the
quadric-fit normals and principal curvatures of :mod:`.quadric`, written as ``<shape>.normals`` and ``<shape>.curv`` (one scale),
``<shape>.quadric_curv`` and ``<shape>.quadric_count`` (every scale).  ``--knn K[,K...]`` fits either of the two over the K nearest
neighbours instead of balls and adds ``<shape>.knn_radius``; ``--patch_radius R [R ...]`` gives the balls one to four radii of the
caller's in place of the model configuration's.  ``--estimator hough --knn K[,K...]`` is the Hough-transform estimator of
:mod:`.hough`, which exists over neighbour lists only: ``<shape>.normals`` (one scale), ``<shape>.hough_conf``, ``<shape>.hough_votes`` and
``<shape>.hough_count`` (every scale) and ``<shape>.knn_radius``.  ``--smooth ITERS`` smooths the written normals of any estimator with
the feature-preserving filter of :mod:`.smooth` before the orientation and adds ``<shape>.smooth_support``.  ``--estimator pca
--knn_ladder K[,K...]`` is the scale-selected plane fit of :mod:`.select`: every row chooses its own neighbour count from the ladder;
``<shape>.normals``, ``<shape>.select_k``, ``<shape>.select_eig``, ``<shape>.select_variation`` and ``<shape>.knn_radius``.
``--estimator robust --knn K[,K...]`` is the robust plane fit of :mod:`.robust` (iteratively re-weighted least squares), over neighbour
lists only: ``<shape>.normals`` (one scale), ``<shape>.robust_support``, ``<shape>.robust_inliers`` and ``<shape>.robust_count`` (every
scale) and ``<shape>.knn_radius``.  ``--outliers statistical | radius`` removes outliers with the filter of :mod:`.outliers` before any
estimator runs: every file keeps the rows of ``<shape>.xyz`` (a removed row is written as 0, its expert as -1) and
``<shape>.inliers`` and ``<shape>.outlier_score`` are added.  ``--voxel_size V`` downsamples the cloud on a voxel grid
(:mod:`.downsample`) before all of that, for the model-free estimators: every file still has the rows of the ``.xyz``, a row holding the
result of its voxel, and ``<shape>.voxel_xyz``, ``<shape>.voxel_of`` and ``<shape>.voxel_count`` are added.  ``--denoise ITERS`` moves the
positions with the bilateral point filter of :mod:`.denoise` after those two and before a model-free estimator, and adds
``<shape>.denoised.xyz`` and ``<shape>.denoise_delta``.  ``--depth_images 1 --depth_window auto | R`` with ``--estimator pca | quadric |
hough | robust`` and ``--knn`` (or ``--knn_ladder``) runs those estimators on depth frames over image-window neighbour lists
(``depth.depth_normals``; DESIGN.md 2 "Image-window neighbourhoods"): the estimator's row files, ``<name>.pix``,
``<name>.normal_map.npy``, ``<name>.knn_radius`` and ``<name>.window_proven``."""
import argparse
import ctypes
import os
import sys

import torch

from . import pca as _pca
from . import hough as _hough
from . import denoise as _denoise
from . import downsample as _downsample
from . import outliers as _outliers
from . import smooth as _smooth
from . import stages
from . import quadric as _quadric
from . import robust as _robust
from . import select as _select
from . import textio
from . import weights as wts
from .config import ARCH_EXPERTS, ARCH_MULTI, ARCH_SINGLE, ARCH_SWITCH, MAX_SCALES, NestiConfig
from .pipeline import NormalEstimator
from .provider import PointcloudPatchDataset


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--results_path", default="log/my_experts/", help="path to trained model, default log/my_experts/")
    p.add_argument("--model", default="experts_n_est", help="Model name [default: experts_n_est]")
    p.add_argument("--dataset_name", type=str, default="pcpnet", help="Relative path to data directory, default pcpnet")
    p.add_argument("--dataset_path", type=str, default=None, help="full path to dataset for datasets outside the local data dir")
    p.add_argument("--sparse_patches", type=int, default=False,
                   help="test on a subset of the points in each point cloud in the test data, default False")
    p.add_argument("--gpu", type=int, default=0, help="GPU to use [default: GPU 0]")
    p.add_argument("--batch_size", type=int, default=128, help="Batch size [default: 128]; the library batches internally")
    p.add_argument("--testset", type=str, default="testset_temp.txt", help="test set file name, default testset_temp.txt")
    # extensions (not in the reference)
    p.add_argument("--dtype", default="auto", choices=["auto", "f16x8c", "f16x8", "f16x3c", "f16x3", "bf16x3", "f16", "bf16", "f32"],
                   help="MFMA precision mode.  auto (default): the modes that keep .normals and .experts within the reference's "
                        "tolerance (arg-max exact up to fp32 ties, 1e-5 cosine) -- f16x8c for experts_n_est on the 8^3 grid (f16 hi + lo "
                        "pairs behind the two-stage gate, whose margin is calibrated on every shape and widens itself when the measured "
                        "error approaches it; the experts' tap layers at 8^3 take their two cross terms through one block-scaled FP6 MFMA and outputs of "
                        "small norm are evaluated again in f16x3: .experts equal f16x3c's, .normals stay within ~1e-6 cosine of f16x3's), f16x3c on the 3^3 grid, f16x3 for the other "
                        "models.  NOTE: with f16x3c / f16x8c the .experts_probs rows of queries "
                        "the filter pass decided alone (~90 %%) are that pass's probabilities, within ~0.013 of the fp32 values; "
                        "use --dtype f16x3 when the probabilities themselves must hold 1e-4.  f16 / bf16: plain 16-bit, ~1.7x "
                        "faster, hundreds of arg-max flips per 100k points (DESIGN.md 2); f32: the exact-fp32 MFMA mode")
    p.add_argument("--x8_format", type=int, default=None, choices=[6, 8],
                   help="dtypes f16x8 / f16x8c: the experts' cross terms as block-scaled FP6 e2m3 (6, the default: half the matrix-pipe time of "
                        "FP8 for ~1.15x its residual, bounded by the same conditioning guard) or FP8 e4m3 (8)")
    p.add_argument("--x8_layers", type=int, default=None,
                   help="dtypes f16x8 / f16x8c: which expert tap layers at 8^3 take their cross terms through the narrow format (bit 0 / 1 = inception1 "
                        "conv2 (3^3) / conv3 (5^3), bit 2 / 3 = inception2 conv2 / conv3).  Default 15 = all four (outputs of small norm are "
                        "re-evaluated in f16x3 by the conditioning guard: 1 - cos <= 1.1e-6 against f16x3 on every other query); 10 = the "
                        "5^3 layers only (~2 %% slower); 0 = f16x3c proper")
    p.add_argument("--lib_batch", type=int, default=0,
                   help="queries per library batch (0 = by dtype: 50000 for f16x3c / f16 / bf16, 25000 for the pair modes, 8192 "
                        "for f32; two such batches are in flight on two HIP streams)")
    p.add_argument("--subsample", default="hash", choices=["hash", "reference", "reference_host"],
                   help="how balls with more than num_point points are thinned: hash = on the GPU, order-independent (default); "
                        "reference = exactly like the reference (cKDTree visiting order + its shared RandomState stream: "
                        "utils/pcpnet_dataset.py:304, 320-321) for row-by-row diffs against a real reference run -- on the GPU since "
                        "round 6 (ball sizes counted on the device, the stream replayed natively on the host from the sizes, the balls "
                        "sorted into tree order in LDS); reference_host = the same rows by scipy + numpy on the host "
                        "(nesti-net_amd/refsample.py), several times slower")
    p.add_argument("--reproducible", type=int, default=0, choices=[0, 1],
                   help="1: the written files are a function of the model and the cloud alone -- not of --batch_size, --lib_batch, "
                        "the free device memory or what ran before.  The gate margin and the cross-term guard's threshold are calibrated "
                        "without floating-point sums and frozen, every shape is checked against them after it ran and runs again as a "
                        "whole with wider ones if the check fails (the log names the passes).  Default 0: the thresholds follow the "
                        "measurements on the device while a shape runs, which is a little faster")
    p.add_argument("--query_positions", type=int, default=0, choices=[0, 1],
                   help="1: estimate at the positions listed in <shape>.qxyz (M rows of x y z, read like .xyz) instead of at the cloud's "
                        "own points; neighbourhoods and radii still come from <shape>.xyz.  The three output files then have M rows; a "
                        "position with no cloud point inside any of its balls is written as normal 0 0 0, expert -1, probabilities 0.  "
                        "Mutually exclusive with --sparse_patches 1; needs --subsample hash")
    p.add_argument("--depth_images", type=int, default=0, choices=[0, 1],
                   help="1: every name of the test set is a depth frame -- <name>.depth.npy ([H,W] uint16 or float32), <name>.camera (one "
                        "line: fx fy cx cy depth_scale; pixel coordinates are 0-based, so MATLAB-convention intrinsics lose 1 from cx and "
                        "cy) and optionally <name>.cam2world (4 x 4, camera to world, applied with its translation).  The frame is "
                        "back-projected on the GPU, normals are estimated at its valid pixels (depth finite and > 0) and written as one "
                        "row per estimated pixel in row-major pixel order, with <name>.pix (the pixel index v W + u of each row), "
                        "<name>.normal_map.npy ([H,W,3], 0 0 0 where nothing was estimated) and <name>.expert_map.npy ([H,W], -1 "
                        "there).  --orient defaults to viewpoint, the camera centre; --viewpoint is refused.  Mutually exclusive with "
                        "--sparse_patches 1 and --query_positions 1")
    p.add_argument("--depth_stride", type=int, default=1,
                   help="--depth_images 1: estimate at the valid pixels whose row and column are multiples of S only (neighbourhoods "
                        "still come from every valid pixel) [default: 1]")
    p.add_argument("--depth_window", default="0", metavar="{0,auto,R}",
                   help="--depth_images 1 with --estimator pca / quadric / hough / robust and --knn K[,K...] (or --knn_ladder): the "
                        "model-free estimators on depth frames (DESIGN.md 2 'Image-window neighbourhoods').  The neighbour lists come "
                        "from a (2 R + 1) x (2 R + 1) pixel window round every pixel instead of a grid search; auto picks R from the "
                        "largest neighbour count, R is 1 .. 15.  Writes <name>.normals, <name>.pix, <name>.normal_map.npy, the "
                        "estimator's own row files, <name>.knn_radius and <name>.window_proven (1 where the window's list is proven "
                        "to be the exact k-NN list).  --smooth is served at --depth_stride 1; --outliers, --denoise, --voxel_size and "
                        "--estimator net are left for later [default: 0 = off]")
    p.add_argument("--depth_window_exact", type=int, default=1, choices=[0, 1],
                   help="--depth_window: 1 (default) re-searches the rows the window cannot prove on the search grid, so every list is "
                        "the exact k-NN list and the files equal those of the same estimator on the back-projected cloud; 0 keeps "
                        "the window's lists as they are")
    p.add_argument("--orient", default=None, choices=["0", "mst", "viewpoint"],
                   help="orient the written normals consistently (only signs in <shape>.normals change; .experts and .experts_probs "
                        "do not).  0 (default): signs as the experts produced them.  mst: propagate signs along the minimum spanning "
                        "tree of the --orient_k nearest-neighbour graph inside the largest patch radius, from the highest point "
                        "(made to point up) or, with --viewpoint, from the point nearest to it (made to face it); every connected "
                        "piece is oriented on its own, the log line names their number.  viewpoint: every normal faces --viewpoint "
                        "(a single-sensor scan).  With --depth_images 1 the default is viewpoint and the viewpoint is the camera")
    p.add_argument("--orient_k", type=int, default=8, help="--orient mst: neighbours per point, 1 .. 16 [default: 8]")
    p.add_argument("--viewpoint", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                   help="--orient viewpoint (required) / --orient mst (optional): the sensor position in the cloud's coordinates")
    p.add_argument("--estimator", default="net", choices=["net", "pca", "quadric", "hough", "robust"],
                   help="net (default): Nesti-Net, from the trained model in --results_path.  pca: the classical plane fit at every patch "
                        "radius of --model's configuration (DESIGN.md 2 'Plane-fit normals'); no model.nstw and no --synthetic_weights "
                        "are needed or read.  Writes <shape>.normals (the scale --pca_scale), <shape>.pca_eig (M rows of 3 S "
                        "eigenvalues in units of r^2, ascending per scale; surface variation = the first over the sum of the three) and "
                        "<shape>.pca_count (M rows of S ball sizes); a scale whose ball holds fewer than 3 points is written as 0 0 0.  "
                        "Honours --sparse_patches, --query_positions, --orient, --orient_k and --viewpoint (the orientation radius is "
                        "that of --pca_scale); --depth_images 1, --reproducible 1 and --subsample reference* belong to net.  "
                        "quadric: a degree-2 height function fitted to the same balls in the plane fit's frame (DESIGN.md 2 'Quadric "
                        "fit'), under the same conditions.  Writes <shape>.normals (the fitted surface's normal at the scale "
                        "--quadric_scale), <shape>.curv (M rows k_max k_min at that scale, in 1 / length: the two columns the "
                        "reference's dataset reads; positive where the surface bends toward the written normal), <shape>.quadric_curv "
                        "(M rows of 2 S values, unoriented) and <shape>.quadric_count (M rows of S ball sizes); a fit that fails (fewer "
                        "than 6 points in the ball, or a singular system) is written as 0 0 0 and 0 0.  "
                        "hough: the sharp-feature estimator after Boulch and Marlet (DESIGN.md 2 'Hough-transform normals'), under the "
                        "same conditions; it exists over neighbour lists only and requires --knn.  Writes <shape>.normals (the scale "
                        "--hough_scale), <shape>.hough_conf (M rows of S confidences: the winning bin's share of the valid triplets), "
                        "<shape>.hough_votes (M rows of 2 S integers: winning votes and valid triplets per scale), <shape>.hough_count "
                        "(M rows of S neighbour counts) and <shape>.knn_radius; a row with fewer than 3 neighbours or only degenerate "
                        "triplets is written as 0 0 0 with confidence 0.  "
                        "robust: the robust plane fit (DESIGN.md 2 'Robust plane fit'), under the same conditions; it too exists over "
                        "neighbour lists only and requires --knn.  Iteratively re-weighted least squares from the plane fit's normal: "
                        "neighbours far from the current plane lose their weight, so the fit leans to one face of a crease.  Writes "
                        "<shape>.normals (the scale --robust_scale), <shape>.robust_support (M rows of S weight sums of the last "
                        "iteration), <shape>.robust_inliers (M rows of S counts of neighbours within the scale of the residuals), "
                        "<shape>.robust_count (M rows of S neighbour counts) and <shape>.knn_radius; a row with fewer than 3 "
                        "neighbours is written as 0 0 0")
    p.add_argument("--pca_scale", type=int, default=-1,
                   help="--estimator pca: the scale whose normals go to <shape>.normals, an index into the patch radii; negative "
                        "counts from the end [default: -1, the largest]")
    p.add_argument("--quadric_scale", type=int, default=-1,
                   help="--estimator quadric: the scale whose normals and curvatures go to <shape>.normals and <shape>.curv, an index "
                        "into the patch radii; negative counts from the end [default: -1, the largest]")
    p.add_argument("--patch_radius", type=float, nargs="+", default=None, metavar="R",
                   help="--estimator pca / quadric without --knn: the patch radii as fractions of the bounding-box diagonal, 1 to 4 "
                        "positive numbers in any order, in place of those of --model's configuration; --pca_scale / --quadric_scale "
                        "index them and the files have as many scales [default: the radii of --model's configuration]")
    p.add_argument("--hough_scale", type=int, default=-1,
                   help="--estimator hough: the scale whose normals go to <shape>.normals, an index into --knn; negative counts from "
                        "the end [default: -1, the largest]")
    p.add_argument("--hough_triplets", type=int, default=_hough.DEFAULT_TRIPLETS,
                   help="--estimator hough: planes drawn per row and scale, 1 .. 4096 [default: %d]" % _hough.DEFAULT_TRIPLETS)
    p.add_argument("--hough_bins", type=int, default=_hough.DEFAULT_BINS,
                   help="--estimator hough: bins per axis of the accumulator, 2 .. 16 [default: %d]" % _hough.DEFAULT_BINS)
    p.add_argument("--hough_rotations", type=int, default=_hough.DEFAULT_ROTATIONS,
                   help="--estimator hough: rotated copies of the accumulator, 1 .. 8 [default: %d]" % _hough.DEFAULT_ROTATIONS)
    p.add_argument("--hough_seed", type=int, default=0, help="--estimator hough: the seed of the triplet hash [default: 0]")
    p.add_argument("--robust_scale", type=int, default=-1,
                   help="--estimator robust: the scale whose normals go to <shape>.normals, an index into --knn; negative counts from "
                        "the end [default: -1, the largest]")
    p.add_argument("--robust_iters", type=int, default=_robust.DEFAULT_ITERS,
                   help="--estimator robust: re-weighting iterations, 0 .. 64 [default: %d]" % _robust.DEFAULT_ITERS)
    p.add_argument("--robust_sigma", type=float, default=_robust.DEFAULT_SIGMA,
                   help="--estimator robust: the scale of the residuals in median absolute residuals, in (0, 1e6] [default: %g]"
                        % _robust.DEFAULT_SIGMA)
    p.add_argument("--robust_falloff", type=float, default=_robust.DEFAULT_FALLOFF,
                   help="--estimator robust: the distance falloff in [0, 1]; the farthest neighbour weighs (1 - falloff)^2 [default: %g]"
                        % _robust.DEFAULT_FALLOFF)
    p.add_argument("--robust_floor", type=float, default=_robust.DEFAULT_FLOOR,
                   help="--estimator robust: the smallest scale of the residuals as a fraction of the neighbourhood radius, in "
                        "[1e-6, 1] [default: %g]" % _robust.DEFAULT_FLOOR)
    p.add_argument("--knn", default=None, metavar="K[,K...]",
                   help="--estimator pca / quadric: fit over the K nearest neighbours of every query instead of balls (DESIGN.md 2 "
                        "'k-nearest neighbourhoods'): one neighbour count per scale, at most 4, ascending, each in 1 .. 256.  The files "
                        "are those of the estimator -- <shape>.pca_count / <shape>.quadric_count then hold the neighbour counts, "
                        "--pca_scale / --quadric_scale index the counts -- plus <shape>.knn_radius (M rows of S distances to the "
                        "farthest neighbour).  --orient mst then uses the largest patch radius of --model's configuration")
    p.add_argument("--knn_ladder", default=None, metavar="K[,K...]",
                   help="--estimator pca: the scale-selected plane fit (DESIGN.md 2 'Scale-selected plane fit'): the plane fit over the "
                        "K nearest neighbours for every K of the ladder -- 1 to 32 strictly ascending counts in 1 .. 256, or the word "
                        "auto for %s -- and per row the candidate of smallest surface variation.  Writes <shape>.normals (the "
                        "selected candidate), <shape>.select_k (M rows: the neighbours it used; 0: no candidate could be fitted, the "
                        "normal is 0 0 0), <shape>.select_eig (M rows of its 3 eigenvalues), <shape>.select_variation (M rows of L "
                        "scores, one per candidate) and <shape>.knn_radius (M rows: its radius).  Mutually exclusive with --knn, "
                        "--patch_radius and --pca_scale; honours --sparse_patches, --query_positions, --smooth and --orient"
                        % ",".join(map(str, _select.DEFAULT_LADDER)))
    p.add_argument("--select_slack", type=float, default=None, metavar="X",
                   help="--knn_ladder: choose the largest candidate whose surface variation is within (1 + X) of the row's smallest, "
                        "X >= 0; 0 is the arg-min with ties to the larger count [default: 0]")
    p.add_argument("--smooth", type=int, default=0, metavar="ITERS",
                   help="smooth the written normals with ITERS passes (1 .. 64) of the feature-preserving filter of DESIGN.md 2 'Normal "
                        "smoothing', for every --estimator, before --orient: a row's normal becomes the weighted mean of its nearest "
                        "neighbours' normals, a neighbour beyond --smooth_angle of the row's own normal having no weight, so creases are "
                        "kept.  Only <shape>.normals changes (.experts and .experts_probs stay byte-identical); writes "
                        "<shape>.smooth_support (M rows: the weight sum and the number of weighted neighbours of the last pass).  Needs a "
                        "normal at every point: refused with --sparse_patches 1, --query_positions 1 and --depth_images 1 [default: 0 = off]")
    p.add_argument("--smooth_k", type=int, default=_smooth.DEFAULT_K,
                   help="--smooth: nearest neighbours per row, 1 .. 256 [default: %d]" % _smooth.DEFAULT_K)
    p.add_argument("--smooth_angle", type=float, default=_smooth.DEFAULT_ANGLE,
                   help="--smooth: the angle in degrees, in (0, 90], at which a neighbour's weight reaches 0 [default: %g]" % _smooth.DEFAULT_ANGLE)
    p.add_argument("--smooth_falloff", type=float, default=_smooth.DEFAULT_FALLOFF,
                   help="--smooth: the distance falloff in [0, 1]; the farthest neighbour weighs (1 - falloff)^2 [default: %g]"
                        % _smooth.DEFAULT_FALLOFF)
    p.add_argument("--outliers", choices=["0", "statistical", "radius"], default="0",
                   help="remove outliers before estimating (DESIGN.md 2 'Outlier removal'), for every --estimator and for --depth_images "
                        "1 at --depth_stride 1.  statistical: a point leaves when the mean distance to its --outlier_k nearest other "
                        "points exceeds the cloud's mean of that figure by --outlier_std standard deviations; radius: when fewer than "
                        "--outlier_k other points lie within --outlier_radius.  The estimator, --smooth and --orient then see the kept "
                        "points alone; every file keeps the rows of <shape>.xyz (a removed row is written as 0, its expert as -1) and "
                        "<shape>.inliers (0 / 1) and <shape>.outlier_score are added.  Goes with --reproducible 1; refused with "
                        "--sparse_patches 1 and --subsample reference* [default: 0 = off]")
    p.add_argument("--outlier_k", type=int, default=_outliers.DEFAULT_K,
                   help="--outliers: the nearest other points per row, 1 .. 255 [default: %d]" % _outliers.DEFAULT_K)
    p.add_argument("--outlier_std", type=float, default=_outliers.DEFAULT_STD_RATIO,
                   help="--outliers statistical: the threshold in standard deviations above the mean, >= 0 [default: %g]"
                        % _outliers.DEFAULT_STD_RATIO)
    p.add_argument("--outlier_radius", type=float, default=None, metavar="R",
                   help="--outliers radius: the radius, in the cloud's units (required)")
    p.add_argument("--outlier_passes", type=int, default=_outliers.DEFAULT_PASSES,
                   help="--outliers: filter passes, 1 .. 8; each searches the kept points again [default: %d]" % _outliers.DEFAULT_PASSES)
    p.add_argument("--voxel_size", type=float, default=0.0, metavar="V",
                   help="downsample the cloud on a voxel grid of this cell size, in the cloud's units, before anything else (DESIGN.md 2 "
                        "'Voxel downsampling'), for --estimator pca | quadric | hough | robust and for --knn_ladder; 0: off [default].  "
                        "--outliers, the estimator, --smooth and --orient then see one point per occupied cell; every file keeps one row "
                        "per row of the .xyz (a row holds the result of its voxel), and <shape>.voxel_xyz, <shape>.voxel_of and "
                        "<shape>.voxel_count are added.  Refused with --estimator net, --depth_images 1, --sparse_patches 1, "
                        "--query_positions 1 and --subsample reference*")
    p.add_argument("--voxel_mode", choices=list(_downsample.MODES), default=None,
                   help="--voxel_size: a cell's point is the centroid of its points, or the nearest of them to it [default: centroid]")
    p.add_argument("--denoise", type=int, default=0, metavar="ITERS",
                   help="denoise the positions with ITERS passes (1 .. 64) of the bilateral point filter of DESIGN.md 2 'Point denoising', "
                        "for --estimator pca | quadric | hough | robust and for --knn_ladder, after --voxel_size and --outliers and before "
                        "the estimator: a point moves along its plane-fit normal by the weighted mean of its neighbours' heights.  The "
                        "estimator, --smooth and --orient then see the denoised positions; <shape>.denoised.xyz and "
                        "<shape>.denoise_delta (one row per row of the .xyz) are added.  0: off [default].  Refused with --estimator net, "
                        "--depth_images 1, --sparse_patches 1, --query_positions 1, --subsample reference* and --reproducible 1")
    p.add_argument("--denoise_k", type=int, default=_denoise.DEFAULT_K,
                   help="--denoise: nearest neighbours per row, 1 .. 256; the normals are fitted over twice as many [default: %d]"
                        % _denoise.DEFAULT_K)
    p.add_argument("--denoise_angle", type=float, default=_denoise.DEFAULT_ANGLE,
                   help="--denoise: the angle in degrees, in (0, 90], at which a neighbour's weight reaches 0 [default: %g]"
                        % _denoise.DEFAULT_ANGLE)
    p.add_argument("--denoise_falloff", type=float, default=_denoise.DEFAULT_FALLOFF,
                   help="--denoise: the distance falloff in [0, 1] [default: %g]" % _denoise.DEFAULT_FALLOFF)
    p.add_argument("--denoise_sigma", type=float, default=_denoise.DEFAULT_SIGMA,
                   help="--denoise: the height scale in neighbourhood radii, in (0, 1e6]; 1e6 switches the height weight off [default: %g]"
                        % _denoise.DEFAULT_SIGMA)
    p.add_argument("--denoise_step", type=float, default=_denoise.DEFAULT_STEP,
                   help="--denoise: the share of the weighted mean height a pass moves a point by, in (0, 1] [default: %g]"
                        % _denoise.DEFAULT_STEP)
    p.add_argument("--synthetic_weights", action="store_true", help="use seeded synthetic weights if model.nstw is absent")
    return p


def denoise_line(name, rows, params, moved, delta):
    """The log line of ``--denoise`` for shape ``name``: the rows, the passes, the rows that moved and the largest displacement."""
    return ("denoising of %s: %d rows, %d pass%s over %d nearest neighbours (%g degrees, falloff %g, sigma %g, step %g); %d rows moved, "
            "largest displacement %.6g"
            % (name, rows, params.iters, "" if params.iters == 1 else "es", params.k, params.angle, params.falloff, params.sigma, params.step,
               moved, float(delta.max()) if len(delta) else 0.0))


def smooth_line(name, rows, params, count):
    """The log line of ``--smooth`` for shape ``name``: the rows, the passes and the rows whose count is 1 (nothing but the row's own
    normal had a weight in the last pass); ``count``: the int32 counts of the last pass."""
    return ("smoothing of %s: %d rows, %d pass%s over %d nearest neighbours (%g degrees, falloff %g); %d rows with count 1"
            % (name, rows, params.iters, "" if params.iters == 1 else "es", params.k, params.angle, params.falloff, int((count == 1).sum())))


def write_smooth_support(path, support, count):
    """``<shape>.smooth_support``: M rows of ``support count``."""
    with open(path, "w") as f:
        for s, c in zip(support.tolist(), count.tolist()):
            f.write("%.9g %d\n" % (s, c))


def outlier_line(name, params, rows, passes):
    """The log line of ``--outliers`` for shape ``name``: the rows removed and the threshold of every pass (``outliers.remove_outliers``)."""
    removed = sum(p["removed"] for p in passes)
    what = ("mean distance to %d nearest other points, %g standard deviations" % (params.k, params.std_ratio) if params.mode == "statistical"
            else "at least %d other points within %g" % (params.min_neighbours, params.radius))
    return ("outlier filter of %s (%s: %s): %d of %d rows removed in %d pass%s; threshold %s"
            % (name, params.mode, what, removed, rows, len(passes), "" if len(passes) == 1 else "es",
               ", ".join("%.9g" % p["threshold"] for p in passes)))


def write_outlier_files(output_dir, name, inlier, score):
    """``<shape>.inliers`` (0 / 1) and ``<shape>.outlier_score``: one row per row of the cloud."""
    import numpy as np
    textio.write_i32(os.path.join(output_dir, name + ".inliers"), np.ascontiguousarray(inlier, dtype=np.int32))
    with open(os.path.join(output_dir, name + ".outlier_score"), "w") as f:
        for v in np.asarray(score, np.float64).tolist():
            f.write("%.17g\n" % v)


def voxel_line(name, params, rows, count):
    """The log line of ``--voxel_size`` for shape ``name``: voxels, rows, largest count; ``count``: the int32 counts of the voxels."""
    return ("voxel grid of %s (cell %s, %s): %d voxels from %d rows; largest count %d"
            % (name, " ".join("%g" % v for v in params.voxel), params.mode, len(count), rows, int(count.max()) if len(count) else 0))


def stage_shape(cloud, voxel, outliers, denoise, name, output_dir, printout):
    """``--voxel_size``, ``--outliers`` and ``--denoise`` for one shape: run the preprocessing chain (``stages.run``) on the cloud's
    points, write each stage's log line and its files -- with the rows of the input: a removed row holds 0, a row of a voxel what its
    voxel holds -- and prepare the resulting points the way ``cloud`` was (configuration, seed, query positions).  Returns (the
    cloud to estimate on -- ``cloud`` itself where no stage is given --, the ``stages.Chain``)."""
    import numpy as np
    from .provider import CloudPatches
    path = os.path.join(output_dir, name)
    seen = []

    def report(stage, out, chain):
        seen.append(stage)
        if stage == "downsample":
            printout(voxel_line(name, voxel, chain.n, out["count"]))
            textio.write_f32(path + ".voxel_xyz", stages.take_rows(out["points"], out["voxel_of"]))
            textio.write_i32(path + ".voxel_of", np.ascontiguousarray(out["voxel_of"], dtype=np.int32))
            textio.write_i32(path + ".voxel_count", stages.take_rows(out["count"], out["voxel_of"]))
        elif stage == "outliers":
            printout(outlier_line(name, outliers, len(out["inlier"]), out["passes"]))
            write_outlier_files(output_dir, name, chain.to_input(out["inlier"]), chain.to_input(out["score"]))
            if not len(out["kept"]):
                raise SystemExit("--outliers: the filter kept none of the %d points of %s" % (len(out["inlier"]), name))
        else:
            printout(denoise_line(name, len(out["points"]), denoise, out["moved"], out["delta"]))
            textio.write_f32(path + ".denoised.xyz", chain.to_input(out["points"]))
            textio.write_f32(path + ".denoise_delta", chain.to_input(out["delta"]))

    params = None if voxel is outliers is denoise is None else stages.Stages(voxel, outliers, denoise)
    queries = None if cloud.queries is None else cloud.queries.cpu().numpy()
    try:
        chain = stages.run(cloud.host_pts, params, queries, cloud.device, report)
    except ValueError as e:
        if voxel is None or seen:
            raise
        raise SystemExit("--voxel_size: %s: %s" % (name, e))
    if params is not None:
        cloud = CloudPatches(chain.points, cloud.cfg, cloud.device, cloud.seed, queries=queries)
    return cloud, chain


def fit_batch(cfg, dtype, batch, device, lanes=2, reserve=2 << 30):
    """The largest batch <= ``batch`` (halving, 256-row granularity, >= 256) whose ``lanes`` arenas fit the device's free
    memory with ``reserve`` bytes to spare.  The arena size comes from the library's own layout, from the configuration alone
    (``nesti_estimate_workspace_bytes_for_config`` == ``nesti_estimate_workspace_bytes`` of the model that will be created:
    tests/test_abi.py), before any model exists."""
    from . import _lib
    from .config import DTYPES
    lib = _lib.load()
    free = torch.cuda.mem_get_info(device)[0] - reserve
    c = cfg.to_c()
    while batch > 256:
        arena = lib.nesti_estimate_workspace_bytes_for_config(ctypes.byref(c), DTYPES[dtype], batch)
        if arena and lanes * arena <= free:
            break
        batch = max(256, (batch // 2 + 255) // 256 * 256)
    return batch


class DepthFrames:
    """The frames of ``--depth_images 1``: the names of the test set and, from the ``.npy`` headers alone, an upper bound on the rows
    each can produce (sizes the library batch)."""

    def __init__(self, root, testset, stride):
        import numpy as np
        self.root, self.stride = root, int(stride)
        with open(os.path.join(root, testset)) as f:
            self.names = list(filter(None, (x.strip() for x in f.readlines())))
        self.max_rows = []
        for name in self.names:
            H, W = np.load(self.path(name, ".depth.npy"), mmap_mode="r").shape
            self.max_rows.append(((H + self.stride - 1) // self.stride) * ((W + self.stride - 1) // self.stride))

    def path(self, name, ext):
        return os.path.join(self.root, name + ext)

    def load(self, name):
        """(depth [H,W], Camera) of a frame; the pose from ``<name>.cam2world`` when that file exists."""
        import dataclasses
        from . import depth as _depth
        cam = _depth.read_camera(self.path(name, ".camera"))
        if os.path.exists(self.path(name, ".cam2world")):
            cam = dataclasses.replace(cam, pose=_depth.read_cam2world(self.path(name, ".cam2world")))
        return _depth.read_depth(self.path(name, ".depth.npy")), cam


def run_depth_frame(est, frames, name, FLAGS, output_dir, printout, on_cloud, write_experts=True, outliers=None):
    """One frame of ``--depth_images 1``: estimate, then the row files, ``.pix`` and the two images."""
    import numpy as np
    depth, cam = frames.load(name)
    res = est.estimate_depth(depth, cam, stride=FLAGS.depth_stride, orient=None if FLAGS.orient == "0" else FLAGS.orient,
                             orient_k=FLAGS.orient_k, on_cloud=on_cloud, outliers=outliers)
    H, W = depth.shape
    if outliers is not None and len(res["pix"]):
        lo = est.last_outliers
        printout(outlier_line(name, outliers, len(res["pix"]), lo["passes"]))
        write_outlier_files(output_dir, name, lo["inlier"], lo["score"])
    printout("depth frame %s: %d x %d, %d normals estimated (stride %d), oriented: %s"
             % (name, H, W, len(res["pix"]), FLAGS.depth_stride, FLAGS.orient))
    textio.write_f32(os.path.join(output_dir, name + ".normals"), res["normals"])
    textio.write_i32(os.path.join(output_dir, name + ".pix"), res["pix"])
    np.save(os.path.join(output_dir, name + ".normal_map.npy"), res["normal_map"])
    printout("saved normals for " + name)
    if res["expert"] is None or not write_experts:
        return
    textio.write_i32(os.path.join(output_dir, name + ".experts"), res["expert"])
    textio.write_f32(os.path.join(output_dir, name + ".experts_probs"), res["probs"])
    np.save(os.path.join(output_dir, name + ".expert_map.npy"), res["expert_map"])
    printout("saved experts for " + name)


def depth_window_args(FLAGS, parser, fit, ks, ladder):
    """``--depth_window`` / ``--depth_window_exact`` resolved: None (off), or (window, exact) -- ``'auto'`` or R, and a bool -- after the
    refusals of what the window route does not serve."""
    if FLAGS.depth_window == "0":
        if FLAGS.depth_window_exact != 1:
            parser.error("--depth_window_exact belongs to --depth_window auto / R")
        return None
    from . import depth as _depth
    word = FLAGS.depth_window.strip()
    try:
        window = "auto" if word == "auto" else int(word)
        _depth.check_window(window, 1)
    except ValueError:
        parser.error("--depth_window takes 0, auto or R in 1 .. 15: got %r" % FLAGS.depth_window)
    if not FLAGS.depth_images:
        parser.error("--depth_window belongs to --depth_images 1: the window is a window of pixels")
    if not fit:
        parser.error("--depth_window does not go with --estimator net: the network on window lists is left for later; it serves "
                     "--estimator pca / quadric / hough / robust")
    if ks is None and ladder is None:
        parser.error("--depth_window needs --knn K[,K...] or --knn_ladder: the window's lists are neighbour lists, not balls")
    for given, flag, why in ((FLAGS.outliers != "0", "--outliers %s" % FLAGS.outliers,
                              "left for later: the filter renumbers the cloud and the frame's rank image no longer names its rows"),
                             (bool(FLAGS.denoise), "--denoise",
                              "left for later: the filter moves points off their pixels' rays and the window's proof is void"),
                             (FLAGS.voxel_size != 0.0, "--voxel_size", "left for later: a voxel grid's points have no pixels")):
        if given:
            parser.error("%s does not go with --depth_window: %s" % (flag, why))
    return window, bool(FLAGS.depth_window_exact)


def window_line(name, res, exact):
    """The log line of ``--depth_window`` for frame ``name``: the window, the share of rows it proved and the rows re-searched."""
    rows = len(res["window_proven"])
    return ("image window of %s: R = %d (%d x %d pixels), %d rows, %.1f %% proven exact by the window, %d rows re-searched on the grid%s"
            % (name, res["window"], 2 * res["window"] + 1, 2 * res["window"] + 1, rows,
               100.0 * float(res["window_proven"].mean()) if rows else 100.0, res["window_exact_rows"],
               "" if exact else " (--depth_window_exact 0: the window's lists as they are)"))


def run_window_frame(frames, name, FLAGS, window, ks, ladder, slack, scale, smooth, output_dir, printout):
    """One frame of ``--depth_images 1 --depth_window``: ``depth.depth_normals`` with the estimator of the command line, then
    ``.normals``, ``.pix``, ``.normal_map.npy``, the estimator's row files, ``.knn_radius`` and ``.window_proven``."""
    import numpy as np
    from . import depth as _depth
    depth, cam = frames.load(name)
    orient = None if FLAGS.orient == "0" else FLAGS.orient
    common = dict(window=window[0], exact=window[1], stride=FLAGS.depth_stride, orient=orient, orient_k=FLAGS.orient_k, smooth=smooth,
                  device="cuda:%d" % FLAGS.gpu)
    if ladder is not None:
        res = _depth.depth_normals(depth, cam, estimator="select", ladder=ladder, slack=slack, **common)
        files = ((".normals", textio.write_f32, "normals"), (".select_k", textio.write_i32, "k"), (".select_eig", textio.write_f32, "eig"),
                 (".select_variation", textio.write_f32, "variation_all"))
    else:
        fit = FITS[FLAGS.estimator]
        params = {kw: getattr(FLAGS, flag) for kw, flag in fit.get("params", ())}
        res = _depth.depth_normals(depth, cam, estimator=FLAGS.estimator, knn=ks, scale=scale, **common, **params)
        files = fit["files"]
    H, W = depth.shape
    rows = len(res["pix"])
    printout("depth frame %s: %d x %d, %d normals estimated (stride %d), oriented: %s" % (name, H, W, rows, FLAGS.depth_stride, FLAGS.orient))
    printout(window_line(name, res, window[1]))
    if rows:
        if ladder is not None:
            printout(select_line(name, rows, ladder, slack, res["sel"]))
        else:
            printout(fit_line(FLAGS.estimator, name, rows, scale, len(ks), int(FITS[FLAGS.estimator]["missing"](res, scale, ks)), k=ks[scale]))
            if "line" in FITS[FLAGS.estimator]:
                printout(FITS[FLAGS.estimator]["line"](name, res, scale, params))
        if smooth is not None:
            printout(smooth_line(name, rows, smooth, res["smooth_count"]))
            write_smooth_support(os.path.join(output_dir, name + ".smooth_support"), res["smooth_support"], res["smooth_count"])
        if res.get("orient") is not None:
            printout(orient_line(name, FLAGS.orient, res["orient"], rows))
        for ext, write, key in files:
            write(os.path.join(output_dir, name + ext), res[key].reshape(len(res[key]), -1) if write is not textio.write_i32 else res[key])
        textio.write_f32(os.path.join(output_dir, name + ".knn_radius"), res["radius"])
    else:
        textio.write_f32(os.path.join(output_dir, name + ".normals"), res["normals"])
    textio.write_i32(os.path.join(output_dir, name + ".pix"), res["pix"])
    textio.write_i32(os.path.join(output_dir, name + ".window_proven"), res["window_proven"].astype(np.int32))
    np.save(os.path.join(output_dir, name + ".normal_map.npy"), res["normal_map"])
    if "curv_map" in res:
        np.save(os.path.join(output_dir, name + ".curv_map.npy"), res["curv_map"])
    printout("saved normals, the normal image and the window's proof flags for " + name)


# --estimator pca / quadric: what differs between the two model-free fits.  ``missing(res, scale, ks)`` counts the rows without a fit at
# the written scale, ``no_fit`` says what they are for balls and for neighbour counts; ``files`` = (extension, writer, key of the result)
FITS = {
    "pca": {
        "fit": _pca.pca_cloud, "noun": "plane fit", "scale_flag": "pca_scale",
        "missing": lambda res, scale, ks: (res["n_ball"][:, scale] < 3).sum() if ks is None else (res["normals"] == 0).all(axis=1).sum(),
        "no_fit": ("with fewer than 3 points in that ball (written as 0 0 0)", "without a fit (written as 0 0 0)"),
        "files": ((".normals", textio.write_f32, "normals"), (".pca_eig", textio.write_f32, "eig"),
                  (".pca_count", textio.write_i32_rows, "n_ball")),
        "saved": "saved normals, eigenvalues and ball sizes for "},
    "quadric": {
        "fit": _quadric.quadric_cloud, "noun": "quadric fit", "scale_flag": "quadric_scale",
        "missing": lambda res, scale, ks: (res["normals_all"][:, scale] == 0).all(axis=1).sum(),
        "no_fit": ("without a fit in that ball (fewer than 6 points or a singular system: written as 0 0 0 and 0 0)",
                   "without a fit (fewer than 6 points or a singular system: written as 0 0 0 and 0 0)"),
        "files": ((".normals", textio.write_f32, "normals"), (".curv", textio.write_f32, "curv"),
                  (".quadric_curv", textio.write_f32, "curv_all"), (".quadric_count", textio.write_i32_rows, "n_ball")),
        "saved": "saved normals, curvatures and ball sizes for "},
    # over neighbour lists only (--knn is required): ``params`` = (keyword of the fit, flag) pairs passed on from the command line
    "hough": {
        "fit": _hough.hough_cloud, "noun": "Hough transform", "scale_flag": "hough_scale",
        "params": (("triplets", "hough_triplets"), ("bins", "hough_bins"), ("rotations", "hough_rotations"), ("seed", "hough_seed")),
        "missing": lambda res, scale, ks: (res["normals_all"][:, scale] == 0).all(axis=1).sum(),
        "no_fit": (None, "without a fit (fewer than 3 neighbours or only degenerate triplets: written as 0 0 0)"),
        "subsamples": "the Hough transform draws its triplets by hash over the whole neighbourhood and subsamples no patch",
        "files": ((".normals", textio.write_f32, "normals"), (".hough_conf", textio.write_f32, "conf"),
                  (".hough_votes", textio.write_i32_rows, "votes"), (".hough_count", textio.write_i32_rows, "n_ball")),
        "saved": "saved normals, confidences, votes and neighbour counts for "},
    "robust": {
        "fit": _robust.robust_cloud, "noun": "robust plane fit", "scale_flag": "robust_scale",
        "params": (("iters", "robust_iters"), ("sigma", "robust_sigma"), ("falloff", "robust_falloff"), ("floor", "robust_floor")),
        "missing": lambda res, scale, ks: (res["normals_all"][:, scale] == 0).all(axis=1).sum(),
        "no_fit": (None, "without a fit (fewer than 3 neighbours, or all of them at the query: written as 0 0 0)"),
        "subsamples": "the robust plane fit weighs the whole neighbourhood and subsamples no patch",
        "files": ((".normals", textio.write_f32, "normals"), (".robust_support", textio.write_f32, "support"),
                  (".robust_inliers", textio.write_i32_rows, "inliers"), (".robust_count", textio.write_i32_rows, "n_ball")),
        "line": lambda name, res, scale, params: robust_line(name, params, res["iters_done"][:, scale], res["inliers"][:, scale],
                                                             res["n_ball"][:, scale]),
        "saved": "saved normals, weight sums, inlier counts and neighbour counts for "},
}


def robust_line(name, params, iters_done, inliers, count):
    """The second log line of ``--estimator robust`` for shape ``name``: the parameters, the rows that stopped before the last iteration
    and the inliers' share of the neighbours at the written scale; the three int32 columns of that scale."""
    total = int(count.sum())
    return ("re-weighting of %s: %d iterations (sigma %g, falloff %g, floor %g); %d rows stopped early; %.1f %% of the neighbours are inliers"
            % (name, params["iters"], params["sigma"], params["falloff"], params["floor"], int((iters_done < params["iters"]).sum()),
               100.0 * float(inliers.sum()) / total if total else 0.0))


def select_line(name, rows, ladder, slack, sel):
    """The log line of ``--knn_ladder`` for shape ``name``: how many of the ``rows`` rows chose each count of the ladder; ``sel``: the
    int32 indices into the ladder, -1 for a row without a fit."""
    import numpy as np
    hist = np.bincount(np.asarray(sel, dtype=np.int64) + 1, minlength=len(ladder) + 1)
    return ("scale-selected plane fit of %s: %d rows, slack %g; chosen neighbour counts: %s; %d rows without a fit (written as 0 0 0)"
            % (name, rows, slack, ", ".join("%d: %d" % (k, n) for k, n in zip(ladder, hist[1:].tolist())), int(hist[0])))


def run_select(FLAGS, cfg, ladder, slack, pc_path, output_dir, printout, smooth=None, outliers=None, voxel=None, denoise=None):
    """``--estimator pca --knn_ladder``: per shape the selected fit, the optional smoothing and orientation of its normals, and its
    files.  No model is loaded."""
    dataset = PointcloudPatchDataset(pc_path, FLAGS.testset, cfg, seed=3627473, sparse_patches=FLAGS.sparse_patches,
                                     device="cuda:%d" % FLAGS.gpu, query_positions=bool(FLAGS.query_positions))
    for ind, name in enumerate(dataset.shape_names):
        cloud = dataset.get_shape(ind)
        cloud, chain = stage_shape(cloud, voxel, outliers, denoise, name, output_dir, printout)
        res = _select.select_cloud(cloud, ladder, slack, orient=None if FLAGS.orient == "0" else FLAGS.orient, viewpoint=FLAGS.viewpoint,
                                   orient_k=FLAGS.orient_k, smooth=smooth)
        printout(select_line(name, cloud.patch_count, ladder, slack, res["sel"]))
        if smooth is not None:
            printout(smooth_line(name, cloud.patch_count, smooth, res["smooth_count"]))
        res = chain.back(res)                                  # the log lines above count the estimated rows; the files hold every row
        if smooth is not None:
            write_smooth_support(os.path.join(output_dir, name + ".smooth_support"), res["smooth_support"], res["smooth_count"])
        if res["orient"] is not None:
            printout(orient_line(name, FLAGS.orient, res["orient"], cloud.patch_count))
        textio.write_f32(os.path.join(output_dir, name + ".normals"), res["normals"])
        textio.write_i32(os.path.join(output_dir, name + ".select_k"), res["k"])
        textio.write_f32(os.path.join(output_dir, name + ".select_eig"), res["eig"])
        textio.write_f32(os.path.join(output_dir, name + ".select_variation"), res["variation_all"])
        textio.write_f32(os.path.join(output_dir, name + ".knn_radius"), res["radius"])
        printout("saved normals, chosen neighbour counts, eigenvalues and surface variations for " + name)
    return 0


def orient_line(name, mode, stats, rows):
    """The log line of an orientation pass over the ``rows`` rows of shape ``name``; ``stats``: ``orient.stats_dict``."""
    return ("orientation of %s (%s): %d of %d rows oriented, %d flipped, %d connected piece%s, %d edges"
            % (name, mode, stats["n_eligible"], rows, stats["n_flipped"], stats["n_components"],
               "" if stats["n_components"] == 1 else "s", stats["n_edges"]))


def fit_line(estimator, name, rows, scale, n_scales, missing, radius=None, k=None):
    """The log line of ``--estimator pca / quadric`` for shape ``name``: the written scale is the ball of ``radius`` or, with ``--knn``,
    the ``k`` nearest neighbours; ``missing`` of the ``rows`` rows have no fit there."""
    fit = FITS[estimator]
    return ("%s of %s: %d rows, %s (scale %d of %d); %d rows %s"
            % (fit["noun"], name, rows, "radius %.6g" % radius if k is None else "%d nearest neighbours" % k, scale, n_scales, missing,
               fit["no_fit"][k is not None]))


def run_fit(FLAGS, cfg, scale, pc_path, output_dir, printout, ks=None, smooth=None, outliers=None, voxel=None, denoise=None):
    """``--estimator pca / quadric`` (``FITS``): per shape the fit at every scale, the optional orientation of the rows of scale ``scale``
    (>= 0; the quadric fit flips their curvatures with them), and the estimator's files.  No model is loaded."""
    fit = FITS[FLAGS.estimator]
    dataset = PointcloudPatchDataset(pc_path, FLAGS.testset, cfg, seed=3627473, sparse_patches=FLAGS.sparse_patches,
                                     device="cuda:%d" % FLAGS.gpu, query_positions=bool(FLAGS.query_positions))
    for ind, name in enumerate(dataset.shape_names):
        cloud = dataset.get_shape(ind)
        cloud, chain = stage_shape(cloud, voxel, outliers, denoise, name, output_dir, printout)
        params = {kw: getattr(FLAGS, flag) for kw, flag in fit.get("params", ())}
        res = fit["fit"](cloud, scale=scale, orient=None if FLAGS.orient == "0" else FLAGS.orient, viewpoint=FLAGS.viewpoint,
                         orient_k=FLAGS.orient_k, knn=ks, smooth=smooth, **params)
        missing = int(fit["missing"](res, scale, ks))
        if ks is None:
            printout(fit_line(FLAGS.estimator, name, cloud.patch_count, scale, cfg.n_scales, missing, radius=cloud.r_abs[scale]))
        else:
            printout(fit_line(FLAGS.estimator, name, cloud.patch_count, scale, len(ks), missing, k=ks[scale]))
        if "line" in fit:
            printout(fit["line"](name, res, scale, params))
        if smooth is not None:
            printout(smooth_line(name, cloud.patch_count, smooth, res["smooth_count"]))
        res = chain.back(res)                                  # the log lines above count the estimated rows; the files hold every row
        if ks is not None:
            textio.write_f32(os.path.join(output_dir, name + ".knn_radius"), res["radius"])
        if smooth is not None:
            write_smooth_support(os.path.join(output_dir, name + ".smooth_support"), res["smooth_support"], res["smooth_count"])
        if res["orient"] is not None:
            printout(orient_line(name, FLAGS.orient, res["orient"], cloud.patch_count))
        for ext, write, key in fit["files"]:
            write(os.path.join(output_dir, name + ext), res[key].reshape(len(res[key]), -1))
        printout(fit["saved"] + name)
    return 0


def main(argv=None):
    parser = build_parser()
    FLAGS = parser.parse_args(argv)
    for est, fit in FITS.items():
        if getattr(FLAGS, fit["scale_flag"]) != -1 and FLAGS.estimator != est:
            parser.error("--%s belongs to --estimator %s" % (fit["scale_flag"], est))
        for _, flag in fit.get("params", ()):
            if getattr(FLAGS, flag) != parser.get_default(flag) and FLAGS.estimator != est:
                parser.error("--%s belongs to --estimator %s" % (flag, est))
    ks = None
    if FLAGS.knn is not None:
        if FLAGS.estimator == "net":
            parser.error("--knn belongs to --estimator pca / --estimator quadric")
        from .knn import check_ks
        try:
            ks = check_ks([int(v) for v in FLAGS.knn.split(",")])
        except ValueError as e:
            parser.error("--knn %s: %s" % (FLAGS.knn, e))
    ladder, slack = None, 0.0
    if FLAGS.knn_ladder is not None:
        if FLAGS.estimator != "pca":
            parser.error("--knn_ladder belongs to --estimator pca")
        for given, flag in ((FLAGS.knn is not None, "--knn"), (FLAGS.patch_radius is not None, "--patch_radius"),
                            (FLAGS.pca_scale != -1, "--pca_scale")):
            if given:
                parser.error("--knn_ladder and %s are mutually exclusive: every row chooses its own neighbour count from the ladder" % flag)
        try:
            ladder = _select.check_ladder(_select.DEFAULT_LADDER if FLAGS.knn_ladder.strip() == "auto"
                                          else [int(v) for v in FLAGS.knn_ladder.split(",")])
        except ValueError as e:
            parser.error("--knn_ladder %s: %s" % (FLAGS.knn_ladder, e))
    if FLAGS.select_slack is not None:
        if ladder is None:
            parser.error("--select_slack belongs to --estimator pca --knn_ladder K[,K...]")
        try:
            slack = _select.check_slack(FLAGS.select_slack)
        except ValueError as e:
            parser.error("--select_slack: %s" % e)
    fit = FITS.get(FLAGS.estimator)
    if FLAGS.patch_radius is not None:
        if FLAGS.estimator not in ("pca", "quadric") or ks is not None:
            parser.error("--patch_radius belongs to --estimator pca / --estimator quadric without --knn: the network's radii are its "
                         "model's, and the scales of a k-NN fit are neighbour counts")
        if len(FLAGS.patch_radius) > MAX_SCALES or not all(0.0 < r < float("inf") for r in FLAGS.patch_radius):
            parser.error("--patch_radius takes 1 to %d positive finite numbers" % MAX_SCALES)
    if FLAGS.estimator == "hough":
        if ks is None:
            parser.error("--estimator hough needs --knn K[,K...]: the Hough transform exists over neighbour lists only")
        try:
            _hough.check_params(FLAGS.hough_triplets, FLAGS.hough_bins, FLAGS.hough_rotations, FLAGS.hough_seed)
        except ValueError as e:
            parser.error("--estimator hough: %s" % e)
    if FLAGS.estimator == "robust":
        if ks is None:
            parser.error("--estimator robust needs --knn K[,K...]: the robust plane fit exists over neighbour lists only")
        try:
            _robust.check_params(FLAGS.robust_iters, FLAGS.robust_sigma, FLAGS.robust_falloff, FLAGS.robust_floor)
        except ValueError as e:
            parser.error("--estimator robust: %s" % e)
    window = depth_window_args(FLAGS, parser, fit, ks, ladder)
    voxel = None
    if FLAGS.voxel_size != 0.0:
        later = "left for later: the network route and depth frames are a pull request of their own"
        for given, flag, why in ((FLAGS.depth_images, "--depth_images 1", later),
                                 (FLAGS.sparse_patches, "--sparse_patches 1",
                                  "left for later: the grid renumbers the cloud and a .pidx entry names a row that no longer exists"),
                                 (FLAGS.query_positions, "--query_positions 1",
                                  "left for later: the rows of the files would be positions, not the rows of the .xyz"),
                                 (FLAGS.subsample != "hash", "--subsample %s" % FLAGS.subsample,
                                  "left for later: the reference's subsample order is that of the full cloud"),
                                 (not fit, "--estimator net", later)):
            if given:
                parser.error("--voxel_size does not go with %s: %s" % (flag, why))
        try:
            voxel = _downsample.check_params(FLAGS.voxel_size, FLAGS.voxel_mode or "centroid")
        except ValueError as e:
            parser.error("--voxel_size: %s" % e)
    elif FLAGS.voxel_mode is not None:
        parser.error("--voxel_mode belongs to --voxel_size V")
    denoise = None
    if FLAGS.denoise:
        later = "left for later: the network route and depth frames are a pull request of their own"
        for given, flag, why in ((FLAGS.depth_images, "--depth_images 1", later),
                                 (FLAGS.sparse_patches, "--sparse_patches 1",
                                  "the filter moves all points and the rows of a .pidx would not be the rows of the denoised cloud"),
                                 (FLAGS.query_positions, "--query_positions 1",
                                  "left for later: the rows of the files would be positions, not the rows of the .xyz"),
                                 (FLAGS.subsample != "hash", "--subsample %s" % FLAGS.subsample,
                                  "the reference's subsample order is that of the cloud as given"),
                                 (FLAGS.reproducible, "--reproducible 1", "it belongs to the network route"),
                                 (not fit, "--estimator net", later)):
            if given:
                parser.error("--denoise does not go with %s: %s" % (flag, why))
        try:
            denoise = _denoise.check_params(FLAGS.denoise_k, FLAGS.denoise, FLAGS.denoise_angle, FLAGS.denoise_falloff, FLAGS.denoise_sigma,
                                            FLAGS.denoise_step)
        except ValueError as e:
            parser.error("--denoise: %s" % e)
    else:
        for flag in ("denoise_k", "denoise_angle", "denoise_falloff", "denoise_sigma", "denoise_step"):
            if getattr(FLAGS, flag) != parser.get_default(flag):
                parser.error("--%s belongs to --denoise ITERS" % flag)
    if fit:
        for given, flag, why in ((FLAGS.depth_images and window is None, "--depth_images 1",
                                  "depth frames belong to the network path (--estimator net), or to --depth_window auto with --knn"),
                                 (FLAGS.reproducible, "--reproducible 1",
                                  "it freezes the network's thresholds (--estimator net); the %s has none" % fit["noun"]),
                                 (FLAGS.subsample != "hash", "--subsample %s" % FLAGS.subsample,
                                  fit.get("subsamples", "the %s uses the full ball and subsamples nothing" % fit["noun"]))):
            if given:
                parser.error("--estimator %s does not take %s: %s" % (FLAGS.estimator, flag, why))
    smooth = None
    if FLAGS.smooth:
        for given, flag, why in ((FLAGS.sparse_patches, "--sparse_patches 1", "not all rows have normals"),
                                 (FLAGS.query_positions, "--query_positions 1", "not all rows have normals"),
                                 (FLAGS.depth_images and window is None, "--depth_images 1",
                                  "smoothing of depth frames is left for later on the network path (--depth_window serves it)"),
                                 (window is not None and FLAGS.depth_stride != 1, "--depth_stride %d" % FLAGS.depth_stride,
                                  "not all rows have normals; use --depth_stride 1")):
            if given:
                parser.error("--smooth does not go with %s: %s" % (flag, why))
        try:
            smooth = _smooth.check_params(FLAGS.smooth_k, FLAGS.smooth, FLAGS.smooth_angle, FLAGS.smooth_falloff)
        except ValueError as e:
            parser.error("--smooth: %s" % e)
    else:
        for flag in ("smooth_k", "smooth_angle", "smooth_falloff"):
            if getattr(FLAGS, flag) != parser.get_default(flag):
                parser.error("--%s belongs to --smooth ITERS" % flag)
    outliers = None
    if FLAGS.outliers != "0":
        for given, flag, why in ((FLAGS.sparse_patches, "--sparse_patches 1",
                                  "the filter renumbers the cloud and a .pidx entry could name a removed point (left for later)"),
                                 (FLAGS.subsample != "hash", "--subsample %s" % FLAGS.subsample,
                                  "the reference's subsample order is that of the unfiltered cloud"),
                                 (FLAGS.depth_images and FLAGS.depth_stride != 1, "--depth_stride %d" % FLAGS.depth_stride,
                                  "a strided frame estimates at a subset of the cloud; use --depth_stride 1")):
            if given:
                parser.error("--outliers does not go with %s: %s" % (flag, why))
        if FLAGS.outliers == "radius" and FLAGS.outlier_radius is None:
            parser.error("--outliers radius needs --outlier_radius R")
        if FLAGS.outliers == "statistical" and FLAGS.outlier_radius is not None:
            parser.error("--outlier_radius belongs to --outliers radius")
        if FLAGS.outliers == "radius" and FLAGS.outlier_std != parser.get_default("outlier_std"):
            parser.error("--outlier_std belongs to --outliers statistical")
        try:
            outliers = _outliers.check_params(FLAGS.outliers, FLAGS.outlier_k, FLAGS.outlier_std, FLAGS.outlier_radius, None,
                                              FLAGS.outlier_passes)
        except ValueError as e:
            parser.error("--outliers: %s" % e)
    else:
        for flag in ("outlier_k", "outlier_std", "outlier_radius", "outlier_passes"):
            if getattr(FLAGS, flag) != parser.get_default(flag):
                parser.error("--%s belongs to --outliers statistical / radius" % flag)
    if FLAGS.query_positions and FLAGS.sparse_patches:
        parser.error("--query_positions 1 and --sparse_patches 1 are mutually exclusive: the queries are positions or cloud points")
    if FLAGS.query_positions and FLAGS.subsample != "hash":
        parser.error("--query_positions 1 needs --subsample hash: the reference's subsample order is defined for cloud points only")
    if FLAGS.depth_images:
        if FLAGS.sparse_patches or FLAGS.query_positions:
            parser.error("--depth_images 1 is mutually exclusive with --sparse_patches 1 and --query_positions 1: the queries are the "
                         "frame's valid pixels (--depth_stride thins them)")
        if FLAGS.viewpoint is not None:
            parser.error("--viewpoint does not go with --depth_images 1: the camera is the viewpoint")
        if FLAGS.depth_stride < 1:
            parser.error("--depth_stride must be >= 1")
    elif FLAGS.depth_stride != 1:
        parser.error("--depth_stride belongs to --depth_images 1")
    if FLAGS.orient is None:
        FLAGS.orient = "viewpoint" if FLAGS.depth_images else "0"
    if FLAGS.orient == "viewpoint" and FLAGS.viewpoint is None and not FLAGS.depth_images:
        parser.error("--orient viewpoint needs --viewpoint X Y Z")
    if FLAGS.orient == "0" and FLAGS.viewpoint is not None:
        parser.error("--viewpoint belongs to --orient mst / --orient viewpoint")
    if not 1 <= FLAGS.orient_k <= 16:
        parser.error("--orient_k must be in 1 .. 16")
    archs = {"experts_n_est": ARCH_EXPERTS, "ss_norm_est": ARCH_SINGLE, "ms_norm_est": ARCH_MULTI,
             "ms_sw_n_est": ARCH_SWITCH}      # test_n_est_w_experts.py / test_n_est.py / test_n_est_w_switching.py
    if FLAGS.model not in archs:
        raise SystemExit("--model must be one of %s" % sorted(archs))
    arch = archs[FLAGS.model]
    results_path = FLAGS.results_path
    base = os.getcwd()
    pc_path = FLAGS.dataset_path if FLAGS.dataset_path is not None else os.path.join(base, "data/" + FLAGS.dataset_name + "/")
    output_dir = os.path.join(results_path, FLAGS.dataset_name + "_results/")
    os.makedirs(output_dir, exist_ok=True)
    flog = open(os.path.join(output_dir, "log.txt"), "w")

    def printout(data):
        print(data)
        flog.write(data + "\n")
        sys.stdout.flush()

    if window is not None:
        try:
            scale = 0 if ladder is not None else _pca.check_scale(getattr(FLAGS, fit["scale_flag"]), len(ks))
        except ValueError as e:
            raise SystemExit("--%s: %s" % (fit["scale_flag"], e))
        frames = DepthFrames(pc_path, FLAGS.testset, FLAGS.depth_stride)
        for name in frames.names:
            run_window_frame(frames, name, FLAGS, window, ks, ladder, slack, scale, smooth, output_dir, printout)
        flog.close()
        return 0
    if fit:
        cfg = NestiConfig.for_model(FLAGS.model)
        if ladder is not None:
            rc = run_select(FLAGS, cfg, ladder, slack, pc_path, output_dir, printout, smooth, outliers, voxel, denoise)
            flog.close()
            return rc
        if FLAGS.patch_radius is not None:
            cfg.patch_radius = list(FLAGS.patch_radius)       # the fits read the radii and their number, nothing else of cfg
        try:
            scale = _pca.check_scale(getattr(FLAGS, fit["scale_flag"]), cfg.n_scales if ks is None else len(ks))
        except ValueError as e:
            raise SystemExit("--%s with --model %s: %s" % (fit["scale_flag"], FLAGS.model, e))
        rc = run_fit(FLAGS, cfg, scale, pc_path, output_dir, printout, ks, smooth, outliers, voxel, denoise)
        flog.close()
        return rc

    model_file = os.path.join(results_path, "model.nstw")
    if os.path.exists(model_file):
        printout("Loading model %s" % model_file)
        W, cfg = wts.load(model_file)
        cfg = cfg or NestiConfig()
    elif os.path.exists(os.path.join(results_path, "model.ckpt.index")) and os.path.exists(os.path.join(results_path, "parameters.p")):
        # the reference's own artefacts: parameters.p / gmm.p / model.ckpt (test_n_est_w_experts.py:46-54, 98-105, 201)
        from . import tf_ckpt
        printout("Loading model %s" % os.path.join(results_path, "model.ckpt"))
        cfg, W = tf_ckpt.load_reference_model(results_path)
    elif FLAGS.synthetic_weights:
        cfg = NestiConfig.for_model(FLAGS.model)
        printout("No %s: using synthetic weights (seed %d)" % (model_file, wts.WEIGHT_SEED))
        W = wts.synthetic_weights(cfg)
    else:
        raise SystemExit("%s not found (pass --synthetic_weights to run without a trained model)" % model_file)
    if cfg.arch != arch:
        raise SystemExit("--model %s does not match the trained model in %s" % (FLAGS.model, results_path))
    device = "cuda:%d" % FLAGS.gpu
    from .config import CASCADE_DTYPES
    dtype = FLAGS.dtype if FLAGS.dtype != "auto" else (("f16x8c" if cfg.n_gaussians == 8 else "f16x3c") if arch == ARCH_EXPERTS else "f16x3")
    if dtype in CASCADE_DTYPES + ("f16x8",) and arch != ARCH_EXPERTS:
        raise SystemExit("--dtype %s belongs to experts_n_est (two-stage gate / narrow-format cross terms in the expert towers); use f16x3 for "
                         "--model %s" % (dtype, FLAGS.model))
    if dtype in ("f16x8", "f16x8c") and cfg.n_gaussians != 8:
        raise SystemExit("--dtype %s needs the 8^3 Gaussian grid; use f16x3c" % dtype)
    if FLAGS.depth_images:
        frames = DepthFrames(pc_path, FLAGS.testset, FLAGS.depth_stride)
        patch_counts = frames.max_rows
    else:
        dataset = PointcloudPatchDataset(pc_path, FLAGS.testset, cfg, seed=3627473, sparse_patches=FLAGS.sparse_patches,
                                         device=device, query_positions=bool(FLAGS.query_positions))
        patch_counts = dataset.shape_patch_count
    # two library batches in flight on two HIP streams; a batch is half the largest shape (rounded up to 256 rows) unless
    # that exceeds what the workspace of the dtype allows (~2 MB per query in f16x3c, twice that in the full pair modes)
    lib_batch = FLAGS.lib_batch or {"f16x3c": 50000, "f16x8c": 50000, "f16": 50000, "bf16": 50000, "f32": 8192}.get(dtype, 25000)
    half = (max(patch_counts + [1]) + 1) // 2
    batch = max(FLAGS.batch_size, min(lib_batch, max(1024, (half + 255) // 256 * 256)))
    # ... and what the device has free right now: two arenas (one per stream) + the 1024-query calibration workspace must fit
    # (the defaults are sized for an otherwise idle 288 GB MI355X; a shared or smaller device gets smaller batches, not an OOM)
    fit = fit_batch(cfg, dtype, batch, device, lanes=2)
    if fit != batch:
        printout("library batch %d -> %d rows: %.1f GB free on %s" % (batch, fit, torch.cuda.mem_get_info(device)[0] / 1e9, device))
        batch = fit
    if (FLAGS.x8_layers is not None or FLAGS.x8_format is not None) and dtype not in ("f16x8", "f16x8c"):
        raise SystemExit("--x8_layers / --x8_format belong to --dtype f16x8 / f16x8c")
    est = NormalEstimator(cfg, W, dtype=dtype, device=device, batch=batch, n_streams=2, subsample=FLAGS.subsample,
                          x8_layers=FLAGS.x8_layers, x8_format=FLAGS.x8_format, reproducible=bool(FLAGS.reproducible))
    repro = bool(FLAGS.reproducible)
    if repro and FLAGS.subsample != "hash":
        raise SystemExit("--reproducible 1 needs --subsample hash")
    printout("Model restored.")

    def calibrate(name, cloud):
        if dtype in CASCADE_DTYPES:
            # the gate margin, from up to 1024 queries of THIS shape (noise level and density change the activation and
            # error statistics from shape to shape); calibrate_gate_margin resets the gate's counters, so the statistics
            # printed below are this shape's
            from .calibrate import calibrate_gate_margin
            sp, sn = cloud.build(0, min(1024, cloud.patch_count))
            printout("gate margin for %s: tau = %.4g" % (name, calibrate_gate_margin(est.net, sp, sn, reproducible=repro,
                                                                                     shape_queries=cloud.patch_count)))
            del sp, sn
        if dtype in ("f16x8", "f16x8c"):
            # the conditioning guard of the FP6 / FP8 cross-term layers: its |n| threshold from the same sample of THIS shape
            from .calibrate import calibrate_x8_guard
            sp, sn = cloud.build(0, min(1024, cloud.patch_count))
            printout("cross-term guard threshold for %s: |n| < %.4g" % (name, calibrate_x8_guard(est.net, sp, sn, reproducible=repro)))
            del sp, sn

    if FLAGS.depth_images:
        for name in frames.names:
            run_depth_frame(est, frames, name, FLAGS, output_dir, printout, lambda cloud: calibrate(name, cloud),
                            write_experts=arch != ARCH_SWITCH, outliers=outliers)
        flog.close()
        return 0

    for ind, name in enumerate(dataset.shape_names):
        cloud = dataset.get_shape(ind)
        # before anything looks at the cloud: the calibration, the network, --smooth and --orient see the kept points alone
        cloud, chain = stage_shape(cloud, None, outliers, None, name, output_dir, printout)
        calibrate(name, cloud)
        if repro:
            normals, expert, probs = est.run_verified(cloud)
            lv, rs = est.last_verified, est.net.reproducible_stats()
            printout("reproducible run of %s: %d pass%s, thresholds used: tau %.9g, |n| < %.9g; violations == 0: %s "
                     "(largest gate error %.4g, largest |dn| %.3g)"
                     % (name, lv["passes"], "" if lv["passes"] == 1 else "es", lv["tau"], lv["thr"],
                        rs["gate_violations"] + rs["guard_violations"] == 0, lv["max_margin_err"], lv["max_dn"]))
        else:
            normals, expert, probs = est.run(cloud)
        support = None
        if smooth is not None:
            # after the whole shape is estimated and before the orientation; a pure function of the estimated normals, so a
            # reproducible run stays one
            normals, support, count = _smooth.smooth_cloud(cloud, normals.contiguous(), smooth)
            printout(smooth_line(name, cloud.patch_count, smooth, count.cpu().numpy()))
        if FLAGS.orient != "0":
            # after the whole shape is estimated (in the reproducible mode: after its last verified pass); only signs change
            from .orient import stats_dict
            ost = stats_dict(est.orient(cloud, normals, FLAGS.orient, FLAGS.viewpoint, FLAGS.orient_k))
            printout(orient_line(name, FLAGS.orient, ost, cloud.patch_count))
        torch.cuda.synchronize()
        if FLAGS.query_positions:
            # the sentinel (decide.hip: mask_empty_queries_kernel): expert -1; the single-tower models have only the (0, 0, 0) normal
            alone = (expert == -1) if expert is not None else (normals == 0).all(dim=1)
            printout("query positions of %s: %d, of which %d had no neighbourhood (no cloud point inside any ball: written as 0 0 0 / -1 / 0)"
                     % (name, cloud.patch_count, int(alone.sum().item())))
        if chain.kept is not None and cloud.queries is None:
            # back to the rows of <shape>.xyz: a removed row is 0 0 0 / -1 / 0 (nesti_image_scatter over an image one row high)
            kept = torch.from_numpy(chain.kept.astype("int32")).to(normals.device)
            normals = _outliers.scatter_rows(normals.contiguous(), kept, chain.n, 0.0)
            if expert is not None:
                expert, probs = _outliers.scatter_rows(expert.contiguous(), kept, chain.n, -1), _outliers.scatter_rows(probs.contiguous(), kept, chain.n, 0.0)
            if support is not None:
                support, count = _outliers.scatter_rows(support.contiguous(), kept, chain.n, 0.0), _outliers.scatter_rows(count.contiguous(), kept, chain.n, 0)
        # byte-identical to the reference's np.savetxt calls (test_n_est_w_experts.py:182-188), ~6x faster
        textio.write_f32(os.path.join(output_dir, name + ".normals"), normals.cpu().numpy())
        if support is not None:
            write_smooth_support(os.path.join(output_dir, name + ".smooth_support"), support.cpu().numpy(), count.cpu().numpy())
        printout("saved normals for " + name)
        if expert is None or arch == ARCH_SWITCH:   # the ablation drivers write .normals only (test_n_est.py:118,
            continue                                 # test_n_est_w_switching.py:158)
        textio.write_i32(os.path.join(output_dir, name + ".experts"), expert.cpu().numpy())
        textio.write_f32(os.path.join(output_dir, name + ".experts_probs"), probs.cpu().numpy())
        printout("saved experts for " + name)
        if dtype in CASCADE_DTYPES:
            st = est.net.cascade_stats()
            printout("two-stage gate on %s: %d of %d queries decided by the f16x3 gate, f16 gate error on a logit difference "
                     "<= %.4g (tau %.4g, threshold now %.4g)" % (name, st["rechecked"], st["queries"], st["max_margin_err"],
                                                                st["tau"], st["tau_eff"]))
            if st.get("stage2"):
                printout("  of those, %d were decided by the gating net with FP6 cross terms at 8^3 (its error on a logit difference "
                         "<= %.4g, margin %.4g) and %d went on to the f16x3 gate" % (st["stage2_decided"], st["max_margin_err2"],
                                                                                    st["tau2_eff"], st["stage2_residual"]))
            if st["widen_events"]:
                printout("  the measured error came within a factor 1.5 of the margin: the library widened it and re-decided "
                         "%d more queries with the f16x3 gate before these files were written" % st["widened"])
        if dtype in ("f16x8", "f16x8c"):
            gs = est.net.x8_guard_stats()
            printout("narrow-format cross terms on %s: %d of %d expert outputs re-evaluated in f16x3 (|n| below %.4g), largest |dn| measured %.3g"
                     % (name, gs["rechecked"], gs["queries"], gs["thr_eff"], gs["max_dn"]))
            if gs["dropped"]:
                printout("  WARNING: %d flagged outputs did not fit the guard's lists and keep their narrow-format cross-term values: the "
                         "1 - cos <= 2.5e-6 bound against f16x3 is not established for them (use --dtype f16x3c for this shape)" % gs["dropped"])
    flog.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
