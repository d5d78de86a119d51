"""What the robust plane fit (csrc/robust.hip) buys and costs, in one process on one box.

ACCURACY: on the six 20 000-point clouds of scripts/hough_check.py and scripts/select_check.py (box and torus, seed 3, noise 0 / 0.002 /
0.006 of the bounding-box diagonal) at ``--knn`` (default 100), the share of rows within 10 degrees of the analytic normal and the RMS
angle for ``pca_knn``, ``quadric_knn``, ``hough_knn`` (defaults), ``robust_knn`` (defaults) and ``robust_knn`` with ``init =`` the Hough
normals at ``iters = 2``, all over the same lists.  NEAR-EDGE rows of the box -- closer to a box edge (the second-smallest of 1 -
|coord|, clipped at 0) than their neighbourhood radius -- and the other rows are reported separately; the torus has no edges.
ITERATIONS: the same shares for ``iters`` 1 .. 16 at the other defaults.
TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234), all rows over lists searched once:
``robust_knn`` against ``pca_knn`` and ``hough_knn`` over the same lists, a warm-up each, then ``--reps`` repetitions, the three
alternating, each between two stream events.  Recorded, not gated.  Writes one JSON object (default: profiles/robust_check.json).

    python scripts/robust_check.py [--points 100000] [--knn 100] [--reps 5] [--out profiles/robust_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import hough, robust, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

HOUGH = (hough.DEFAULT_TRIPLETS, hough.DEFAULT_BINS, hough.DEFAULT_ROTATIONS, 0)
ROBUST = (robust.DEFAULT_ITERS, robust.DEFAULT_SIGMA, robust.DEFAULT_FALLOFF, robust.DEFAULT_FLOOR)
CLOUDS = (("box", 0.0), ("box", 0.002), ("box", 0.006), ("torus", 0.0), ("torus", 0.002), ("torus", 0.006))


def angles_deg(normals, gt):
    a, b = normals.astype(np.float64), gt.astype(np.float64)
    cos = np.abs((a * b).sum(1)) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
    return np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))


def summary(normals, gt, rows):
    """Share within 10 degrees and RMS angle over ``rows`` (a mask); a sentinel row counts as 90 degrees."""
    if not rows.any():
        return {"rows": 0}
    ang = np.where((normals[rows] != 0).any(axis=1), angles_deg(normals[rows], gt[rows]), 90.0)
    return {"rows": int(rows.sum()), "within_10_deg": float((ang <= 10.0).mean()), "rms_angle_deg": float(np.sqrt(np.mean(ang ** 2)))}


def accuracy(shape, noise, k, dev, n=20000, most=16):
    pts, gt = synth.make_cloud(shape, n=n, seed=3, noise=noise)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    nbr = cp.knn(0, n, k)[0]
    h = cp.hough_knn(0, n, (k,), *HOUGH, nbr=nbr)
    fits = {"pca": cp.pca_knn(0, n, (k,), nbr=nbr)[0], "quadric": cp.quadric_knn(0, n, (k,), nbr=nbr)[0], "hough": h[0],
            "robust": cp.robust_knn(0, n, (k,), *ROBUST, nbr=nbr)[0],
            "robust_from_hough_2": cp.robust_knn(0, n, (k,), 2, *ROBUST[1:], init=h[0].contiguous(), nbr=nbr)[0]}
    radius = h[-2].cpu().numpy()[:, 0].astype(np.float64)
    if shape == "box":
        edge = np.sort(np.clip(1.0 - np.abs(pts.astype(np.float64)), 0.0, None), axis=1)[:, 1]
        near = edge < radius
    else:
        near = np.zeros(n, bool)
    rec = {"shape": shape, "points": n, "noise_x_bbdiag": noise, "knn": k, "mean_radius": float(radius.mean())}
    for name, out in fits.items():
        normals = out.cpu().numpy()[:, 0]
        rec[name] = {"near_edge": summary(normals, gt, near), "other": summary(normals, gt, ~near)}
    rec["by_iters"] = []
    for it in range(1, most + 1):
        normals = cp.robust_knn(0, n, (k,), it, *ROBUST[1:], nbr=nbr)[0].cpu().numpy()[:, 0]
        rec["by_iters"].append({"iters": it, "near_edge": summary(normals, gt, near), "other": summary(normals, gt, ~near)})
    return rec


def timing(points, k, reps, dev):
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    M = cp.patch_count
    nbr = cp.knn(0, M, k)[0]
    calls = {"robust": lambda: cp.robust_knn(0, M, (k,), *ROBUST, nbr=nbr), "pca_knn": lambda: cp.pca_knn(0, M, (k,), nbr=nbr),
             "hough": lambda: cp.hough_knn(0, M, (k,), *HOUGH, nbr=nbr)}
    for fn in calls.values():                                   # warm-up: the code objects and the allocator
        fn()
    torch.cuda.synchronize(dev)
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():                          # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    med = {name: float(np.median(t)) for name, t in ms.items()}
    iters, sigma, falloff, floor = ROBUST
    return {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": M, "knn": k, "iters": iters, "sigma": sigma,
            "falloff": falloff, "floor": floor, "reps": reps, "robust_ms": ms["robust"], "pca_knn_ms": ms["pca_knn"], "hough_ms": ms["hough"],
            "robust_median_ms": med["robust"], "pca_knn_median_ms": med["pca_knn"], "hough_median_ms": med["hough"],
            "robust_rows_per_s": M / (med["robust"] * 1e-3), "robust_over_pca_knn": med["robust"] / med["pca_knn"],
            "robust_over_hough": med["robust"] / med["hough"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--knn", type=int, default=robust.DEFAULT_KNN)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "accuracy": [accuracy(shape, noise, args.knn, dev) for shape, noise in CLOUDS],
           "time": timing(args.points, args.knn, args.reps, dev)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
