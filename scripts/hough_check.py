"""What the Hough-transform estimator (csrc/hough.hip) buys and costs, in one process on one box.

ACCURACY: on the box (20 000 points, seed 3) at noise 0 / 0.002 / 0.006 of the bounding-box diagonal and on the torus at noise 0.006, the
share of rows within 10 degrees of the analytic normal and the RMS angle, for ``hough_knn``, ``pca_knn`` and ``quadric_knn`` over the same
lists (``--knn``, default 100; Hough at its defaults T = 1000, B = 16, R = 5).  NEAR-EDGE rows of the box -- closer to a box edge (the
second-smallest of 1 - |coord|, clipped at 0) than their neighbourhood radius -- and the other rows are reported separately; the torus
has no edges.
TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234), K = 100, defaults, ``hough_knn`` against
``pca_knn`` over the same lists searched once: a warm-up each, then ``--reps`` repetitions, the two alternating, each between two stream
events.  Recorded, not gated.  Writes one JSON object (default: profiles/hough_check.json).

    python scripts/hough_check.py [--points 100000] [--knn 100] [--reps 5] [--out profiles/hough_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import hough, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

PARAMS = (hough.DEFAULT_TRIPLETS, hough.DEFAULT_BINS, hough.DEFAULT_ROTATIONS, 0)


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


def accuracy(shape, noise, k, dev, n=20000):
    pts, gt = synth.make_cloud(shape, n=n, seed=3, noise=noise)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    nbr = cp.knn(0, n, k)[0]
    fits = {"hough": cp.hough_knn(0, n, (k,), *PARAMS, nbr=nbr), "pca": cp.pca_knn(0, n, (k,), nbr=nbr),
            "quadric": cp.quadric_knn(0, n, (k,), nbr=nbr)}
    radius = fits["pca"][-2].cpu().numpy()[:, 0].astype(np.float64)
    if shape == "box":
        edge = np.sort(np.clip(1.0 - np.abs(pts.astype(np.float64)), 0.0, None), axis=1)[:, 1]
        near = edge < radius
    else:
        near = np.zeros(n, bool)
    rec = {"shape": shape, "points": n, "noise_x_bbdiag": noise, "knn": k, "mean_radius": float(radius.mean())}
    for name, out in fits.items():
        normals = out[0].cpu().numpy()[:, 0]
        rec[name] = {"near_edge": summary(normals, gt, near), "other": summary(normals, gt, ~near)}
    return rec


def timing(points, k, reps, dev):
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    M = cp.patch_count
    nbr = cp.knn(0, M, k)[0]
    calls = {"hough": lambda: cp.hough_knn(0, M, (k,), *PARAMS, nbr=nbr), "pca_knn": lambda: cp.pca_knn(0, M, (k,), nbr=nbr)}
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
    T, B, R, _ = PARAMS
    return {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": M, "knn": k, "triplets": T, "bins": B, "rotations": R,
            "reps": reps, "hough_ms": ms["hough"], "pca_knn_ms": ms["pca_knn"], "hough_median_ms": med["hough"],
            "pca_knn_median_ms": med["pca_knn"], "hough_rows_per_s": M / (med["hough"] * 1e-3),
            "hough_triplets_per_s": M * T / (med["hough"] * 1e-3), "hough_over_pca_knn": med["hough"] / med["pca_knn"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--knn", type=int, default=hough.DEFAULT_KNN)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hough_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "accuracy": [accuracy("box", 0.0, args.knn, dev), accuracy("box", 0.002, args.knn, dev), accuracy("box", 0.006, args.knn, dev),
                        accuracy("torus", 0.006, args.knn, dev)],
           "time": timing(args.points, args.knn, args.reps, dev)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
