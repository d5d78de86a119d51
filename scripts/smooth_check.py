"""What the normal-smoothing pass (csrc/smooth.hip) buys and costs, in one process on one box.

ACCURACY: on the box (20 000 points, seed 3) at noise 0 and 0.002 of the bounding-box diagonal and on the torus at noise 0.006 -- the
clouds of scripts/hough_check.py -- the share of rows within 10 degrees of the analytic normal and the RMS angle for ``hough_knn``,
``pca_knn`` and ``quadric_knn`` over the same lists (``--knn``, default 100; Hough at its defaults), before the smoothing and after 1,
2, 3 and 5 passes at the defaults (k = 16, 45 degrees, falloff 0.75) over the leading 16 entries of those lists.  NEAR-EDGE rows of the
box -- closer to a box edge than their neighbourhood radius -- and the other rows are reported separately; the torus has no edges.
TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234), milliseconds per pass at k = 16 / 32 / 64 over
lists searched once at K = 64, smoothing the plane-fit normals of the 16 nearest neighbours: the default lane group (16, 32, 64 lanes
per row) against the one-wave-per-row form (``nesti_debug_smooth_lanes(64)``): a warm-up each, then ``--reps`` repetitions, the two
alternating, each repetition ``--calls`` calls between two stream events (a single pass is too short a window).  Recorded, not gated.
Writes one JSON object (default: profiles/smooth_check.json).

    python scripts/smooth_check.py [--points 100000] [--knn 100] [--reps 9] [--calls 20] [--out profiles/smooth_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import _lib, hough, smooth, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

HOUGH = (hough.DEFAULT_TRIPLETS, hough.DEFAULT_BINS, hough.DEFAULT_ROTATIONS, 0)
ITERS = (1, 2, 3, 5)


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
    fits = {"hough": cp.hough_knn(0, n, (k,), *HOUGH, nbr=nbr), "pca": cp.pca_knn(0, n, (k,), nbr=nbr),
            "quadric": cp.quadric_knn(0, n, (k,), nbr=nbr)}
    radius = fits["pca"][-2].cpu().numpy()[:, 0].astype(np.float64)
    if shape == "box":
        edge = np.sort(np.clip(1.0 - np.abs(pts.astype(np.float64)), 0.0, None), axis=1)[:, 1]
        near = edge < radius
    else:
        near = np.zeros(n, bool)
    p = smooth.check_params()
    rec = {"shape": shape, "points": n, "noise_x_bbdiag": noise, "knn": k, "mean_radius": float(radius.mean()),
           "smooth": {"k": p.k, "angle_deg": p.angle, "falloff": p.falloff}}
    for name, out in fits.items():
        cur = out[0][:, 0].contiguous()
        rows = {"before": cur.cpu().numpy()}
        done = 0
        for it in ITERS:                                       # the passes of `it` continue those of the smaller count
            cur, support, count = smooth.smooth_cloud(cp, cur, p._replace(iters=it - done), nbr=nbr)
            done = it
            rows["iters_%d" % it] = cur.cpu().numpy()
        rec[name] = {key: {"near_edge": summary(v, gt, near), "other": summary(v, gt, ~near)} for key, v in rows.items()}
    return rec


def timing(points, reps, calls, dev):
    lib = _lib.load()
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    M = cp.patch_count
    nbr = cp.knn(0, M, 64)[0]
    normals = cp.pca_knn(0, M, (16,), nbr=nbr)[0][:, 0].contiguous()
    p = smooth.check_params()
    rec = {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": M, "list_K": 64, "reps": reps, "calls_per_rep": calls,
           "input": "plane-fit normals of the 16 nearest neighbours", "angle_deg": p.angle, "falloff": p.falloff, "per_k": []}
    for k in (16, 32, 64):
        forms = {"group": 0, "wave": 64}                        # nesti_debug_smooth_lanes: 0 = the smallest group that holds k
        ms = {name: [] for name in forms}
        same = None
        try:
            outs = {}
            for name, lanes in forms.items():                   # warm-up: the code objects and the allocator
                _lib.check(lib.nesti_debug_smooth_lanes(lanes), "nesti_debug_smooth_lanes")
                outs[name] = cp.smooth_knn(normals, 0, M, k, p.cos_t, p.falloff, nbr=nbr)
            torch.cuda.synchronize(dev)
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["group"], outs["wave"]))
            for _ in range(reps):
                for name, lanes in forms.items():               # alternating
                    _lib.check(lib.nesti_debug_smooth_lanes(lanes), "nesti_debug_smooth_lanes")
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        cp.smooth_knn(normals, 0, M, k, p.cos_t, p.falloff, nbr=nbr)
                    b.record()
                    b.synchronize()
                    ms[name].append(a.elapsed_time(b) / calls)
        finally:
            lib.nesti_debug_smooth_lanes(0)
        med = {name: float(np.median(t)) for name, t in ms.items()}
        rec["per_k"].append({"k": k, "group_lanes": 16 if k <= 16 else 32 if k <= 32 else 64, "group_ms": ms["group"], "wave_ms": ms["wave"],
                             "group_median_ms": med["group"], "wave_median_ms": med["wave"], "wave_over_group": med["wave"] / med["group"],
                             "group_rows_per_s": M / (med["group"] * 1e-3), "same_bytes": bool(same)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--knn", type=int, default=hough.DEFAULT_KNN)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "smooth_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "accuracy": [accuracy("box", 0.0, args.knn, dev), accuracy("box", 0.002, args.knn, dev), accuracy("torus", 0.006, args.knn, dev)],
           "time": timing(args.points, args.reps, args.calls, dev)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
