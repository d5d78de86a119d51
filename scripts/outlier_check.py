"""What the outlier filter (csrc/outlier.hip, nesti_net_amd/outliers.py) buys and costs, in one process on one box.

ACCURACY: box and torus, 20 000 surface points each (seed 3), at noise 0 and 0.006 of the bounding-box diagonal, plus 5 % (1 000 points)
drawn uniformly in the surface points' bounding box (``RandomState(7)``), appended behind them.  The filter runs at its defaults
(statistical, k = 16, std_ratio = 1, one pass).  Recorded: precision and recall of the removed set against the injected points; and, over
the SURFACE rows only, the share within 10 degrees of the analytic normal for the plane fit (``pca_knn``) and the robust plane fit
(``robust_knn``, defaults) at ``--knn`` (default 100) -- on the clean cloud, on the polluted cloud, and on the polluted cloud with
``outliers=`` (a removed surface row is a sentinel and counts as 90 degrees).
TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234), the four steps of one pass each on its own --
the search at K = k + 1, the scores over those lists, the statistics, the compaction -- a warm-up each, then ``--reps`` repetitions, the
four alternating, each between two stream events.  Recorded, not gated.  Writes one JSON object (default: profiles/outlier_check.json).

    python scripts/outlier_check.py [--points 100000] [--knn 100] [--reps 7] [--out profiles/outlier_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import outliers, pca, robust, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

CLOUDS = (("box", 0.0), ("box", 0.006), ("torus", 0.0), ("torus", 0.006))
SHARE = 0.05


def within_10(normals, gt):
    """Share of rows within 10 degrees of ``gt`` (unoriented); a sentinel row (0 0 0) counts as 90 degrees."""
    a, b = normals.astype(np.float64), gt.astype(np.float64)
    cos = np.abs((a * b).sum(1)) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
    ang = np.where((normals != 0).any(axis=1), np.degrees(np.arccos(np.clip(cos, 0.0, 1.0))), 90.0)
    return float((ang <= 10.0).mean())


def accuracy(shape, noise, k, dev, n=20000):
    pts, gt = synth.make_cloud(shape, n=n, seed=3, noise=noise)
    n_out = int(round(SHARE * n))
    lo, hi = pts.min(0), pts.max(0)
    extra = (lo + np.random.RandomState(7).rand(n_out, 3) * (hi - lo)).astype(np.float32)
    dirty = np.ascontiguousarray(np.concatenate([pts, extra]))
    injected = np.arange(len(dirty)) >= n
    f = outliers.remove_outliers(dirty, device=str(dev))
    removed = ~f["inlier"]
    rec = {"shape": shape, "surface_points": n, "injected_points": n_out, "noise_x_bbdiag": noise, "knn": k,
           "filter": dict(outliers.check_params()._asdict()), "passes": f["passes"], "removed": int(removed.sum()),
           "precision": float(injected[removed].mean()) if removed.any() else None, "recall": float(removed[injected].mean()),
           "surface_rows_removed": float(removed[~injected].mean())}
    fits = {"pca": lambda p, **kw: pca.pca_normals(p, knn=k, device=str(dev), **kw),
            "robust": lambda p, **kw: robust.robust_normals(p, knn=k, device=str(dev), **kw)}
    for name, fit in fits.items():
        rec[name + "_within_10_deg"] = {"clean_cloud": within_10(fit(pts)["normals"], gt),
                                        "polluted": within_10(fit(dirty)["normals"][:n], gt),
                                        "polluted_filtered": within_10(fit(dirty, outliers="statistical")["normals"][:n], gt)}
    return rec


def timing(points, reps, dev):
    p = outliers.check_params()
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    N = cp.n_points
    nbr = cp.knn(0, N, p.k + 1)[0]
    mean = cp.outlier_scores(0, N, p.k, nbr=nbr)[0]
    stats = cp.outlier_threshold(mean, p.std_ratio)
    calls = {"search": lambda: cp.knn(0, N, p.k + 1), "scores": lambda: cp.outlier_scores(0, N, p.k, nbr=nbr),
             "statistics": lambda: cp.outlier_threshold(mean, p.std_ratio), "compaction": lambda: cp.outlier_compact(mean, stats[3:])}
    for fn in calls.values():                                   # warm-up: the code objects, the search grid and the allocator
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
    n_kept = int(cp.outlier_compact(mean, stats[3:])[4].cpu()[0])
    rec = {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": N, "k": p.k, "std_ratio": p.std_ratio, "reps": reps,
           "kept": n_kept, "what_is_timed": "each step's call between two stream events: its launches, its output allocations and the host "
                                            "time to enqueue them; the statistics are 4 launches, the compaction 3"}
    for name, t in ms.items():
        rec[name + "_ms"] = t
        rec[name + "_median_ms"] = float(np.median(t))
    rec["pass_median_ms"] = float(sum(np.median(t) for t in ms.values()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--knn", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "outlier_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "accuracy": [accuracy(shape, noise, args.knn, dev) for shape, noise in CLOUDS],
           "time": timing(args.points, args.reps, dev)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
