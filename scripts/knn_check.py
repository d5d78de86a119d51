"""What the k-nearest-neighbour path (csrc/knn.hip) costs, on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed
1234), in one process on one box: the search ``CloudPatches.knn`` over all rows at K = 16 / 64 / 256 under the default grid rule
(``knn.default_radius``) and with cells half and twice as wide; the list fits ``nesti_pca_normals_nbr`` / ``nesti_quadric_fit_nbr`` at
ks = (16, 64, 256) over a list searched once; and, for scale, the radius path's ``CloudPatches.pca`` / ``CloudPatches.quadric`` on the
same rows at the default radii.  A warm-up, then ``--reps`` timed repetitions between stream events each.  Also the RMS angle of every
scale of both neighbourhood kinds against the analytic normals.  Recorded, not gated: the radius path does different work (other
neighbourhood sizes), so there is no pass threshold.  Writes one JSON object (default: profiles/knn_check.json).

    python scripts/knn_check.py [--points 100000] [--reps 5] [--out profiles/knn_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import knn as _knn  # noqa: E402
from nesti_net_amd import synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

KS = (16, 64, 256)


def timed(fn, reps, dev):
    """Times of ``reps`` single calls in ms, each between two events on the current stream, after one warm-up call."""
    fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def angle_rms_deg(normals, gt):
    live = (normals != 0).any(axis=1)
    a, b = normals[live].astype(np.float64), gt[live].astype(np.float64)
    cos = np.abs((a * b).sum(1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return float(np.degrees(np.sqrt(np.mean(np.arccos(np.clip(cos, 0.0, 1.0)) ** 2)))), int(live.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "knn_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = NestiConfig()
    pts, gt = synth.make_cloud("ellipsoid", n=args.points, seed=1234)
    cp = CloudPatches(pts, cfg, device=dev)
    M = cp.patch_count
    extent = pts.max(0).astype(np.float64) - pts.min(0)
    med = lambda t: float(np.median(t))

    search = []
    for k in KS:
        r0 = _knn.default_radius(M, k, extent)
        row = {"K": k, "default_pseudo_radius": r0}
        for label, grid in (("default", None), ("half_cell", 0.5 * r0), ("double_cell", 2.0 * r0), ("radius_grid", "radius")):
            t = timed(lambda: cp.knn(0, M, k, grid=grid), args.reps, dev)
            row[label + "_ms"] = t
            row[label + "_rows_per_s"] = M / (med(t) * 1e-3)
        search.append(row)
    nbr = cp.knn(0, M, KS[-1])[0]
    t_plane = timed(lambda: cp.pca_knn(0, M, KS, nbr=nbr), args.reps, dev)
    t_quad = timed(lambda: cp.quadric_knn(0, M, KS, nbr=nbr), args.reps, dev)
    t_pca = timed(lambda: cp.pca(0, M), args.reps, dev)
    t_quadric = timed(lambda: cp.quadric(0, M), args.reps, dev)

    kn, _, kr, kc = (t.cpu().numpy() for t in cp.pca_knn(0, M, KS, nbr=nbr))
    qn = cp.quadric_knn(0, M, KS, nbr=nbr)[0].cpu().numpy()
    bn, _, bc = (t.cpu().numpy() for t in cp.pca(0, M))
    bq = cp.quadric(0, M)[0].cpu().numpy()
    knn_scales, radius_scales = [], []
    for s, k in enumerate(KS):
        rms, live = angle_rms_deg(kn[:, s], gt)
        qrms, qlive = angle_rms_deg(qn[:, s], gt)
        knn_scales.append({"k": k, "mean_radius": float(kr[:, s].mean()), "plane_rows_fitted": live, "plane_rms_angle_deg": rms,
                           "quadric_rows_fitted": qlive, "quadric_rms_angle_deg": qrms})
    for s in range(cfg.n_scales):
        rms, live = angle_rms_deg(bn[:, s], gt)
        qrms, qlive = angle_rms_deg(bq[:, s], gt)
        radius_scales.append({"radius_x_bbdiag": cfg.patch_radius[s], "r_abs": cp.r_abs[s], "mean_ball": float(bc[:, s].mean()),
                              "plane_rows_fitted": live, "plane_rms_angle_deg": rms, "quadric_rows_fitted": qlive,
                              "quadric_rms_angle_deg": qrms})
    res = {"device": torch.cuda.get_device_name(dev), "cloud": "ellipsoid, %d points, seed 1234, no noise" % args.points, "rows": M,
           "reps": args.reps, "ks": list(KS), "search": search,
           "list_plane_fit_ms": t_plane, "list_plane_fit_rows_per_s": M / (med(t_plane) * 1e-3),
           "list_quadric_fit_ms": t_quad, "list_quadric_fit_rows_per_s": M / (med(t_quad) * 1e-3),
           "radius_pca_ms": t_pca, "radius_pca_rows_per_s": M / (med(t_pca) * 1e-3),
           "radius_quadric_ms": t_quadric, "radius_quadric_rows_per_s": M / (med(t_quadric) * 1e-3),
           "knn_scales": knn_scales, "radius_scales": radius_scales}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
