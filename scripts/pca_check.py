"""What the plane-fit kernel (csrc/pca.hip) costs next to its floor, on the bench's 100k cloud (cloud 0 of bench.py: the noise-free
ellipsoid, seed 1234), default radii, in one process on one box: ``CloudPatches.pca`` over all rows, and in the same process
``CloudPatches.count_balls`` over the same rows -- the same sweep over the candidates without moments or solve, the floor the kernel
can approach.  A warm-up, then ``--reps`` timed repetitions between stream events each.  Also the RMS angle of every scale against
the analytic normals.  Recorded, not gated.  Writes one JSON object (default: profiles/pca_check.json).

    python scripts/pca_check.py [--points 100000] [--reps 5] [--out profiles/pca_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pca_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = NestiConfig()
    pts, gt = synth.make_cloud("ellipsoid", n=args.points, seed=1234)
    cp = CloudPatches(pts, cfg, device=dev)
    M, S = cp.patch_count, cfg.n_scales
    out = (torch.empty((M, S, 3), dtype=torch.float32, device=dev), torch.empty((M, S, 3), dtype=torch.float32, device=dev),
           torch.empty((M, S), dtype=torch.int32, device=dev))
    t_pca = timed(lambda: cp.pca(0, M, out=out), args.reps, dev)
    t_cnt = timed(lambda: cp.count_balls(0, M), args.reps, dev)
    normals, eig, n_ball = (t.cpu().numpy() for t in out)
    assert np.array_equal(n_ball, cp.count_balls(0, M).cpu().numpy())
    med_pca, med_cnt = float(np.median(t_pca)), float(np.median(t_cnt))
    scales = []
    for s in range(S):
        rms, live = angle_rms_deg(normals[:, s], gt)
        scales.append({"radius_x_bbdiag": cfg.patch_radius[s], "r_abs": cp.r_abs[s], "mean_ball": float(n_ball[:, s].mean()),
                       "rows_with_3_or_more": live, "rms_angle_deg": rms,
                       "mean_variation": float(np.mean(eig[:, s, 0] / np.maximum(eig[:, s].sum(1), 1e-30)))})
    res = {"device": torch.cuda.get_device_name(dev), "cloud": "ellipsoid, %d points, seed 1234, no noise" % args.points, "rows": M,
           "reps": args.reps, "pca_ms": t_pca, "count_ms": t_cnt, "pca_rows_per_s": M / (med_pca * 1e-3),
           "count_rows_per_s": M / (med_cnt * 1e-3), "pca_over_count_rate": med_cnt / med_pca, "scales": scales}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
