"""What the image-window search (csrc/window.hip; DESIGN.md 2 "Image-window neighbourhoods") costs and proves, in one process on one
box, on the depth tests' analytic scene -- a sphere of radius 0.6 at (0, 0, 2.2) before the plane z = 3 + 0.3 x, stored as uint16
millimetres, with a rectangle of holes, every 97th pixel and four whole rows empty -- at 480 x 640 (fx = fy = 600) and at 96 x 128
(fx = fy = 120).  At K = 16 / 64 / 256: the window search at the default window (``depth.default_window``); ``nesti_knn`` on the same
cloud with its grid build and without; the exact mode end to end (window, compaction, grid search of the unproven rows, write-back);
and the plane fit over the lists.  A warm-up, then medians of ``--reps`` repetitions, each between two stream events.  Also the share
of rows the window proves per (R, K) on a small grid of R -- what the default rule was chosen from -- and the RMS angle of the
plane-fit normals of ``depth_normals`` against the analytic sphere normal.  Recorded, not gated: no time is a pass criterion.  Writes
one JSON object (default: profiles/window_check.json).

    python scripts/window_check.py [--reps 7] [--out profiles/window_check.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import depth as _depth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

KS = (16, 64, 256)
SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 2.2]), 0.6


def scene(H, W, f):
    """The analytic scene as uint16 millimetres and its camera: the nearer of the sphere and the plane along each pixel's ray."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = (u - cx) / f, (v - cy) / f
    plane = 3.0 / (1.0 - 0.3 * dx)
    dd = dx * dx + dy * dy + 1.0
    dc = dx * SPHERE_C[0] + dy * SPHERE_C[1] + SPHERE_C[2]
    disc = dc * dc - dd * (SPHERE_C @ SPHERE_C - SPHERE_R ** 2)
    sphere = np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0.0))) / dd, np.inf)
    d = np.round(np.minimum(plane, sphere) * 1000.0).astype(np.uint16)
    d[H * 20 // 96:H * 29 // 96, W * 30 // 128:W * 43 // 128] = 0
    d.reshape(-1)[::97] = 0
    d[H * 40 // 96:H * 40 // 96 + 4] = 0
    return d, _depth.Camera(f, f, cx, cy, depth_scale=1e-3)


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


def sphere_rms_deg(res):
    p = res["xyz"].astype(np.float64)
    rel = p - SPHERE_C
    dist = np.linalg.norm(rel, axis=1)
    inner = (np.abs(dist - SPHERE_R) < 2e-3) & (rel[:, 2] < -0.35)
    want = rel[inner] / dist[inner, None]
    cos = np.clip((res["normals"][inner].astype(np.float64) * want).sum(axis=1), -1.0, 1.0)
    return float(np.degrees(np.sqrt(np.mean(np.arccos(cos) ** 2)))), int(inner.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    med = lambda t: float(np.median(t))
    frames = []
    for H, W, f in ((480, 640, 600.0), (96, 128, 120.0)):
        d, cam = scene(H, W, f)
        dc = _depth.depth_to_cloud(d, cam, device=dev)
        M = dc.n_valid
        host = dc.xyz.cpu().numpy()
        cloud = CloudPatches(host, NestiConfig(), device=dev, radius_grid=False)
        rows = []
        for k in KS:
            R = _depth.default_window(k)
            t_win = timed(lambda: _depth.window_knn(dc, k, R, exact=False), args.reps, dev)
            t_grid = timed(lambda: cloud.knn(0, M, k), args.reps, dev)              # the grid is built by the warm-up and kept

            def with_build():
                cloud._knn_grids.clear()
                cloud.knn(0, M, k)
            t_build = timed(with_build, args.reps, dev)

            def exact_mode():
                cloud._knn_grids.clear()                                            # the exact mode pays for its grid
                _depth.window_knn(dc, k, R, exact=True, cloud=cloud)
            t_exact = timed(exact_mode, args.reps, dev)
            lists, _, _, proven = _depth.window_knn(dc, k, R, exact=True, cloud=cloud)
            ref = cloud.knn(0, M, k)[0]
            t_fit = timed(lambda: cloud.pca_knn(0, M, (k,), nbr=lists), args.reps, dev)
            share = {}
            for r in sorted({max(1, R - 2), max(1, R - 1), R, min(15, R + 1), min(15, R + 2), min(15, R + 4),
                             max(1, min(15, int(math.ceil(math.sqrt(k / math.pi)))))}):
                share[str(r)] = float(_depth.window_knn(dc, k, r, exact=False)[3].float().mean().item())
            rows.append({"K": k, "default_R": R, "window_ms": med(t_win), "grid_search_ms": med(t_grid), "grid_build_and_search_ms": med(t_build),
                         "exact_mode_ms": med(t_exact), "plane_fit_over_lists_ms": med(t_fit),
                         "window_speedup_over_grid_search": med(t_grid) / med(t_win),
                         "exact_mode_speedup_over_build_and_search": med(t_build) / med(t_exact),
                         "proven_share_at_default": float(proven.float().mean().item()), "rows_researched": int((proven == 0).sum().item()),
                         "exact_equals_grid_search": bool(torch.equal(lists, ref)), "proven_share_by_R": share,
                         "window_ms_all": t_win, "grid_search_ms_all": t_grid, "grid_build_and_search_ms_all": t_build,
                         "exact_mode_ms_all": t_exact})
        res = _depth.depth_normals(d, cam, estimator="pca", knn=(32,), device=dev)
        rms, n_inner = sphere_rms_deg(res)
        frames.append({"H": H, "W": W, "fx": f, "rows": M, "by_K": rows,
                       "depth_normals_pca_k32": {"sphere_interior_rows": n_inner, "rms_angle_deg_to_analytic_sphere_normal": rms,
                                                 "window": res["window"], "window_proven_share": float(res["window_proven"].mean()),
                                                 "window_exact_rows": res["window_exact_rows"]}})
    out = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "window_factor": _depth.WINDOW_FACTOR, "frames": frames}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
