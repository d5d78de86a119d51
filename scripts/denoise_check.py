"""What the point-denoising pass (csrc/denoise.hip) buys and costs, in one process on one box.

QUALITY: on the box and the torus (20 000 points, seed 3) at noise 0, 0.002 and 0.006 of the bounding-box diagonal, the RMS and the
95th-percentile distance to the analytic surface before and after 1, 2, 3 and 5 passes of ``denoise.denoise_points`` -- at the defaults,
with ``sigma`` at its upper bound (no height weight), at ``k = 32`` and at ``sigma`` 0.25, 0.5 and 1 whatever the default is.  The torus
distance is ``|hypot(hypot(x, y) - 1, z) - 0.35|``, the box distance that to the surface of [-1, 1]^3; on the box the rows within 0.1 of
an edge (by their input position) are reported separately.  With it the share of rows within 10 degrees of the analytic normal for the plane fit, the Hough transform and the robust
fit at ``--knn`` (default 100) neighbours over the input and over every denoised cloud.
TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234), milliseconds per pass at k = 16 / 32 / 64 over
lists searched once at K = 64 with the plane-fit normals of the 32 nearest neighbours: the default lane group (16, 32, 64 lanes per row)
against the one-wave-per-row form (``nesti_debug_denoise_lanes(64)``) and against ``nesti_smooth_normals_nbr`` at the same k -- the same
gather shape, the yardstick -- the three alternating, each repetition ``--calls`` calls between two stream events after a warm-up;
medians of ``--reps``.  A torch composition of the same arithmetic (``pts[nbr]`` gathers, fp64 reductions) is timed the same way, and a
whole default ``denoise_points`` call is split into search, normals and pass (stream events) beside its wall time.  Recorded, not gated.
Writes one JSON object (default: profiles/denoise_check.json).

    python scripts/denoise_check.py [--points 100000] [--knn 100] [--reps 7] [--calls 200] [--out profiles/denoise_check.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import _lib, denoise, hough, robust, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

HOUGH = (hough.DEFAULT_TRIPLETS, hough.DEFAULT_BINS, hough.DEFAULT_ROTATIONS, 0)
ROBUST = (robust.DEFAULT_ITERS, robust.DEFAULT_SIGMA, robust.DEFAULT_FALLOFF, robust.DEFAULT_FLOOR)
ITERS = (1, 2, 3, 5)
SETTINGS = {"default": {}, "no_height_weight": {"sigma": denoise.MAX_SIGMA}, "k_32": {"k": 32}, "sigma_0.25": {"sigma": 0.25}, "sigma_0.5": {"sigma": 0.5},
            "sigma_1": {"sigma": 1.0}}


def surface_distance(shape, pts):
    p = pts.astype(np.float64)
    if shape == "torus":
        return np.abs(np.hypot(np.hypot(p[:, 0], p[:, 1]) - 1.0, p[:, 2]) - 0.35)
    q = np.abs(p) - 1.0                                                      # the box [-1, 1]^3
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.abs(np.minimum(q.max(1), 0.0))


def distances(shape, pts, near):
    d = surface_distance(shape, pts)
    out = {}
    for name, rows in (("all", np.ones(len(pts), bool)), ("near_edge", near), ("other", ~near)):
        if rows.any() and (name == "all" or near.any()):
            out[name] = {"rows": int(rows.sum()), "rms": float(np.sqrt(np.mean(d[rows] ** 2))), "p95": float(np.percentile(d[rows], 95.0))}
    return out


def within_10_deg(pts, gt, k, dev):
    """The share of rows within 10 degrees of the analytic normal for the three fits over one search at ``k``; a sentinel row misses."""
    n = len(pts)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    nbr = cp.knn(0, n, k)[0]
    fits = {"pca": cp.pca_knn(0, n, (k,), nbr=nbr)[0], "hough": cp.hough_knn(0, n, (k,), *HOUGH, nbr=nbr)[0],
            "robust": cp.robust_knn(0, n, (k,), *ROBUST, nbr=nbr)[0]}
    out = {}
    for name, t in fits.items():
        a, b = t[:, 0].cpu().numpy().astype(np.float64), gt.astype(np.float64)
        cos = np.abs((a * b).sum(1)) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
        ang = np.where((a != 0).any(1), np.degrees(np.arccos(np.clip(cos, 0.0, 1.0))), 90.0)
        out[name] = float((ang <= 10.0).mean())
    return out


def quality(shape, noise, knn, dev, n=20000):
    pts, gt = synth.make_cloud(shape, n=n, seed=3, noise=noise)
    if shape == "box":
        near = np.sort(np.clip(1.0 - np.abs(pts.astype(np.float64)), 0.0, None), axis=1)[:, 1] < 0.1
    else:
        near = np.zeros(n, bool)
    rec = {"shape": shape, "points": n, "noise_x_bbdiag": noise, "knn": knn,
           "input": {"distance": distances(shape, pts, near), "within_10_deg": within_10_deg(pts, gt, knn, dev)}}
    for label, kw in SETTINGS.items():
        p = denoise.check_params(**kw)
        rows = {"params": {"k": p.k, "normal_k": p.normal_k, "angle_deg": p.angle, "falloff": p.falloff, "sigma": p.sigma, "step": p.step}}
        cur, done = pts, 0
        for it in ITERS:                                                     # the passes of `it` continue those of the smaller count
            cur = denoise.denoise_points(cur, iters=it - done, device=str(dev), **kw)["points"]
            done = it
            rows["iters_%d" % it] = {"distance": distances(shape, cur, near), "within_10_deg": within_10_deg(cur, gt, knn, dev),
                                     "moved": int((cur.view(np.uint32) != pts.view(np.uint32)).any(1).sum())}
        rec[label] = rows
    print("quality: %s, noise %g done" % (shape, noise), file=sys.stderr, flush=True)
    return rec


def torch_pass(pts, normals, nbr, k, cos_t, falloff, sigma, step):
    """The arithmetic of the pass as a torch composition (valid lists, eligible normals): gathers and fp64 reductions."""
    J = nbr[:, :k].long()
    p64, n64 = pts.double(), normals.double()
    D = p64[J] - p64[:, None, :]
    d2 = (D * D).sum(-1)
    r2 = d2.max(1).values
    qc = (n64 * n64).sum(-1)
    v = n64 / qc.sqrt()[:, None]
    nj = n64[J]
    qj = (nj * nj).sum(-1)
    dd = (n64[:, None, :] * nj).sum(-1)
    t = (dd.abs() / (qc[:, None] * qj).sqrt() - cos_t) / (1.0 - cos_t)
    take = t > 0
    t = t.clamp(max=1.0)
    u = 1.0 - falloff * d2 / r2[:, None]
    h = (v[:, None, :] * D).sum(-1)
    x = h / (sigma * r2.sqrt())[:, None]
    a = u * t / (1.0 + x * x)
    W = torch.where(take, a * a, torch.zeros_like(a))
    delta = step * (W * h).sum(1) / W.sum(1)
    return (p64 + delta[:, None] * v).float()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timing(points, reps, calls, dev):
    lib = _lib.load()
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    M = cp.patch_count
    nbr = cp.knn(0, M, 64)[0]
    normals = cp.pca_knn(0, M, (32,), nbr=nbr)[0][:, 0].contiguous()
    p = denoise.check_params()
    par = (p.cos_t, p.falloff, p.sigma, p.step)
    rec = {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": M, "list_K": 64, "reps": reps, "calls_per_rep": calls,
           "input": "plane-fit normals of the 32 nearest neighbours", "angle_deg": p.angle, "falloff": p.falloff, "sigma": p.sigma,
           "step": p.step, "per_k": []}

    def lanes(n):
        _lib.check(lib.nesti_debug_denoise_lanes(n), "nesti_debug_denoise_lanes")

    for k in (16, 32, 64):
        forms = {"group": lambda: (lanes(0), cp.denoise_knn(normals, 0, M, k, *par, nbr=nbr))[1],
                 "wave": lambda: (lanes(64), cp.denoise_knn(normals, 0, M, k, *par, nbr=nbr))[1],
                 "smooth": lambda: cp.smooth_knn(normals, 0, M, k, p.cos_t, p.falloff, nbr=nbr),
                 "torch": lambda: torch_pass(cp.cloud, normals, nbr, k, *par)}
        ms = {name: [] for name in forms}
        try:
            outs = {name: fn() for name, fn in forms.items()}              # warm-up: the code objects and the allocator
            torch.cuda.synchronize(dev)
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["group"], outs["wave"]))
            torch_diff = float((outs["torch"].double() - outs["group"][0].double()).abs().max())
            for _ in range(reps):
                for name, fn in forms.items():                              # alternating
                    ms[name].append(timed(fn, calls if name != "torch" else max(1, calls // 4)))
        finally:
            lib.nesti_debug_denoise_lanes(0)
        med = {name: float(np.median(t)) for name, t in ms.items()}
        rec["per_k"].append({"k": k, "group_lanes": 16 if k <= 16 else 32 if k <= 32 else 64, "ms": ms, "median_ms": med,
                             "wave_over_group": med["wave"] / med["group"], "group_over_smooth": med["group"] / med["smooth"],
                             "torch_over_group": med["torch"] / med["group"], "group_rows_per_s": M / (med["group"] * 1e-3),
                             "same_bytes": bool(same), "torch_max_abs_diff": torch_diff})
        print("time: k = %d done" % k, file=sys.stderr, flush=True)
    # a whole default call: wall time (host clock round a call that synchronises), and its stages between stream events
    walls, stages = [], {"search": [], "normals": [], "pass": []}
    K = max(p.k, p.normal_k)
    for rep in range(reps + 1):                                              # the first is the warm-up
        t0 = time.perf_counter()
        denoise.denoise_points(pts, device=str(dev))
        wall = (time.perf_counter() - t0) * 1e3
        cur, split = cp, {"search": 0.0, "normals": 0.0, "pass": 0.0}
        for it in range(p.iters):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            lists = cur.knn(0, M, K)[0]
            ev[1].record()
            nrm = cur.pca_knn(0, M, (p.normal_k,), nbr=lists)[0][:, 0].contiguous()
            ev[2].record()
            moved = cur.denoise_knn(nrm, 0, M, p.k, *par, nbr=lists)[0]
            ev[3].record()
            ev[3].synchronize()
            for i, name in enumerate(("search", "normals", "pass")):
                split[name] += ev[i].elapsed_time(ev[i + 1])
            if it + 1 < p.iters:
                cur = CloudPatches(moved.cpu().numpy(), NestiConfig(), device=dev, radius_grid=False)
        if rep:
            walls.append(wall)
            for name in stages:
                stages[name].append(split[name])
    rec["default_call"] = {"iters": p.iters, "k": p.k, "normal_k": p.normal_k, "wall_ms": walls, "wall_median_ms": float(np.median(walls)),
                           "stage_median_ms": {name: float(np.median(t)) for name, t in stages.items()},
                           "note": "wall: numpy in, numpy out, with the upload, the grids' builds, the host copy between the passes and the "
                                   "readback; the stages: stream events round the %d passes' search, plane fit and pass" % p.iters}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--knn", type=int, default=hough.DEFAULT_KNN)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_check.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_check.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "quality": [quality(shape, noise, args.knn, dev) for shape in ("box", "torus") for noise in (0.0, 0.002, 0.006)],
           "time": timing(args.points, args.reps, args.calls, dev)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
