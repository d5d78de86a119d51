"""What the voxel downsampling (csrc/voxel.hip, nesti_net_amd/downsample.py) costs and buys, in one process on one box.

TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234) and on the same shape at 1 000 000 points, at
three voxel sizes found by bisection so that about 50 %, 10 % and 1 % of the points remain: the three steps each on its own -- the keys,
the sort (with its pass count), the reduce -- a warm-up each, then ``--reps`` repetitions, the steps alternating, each between two
stream events (launches and output allocations included).  In the same run, on the same device and over the same keys, what a caller
would write today: ``torch.unique(keys, return_inverse=True)``, ``index_add_`` for the fp64 sums and the counts, a division.  That route
sums with floating-point atomics; whether its centroid bytes differ from run to run is recorded (``--torch_runs`` runs).
QUALITY: box and torus, 20 000 points each (seed 3), at noise 0 and 0.006 of the bounding-box diagonal: the share within 10 degrees of
the analytic normal for the plane fit at ``--knn`` (default 100) over the full cloud, against the plane fit at the ORIGINAL positions
(``queries=pts``) over clouds downsampled to about 50 % and 25 %, k scaled by the kept share; and the milliseconds per call of each
(numpy in, numpy out, the median of 3 after a warm-up).  Recorded, not gated.  Writes one JSON object (default:
profiles/voxel_check.json).

    python scripts/voxel_check.py [--points 100000 1000000] [--knn 100] [--reps 7] [--out profiles/voxel_check.json]"""
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
from nesti_net_amd import downsample, pca, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

CLOUDS = (("box", 0.0), ("box", 0.006), ("torus", 0.0), ("torus", 0.006))


def within_10(normals, gt):
    """Share of rows within 10 degrees of ``gt`` (unoriented); a sentinel row (0 0 0) counts as 90 degrees."""
    a, b = normals.astype(np.float64), gt.astype(np.float64)
    cos = np.abs((a * b).sum(1)) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
    ang = np.where((normals != 0).any(axis=1), np.degrees(np.arccos(np.clip(cos, 0.0, 1.0))), 90.0)
    return float((ang <= 10.0).mean())


def voxel_for_share(cloud, share, steps=24):
    """The voxel size at which about ``share`` of the cloud's points remain: bisection on log(voxel) over ``voxel_cloud``."""
    ext = float((cloud.host_pts.max(0).astype(np.float64) - cloud.host_pts.min(0)).max())
    lo, hi = ext * 1e-6, ext
    for _ in range(steps):
        mid = float(np.sqrt(lo * hi))
        kept = downsample.voxel_cloud(cloud, mid)["n_voxels"] / cloud.n_points
        lo, hi = (mid, hi) if kept > share else (lo, mid)
    return float(np.sqrt(lo * hi))


def torch_route(cloud_t, keys, origin_t):
    """What a caller would write today: unique, index_add_ (atomic float sums), a division."""
    uniq, inv = torch.unique(keys, return_inverse=True)
    d = cloud_t.double() - origin_t
    sums = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=keys.device).index_add_(0, inv, d)
    cnt = torch.zeros(uniq.shape[0], dtype=torch.float64, device=keys.device).index_add_(0, inv, torch.ones_like(d[:, 0]))
    return (origin_t + sums / cnt[:, None]).float(), cnt.int(), uniq, inv


def timing(points, shares, reps, torch_runs, dev):
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    N = cp.n_points
    out = {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": N, "reps": reps,
           "sort_tile_items": cp.lib.nesti_sort_tile_items(), "workspace_bytes": cp.lib.nesti_voxel_workspace_bytes(N),
           "what_is_timed": "each step's call between two stream events: its launches, its output allocations and the host time to enqueue "
                            "them; the keys are 1 launch, the sort 4 per pass, the reduce 4; the torch route is unique + 2 index_add_ + a "
                            "division over the same keys, and the ratio adds the keys' time to both sides", "sizes": []}
    for share in shares:
        voxel = voxel_for_share(cp, share)
        origin, vox, dims, lost, bits = downsample.grid_of(pts.min(0), pts.max(0), downsample.check_params(voxel))
        keys = cp.voxel_keys(origin, vox, dims)
        sk, si = cp.sort_pairs(keys, bits)
        origin_t = torch.tensor(origin, dtype=torch.float64, device=dev)
        calls = {"keys": lambda: cp.voxel_keys(origin, vox, dims), "sort": lambda: cp.sort_pairs(keys, bits),
                 "reduce": lambda: cp.voxel_reduce(sk, si, lost, origin), "torch_route": lambda: torch_route(cp.cloud, keys, origin_t)}
        for fn in calls.values():                               # warm-up: the code objects and the allocator
            fn()
        torch.cuda.synchronize(dev)
        ms = {name: [] for name in calls}
        for _ in range(reps):
            for name, fn in calls.items():                      # alternating
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        red = cp.voxel_reduce(sk, si, lost, origin)
        V = int(red[5].cpu()[0])
        ours = [cp.voxel_reduce(sk, si, lost, origin)[0][:V].cpu().numpy().tobytes() for _ in range(torch_runs)]
        theirs = [torch_route(cp.cloud, keys, origin_t)[0].cpu().numpy().tobytes() for _ in range(torch_runs)]
        t_cent = np.frombuffer(theirs[0], np.float32).reshape(-1, 3)
        rec = {"target_share": share, "voxel": voxel, "dims": list(dims), "key_bits": bits, "sort_passes": (bits + 7) // 8, "voxels": V,
               "kept_share": V / N, "largest_count": int(red[2][:V].max().cpu()),
               "torch_voxels": int(t_cent.shape[0]),
               "distinct_centroid_byte_strings_over_%d_runs" % torch_runs: {"hand_written": len(set(ours)), "torch_route": len(set(theirs))},
               "max_abs_centroid_difference_hand_written_vs_torch": float(np.abs(np.frombuffer(ours[0], np.float32).reshape(-1, 3).astype(np.float64)
                                                                                  - t_cent).max()) if t_cent.shape[0] == V else None}
        for name, t in ms.items():
            rec[name + "_ms"] = t
            rec[name + "_median_ms"] = float(np.median(t))
        rec["hand_written_median_ms"] = float(sum(np.median(ms[k]) for k in ("keys", "sort", "reduce")))
        rec["hand_written_over_torch_route"] = rec["hand_written_median_ms"] / (rec["keys_median_ms"] + rec["torch_route_median_ms"])
        out["sizes"].append(rec)
    return out


def _ms(fn, reps=3):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def quality(shape, noise, k, dev, n=20000):
    pts, gt = synth.make_cloud(shape, n=n, seed=3, noise=noise)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    full = lambda: pca.pca_normals(pts, knn=k, device=str(dev))  # noqa: E731
    rec = {"shape": shape, "points": n, "noise_x_bbdiag": noise,
           "full_cloud": {"knn": k, "within_10_deg": within_10(full()["normals"], gt), "ms_per_call": _ms(full)}, "downsampled": []}
    for share in (0.5, 0.25):
        voxel = voxel_for_share(cp, share)
        kk = max(3, int(round(k * share)))
        fit = lambda: pca.pca_normals(pts, knn=kk, queries=pts, downsample=voxel, device=str(dev))  # noqa: E731
        res = fit()
        rec["downsampled"].append({"target_share": share, "voxel": voxel, "kept_share": len(res["voxel_count"]) / n, "knn": kk,
                                   "within_10_deg": within_10(res["normals"], gt), "ms_per_call": _ms(fit)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--shares", type=float, nargs="+", default=[0.5, 0.1, 0.01])
    ap.add_argument("--knn", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch_runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev),
           "time": [timing(p, args.shares, args.reps, args.torch_runs, dev) for p in args.points],
           "quality": [quality(shape, noise, args.knn, dev) for shape, noise in CLOUDS]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
