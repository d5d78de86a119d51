"""What the orientation post-pass (csrc/orient.hip) costs next to an estimate, on the bench's 100k ellipsoid, in one process on one
box: ``NormalEstimator.orient`` alone (grid, kNN, edges, Boruvka, roots, apply) between two events, 5 repetitions after a warm-up,
next to one f16x8c estimate step; plus the launch plan, the candidates a row's kNN scan visits, the stats, and the number of edge
weights whose bits differ from the numpy restatement's on the GPU tests' graph cases (expected 0).  Recorded, not gated.
Writes one JSON object (default: profiles/orient_check.json).

    python scripts/orient_check.py [--points 100000] [--reps 5] [--out profiles/orient_check.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import synth, weights  # noqa: E402
from nesti_net_amd.calibrate import calibrate_gate, calibrate_gate_margin, calibrate_x8_guard  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.orient import orient_device, stats_dict  # noqa: E402
from nesti_net_amd.pipeline import NormalEstimator  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402


def launch_plan(M):
    """The launches of one NESTI_ORIENT_MST call, from the fixed plan in nesti_orient_normals (memsets and the stats copy not counted)."""
    clog = lambda n: max(0, math.ceil(math.log2(n))) if n > 1 else 0      # noqa: E731
    rounds = min(40, clog(M) + 1)
    jumps = sum(clog((M >> r) + 2) + 1 for r in range(rounds))
    return {"grid": 6, "eligible_knn_edges": 3, "boruvka_rounds": rounds, "boruvka": 1 + 3 * rounds + jumps, "root_apply": 5,
            "total": 6 + 3 + 1 + 3 * rounds + jumps + 5}


def candidates_per_row(pts, R):
    """Mean number of points in the 3 x 3 x 3 cell block of a point's cell, for the grid nesti_patches_grid builds at radius R."""
    p = pts.astype(np.float64)
    lo, ext = p.min(0), (p.max(0) - p.min(0)).max()
    cell = max(R * 1.0001, ext / 127.0)
    ijk = np.minimum(127, np.floor((p - lo) / cell).astype(np.int64))
    dims = ijk.max(0) + 1
    vol = np.zeros(tuple(dims + 2), np.int64)
    np.add.at(vol, tuple((ijk + 1).T), 1)
    box = sum(np.roll(vol, (a, b, c), (0, 1, 2)) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    return float(box[tuple((ijk + 1).T)].mean()), float(cell)


def timed(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "all_ms": [round(v, 3) for v in ms]}


def weight_bit_differences(dev):
    import _orient_fixture as F
    from test_gpu_orient import lib_graph
    out = {}
    for name in ("ellipsoid3001", "ellipsoid3001_k1", "ellipsoid3001_k16", "lattice", "ellipsoid3001_zero10"):
        c = F.case(name)
        ref, got = F.predicted(name)["g"], lib_graph(c["xyz"], c["normals"], c["R"], c["K"], dev)
        e = ref["u"] >= 0
        out[name] = {"edges": int(e.sum()), "weight_bits_differ": int((got["wbits"][e] != ref["wbits"][e]).sum()),
                     "structure_equal": bool(np.array_equal(got["nbr"], ref["nbr"]) and np.array_equal(got["u"], ref["u"])
                                             and np.array_equal(got["v"], ref["v"]) and np.array_equal(got["flip"][e], ref["flip"][e]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "orient_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = NestiConfig()
    pts, gt = synth.make_cloud("ellipsoid", n=args.points, seed=1234)       # the bench's cloud
    cp = CloudPatches(pts, cfg, device=dev)
    sp, sn = cp.build(0, 512)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=dev)
    del cp, sp, sn
    half = ((args.points + 1) // 2 + 255) // 256 * 256
    est = NormalEstimator(cfg, W, dtype="f16x8c", device=dev, batch=min(50000, half), n_streams=2)
    cloud = est.prepare(pts)
    sp, sn = cloud.build(0, min(1024, cloud.patch_count))
    calibrate_gate_margin(est.net, sp, sn)
    calibrate_x8_guard(est.net, sp, sn)
    del sp, sn
    R = float(cloud.r_abs[-1])
    step = timed(lambda: est.run(cloud), 2, dev)
    estimated = est.run(cloud)[0]
    # (a) what the product orients: the step's own output (synthetic weights: directions without geometry, the graph is the cloud's)
    work = estimated.clone()
    t_est = timed(lambda: (work.copy_(estimated), orient_device(cloud.cloud, work, R, args.k))[1], args.reps, dev)
    copy = timed(lambda: work.copy_(estimated), args.reps, dev)
    st_est = stats_dict(orient_device(cloud.cloud, work.copy_(estimated), R, args.k))
    # (b) normals with geometry: the analytic ones tilted (sigma 0.15), scaled to [0.3, 3], random sign
    rs = np.random.RandomState(7)
    n = (gt + rs.normal(0, 0.15, gt.shape)) * rs.uniform(0.3, 3.0, (len(gt), 1)) * rs.choice([-1.0, 1.0], (len(gt), 1))
    nd = torch.from_numpy(n.astype(np.float32)).to(dev)
    work2 = nd.clone()
    t_geo = timed(lambda: (work2.copy_(nd), orient_device(cloud.cloud, work2, R, args.k))[1], args.reps, dev)
    st_geo = stats_dict(orient_device(cloud.cloud, work2.copy_(nd), R, args.k))
    inward = int(((work2.cpu().numpy().astype(np.float64) * gt).sum(1) < 0).sum())
    t_view = timed(lambda: (work2.copy_(nd), orient_device(cloud.cloud, work2, R, args.k, viewpoint=(0.0, 0.0, 9.0), mode="viewpoint"))[1],
                   args.reps, dev)
    cand, cell = candidates_per_row(pts, R)
    result = {"workload": "%d-point ellipsoid (seed 1234), K = %d, R = r_abs[-1] = %.6g" % (args.points, args.k, R),
              "device": torch.cuda.get_device_name(dev),
              "estimate_step_f16x8c_ms": step, "orient_mst_on_estimated_normals_ms": t_est, "orient_mst_on_tilted_analytic_normals_ms": t_geo,
              "orient_viewpoint_mode_ms": t_view, "normals_copy_included_in_each_ms": copy,
              "orient_over_step": t_est["median_ms"] / step["median_ms"],
              "launches_per_mst_call": launch_plan(args.points), "knn_candidates_per_row": cand, "grid_cell": cell,
              "fp64_distance_tests_per_cloud": cand * args.points,
              "stats_estimated_normals": st_est, "stats_tilted_analytic_normals": st_geo, "inward_after_orientation_tilted_analytic": inward,
              "graph_cases_vs_numpy_restatement": weight_bit_differences(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
