"""What the reproducible mode costs and whether it delivers, on the bench's 100k cloud, in one process on one box:
the default mode (thresholds follow the measurements on the device) against ``NormalEstimator(..., reproducible=True).run_verified``
with the command line's calibration, at two library batch sizes.  Reports normals/s of both, the passes run_verified needed, the
rechecked fractions, the thresholds it ended with, and whether the two reproducible runs are bit-equal at full size (the only
requirement; rate and pass count are recorded, not gated).  Writes one JSON object (default: profiles/reproducible_check.json).

    python scripts/reproducible_check.py [--points 100000] [--steps 3] [--out profiles/reproducible_check.json]"""
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
from nesti_net_amd import synth, weights  # noqa: E402
from nesti_net_amd.calibrate import calibrate_gate, calibrate_gate_margin, calibrate_x8_guard  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.pipeline import NormalEstimator  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402


def one(cfg, W, pts, dev, batch, streams, reproducible, steps):
    est = NormalEstimator(cfg, W, dtype="f16x8c", device=dev, batch=batch, n_streams=streams, reproducible=reproducible)
    cloud = est.prepare(pts)
    # the command line's calibration (cli.py): up to 1024 queries of the shape
    sp, sn = cloud.build(0, min(1024, cloud.patch_count))
    tau = calibrate_gate_margin(est.net, sp, sn, reproducible=reproducible, shape_queries=cloud.patch_count)
    thr = calibrate_x8_guard(est.net, sp, sn, reproducible=reproducible)
    del sp, sn
    run = (lambda: est.run_verified(cloud)) if reproducible else (lambda: est.run(cloud))
    run()                                                   # warm-up
    torch.cuda.synchronize(dev)
    est.net.reproducible_stats(reset=True)
    passes = []
    t0 = time.perf_counter()
    for _ in range(steps):
        out = run()
        if reproducible:
            passes.append(est.last_verified["passes"])
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    cs, gs = est.net.cascade_stats(), est.net.x8_guard_stats()
    res = {"batch": batch, "streams": streams, "reproducible": reproducible, "normals_per_s": cloud.patch_count * steps / el,
           "calibrated_tau": tau, "calibrated_thr": thr,
           # default mode: the counters of all timed steps; reproducible: those of the last pass of the last step
           "gate_rechecked_fraction": cs["rechecked"] / max(1, cs["queries"]),
           "guard_rechecked_fraction": gs["rechecked"] / max(1, gs["queries"]),
           "max_margin_err": cs["max_margin_err"], "max_dn": gs["max_dn"]}
    if reproducible:
        res.update(passes=passes, final_tau=est.last_verified["tau"], final_thr=est.last_verified["thr"])
    else:
        res.update(tau_eff=cs["tau_eff"], thr_eff=gs["thr_eff"], widened=cs["widened"])
    out = [t.cpu().numpy() for t in out]
    del est, cloud
    torch.cuda.empty_cache()
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reproducible_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = NestiConfig()
    pts = synth.make_cloud("ellipsoid", n=args.points, seed=1234)[0]       # the bench's cloud
    cp = CloudPatches(pts, cfg, device=dev)
    sp, sn = cp.build(0, 512)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=dev)
    del cp, sp, sn
    half = ((args.points + 1) // 2 + 255) // 256 * 256
    shapes = ((min(50000, half), 2), (max(256, min(50000, half) // 3 // 256 * 256), 1))      # the command line's default, and a third of it on one stream
    runs, outs = [], {}
    for batch, streams in shapes:
        for reproducible in (False, True):
            res, out = one(cfg, W, pts, dev, batch, streams, reproducible, args.steps)
            print(json.dumps(res))
            runs.append(res)
            outs[(batch, reproducible)] = out
    (b0, _), (b1, _) = shapes
    same = lambda r: all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(outs[(b0, r)], outs[(b1, r)]))      # noqa: E731
    result = {"workload": "%d-point ellipsoid (seed 1234), f16x8c, calibrated on 1024 queries" % args.points, "steps": args.steps,
              "device": torch.cuda.get_device_name(dev), "runs": runs,
              "reproducible_runs_bit_equal": bool(same(True)), "default_runs_bit_equal": bool(same(False))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))
    return 0 if result["reproducible_runs_bit_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
