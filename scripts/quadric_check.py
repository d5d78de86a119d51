"""What the quadric-fit kernel (csrc/quadric.hip) costs next to the plane fit it contains (csrc/pca.hip), on ONE grid and the same rows:
the 20 000-point sphere of the tests (seed 7, radii 0.05 / 0.1 / 0.2 of the bounding-box diagonal: balls of ~150 / 600 / 2 400 points) --
the 256 rows tests/test_gpu_quadric.py takes from it, and all of its rows.  ``CloudPatches.quadric`` and ``CloudPatches.pca`` alternate:
after a warm-up of both, ``--reps`` windows each, a window being ``--calls`` back-to-back calls between two stream events (one call on
256 rows is tens of microseconds: a single one would time the launch).  Reports the median time per call and per query and the ratio.
Recorded, not gated.  Writes one JSON object (default: profiles/quadric_check.json).

    python scripts/quadric_check.py [--reps 7] [--calls 200] [--out profiles/quadric_check.json]"""
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


def window(fn, calls):
    """ms per call over ``calls`` back-to-back calls between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def compare(cp, reps, calls, dev):
    M, S = cp.patch_count, cp.cfg.n_scales
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    n_ball = torch.empty((M, S), dtype=torch.int32, device=dev)
    out_p = (f32(M, S, 3), f32(M, S, 3), n_ball)
    out_q = (f32(M, S, 3), f32(M, S, 2), f32(M, S, 3), torch.empty_like(n_ball))
    run_p, run_q = (lambda: cp.pca(0, M, out=out_p)), (lambda: cp.quadric(0, M, out=out_q))
    window(run_p, 3), window(run_q, 3)
    torch.cuda.synchronize(dev)
    t_p, t_q = [], []
    for _ in range(reps):
        t_p.append(window(run_p, calls))
        t_q.append(window(run_q, calls))
    assert torch.equal(out_p[0].view(torch.int32), out_q[2].view(torch.int32)) and torch.equal(out_p[2], out_q[3])
    mp, mq = float(np.median(t_p)), float(np.median(t_q))
    live = (out_q[0] != 0).any(dim=2)
    return {"rows": M, "calls_per_window": calls, "pca_ms_per_call": t_p, "quadric_ms_per_call": t_q, "pca_us_per_query": 1e3 * mp / M,
            "quadric_us_per_query": 1e3 * mq / M, "quadric_over_pca": mq / mp, "mean_ball": n_ball.float().mean(0).tolist(),
            "fitted_per_scale": live.sum(0).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quadric_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = NestiConfig(patch_radius=[0.05, 0.1, 0.2])
    pts, _ = synth.make_cloud("sphere", 20000, seed=7)
    rows = np.arange(0, len(pts), 39)[:256]
    cp = CloudPatches(pts, cfg, device=dev, pidx=rows)
    res = {"device": torch.cuda.get_device_name(dev), "cloud": "sphere, 20000 points, seed 7, radii x bbdiag %s" % cfg.patch_radius,
           "reps": args.reps, "test_rows": compare(cp, args.reps, args.calls, dev)}
    cp.pidx, cp.patch_count = None, cp.n_points            # the same grid, every point a query
    res["all_rows"] = compare(cp, args.reps, max(1, args.calls // 20), dev)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
