#!/usr/bin/env python3
"""Position queries on the bench's 100k cloud (no-noise ellipsoid, seed 1234), dtype f16x8c, the command line's calibration with
the reproducible mode on (thresholds calibrated once, on the index path's first 1024 rows, and frozen for all four legs):

  (a) the index path: every cloud point, file order;
  (b) positions equal to the cloud's own points in file order     -- the three outputs must equal (a)'s bit for bit;
  (c) the same positions in a random permutation `perm` -- the outputs must be (b)'s rows permuted, bit for bit.  NOTE: the
      subsample key is the patch ROW (row i of (c) is keyed i, the same position is keyed perm[i] in (b)), so a ball above P
      points is thinned to another uniform subset and this statement can hold only for rows whose three balls hold <= P
      points; the script reports it as it is (`all_rows_bit_equal_to_b_permuted`, part of the exit status) and records next
      to it the two statements the row key does allow: those rows alone, and ALL rows against the index path with
      pidx = perm, which gives row i the same key;
  (d) positions jittered by sigma = 0.02 x bbdiag.

Writes normals/s per leg and the number of sentinel rows to profiles/query_positions_check.json.  The timings are recorded, not
gated: (c) measures what losing the memory order of the queries costs, (d) what empty and small balls change.

    python scripts/query_positions_check.py [--points 100000] [--steps 2] [--out profiles/query_positions_check.json]
"""
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


def timed(est, cloud, steps, warmup=1):
    for _ in range(warmup):
        out = est.run(cloud)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = est.run(cloud)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return [t.cpu().numpy() for t in out], cloud.patch_count / dt


def bits_equal(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "query_positions_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = NestiConfig()
    pts = synth.make_cloud("ellipsoid", n=args.points, seed=1234)[0]
    est = NormalEstimator(cfg, weights.synthetic_weights(cfg), dtype="f32", device=dev, batch=512)
    sp, sn = est.prepare(pts).build(0, 512)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=dev)
    del est
    est = NormalEstimator(cfg, W, dtype="f16x8c", device=dev, batch=min(args.batch, args.points), n_streams=2, reproducible=True)
    by_idx = est.prepare(pts)
    sp, sn = by_idx.build(0, min(1024, by_idx.patch_count))
    tau = calibrate_gate_margin(est.net, sp, sn, reproducible=True, shape_queries=by_idx.patch_count)
    thr = calibrate_x8_guard(est.net, sp, sn, reproducible=True)
    del sp, sn
    perm = np.random.RandomState(11).permutation(len(pts))
    jit = (pts + np.random.RandomState(5).normal(0, 0.02 * by_idx.bbdiag, size=pts.shape)).astype(np.float32)
    res = {"points": int(args.points), "dtype": "f16x8c", "batch": est.batch, "streams": est.n_streams, "steps": args.steps,
           "tau": tau, "thr": thr, "device": torch.cuda.get_device_name(0), "legs": {}}
    a, rate = timed(est, by_idx, args.steps)
    res["legs"]["a_index"] = {"normals_per_s": rate}
    b, rate = timed(est, est.prepare(pts, queries=pts), args.steps)
    res["legs"]["b_positions_file_order"] = {"normals_per_s": rate, "sentinel_rows": int((b[1] == -1).sum()),
                                             "bit_equal_to_a": all(bits_equal(x, y) for x, y in zip(a, b))}
    cloud_c = est.prepare(pts, queries=pts[perm])
    c, rate = timed(est, cloud_c, args.steps)
    # the subsample key is the patch row: only rows whose balls all hold <= P points are promised to follow the permutation
    n_ball = torch.cat([cloud_c.build(lo, min(8192, len(pts) - lo), want_idx=True)[3] for lo in range(0, len(pts), 8192)]).cpu().numpy()
    small = (n_ball <= cfg.num_point).all(axis=1)
    res["legs"]["c_positions_permuted"] = {
        "normals_per_s": rate, "sentinel_rows": int((c[1] == -1).sum()), "rows_with_all_balls_within_P": int(small.sum()),
        "those_rows_bit_equal_to_b_permuted": all(bits_equal(x[small], y[perm][small]) for x, y in zip(c, b)),
        "all_rows_bit_equal_to_b_permuted": all(bits_equal(x, y[perm]) for x, y in zip(c, b))}
    c_idx = [t.cpu().numpy() for t in est.run(est.prepare(pts, pidx=perm))]
    res["legs"]["c_positions_permuted"]["bit_equal_to_index_path_with_pidx_perm"] = all(bits_equal(x, y) for x, y in zip(c, c_idx))
    d, rate = timed(est, est.prepare(pts, queries=jit), args.steps)
    res["legs"]["d_positions_jittered"] = {"normals_per_s": rate, "sentinel_rows": int((d[1] == -1).sum())}
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    lc = res["legs"]["c_positions_permuted"]
    ok = res["legs"]["b_positions_file_order"]["bit_equal_to_a"] and lc["all_rows_bit_equal_to_b_permuted"] and \
        lc["those_rows_bit_equal_to_b_permuted"] and lc["bit_equal_to_index_path_with_pidx_perm"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
