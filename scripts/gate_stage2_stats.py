#!/usr/bin/env python3
"""Recheck stage 2 of the f16x8c gate (include/nesti_hip.h) on the bench workload: what bench.py does not print.

    python scripts/gate_stage2_stats.py [--points 100000] [--steps 2] [--out FILE.json]

Builds cloud 0 of the bench (the no-noise ellipsoid), spreads the synthetic gate like bench.py does, calibrates both gate margins
on the bench's 1024-query sample and prints one JSON line with

  calibration  the sample's statistics with both margins at infinity: the filter's and stage 2's error on a logit difference
               (sigma, max), tau and tau2;
  stage2_on    the library's counters over ``steps`` single-stream passes over the cloud with the stage on (queries, rechecked,
               stage2_rows / _decided / _residual, max_margin_err2, tau2, tau2_eff, ...) and the seconds per pass;
  stage2_off   the same with nesti_model_set_gate_stage2(0) -- the parent's two-pass recheck;
  compare      on vs off over the whole cloud: rows whose arg-max differs, rows whose normals differ in any bit among those with
               equal arg-max, the largest |probs_on - probs_off| and the number of rows whose probabilities moved at all."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import synth, weights  # noqa: E402
from nesti_net_amd.calibrate import calibrate_gate, calibrate_gate_margin, calibrate_x8_guard  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.pipeline import NormalEstimator  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = NestiConfig()
    pts, _ = synth.make_cloud("ellipsoid", n=args.points, seed=1234, noise=synth.PCPNET_NOISE[0])
    W = weights.synthetic_weights(cfg)
    cp = CloudPatches(pts, cfg, device=dev)
    sp, sn = cp.build(0, min(512, args.points))
    W = calibrate_gate(cfg, W, sp, sn, device=dev)
    del cp, sp, sn
    est = NormalEstimator(cfg, W, dtype="f16x8c", device=dev, batch=min(args.points, 100000), n_streams=1)
    cloud = est.prepare(pts)
    sp, sn = cloud.build(0, min(1024, cloud.patch_count))
    net = est.net
    # what calibrate_gate_margin measures, kept: both margins at infinity, every sample query through all three passes
    net.cascade_stats(reset=True)
    net.set_gate_margin(1e30)
    net.set_gate_margin2(1e30)
    net.gate(net.mups(sp, sn))
    cal = net.cascade_stats(reset=True)
    tau = calibrate_gate_margin(net, sp, sn)
    calibrate_x8_guard(net, sp, sn)
    st = net.cascade_stats()
    res = {"points": args.points, "calibration": {**cal, "tau_set": tau, "tau2_set": st["tau2"]}}
    outs = {}
    for key, on in (("stage2_on", True), ("stage2_off", False)):
        net.set_gate_stage2(on)
        cloud.build_grid()
        est.run(cloud)                                    # warm-up
        torch.cuda.synchronize(dev)
        net.cascade_stats(reset=True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            cloud.build_grid()
            out = est.run(cloud)
        torch.cuda.synchronize(dev)
        res[key] = {**net.cascade_stats(reset=True), "seconds_per_pass": (time.perf_counter() - t0) / args.steps}
        outs[key] = [t.cpu().numpy() for t in out]
    (n1, e1, p1), (n0, e0, p0) = outs["stage2_on"], outs["stage2_off"]
    same = e1 == e0
    dp = np.abs(p1 - p0).max(1)
    res["compare"] = {"argmax_differs": int((~same).sum()),
                      "normal_bits_differ_where_argmax_equal": int((n1.view(np.uint32)[same] != n0.view(np.uint32)[same]).any(1).sum()),
                      "max_abs_dprobs": float(dp.max()), "rows_with_moved_probs": int((dp > 0).sum())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
