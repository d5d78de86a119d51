"""Child process of tests/test_gpu_query_positions.py: one rank of a world-size-1 or -2 job on ONE GPU (gloo, cuda:0) running the
sharded estimator on POSITION queries (the jittered set of tests/_query_positions_fixture.py) in the headline dtype with the
reproducible mode on and the deterministic calibration; writes its gathered result and what the verified loop did to
<out>.rank<r>.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import nesti_net_amd  # noqa: E402,F401
import _query_positions_fixture as F  # noqa: E402
from nesti_net_amd import dist as nd  # noqa: E402
from nesti_net_amd import weights  # noqa: E402
from nesti_net_amd.calibrate import calibrate_gate, calibrate_gate_margin, calibrate_x8_guard  # noqa: E402
from nesti_net_amd.pipeline import NormalEstimator  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402


def main():
    out = sys.argv[1]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo")
    f = F.make()
    cfg, pts = f["cfg"], f["pts"]
    cp = CloudPatches(pts, cfg, device=dev, pidx=np.arange(7, 20000, 39)[:512])
    sp, sn = cp.build(0, 512)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=dev)
    del cp
    est = NormalEstimator(cfg, W, dtype="f16x8c", device=dev, batch=128, reproducible=True)     # a 250-row shard: two library batches
    cloud = est.prepare(pts, queries=f["jittered"])
    # every rank calibrates on the same sample of the shape, without floating-point sums: the same thresholds, bit for bit
    sp, sn = cloud.build(0, cloud.patch_count)
    tau = calibrate_gate_margin(est.net, sp, sn, reproducible=True, shape_queries=cloud.patch_count)
    thr = calibrate_x8_guard(est.net, sp, sn, reproducible=True)
    normals, expert, probs = nd.estimate_sharded(est, cloud)
    torch.cuda.synchronize()
    lv = est.last_verified
    rank = dist.get_rank() if world > 1 else 0
    print("rank %d: calibrated tau %.9g thr %.9g, verified %s" % (rank, tau, thr, lv))
    np.savez(out + ".rank%d.npz" % rank, normals=normals.cpu().numpy(), expert=expert.cpu().numpy(), probs=probs.cpu().numpy(),
             passes=lv["passes"], tau=lv["tau"], thr=lv["thr"], tau0=tau, thr0=thr)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
