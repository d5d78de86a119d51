"""What the depth-image front end (csrc/depth.hip) costs next to the network, on one 480 x 640 frame, in one process on one box: the three
library calls -- nesti_depth_to_cloud, nesti_image_scatter, nesti_project_to_image -- on preallocated buffers, each as a window of
``--calls`` back-to-back calls between two events after a warm-up (a single call is far too short to time), ``depth_to_cloud`` as a
user calls it (upload, allocations and the one readback included; host clock around a synchronise), and ``estimate_depth`` at stride 1
and 4 in the headline dtype.  Recorded, not gated.  Writes one JSON object (default: profiles/depth_check.json).

    python scripts/depth_check.py [--calls 200] [--reps 5] [--out profiles/depth_check.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import _lib, weights  # noqa: E402
from nesti_net_amd.cli import fit_batch  # noqa: E402
from nesti_net_amd.calibrate import calibrate_gate, calibrate_gate_margin, calibrate_x8_guard  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.depth import Camera, depth_to_cloud  # noqa: E402
from nesti_net_amd.pipeline import NormalEstimator  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

H, W = 480, 640


def vga_frame():
    """A sphere of radius 0.6 at (0, 0, 2.2) in front of the plane z = 3 + 0.3 x, uint16 millimetres, 5 % of the pixels zero."""
    fx = fy = 600.0
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = (u - cx) / fx, (v - cy) / fy
    plane = 3.0 / (1.0 - 0.3 * dx)
    dd, dc = dx * dx + dy * dy + 1.0, 2.2
    disc = dc * dc - dd * (2.2 ** 2 - 0.6 ** 2)
    z = np.minimum(plane, np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0.0))) / dd, np.inf))
    d = np.round(z * 1000.0).astype(np.uint16)
    d[np.random.RandomState(480).uniform(size=d.shape) < 0.05] = 0
    return d, Camera(fx, fy, cx, cy, 1e-3)


def window(fn, calls, reps, dev):
    """Median / min / max time of ONE call in ms, from ``reps`` windows of ``calls`` back-to-back calls between two events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b) / calls)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls_per_window": calls, "windows": reps}


def wall(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "all_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_check.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_check.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    depth, cam = vga_frame()
    n = H * W
    st = _lib.stream_ptr(torch.cuda.current_stream(dev))
    # ---- the three calls on preallocated buffers ------------------------------------------------------------------------------------
    d = torch.from_numpy(depth.view(np.int16)).to(dev)
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    pix = torch.empty((n,), dtype=torch.int32, device=dev)
    rank = torch.empty((n,), dtype=torch.int32, device=dev)
    qidx = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.nesti_depth_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    c = cam.to_c()

    def to_cloud(stride):
        _lib.check(lib.nesti_depth_to_cloud(_lib.ptr(d), _lib.DEPTH_U16, H, W, ctypes.byref(c), stride, _lib.ptr(xyz), _lib.ptr(pix),
                                            _lib.ptr(rank), _lib.ptr(qidx), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), st), "nesti_depth_to_cloud")

    to_cloud(1)
    n_valid = int(counts.cpu()[0])
    rows = torch.randn((n_valid, 3), dtype=torch.float32, device=dev)
    image = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    index = torch.empty((H, W), dtype=torch.int32, device=dev)
    fill = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def scatter():
        _lib.check(lib.nesti_image_scatter(_lib.ptr(rows), _lib.ptr(pix), n_valid, 3, H, W, fill, _lib.ptr(image), st), "nesti_image_scatter")

    def project():
        _lib.check(lib.nesti_project_to_image(_lib.ptr(xyz), _lib.ptr(rows), n_valid, 3, H, W, ctypes.byref(c), fill, _lib.ptr(image),
                                              _lib.ptr(index), _lib.ptr(ws), ws.numel(), st), "nesti_project_to_image")

    front = {"nesti_depth_to_cloud_stride1": window(lambda: to_cloud(1), args.calls, args.reps, dev),
             "nesti_depth_to_cloud_stride4": window(lambda: to_cloud(4), args.calls, args.reps, dev),
             "nesti_image_scatter_C3": window(scatter, args.calls, args.reps, dev),
             "nesti_project_to_image_C3": window(project, args.calls, args.reps, dev)}
    project()
    torch.cuda.synchronize(dev)
    own = bool((index.reshape(-1) == rank).all().item())          # the frame's own cloud lands on its own pixels
    as_called = wall(lambda: depth_to_cloud(depth, cam, device=dev), args.reps, dev)
    # ---- the whole frame in the headline dtype ----------------------------------------------------------------------------------------
    cfg = NestiConfig()
    dc = depth_to_cloud(depth, cam, device=dev)
    cp = CloudPatches(dc.xyz.cpu().numpy(), cfg, device=dev)
    sp, sn = cp.build(0, 512)
    Wc = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=dev)
    del cp, sp, sn
    est = NormalEstimator(cfg, Wc, dtype="f16x8c", device=dev, batch=fit_batch(cfg, "f16x8c", 50000, dev, lanes=2), n_streams=2)

    def calibrate(cloud):
        sp, sn = cloud.build(0, min(1024, cloud.patch_count))
        calibrate_gate_margin(est.net, sp, sn)
        calibrate_x8_guard(est.net, sp, sn)

    frames = {}
    for stride in (4, 1):
        res = est.estimate_depth(depth, cam, stride=stride, on_cloud=calibrate)      # the warm-up; it calibrates
        fn = lambda: est.estimate_depth(depth, cam, stride=stride)                    # noqa: E731
        t = wall(fn, 2, dev) if stride == 1 else wall(fn, args.reps, dev)
        normals = len(res["pix"])
        frames["estimate_depth_stride%d" % stride] = dict(t, normals=normals, normals_per_s=normals / (t["median_ms"] * 1e-3))
    per_frame = frames["estimate_depth_stride1"]["median_ms"]
    front_ms = front["nesti_depth_to_cloud_stride1"]["median_ms"] + 3 * front["nesti_image_scatter_C3"]["median_ms"]
    result = {"workload": "one %d x %d uint16 frame (sphere in front of a tilted plane, 5 %% holes): %d valid pixels" % (H, W, n_valid),
              "device": torch.cuda.get_device_name(dev),
              "library_calls_ms": front, "depth_to_cloud_as_called_ms": as_called,
              "projection_of_own_cloud_index_equals_rank": own,
              "frames": frames,
              "front_end_over_frame": front_ms / per_frame,
              "front_end_over_frame_is": "(nesti_depth_to_cloud + 3 x nesti_image_scatter, device time per call) / estimate_depth at stride 1 (wall)",
              "note": "recorded, not gated; estimate_depth includes the cloud's one pass through the host, the search grid and the orientation"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
