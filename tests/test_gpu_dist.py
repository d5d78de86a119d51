"""The N > 1 path with real kernels: two fresh processes on ONE GPU (gloo backend, both ranks on cuda:0) run the real
``estimate_sharded`` -- contiguous row blocks, one all_gather_into_tensor -- and every rank must end up with exactly
the single-process result; and ``bench.py --gpus 2 --debug-single-device`` must print a valid line.  (RCCL itself
needs two devices; the driver's multi-GPU bench exercises it.)"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "_dist_gpu_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_world(out, model, world):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        if world == 1:
            for k in ("RANK", "WORLD_SIZE", "MASTER_PORT"):
                env.pop(k)
        procs.append(subprocess.Popen([sys.executable, WORKER, out, model], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        o, _ = p.communicate(timeout=900)
        assert p.returncode == 0, o.decode()[-3000:]


@pytest.mark.parametrize("model", ["experts_n_est", "ss_norm_est"])
def test_two_ranks_on_one_gpu_match_single_process(model, tmp_path, gpu_device):
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    _run_world(one, model, 1)
    _run_world(two, model, 2)
    ref = np.load(one + ".rank0.npz")
    assert ref["normals"].shape == (5001, 3)
    if model == "experts_n_est":
        assert len(np.unique(ref["expert"])) >= 5
    for r in range(2):
        got = np.load(two + ".rank%d.npz" % r)
        for k in ("normals", "expert", "probs"):
            assert np.array_equal(got[k], ref[k]), "rank %d %s" % (r, k)


def test_bench_two_ranks_debug_single_device(gpu_device):
    """``python bench.py --gpus 2`` with NO launcher in the command (the shape of the driver's N = 1 command):
    bench.py starts its two ranks itself as children of torch.distributed.run and forwards rank 0's line and the exit code."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--points", "6000", "--batch", "2048", "--debug-single-device", "--full", "--no-cpu-baseline", "--no-secondary"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, cwd=REPO, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["points_per_cloud"] == 6000 and sum(d["config"]["routing_histogram"]) == 6000
    assert d["parity"]["queries"] == 3000 and d["parity"]["one_minus_cos"]["p50"] <= 2e-5
    # the strong-scaling leg: ONE cloud's rows over the two ranks (dist.estimate_sharded), printed next to the weak figure
    assert d["strong"]["scaling"] == "strong" and d["strong"]["value"] > 0 and "ONE 6000-point cloud" in d["strong"]["workload"]
    assert d["dtype"] == "f16x8c" and d["parity"]["meets_north_star"] and d["gate_cascade"]["rechecked"] > 0


def test_bench_eight_ranks_debug_single_device(gpu_device):
    """World size 8 -- the north star's node -- with real kernels: eight ranks on ONE GPU (gloo), each running its row blocks of
    eight 4000-point clouds (500 rows of each: run_many's shared batches) and ONE all-gather per step; the line must carry
    n_gpus 8, the strong-scaling leg (one cloud over eight ranks: 500 rows per rank) and a parity object that meets the north
    star; every rank filters with the same gate margin."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(REPO, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "1",
           "--points", "4000", "--batch", "1024", "--debug-single-device", "--full", "--no-cpu-baseline", "--no-secondary"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 8 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["points_per_cloud"] == 4000 and sum(d["config"]["routing_histogram"]) == 4000
    assert d["strong"]["scaling"] == "strong" and d["strong"]["value"] > 0 and "ONE 4000-point cloud" in d["strong"]["workload"]
    assert d["parity"]["queries"] == 500 and d["parity"]["meets_north_star"]
    assert d["gate_cascade"]["tau_max_minus_min_over_ranks"] < 1e-4 * d["gate_cascade"]["tau"]
    assert d["gate_cascade"]["queries"] == 4000 and d["gate_cascade"]["rechecked"] > 0       # rank 0's 8 x 500 rows


def test_bench_strong_leg_at_one_gpu_equals_the_weak_figure(gpu_device):
    """--strong at N = 1: one cloud over one rank is the headline workload itself, so the two values must agree (VERDICT r02
    item 7; both legs time 2 steps of a 20k cloud, so a few per cent of noise is allowed)."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", "--points", "20000", "--strong",
           "--no-cpu-baseline", "--no-secondary", "--no-parity"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and abs(d["strong"]["value"] / d["value"] - 1) < 0.08, (d["value"], d["strong"]["value"])


def test_second_device_in_one_process(gpu_device):
    """The conv kernels opt in to > 64 KiB of dynamic LDS per DEVICE (hipFuncSetAttribute); a model built on a second
    device after the first must get its own opt-in.  Needs two GPUs; skipped on the 1-GPU pool."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth, weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.pipeline import NormalEstimator
    cfg = NestiConfig()
    W = weights.synthetic_weights(cfg)
    pts = synth.make_cloud("sphere", n=4000, seed=3)[0]
    q = np.arange(0, 4000, 9)
    a = NormalEstimator(cfg, W, dtype="f16", device="cuda:0", batch=256).estimate(pts, pidx=q)
    b = NormalEstimator(cfg, W, dtype="f16", device="cuda:1", batch=256).estimate(pts, pidx=q)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
