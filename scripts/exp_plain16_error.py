"""Error distribution of the plain 16-bit modes against the exact-fp32 mode of the same library (gate probs, all experts' normals)
on 1 024 queries of a 20k ellipsoid with a calibrated gate; NESTI_LIB picks the library (profiles/r07_numerics.txt):
    python scripts/exp_plain16_error.py"""
import os
import sys

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import synth, weights, _lib  # noqa: E402
from nesti_net_amd.calibrate import calibrate_gate  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.model import NestiNet  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

dev = torch.device("cuda:0")
print("lib", _lib.LIB_PATH)
cfg = NestiConfig()
pts, _ = synth.make_cloud("ellipsoid", n=20000, seed=1234)
Q = 1024
q = np.arange(3, len(pts), len(pts) // Q)[:Q]
cp = CloudPatches(pts, cfg, device=dev, pidx=q)
p, n = cp.build(0, Q)
W = calibrate_gate(cfg, weights.synthetic_weights(cfg), p, n, device=dev)
ref = NestiNet(cfg, W, dtype="f32", device=dev, max_batch=Q)
m32 = ref.mups(p, n)
pr32, _ = ref.gate(m32)
na32 = ref.experts(m32, None).double().cpu().numpy()
pr32 = pr32.double().cpu().numpy()
for dt in ("f16", "bf16"):
    net = NestiNet(cfg, W, dtype=dt, device=dev, max_batch=Q)
    m = net.mups(p, n)
    pr, _ = net.gate(m)
    na = net.experts(m, None).double().cpu().numpy()
    pe = np.abs(pr.double().cpu().numpy() - pr32).max(1)
    c = (na * na32).sum(-1) / np.linalg.norm(na, axis=-1) / np.linalg.norm(na32, axis=-1)
    e = (1 - c).ravel()
    print("%-5s gate |probs| err: median %.3e p90 %.3e p99 %.3e max %.3e | experts 1-cos: median %.3e p90 %.3e p99 %.3e max %.3e" % (
        dt, np.median(pe), np.quantile(pe, .9), np.quantile(pe, .99), pe.max(), np.median(e), np.quantile(e, .9), np.quantile(e, .99), e.max()))
