"""What the scale-selected plane fit (csrc/select.hip) buys and costs, in one process on one box.

ACCURACY: on ``synth.make_cloud(shape, n=20000, seed=3, noise=...)`` for the box and the torus at noise 0, 0.002 and 0.006 of the
bounding-box diagonal, all rows, the default ladder: the share of rows within 10 degrees of the analytic normal and the RMS angle for
every fixed neighbour count of the ladder (the per-candidate outputs of the same call) and for the selection at ``slack`` 0 and 0.5,
with the histogram of the chosen counts.  NEAR-EDGE rows of the box -- closer to a box edge than the radius of their 100 nearest
neighbours -- and the other rows are reported separately; the torus has no edges.
TIME: on the bench's 100k cloud (cloud 0 of bench.py: the noise-free ellipsoid, seed 1234), all rows, the default ladder, over lists
searched once at K = 256: one call of ``nesti_pca_select_nbr`` against what a caller had to do before it -- three calls of
``nesti_pca_normals_nbr`` over the same lists (4 + 4 + 2 counts), the scores and the choice in torch (float64 scores from the float32
eigenvalues, eligibility, the arg-min with ties to the larger count, the gathers of the selected rows).  A warm-up each, then ``--reps``
repetitions, the two alternating, each repetition ``--calls`` calls between two stream events; the outputs of the two are compared on
the bits.  Recorded, not gated.  Writes one JSON object (default: profiles/select_check.json).

    python scripts/select_check.py [--points 100000] [--reps 9] [--calls 100] [--out profiles/select_check.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import select, synth  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

LADDER = select.DEFAULT_LADDER
SLACKS = (0.0, 0.5)
CLOUDS = (("box", 0.0), ("box", 0.002), ("box", 0.006), ("torus", 0.0), ("torus", 0.002), ("torus", 0.006))


def angles_deg(normals, gt):
    a, b = normals.astype(np.float64), gt.astype(np.float64)
    cos = np.abs((a * b).sum(1)) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
    return np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))


def summary(normals, gt, rows):
    """Share within 10 degrees and RMS angle over ``rows`` (a mask); a sentinel row counts as 90 degrees."""
    if not rows.any():
        return {"rows": 0}
    ang = np.where((normals[rows] != 0).any(axis=1), angles_deg(normals[rows], gt[rows]), 90.0)
    return {"rows": int(rows.sum()), "within_10_deg": float((ang <= 10.0).mean()), "rms_angle_deg": float(np.sqrt(np.mean(ang ** 2)))}


def accuracy(shape, noise, dev, n=20000):
    pts, gt = synth.make_cloud(shape, n=n, seed=3, noise=noise)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    nbr = cp.knn(0, n, LADDER[-1])[0]
    if shape == "box":
        radius100 = cp.pca_knn(0, n, (100,), nbr=nbr)[2].cpu().numpy()[:, 0].astype(np.float64)
        edge = np.sort(np.clip(1.0 - np.abs(pts.astype(np.float64)), 0.0, None), axis=1)[:, 1]
        near = edge < radius100
    else:
        near = np.zeros(n, bool)
    every = np.ones(n, bool)
    rec = {"shape": shape, "points": n, "seed": 3, "noise_x_bbdiag": noise, "ladder": list(LADDER), "near_edge_rows": int(near.sum())}
    for slack in SLACKS:
        out = [t.cpu().numpy() for t in cp.pca_select(0, n, LADDER, slack, nbr=nbr)]
        normals, sel, normals_all = out[0], out[2], out[6]
        if "fixed" not in rec:                              # the candidates do not depend on the slack
            rec["fixed"] = [{"k": k, "all": summary(normals_all[:, c], gt, every), "near_edge": summary(normals_all[:, c], gt, near),
                             "other": summary(normals_all[:, c], gt, ~near)} for c, k in enumerate(LADDER)]
        rec["selected_slack_%g" % slack] = {"all": summary(normals, gt, every), "near_edge": summary(normals, gt, near),
                                            "other": summary(normals, gt, ~near), "rows_without_a_fit": int((sel < 0).sum()),
                                            "chosen": dict(zip(map(str, LADDER), np.bincount(sel[sel >= 0], minlength=len(LADDER)).tolist()))}
    shares = [f["all"]["within_10_deg"] for f in rec["fixed"]]
    rec["best_fixed"] = {"k": LADDER[int(np.argmax(shares))], "within_10_deg": max(shares)}
    rec["worst_fixed"] = {"k": LADDER[int(np.argmin(shares))], "within_10_deg": min(shares)}
    return rec


def by_hand(cp, M, nbr):
    """The selection at slack 0 from the entries there were before: three list fits and the choice in torch -> (normals, eig, sel, k,
    radius) as ``pca_select`` returns them."""
    parts = [cp.pca_knn(0, M, LADDER[g:g + 4], nbr=nbr) for g in range(0, len(LADDER), 4)]
    normals_all, eig_all, radius_all, count_all = (torch.cat([p[i] for p in parts], dim=1) for i in range(4))
    e = eig_all.double()
    den = (e[..., 0] + e[..., 1]) + e[..., 2]
    ok = (count_all >= 3) & (radius_all > 0) & (den > 0)
    v = torch.where(ok, e[..., 0] / torch.where(ok, den, torch.ones_like(den)), torch.full_like(den, float("inf")))
    vmin = v.min(dim=1, keepdim=True).values
    index = torch.arange(len(LADDER), device=v.device).expand_as(v)
    sel = torch.where(ok & (v <= vmin), index, torch.full_like(index, -1)).max(dim=1).values
    has = sel >= 0
    at = sel.clamp(min=0)
    rows = torch.arange(M, device=v.device)
    zero3 = torch.zeros((), dtype=torch.float32, device=v.device)
    return (torch.where(has[:, None], normals_all[rows, at], zero3), torch.where(has[:, None], eig_all[rows, at], zero3), sel.int(),
            torch.where(has, count_all[rows, at], torch.zeros_like(count_all[:, 0])), torch.where(has, radius_all[rows, at], zero3))


def timing(points, reps, calls, dev):
    pts, _ = synth.make_cloud("ellipsoid", n=points, seed=1234)
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    M = cp.patch_count
    nbr = cp.knn(0, M, LADDER[-1])[0]
    forms = {"select": lambda: cp.pca_select(0, M, LADDER, 0.0, nbr=nbr)[:5], "by_hand": lambda: by_hand(cp, M, nbr)}
    outs = {name: f() for name, f in forms.items()}         # warm-up: the code objects and the allocator
    torch.cuda.synchronize(dev)
    same = all(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(outs["select"], outs["by_hand"]))
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, f in forms.items():                       # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / calls)
    med = {name: float(np.median(t)) for name, t in ms.items()}
    return {"cloud": "ellipsoid, %d points, seed 1234, no noise" % points, "rows": M, "list_K": LADDER[-1], "ladder": list(LADDER),
            "slack": 0.0, "reps": reps, "calls_per_rep": calls, "what": "milliseconds per call between stream events, the search not included",
            "select_ms": ms["select"], "by_hand_ms": ms["by_hand"], "select_median_ms": med["select"], "by_hand_median_ms": med["by_hand"],
            "by_hand_over_select": med["by_hand"] / med["select"], "select_rows_per_s": M / (med["select"] * 1e-3),
            "by_hand_is": "3 calls of nesti_pca_normals_nbr (4 + 4 + 2 counts) + scores, arg-min and gathers in torch", "same_bytes": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "select_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "accuracy": [accuracy(shape, noise, dev) for shape, noise in CLOUDS],
           "time": timing(args.points, args.reps, args.calls, dev)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
