"""What the model-free fits measure against their restatements at every number of scales, on one MI355X: the inputs of
tests/_fit_scales_fixture.py -- four, two (out of order), one and four (one radius repeated) radii on the 4 000-point ellipsoid and the
12 000-point clean torus, neighbour counts (8, 16, 64, 256), (16, 200) and (24,), and the Hough estimator at (3, 9, 17, 40) and (17, 40)
on the 300-point box -- through ``CloudPatches.pca`` / ``quadric`` / ``pca_knn`` / ``quadric_knn`` / ``hough_knn``.  Per kernel family
and per S: the largest sin / bound, residual / bound, eigenvalue error / bound and curvature error / bound, the ill-conditioned share
and the live counts, in the notation of tests/test_gpu_pca.py and tests/test_gpu_quadric.py.  Recorded, not gated: the assertions are
the bounds in tests/test_gpu_fit_scales.py, which come from the arithmetic; ``checks_pass`` says whether those same ``check`` functions
passed on this run's outputs.  Writes one JSON object (default: profiles/fit_scales_check.json).

    python scripts/fit_scales_check.py [--out profiles/fit_scales_check.json]"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import nesti_net_amd  # noqa: E402,F401
from nesti_net_amd import hough  # noqa: E402
from nesti_net_amd.config import NestiConfig  # noqa: E402
from nesti_net_amd.provider import CloudPatches  # noqa: E402

import _fit_scales_fixture as sx  # noqa: E402
import _hough_fixture as hx  # noqa: E402
import _quadric_fixture as qx  # noqa: E402
from test_gpu_knn import _quadric_check as quadric_list_check  # noqa: E402
from test_gpu_pca import check as plane_check  # noqa: E402
from test_gpu_quadric import check as quadric_check  # noqa: E402

EPS = 2.0 ** -53


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def passes(check, *args, **kw):
    """Whether a ``check`` function of the tests passes, and the line it prints."""
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            check(*args, **kw)
        return True, buf.getvalue().strip()
    except AssertionError as e:
        return False, (buf.getvalue().strip() + " FAILED: %s" % e).strip()


def plane_figures(got, ref):
    """Per scale, the figures of tests/test_gpu_pca.py's ``check`` on (normals, eig, n) against a plane restatement."""
    normals, eig, n_ball = got
    out = []
    for s in range(n_ball.shape[1]):
        live = ref["n_ball"][:, s] >= 3
        row = {"pairs": int(live.size), "live": int(live.sum()), "counts_equal": bool(np.array_equal(n_ball[:, s], ref["n_ball"][:, s])),
               "sentinel_bytes_zero": bool(not normals[:, s][~live].view(np.uint32).any() and not eig[:, s][~live].view(np.uint32).any())}
        if live.any():
            n = ref["n_ball"][:, s][live].astype(np.float64)
            w, C = ref["w"][:, s][live], ref["C"][:, s][live]
            g, r = normals[:, s][live].astype(np.float64), ref["normals"][:, s][live].astype(np.float64)
            with np.errstate(divide="ignore"):
                bound = 2.0 ** -22 + 16 * n * EPS / (w[:, 1] - w[:, 0])
            ill = ~(bound <= 1e-3)
            length = np.linalg.norm(g, axis=1)
            sin = np.linalg.norm(np.cross(g, r), axis=1) / (length * np.linalg.norm(r, axis=1))
            rho = np.einsum("ni,nij,nj->n", g, C, g) / (length * length)
            ge = eig[:, s][live].astype(np.float64)
            row.update({"ill_conditioned": int(ill.sum()), "smallest_gap": float((w[:, 1] - w[:, 0]).min()),
                        "sin_over_bound": float((sin[~ill] / bound[~ill]).max()) if (~ill).any() else 0.0,
                        "residual_over_bound": float(((rho - w[:, 0]) / (2.0 ** -40 * w[:, 2] + 16 * n * EPS)).max()),
                        "length_error": float(np.abs(length - 1).max()),
                        "eigenvalue_error_over_bound": float((np.abs(ge - w) / (2.0 ** -23 * w + 8 * n[:, None] * EPS)).max())})
        out.append(row)
    return out


def quadric_figures(got, ref, r):
    """Per scale, the figures of tests/test_gpu_quadric.py's ``check`` on (normals, curv, plane, n) against a quadric restatement;
    ``r`` [M,S]: the radius of every pair."""
    normals, curv, plane, n_ball = got
    B = qx.bound_B(ref)
    out = []
    for s in range(n_ball.shape[1]):
        short = n_ball[:, s] < 6
        with np.errstate(invalid="ignore"):
            well = ~short & (B[:, s] <= 1e-6)
        ill = ~short & ~well
        live = (normals[:, s] != 0).any(axis=-1)
        row = {"pairs": int(short.size), "n_ge_6": int((~short).sum()), "live": int(live.sum()), "ill_conditioned": int(ill.sum()),
               "ill_share": float(ill.sum() / max(1, (~short).sum())), "counts_equal": bool(np.array_equal(n_ball[:, s], ref["n_ball"][:, s])),
               "failed_fit_bytes_zero": bool(not normals[:, s][~live].view(np.uint32).any() and not curv[:, s][~live].view(np.uint32).any())}
        if well.any():
            g, rn, a, b = normals[:, s][well].astype(np.float64), ref["nu"][:, s][well], ref["a"][:, s][well], B[:, s][well]
            na, length = np.linalg.norm(a, axis=1), np.linalg.norm(g, axis=1)
            sin = np.linalg.norm(np.cross(g, rn), axis=1) / np.where(length > 0, length, 1.0)
            k, kr, rr = curv[:, s][well].astype(np.float64), ref["k"][:, s][well], r[:, s][well]
            k_err = rr[:, None] * np.abs(k - kr)
            k_bound = 2.0 ** -23 * rr[:, None] * np.abs(kr) + (8 * (1 + na) * b)[:, None]
            row.update({"largest_B": float(b.max()), "largest_kappa": float(ref["kappa"][:, s][well].max()),
                        "length_error": float(np.abs(length - 1).max()), "sin_over_bound": float((sin / (2.0 ** -22 + 2 * b)).max()),
                        "curvature_error_over_bound": float((k_err / k_bound).max())})
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit_scales_check.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "rows_per_cloud": 250, "balls": {}, "lists": {}, "hough": {}}
    ok = []

    for key in sx.SCALE_SETS:
        c = sx.scale_set(key)
        cp = CloudPatches(c["pts"], c["cfg"], device=dev, pidx=c["rows"])
        plane, quad = _np(cp.pca(0, cp.patch_count)), _np(cp.quadric(0, cp.patch_count))
        pref, qref = sx.plane_balls(key), sx.quadric_balls(key, quad[2])
        r = np.broadcast_to(np.asarray(c["r_abs"], np.float64)[None, :], quad[3].shape)
        p_ok, p_line = passes(plane_check, plane, pref, key + " plane", allow_excluded=None)
        q_ok, q_line = passes(quadric_check, quad, qref, c["r_abs"], key + " quadric", ill_share_cap=0.01)
        ok += [p_ok, q_ok]
        res["balls"][key] = {"cloud": c["cloud"], "S": len(c["radii"]), "radii_x_bbdiag": c["radii"], "r_abs": c["r_abs"],
                             "pca_kernel": plane_figures(plane, pref), "quadric_kernel": quadric_figures(quad, qref, r),
                             "plane_out_is_pca_normals": bool(np.array_equal(quad[2].view(np.uint32), plane[0].view(np.uint32))),
                             "checks_pass": {"plane": p_ok, "quadric": q_ok}, "check_lines": [p_line, q_line]}
        print(p_line)
        print(q_line)

    for name in sx.CLOUDS:
        c = sx.cloud(name)
        cp = CloudPatches(c["pts"], NestiConfig(), device=dev, pidx=c["rows"], radius_grid=False)
        idx = cp.knn(0, cp.patch_count, 256)[0]
        search_exact = bool(np.array_equal(idx.cpu().numpy(), sx.lists(name)[0]))
        for ks in sx.KS_SETS:
            nbr = idx[:, :ks[-1]].contiguous()
            pn, pe, pr, pc = _np(cp.pca_knn(0, cp.patch_count, ks, nbr=nbr))
            qn, qc, qp, qr, qcount = _np(cp.quadric_knn(0, cp.patch_count, ks, nbr=nbr))
            pref, qref = sx.plane_lists(name, ks), sx.quadric_lists(name, ks, qp)
            label = "%s knn %s" % (name, list(ks))
            p_ok, p_line = passes(plane_check, (pn, pe, pc), pref, label + " plane", allow_excluded=None)
            q_ok, q_line = passes(quadric_list_check, (qn, qc, qp, qcount), qref, label + " quadric", cap_scales=range(len(ks)))
            ok += [p_ok, q_ok]
            res["lists"][label] = {"cloud": name, "S": len(ks), "ks": list(ks), "search_equals_brute_force": search_exact,
                                   "pca_nbr_kernel": plane_figures((pn, pe, pc), pref),
                                   "quadric_nbr_kernel": quadric_figures((qn, qc, qp, qcount), qref, qref["r"]),
                                   "radius_bits_equal": bool(np.array_equal(pr.view(np.uint32), pref["radius"].view(np.uint32))),
                                   "plane_out_is_pca_normals": bool(np.array_equal(qp.view(np.uint32), pn.view(np.uint32))),
                                   "checks_pass": {"plane": p_ok, "quadric": q_ok}, "check_lines": [p_line, q_line]}
            print(p_line)
            print(q_line)

    pts = sx.box()
    cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
    nbr = cp.knn(0, len(pts), sx.HOUGH_K)[0]
    nbr_h = nbr.cpu().numpy()
    rot = hough.rotation_table(sx.HOUGH_R)
    for ks in sx.HOUGH_KS_SETS:
        for T in sx.HOUGH_T:
            got = _np(cp.hough_knn(0, len(pts), ks, T, sx.HOUGH_B, sx.HOUGH_R, sx.HOUGH_SEED, nbr=nbr))
            ref = hx.restate(pts, pts, nbr_h, ks, T, sx.HOUGH_B, sx.HOUGH_R, rot, sx.HOUGH_SEED)
            same = {k: bool(g.dtype == ref[k].dtype and np.array_equal(g.view(np.uint8), ref[k].view(np.uint8)))
                    for k, g in zip(("normals", "conf", "votes", "radius", "count"), got)}
            ok.append(all(same.values()))
            res["hough"]["ks %s, T %d" % (list(ks), T)] = {
                "S": len(ks), "rows": len(pts), "bytes_equal_the_restatement": same,
                "rows_with_a_winner_per_scale": (got[2][..., 0] > 0).sum(0).tolist(),
                "mean_confidence_per_scale": [float(x) for x in got[1].mean(0)]}
            print("hough ks %s, T %d: %s" % (list(ks), T, same))
    res["all_checks_pass"] = bool(all(ok))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
