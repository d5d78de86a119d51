"""The fixture of the scale-selection tests (tests/test_select.py, tests/test_gpu_select.py): the tests' OWN restatement of the selection
step of ``nesti_pca_select_nbr`` on the CPU, written from its definition (include/nesti_hip.h, steps 3 and 4) in numpy, and a float64
plane fit over list prefixes for the property tests.

  score       from the float32 eigenvalues e0 <= e1 <= e2 as written: den = (float64(e0) + float64(e1)) + float64(e2),
              v_c = float64(e0) / den
  eligible    n_c >= 3 and radius_c > 0 (the float32 radius is 0 exactly where r2_c is: sqrt of a positive float64 never rounds to a
              float32 zero for distances of float32 points) and den > 0
  threshold   v_min = the smallest v_c of the eligible; thr = v_min + v_min * slack, a product then a sum, float64
  selection   the LARGEST eligible c with v_c <= thr; -1 and zeros where no candidate is eligible
  variation   float32(v_c), 0 where the candidate is not eligible

  plane fit   ``prefix_fits``: for every row and candidate the float64 moments over the first n_c = min(ladder[c], valid prefix) entries
              of the row's list and numpy.linalg.eigh of the covariance in units of r2_c, as tests/_knn_fixture.py's plane_lists states it
              (the same values up to float64 rounding: the moments come from running sums along the list), vectorised over the rows

Host only, deterministic; what a test shares is computed once and never changed."""
import numpy as np

import _knn_fixture as kx
import _pca_fixture as fx

DEFAULT_LADDER = (12, 16, 24, 32, 48, 64, 96, 128, 192, 256)
_cache = {}


def scores(eig_all, count_all, radius_all):
    """(v [M,L] float64, eligible [M,L] bool) of the float32 eigenvalues [M,L,3], the counts [M,L] and the float32 radii [M,L]."""
    e = np.asarray(eig_all, np.float32).astype(np.float64)
    den = (e[..., 0] + e[..., 1]) + e[..., 2]
    eligible = (np.asarray(count_all) >= 3) & (np.asarray(radius_all) > 0) & (den > 0)
    v = np.divide(e[..., 0], den, out=np.zeros_like(den), where=eligible)
    return v, eligible


def select(eig_all, count_all, radius_all, slack, normals_all=None):
    """The selection of every row -> dict of sel [M] int32, k [M] int32, radius [M] f32, eig [M,3] f32, variation_all [M,L] f32 and,
    where ``normals_all`` [M,L,3] is given, normals [M,3] f32."""
    eig_all = np.asarray(eig_all, np.float32)
    count_all, radius_all = np.asarray(count_all, np.int32), np.asarray(radius_all, np.float32)
    M, L = count_all.shape
    v, eligible = scores(eig_all, count_all, radius_all)
    slack = np.float64(slack)
    sel = np.full(M, -1, np.int32)
    with np.errstate(over="ignore"):
        for q in range(M):
            if not eligible[q].any():
                continue
            vmin = v[q][eligible[q]].min()
            thr = vmin + vmin * slack
            sel[q] = np.flatnonzero(eligible[q] & (v[q] <= thr)).max()
    has = sel >= 0
    rows, cols = np.flatnonzero(has), sel[has]
    out = {"sel": sel, "k": np.zeros(M, np.int32), "radius": np.zeros(M, np.float32), "eig": np.zeros((M, 3), np.float32),
           "variation_all": np.where(eligible, v, 0.0).astype(np.float32)}
    out["k"][has], out["radius"][has], out["eig"][has] = count_all[rows, cols], radius_all[rows, cols], eig_all[rows, cols]
    if normals_all is not None:
        out["normals"] = np.zeros((M, 3), np.float32)
        out["normals"][has] = np.asarray(normals_all, np.float32)[rows, cols]
    return out


def prefix_fits(pts, centres, nbr, ladder):
    """Float64 plane fits over the list prefixes of every row and candidate -> dict of normals_all [M,L,3] f32 (sign rule applied),
    eig_all [M,L,3] f32 (clamped at 0), count_all [M,L] int32, radius_all [M,L] f32.  n_c < 3 or r2_c == 0: zeros."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    centres = np.ascontiguousarray(centres, dtype=np.float32)
    nbr = np.asarray(nbr, np.int64)
    M, K = nbr.shape
    L = len(ladder)
    bad = (nbr < 0) | (nbr >= len(pts))
    valid = np.where(bad.any(1), bad.argmax(1), K)
    valid[~np.isfinite(centres).all(1)] = 0
    d = pts.astype(np.float64)[np.where(bad, 0, nbr)] - centres.astype(np.float64)[:, None, :]          # [M,K,3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    live = np.arange(K)[None, :] < valid[:, None]
    d = np.where(live[..., None], d, 0.0)
    d2 = np.where(live, d2, 0.0)
    s1 = np.cumsum(d, axis=1)                                                                              # [M,K,3]
    s2 = np.cumsum(d[:, :, :, None] * d[:, :, None, :], axis=1)                                            # [M,K,3,3]
    rmax = np.maximum.accumulate(d2, axis=1)
    out = {"normals_all": np.zeros((M, L, 3), np.float32), "eig_all": np.zeros((M, L, 3), np.float32),
           "count_all": np.zeros((M, L), np.int32), "radius_all": np.zeros((M, L), np.float32)}
    rows = np.arange(M)
    for c, k in enumerate(ladder):
        n = np.minimum(int(k), valid)
        out["count_all"][:, c] = n
        at = np.maximum(n, 1) - 1
        r2 = np.where(n > 0, rmax[rows, at], 0.0)
        out["radius_all"][:, c] = np.sqrt(r2).astype(np.float32)
        ok = (n >= 3) & (r2 > 0)
        if not ok.any():
            continue
        nn = n[ok].astype(np.float64)
        m = s1[rows[ok], at[ok]] / nn[:, None]
        C = (s2[rows[ok], at[ok]] / nn[:, None, None] - m[:, :, None] * m[:, None, :]) / r2[ok][:, None, None]
        C = 0.5 * (C + np.swapaxes(C, 1, 2))
        w, V = np.linalg.eigh(C)
        v0 = V[:, :, 0] / np.linalg.norm(V[:, :, 0], axis=1, keepdims=True)
        out["normals_all"][ok, c] = fx.sign_rule(v0.astype(np.float32))
        out["eig_all"][ok, c] = np.maximum(0.0, w).astype(np.float32)
    return out


def within_deg(normals, gt, deg=10.0):
    """The share, in per cent, of the rows whose unoriented angle to ``gt`` is within ``deg`` degrees (a zero normal is a miss)."""
    a, b = np.asarray(normals, np.float64), np.asarray(gt, np.float64)
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    cos = np.divide(np.abs((a * b).sum(1)), na * nb, out=np.zeros(len(a)), where=na * nb > 0)
    return 100.0 * float((cos >= np.cos(np.radians(deg))).mean())


# the six clouds of the accuracy conditions: (shape, noise as a fraction of the bounding-box diagonal)
TABLE_CLOUDS = (("box", 0.0), ("box", 0.002), ("box", 0.006), ("torus", 0.0), ("torus", 0.002), ("torus", 0.006))


def table_cloud(shape, noise, n=20000, seed=3, every=8):
    """``synth.make_cloud(shape, n, seed, noise)``, every ``every``-th row as a centre against the FULL cloud, their exact sorted lists
    at K = the top of ``DEFAULT_LADDER`` and the float64 fits of every candidate; computed once."""
    key = (shape, noise, n, seed, every)
    if key not in _cache:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import synth
        pts, gt = synth.make_cloud(shape, n=n, seed=seed, noise=noise)
        rows = np.arange(0, n, every)
        nbr = kx.search(pts, pts[rows], DEFAULT_LADDER[-1])[0]
        _cache[key] = {"pts": pts, "gt": gt[rows], "rows": rows, "nbr": nbr, "fits": prefix_fits(pts, pts[rows], nbr, DEFAULT_LADDER)}
    return _cache[key]
