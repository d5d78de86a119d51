"""The fixture of the k-nearest-neighbour tests (tests/test_knn.py, tests/test_gpu_knn.py): the tests' OWN restatement of the search and
of the fits over neighbour lists on the CPU, written from their definition (DESIGN.md 2 "k-nearest neighbourhoods", include/nesti_hip.h)
in numpy.

  search      brute force over ALL N points: d = float64(p) - float64(c), d2 = (dx dx + dy dy) + dz dz (numpy rounds each of the five
              operations on its own), order = np.lexsort((j, d2)), the first K.  -1 / +inf beyond min(K, N); a centre with a non-finite
              coordinate has count 0
  lists       the valid prefix of a row ends at its first entry outside [0, N); scale s is its first n_s = min(k_s, prefix) entries;
              r2_s = max d2 of them; a non-finite centre has an empty prefix
  plane fit   tests/_pca_fixture.py's moments and eigen-decomposition over the prefix with r2_s for r^2; n_s < 3 or r2_s == 0: sentinel
  quadric     tests/_quadric_fixture.py's frame, moments, normal_matrix, cholesky_solve and curvatures over the prefix with
              r = sqrt(r2_s); the plane normal n0 is an INPUT (the GPU's own plane_out), as in tests/test_gpu_quadric.py
  stop rule   ``emulate_walk``: the search kernel's shell walk at the level of sets -- the points of the cells within Chebyshev distance R
              of the centre's clamped cell -- with its stop rule and margin in the kernel's own fp64 operations, over a grid header of
              tests/_grid_fixture.py.  What it returns when it stops is compared with the brute force (tests/test_knn.py)

Host only, deterministic; what a test shares is computed once and never changed."""
import numpy as np

import _pca_fixture as fx
import _quadric_fixture as qx

KNN_MAX_K = 256
_cache = {}


def d2_all(p64, c):
    """(dx dx + dy dy) + dz dz of every cloud point to the float64 centre c, each operation rounded on its own."""
    d = p64 - c
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def search(pts, centres, K):
    """Brute-force k-NN of float32 ``centres`` [M,3] over the float32 cloud -> (idx [M,K] int32, d2 [M,K] float64, count [M] int32)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    centres = np.ascontiguousarray(centres, dtype=np.float32)
    p64 = pts.astype(np.float64)
    N, M = len(pts), len(centres)
    idx = np.full((M, K), -1, np.int32)
    d2o = np.full((M, K), np.inf, np.float64)
    count = np.zeros(M, np.int32)
    n = min(K, N)
    for q in range(M):
        c = centres[q].astype(np.float64)
        if not np.isfinite(c).all():
            continue
        d2 = d2_all(p64, c)
        if N > n:                                     # only the points up to the n-th distance can be among the first n (ties included)
            kth = np.partition(d2, n - 1)[n - 1]
            cand = np.flatnonzero(d2 <= kth)
        else:
            cand = np.arange(N)
        order = cand[np.lexsort((cand, d2[cand]))][:n]
        idx[q, :n], d2o[q, :n], count[q] = order, d2[order], n
    return idx, d2o, count


def searched(key, pts, centres, K):
    """``search`` computed once per ``key``; a smaller K is a prefix of it (the order is total)."""
    if key not in _cache:
        _cache[key] = search(pts, centres, K)
    return _cache[key]


def prefixes(N, centre, row, ks):
    """n_s of one list row: min(k_s, valid prefix); 0 for a non-finite centre."""
    row = np.asarray(row, np.int64)
    bad = np.flatnonzero((row < 0) | (row >= N))
    valid = int(bad[0]) if len(bad) else len(row)
    if not np.isfinite(centre).all():
        valid = 0
    return [min(int(k), valid) for k in ks]


def plane_lists(pts, centres, nbr, ks):
    """Plane fit over list prefixes -> the dict of ``_pca_fixture.restate`` (normals, eig, n_ball, w, C) plus radius [M,S] float32 and
    r2 [M,S] float64."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    centres = np.ascontiguousarray(centres, dtype=np.float32)
    p64 = pts.astype(np.float64)
    M, S = len(centres), len(ks)
    out = {"normals": np.zeros((M, S, 3), np.float32), "eig": np.zeros((M, S, 3), np.float32), "n_ball": np.zeros((M, S), np.int32),
           "w": np.zeros((M, S, 3), np.float64), "C": np.zeros((M, S, 3, 3), np.float64), "radius": np.zeros((M, S), np.float32),
           "r2": np.zeros((M, S), np.float64)}
    for q in range(M):
        c = centres[q].astype(np.float64)
        for s, n in enumerate(prefixes(len(pts), c, nbr[q], ks)):
            out["n_ball"][q, s] = n
            if n == 0:
                continue
            ds = p64[np.asarray(nbr[q, :n], np.int64)] - c
            d2 = (ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]
            r2 = float(d2.max())
            out["r2"][q, s], out["radius"][q, s] = r2, np.float32(np.sqrt(r2))
            if n < 3 or r2 == 0.0:
                continue
            m = ds.sum(0) / n
            C = ((ds[:, :, None] * ds[:, None, :]).sum(0) / n - m[:, None] * m[None, :]) / r2
            C = 0.5 * (C + C.T)
            w, V = np.linalg.eigh(C)
            v = V[:, 0] / np.linalg.norm(V[:, 0])
            out["normals"][q, s] = fx.sign_rule(v.astype(np.float32))
            out["eig"][q, s] = np.maximum(0.0, w).astype(np.float32)
            out["w"][q, s], out["C"][q, s] = w, C
    return out


def quadric_lists(pts, centres, nbr, ks, n0):
    """Quadric fit over list prefixes with the plane normals ``n0`` [M,S,3] float32 -> the dict of ``_quadric_fixture.restate``
    (normals, curv, n_ball, a, nu, k, kappa, ok) plus r [M,S] float64 = sqrt(r2_s)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    centres = np.ascontiguousarray(centres, dtype=np.float32)
    n0 = np.asarray(n0, np.float32)
    p64 = pts.astype(np.float64)
    M, S = len(centres), len(ks)
    out = {"normals": np.zeros((M, S, 3), np.float32), "curv": np.zeros((M, S, 2), np.float32), "n_ball": np.zeros((M, S), np.int32),
           "a": np.zeros((M, S, 6)), "nu": np.zeros((M, S, 3)), "k": np.zeros((M, S, 2)), "kappa": np.full((M, S), np.inf),
           "ok": np.zeros((M, S), bool), "r": np.zeros((M, S))}
    for q in range(M):
        c = centres[q].astype(np.float64)
        for s, n in enumerate(prefixes(len(pts), c, nbr[q], ks)):
            out["n_ball"][q, s] = n
            if n == 0:
                continue
            ds = p64[np.asarray(nbr[q, :n], np.int64)] - c
            d2 = (ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]
            r = float(np.sqrt(d2.max()))
            out["r"][q, s] = r
            nrm = n0[q, s].astype(np.float64)
            if n < 6 or not nrm.any() or r == 0.0:
                continue
            t1, t2 = qx.frame(nrm)
            N, b = qx.normal_matrix(qx.moments((ds @ t1) / r, (ds @ t2) / r, (ds @ nrm) / r))
            with np.errstate(all="ignore"):
                out["kappa"][q, s] = np.linalg.cond(N)
            a = qx.cholesky_solve(N, b)
            if a is None:
                continue
            nu = nrm - a[1] * t1 - a[2] * t2
            nu = nu / np.sqrt(nu @ nu)
            k = qx.curvatures(a) / r
            out["ok"][q, s] = True
            out["a"][q, s], out["nu"][q, s], out["k"][q, s] = a, nu, k
            out["normals"][q, s] = nu.astype(np.float32) + np.float32(0.0)
            out["curv"][q, s] = k.astype(np.float32)
    return out


def emulate_walk(pts, centres, K, h):
    """The K nearest of ``centres`` as csrc/knn.hip's walk finds them over the grid header ``h`` (``_grid_fixture.header``): visit the
    cells of the block [c - R, c + R] round the centre's clamped cell, R = 0, 1, ...; after each shell stop if every face of the block
    lies at or past the grid's border, or if K pairs are held and the K-th d2 is STRICTLY below the square of the proven distance --
    the nearest face with grid beyond it, less 2^-50 (|minv| + |m / inv_cell| + |c|), clamped at 0 and scaled by 1 - 2^-50.
    -> (idx [M,K] int32, d2 [M,K] float64, the largest R reached)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    p64 = pts.astype(np.float64)
    minv, inv, dims = np.array(h["minv"], np.float64), float(h["inv_cell"]), np.array(h["dims"])
    cell = np.stack([np.minimum(dims[a] - 1, np.maximum(0.0, np.floor((p64[:, a] - minv[a]) * inv))).astype(np.int64) for a in range(3)], 1)
    idx = np.full((len(centres), K), -1, np.int32)
    d2o = np.full((len(centres), K), np.inf)
    deepest = 0
    for q, cf in enumerate(np.asarray(centres, np.float32)):
        c = cf.astype(np.float64)
        if not np.isfinite(c).all():
            continue
        ic = np.array([int(min(dims[a] - 1, max(0.0, np.floor((c[a] - minv[a]) * inv)))) for a in range(3)])
        ring = np.abs(cell - ic).max(1)
        d2 = d2_all(p64, c)
        R = 0
        while True:
            seen = np.flatnonzero(ring <= R)
            order = seen[np.lexsort((seen, d2[seen]))][:K]
            proven = np.inf
            for a in range(3):
                for m, sign in ((ic[a] - R, 1.0), (ic[a] + R + 1, -1.0)):
                    if (sign > 0 and m > 0) or (sign < 0 and m < dims[a]):
                        off = float(m) / inv
                        face = minv[a] + off
                        dist = (c[a] - face) if sign > 0 else (face - c[a])
                        proven = min(proven, dist - 2.0 ** -50 * ((abs(minv[a]) + abs(off)) + abs(c[a])))
            if proven == np.inf:
                break
            proven = max(proven, 0.0) * (1.0 - 2.0 ** -50)
            if len(order) >= K and d2[order[K - 1]] < proven * proven:
                break
            R += 1
        deepest = max(deepest, R)
        idx[q, :len(order)], d2o[q, :len(order)] = order, d2[order]
    return idx, d2o, deepest
