"""The fixture of the quadric-fit tests (tests/test_quadric.py, tests/test_gpu_quadric.py) and the tests' OWN restatement of steps 2 - 8
of the estimator on the CPU, written from its definition (DESIGN.md 2 "Quadric fit", include/nesti_hip.h) in numpy.  Step 1, the plane
normal n0, is an INPUT: the GPU tests pass the library's own ``plane_out``, so the comparison is about the fit and not about the plane
fit's conditioning, which tests/test_gpu_pca.py covers.

  ball(c, s)   as in tests/_pca_fixture.py: float64 d2 = (dx dx + dy dy) + dz dz <= r r, the full ball
  frame        j = argmin |n0_j| (first on ties), t1 = (n0 x e_j) / |n0 x e_j|, t2 = n0 x t1
  coordinates  (u, v, h) = (t . d) / r for t = t1, t2, n0; phi = (1, u, v, u^2, u v, v^2)
  solve        N = sum phi phi^T, b = sum h phi, Cholesky without pivoting; the fit fails if n < 6, n0 = 0 or a pivot
               s_j = N_jj - sum_k L_jk^2 is not > 2^-44 N_jj
  normal       nu = n0 - a1 t1 - a2 t2, normalised, rounded to float32, zeros +0
  curvatures   eigenvalues of P Hh P / w (g = (a1, a2), w = sqrt(1 + g.g), Hh = [[2 a3, a4], [a4, 2 a5]], P = I - g g^T / (w (1 + w))),
               divided by r; float32 (k_max, k_min)
  failed fit   nu = 0 0 0, k = 0 0; the count stays

Besides what the library returns, ``restate`` keeps in float64 what the tests' bounds are written in: a, nu, k, the 2-norm condition
number of N, and ``ok`` (every pivot passed)."""
import numpy as np

import _pca_fixture as fx

_cache = {}
EPS = 2.0 ** -53
PIVOT_TOL = 2.0 ** -44
TORUS_CLEAN_RADII = [0.03, 0.06, 0.1]


def frame(n0):
    """(t1, t2) of a float64 plane normal."""
    j = int(np.argmin(np.abs(n0)))                  # numpy returns the first of equal minima
    e = np.zeros(3)
    e[j] = 1.0
    c = np.cross(n0, e)
    t1 = c / np.sqrt(c @ c)
    return t1, np.cross(n0, t1)


def cholesky_solve(N, b):
    """a with N a = b by Cholesky without pivoting, or None where a pivot is not > 2^-44 N_jj."""
    K = len(b)
    L = np.zeros((K, K))
    for j in range(K):
        s = N[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not s > PIVOT_TOL * N[j, j]:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, K):
            L[i, j] = (N[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(K)
    for i in range(K):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    a = np.zeros(K)
    for i in range(K - 1, -1, -1):
        a[i] = (y[i] - L[i + 1:, i] @ a[i + 1:]) / L[i, i]
    return a


def curvatures(a):
    """(k_max, k_min) of the height function a . phi at the origin, in the units of the fit."""
    g = np.array([a[1], a[2]])
    w = np.sqrt(1.0 + g @ g)
    Hh = np.array([[2 * a[3], a[4]], [a[4], 2 * a[5]]])
    P = np.eye(2) - np.outer(g, g) / (w * (1.0 + w))
    Sm = P @ Hh @ P / w
    mean, dif, q = (Sm[0, 0] + Sm[1, 1]) / 2, (Sm[0, 0] - Sm[1, 1]) / 2, (Sm[0, 1] + Sm[1, 0]) / 2
    rad = np.sqrt(dif * dif + q * q)
    return np.array([mean + rad, mean - rad])


def monomials(u, v):
    return np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], 1)


def restate(pts, positions, r_abs, n0, tree=None):
    """Quadric fit at ``positions`` [M,3] (float32) over the cloud ``pts`` with the plane normals ``n0`` [M,S,3] (float32) -> dict of
    normals [M,S,3] f32, curv [M,S,2] f32, n_ball [M,S] int32, and in float64 a [M,S,6], nu [M,S,3], k [M,S,2] (absolute units),
    kappa [M,S] (cond_2 of N; inf where n < 6 or n0 = 0), ok [M,S] bool."""
    from scipy import spatial
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n0 = np.asarray(n0, np.float32)
    p64 = pts.astype(np.float64)
    tree = tree or spatial.cKDTree(p64, 10)
    M, S = len(positions), len(r_abs)
    out = {"normals": np.zeros((M, S, 3), np.float32), "curv": np.zeros((M, S, 2), np.float32), "n_ball": np.zeros((M, S), np.int32),
           "a": np.zeros((M, S, 6)), "nu": np.zeros((M, S, 3)), "k": np.zeros((M, S, 2)), "kappa": np.full((M, S), np.inf),
           "ok": np.zeros((M, S), bool)}
    r_big = float(max(r_abs))
    for q in range(M):
        c = positions[q].astype(np.float64)
        if not np.isfinite(c).all():
            continue
        cand = np.asarray(tree.query_ball_point(c, r_big * (1.0 + 1e-9) + 1e-300), np.int64)
        d = p64[cand] - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        for s, r in enumerate(r_abs):
            r = float(r)
            ds = d[d2 <= r * r]
            n = len(ds)
            out["n_ball"][q, s] = n
            nrm = n0[q, s].astype(np.float64)
            if n < 6 or not nrm.any():
                continue
            t1, t2 = frame(nrm)
            u, v, h = (ds @ t1) / r, (ds @ t2) / r, (ds @ nrm) / r
            Phi = monomials(u, v)
            N, b = Phi.T @ Phi, Phi.T @ h
            with np.errstate(all="ignore"):
                out["kappa"][q, s] = np.linalg.cond(N)
            a = cholesky_solve(N, b)
            if a is None:
                continue
            nu = nrm - a[1] * t1 - a[2] * t2
            nu = nu / np.sqrt(nu @ nu)
            k = curvatures(a) / r
            out["ok"][q, s] = True
            out["a"][q, s], out["nu"][q, s], out["k"][q, s] = a, nu, k
            out["normals"][q, s] = nu.astype(np.float32) + np.float32(0.0)
            out["curv"][q, s] = k.astype(np.float32)
    return out


def bound_B(ref):
    """B = 16 n eps kappa_2(N) (||a||_2 + 1) per (row, scale): the first-order bound on ||delta a|| for normal equations whose every
    entry is a length-n float64 sum of terms of magnitude <= 1.  inf where there is no system."""
    with np.errstate(all="ignore"):
        return 16.0 * ref["n_ball"] * EPS * ref["kappa"] * (np.linalg.norm(ref["a"], axis=-1) + 1.0)


def moments(u, v, h):
    """The 21 moments of step 4 from samples (u, v, h), float64."""
    u, v, h = (np.asarray(x, np.float64) for x in (u, v, h))
    one, u2, v2 = np.ones_like(u), u * u, v * v
    mono = [one, u, v, u2, u * v, v2, u2 * u, u2 * v, u * v2, v2 * v, u2 * u2, (u2 * u) * v, u2 * v2, u * (v2 * v), v2 * v2]
    m = [x.sum() for x in mono] + [(h * x).sum() for x in mono[:6]]
    return np.array(m, np.float64)


PU, PV = (0, 1, 0, 2, 1, 0), (0, 0, 1, 0, 1, 2)


def normal_matrix(m):
    """(N, b) read from 21 moments."""
    idx = lambda p, q: (p + q) * (p + q + 1) // 2 + q
    N = np.array([[m[idx(PU[i] + PU[j], PV[i] + PV[j])] for j in range(6)] for i in range(6)], np.float64)
    return N, np.asarray(m[15:21], np.float64)


def cloud(name):
    """The clouds of the GPU test, computed once and never changed: {pts, gt, cfg, r_abs, rows} (rows: point indices)."""
    key = ("cloud", name)
    if key in _cache:
        return _cache[key]
    if name == "torus_clean":
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import synth
        from nesti_net_amd.config import NestiConfig
        pts, gt = synth.make_cloud("torus", 12000, seed=7)
        cfg = NestiConfig(patch_radius=list(TORUS_CLEAN_RADII))
        c = {"name": name, "pts": pts, "gt": gt, "cfg": cfg, "r_abs": fx.radii(pts, cfg), "rows": np.arange(0, len(pts), 24)}
    else:
        c = dict(fx.cloud(name))
        N = len(c["pts"])
        c["rows"] = {"ellipsoid": np.arange(0, N, 8), "sphere_big": c["rows"][:256], "torus": np.arange(0, N, 12),
                     "box": np.arange(0, N, 12), "lattice": np.arange(N)}[name]
    _cache[key] = c
    return c
