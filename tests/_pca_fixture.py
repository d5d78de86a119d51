"""The fixture of the plane-fit tests (tests/test_pca.py, tests/test_gpu_pca.py) and the tests' OWN restatement of the plane-fit
estimator on the CPU, written from its definition (DESIGN.md 2 "Plane-fit normals", include/nesti_hip.h) in numpy:

  ball(c, s)   the cloud points p with float64 d2 = (dx dx + dy dy) + dz dz <= r_s r_s, d = float64(p) - float64(c): candidates from
               scipy's cKDTree with a slightly larger radius, the test itself as the library words it.  The FULL ball: no cap, no subsample
  moments      n, m = sum(d) / n, C = (sum(d d^T) / n - m m^T) / (r_s r_s), float64
  eigen        numpy.linalg.eigh(C): w ascending, the normal is the eigenvector of w[0], normalised, rounded to float32, then signed on
               the float32 values so that the first non-zero of (n_z, n_y, n_x) is positive
  eig          float32(max(0, w))
  sentinel     n < 3: normal 0 0 0, eigenvalues 0 0 0, the count stays
  a position with a non-finite coordinate has n = 0 at every scale

Besides what the library returns, ``restate`` keeps the float64 eigenvalues and matrices the tests' bounds are written in."""
import numpy as np

_cache = {}
EPS = 2.0 ** -53


def radii(pts, cfg):
    """r_abs as ``provider.CloudPatches`` computes them: float64 bounding-box diagonal of the float32 cloud times the configured radii."""
    pts = np.asarray(pts, np.float32)
    bbdiag = float(np.linalg.norm(pts.max(0) - pts.min(0), 2))
    return [bbdiag * r for r in cfg.patch_radius]


def sign_rule(n32):
    """float32 [.., 3] -> the same with the first non-zero of (z, y, x) positive; zeros come back as +0."""
    n32 = np.asarray(n32, np.float32)
    z, y, x = n32[..., 2], n32[..., 1], n32[..., 0]
    lead = np.where(z != 0, z, np.where(y != 0, y, x))
    out = np.where((lead < 0)[..., None], -n32, n32)
    return (out + np.float32(0.0)).astype(np.float32)


def restate(pts, positions, r_abs, tree=None):
    """Plane fit at ``positions`` [M,3] (float32) over the cloud ``pts`` -> dict of
    normals [M,S,3] f32, eig [M,S,3] f32, n_ball [M,S] int32, w [M,S,3] f64 (unclamped eigenvalues, r^2 units), C [M,S,3,3] f64."""
    from scipy import spatial
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    p64 = pts.astype(np.float64)
    tree = tree or spatial.cKDTree(p64, 10)
    M, S = len(positions), len(r_abs)
    out = {"normals": np.zeros((M, S, 3), np.float32), "eig": np.zeros((M, S, 3), np.float32), "n_ball": np.zeros((M, S), np.int32),
           "w": np.zeros((M, S, 3), np.float64), "C": np.zeros((M, S, 3, 3), np.float64)}
    order = np.argsort(r_abs)
    r_big = float(r_abs[order[-1]])
    for q in range(M):
        c = positions[q].astype(np.float64)
        if not np.isfinite(c).all():
            continue
        cand = np.asarray(tree.query_ball_point(c, r_big * (1.0 + 1e-9) + 1e-300), np.int64)
        d = p64[cand] - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        for s, r in enumerate(r_abs):
            r2 = float(r) * float(r)
            ds = d[d2 <= r2]
            n = len(ds)
            out["n_ball"][q, s] = n
            if n < 3:
                continue
            m = ds.sum(0) / n
            C = ((ds[:, :, None] * ds[:, None, :]).sum(0) / n - m[:, None] * m[None, :]) / r2
            C = 0.5 * (C + C.T)
            w, V = np.linalg.eigh(C)
            v = V[:, 0] / np.linalg.norm(V[:, 0])
            out["normals"][q, s] = sign_rule(v.astype(np.float32))
            out["eig"][q, s] = np.maximum(0.0, w).astype(np.float32)
            out["w"][q, s], out["C"][q, s] = w, C
    return out


def variation(eig):
    """w0 / (w0 + w1 + w2), 0 where the sum is 0; float32 like the product."""
    eig = np.asarray(eig, np.float32)
    tot = eig.sum(axis=-1, dtype=np.float32)
    return np.divide(eig[..., 0], tot, out=np.zeros_like(tot), where=tot != 0)


def lattice():
    """A 40 x 40 unit grid in z = 0, its first 100 points again, and 200 collinear points (0.25 k, 60, 0); float32."""
    g = np.arange(40, dtype=np.float64)
    plane = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    plane = np.concatenate([plane, np.zeros((len(plane), 1))], 1)
    line = np.stack([0.25 * np.arange(200), np.full(200, 60.0), np.zeros(200)], 1)
    return np.ascontiguousarray(np.concatenate([plane, plane[:100], line]).astype(np.float32))


LATTICE_PLANE_ROWS = 1700          # rows [0, 1700) of lattice() lie in the grid, rows [1700, 1900) on the line


def angle_rms_deg(normals, gt):
    """RMS of the unoriented angle between rows, degrees (rows with a zero normal left out)."""
    a, b = np.asarray(normals, np.float64), np.asarray(gt, np.float64)
    live = (a != 0).any(axis=1)
    cos = np.abs((a[live] * b[live]).sum(1)) / (np.linalg.norm(a[live], axis=1) * np.linalg.norm(b[live], axis=1))
    return float(np.degrees(np.sqrt(np.mean(np.arccos(np.clip(cos, 0.0, 1.0)) ** 2))))


def cloud(name):
    """The surface clouds of the GPU test, computed once and never changed: {pts, gt, cfg, r_abs, rows}."""
    if name in _cache:
        return _cache[name]
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    from nesti_net_amd.config import NestiConfig
    cfg = NestiConfig()
    if name == "ellipsoid":
        pts, gt = synth.make_cloud("ellipsoid", 4000, seed=7)
        rows = np.arange(len(pts))
    elif name == "box":
        pts, gt = synth.make_cloud("box", 6000, seed=7)
        rows = np.arange(0, len(pts), 3)
    elif name == "torus":
        pts, gt = synth.make_cloud("torus", 6000, seed=7, noise=0.006)
        rows = np.arange(0, len(pts), 3)
    elif name == "sphere_big":
        pts, gt = synth.make_cloud("sphere", 20000, seed=7)
        cfg = NestiConfig(patch_radius=[0.05, 0.1, 0.2])
        rows = np.arange(0, len(pts), 39)[:512]
    elif name == "lattice":
        pts, gt = lattice(), None
        rows = np.arange(len(pts))
    else:
        raise KeyError(name)
    _cache[name] = {"name": name, "pts": pts, "gt": gt, "cfg": cfg, "r_abs": radii(pts, cfg), "rows": rows}
    return _cache[name]


def predicted(name):
    """``restate`` of a cloud's rows, computed once."""
    key = ("pred", name)
    if key not in _cache:
        c = cloud(name)
        _cache[key] = restate(c["pts"], c["pts"][c["rows"]], c["r_abs"])
    return _cache[key]
