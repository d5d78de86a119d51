"""The fixture of the search-grid tests (tests/test_grid_fixture.py, tests/test_gpu_grid.py): clouds that put the uniform grid of
csrc/patches.hip into the regimes the surface clouds of the other tests never reach, and the tests' OWN restatement of ``header_kernel``.

  lattice_exact    the integer lattice 13 x 19 x 37: bbdiag = 42 and r_abs = 3 / 5 / 7 exactly, every d2 an integer, thousands of pairs
                   with d2 == r^2 -- the inclusive ball test.  Ball sizes come from an int64 brute force, not from scipy
  lattice_shifted  the same lattice x 0.25 at an exactly representable offset: the same balls, far from the origin
  plate            uniform in 1 x 0.5 x 0.02, radii <= 0.006: the kMaxDim clamp (cell = ext / 127 > 1.0001 r_max), dims ~ 128 x 64 x 3
  needle_x         5 000 sorted points on the x axis: dims 127-128 x 1 x 1
  needle_diag      5 000 points on the space diagonal: ~127^3 = 2.05 M cells, almost all of them empty
  offset           a slab moved to (1000, -2000, 500): f32 quantisation, the ordered-bits bounding box, (v - min) inv_cell in fp64
  duplicates       2 000 points four times each and one point 1 500 times: balls of ties at d2 = 0, one of them above kListCap

Each case: ``pts`` (float32), ``cfg``, ``r_abs`` (as ``provider.CloudPatches`` computes them), ``rows`` (at most ~400 query indices) and,
for plate and needle_diag, ``positions`` (float32 [M,3]: outside the bounding box and inside empty cells).  Host only, deterministic,
each case computed once and never changed."""
import numpy as np

K_MAX_DIM = 128          # kMaxDim of csrc/patches_dev.h
K_LIST_CAP = 1024        # kListCap

CASES = ("lattice_exact", "lattice_shifted", "plate", "needle_x", "needle_diag", "offset", "duplicates")
CLAMPED = ("plate", "needle_x", "needle_diag")
WITH_POSITIONS = ("plate", "needle_diag")
LATTICE = (13, 19, 37)
LATTICE_CENTRE = (6, 9, 18)
PUSH = (0.5, 0.99, 1.01, 2.5)
EXTREME = 6              # extreme cloud points per bounding-box face among the outside positions

_cache = {}


def radii(pts, cfg):
    """bbdiag and r_abs as ``provider.CloudPatches`` computes them (utils/pcpnet_dataset.py:281-282)."""
    pts = np.asarray(pts, np.float32)
    bbdiag = float(np.linalg.norm(pts.max(0) - pts.min(0), 2))
    return bbdiag, [bbdiag * r for r in cfg.patch_radius]


def header(pts, r_abs):
    """``header_kernel`` in Python floats (IEEE double, like the device): {minv [3], cell, inv_cell, dims [3], ncells, clamped}.
    ``clamped``: the ``ext / (kMaxDim - 1)`` arm of the cell edge is the larger one."""
    pts = np.asarray(pts, np.float32)
    lo = [float(v) for v in pts.min(0)]
    hi = [float(v) for v in pts.max(0)]
    ext = max(0.0, max(h - l for h, l in zip(hi, lo)))
    cell_min = max(float(r) for r in r_abs) * 1.0001
    cell = max(cell_min, ext / float(K_MAX_DIM - 1))
    if not cell > 0.0:
        cell = 1.0
    inv_cell = 1.0 / cell
    dims = [max(1, min(K_MAX_DIM, int(np.floor((h - l) * inv_cell)) + 1)) for h, l in zip(hi, lo)]
    return {"minv": lo, "cell": cell, "inv_cell": inv_cell, "dims": dims, "ncells": dims[0] * dims[1] * dims[2],
            "clamped": ext / float(K_MAX_DIM - 1) > cell_min}


def cells(pts, h):
    """Flat cell (x fastest) of float32 positions: ``cell_axis`` / ``cell_flat`` of csrc/patches_dev.h, clamped into the grid."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    idx = []
    for c in range(3):
        i = np.floor((p[:, c] - h["minv"][c]) * h["inv_cell"])
        idx.append(np.minimum(h["dims"][c] - 1, np.maximum(0.0, i)).astype(np.int64))
    return (idx[2] * h["dims"][1] + idx[1]) * h["dims"][0] + idx[0]


def lattice_points(scale=1.0, offset=(0.0, 0.0, 0.0)):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in LATTICE], indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray((g * scale + np.asarray(offset, np.float64)).astype(np.float32))


def lattice_index(ix, iy, iz):
    return (ix * LATTICE[1] + iy) * LATTICE[2] + iz


def lattice_counts(rows, r2, strict=False):
    """Ball sizes [len(rows), len(r2)] on the integer lattice by brute force: int64 dx^2 + dy^2 + dz^2 <= r2 (``strict``: <) over all points."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.int64) for n in LATTICE], indexing="ij"), -1).reshape(-1, 3)
    out = np.zeros((len(rows), len(r2)), np.int64)
    on = np.zeros((len(rows), len(r2)), bool)
    for k, row in enumerate(rows):
        d = g - g[row]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        for s, rr in enumerate(r2):
            out[k, s] = int((d2 < rr).sum() if strict else (d2 <= rr).sum())
            on[k, s] = bool((d2 == rr).any())
    return out, on


def _lattice_rows():
    n = LATTICE[0] * LATTICE[1] * LATTICE[2]
    corners = [lattice_index(x, y, z) for x in (0, LATTICE[0] - 1) for y in (0, LATTICE[1] - 1) for z in (0, LATTICE[2] - 1)]
    return np.unique(np.concatenate([np.arange(0, n, 31), [lattice_index(*LATTICE_CENTRE)], corners])).astype(np.int64)


def _positions(pts, r_abs, seed):
    """Positions outside the bounding box -- its 8 corners and 6 face centres, and the EXTREME cloud points of every face (most corners and
    face centres of these clouds are far from any point), moved outward by PUSH x r_max along every axis in which they lie on the boundary
    -- and positions inside EMPTY cells at 0.9 r and 1.1 r (every scale's r) from their nearest cloud point.
    -> (positions float32 [M,3], n_outside)."""
    from scipy import spatial
    p64 = np.asarray(pts, np.float32).astype(np.float64)
    lo, hi, r_max = p64.min(0), p64.max(0), max(r_abs)
    mid = 0.5 * (lo + hi)
    anchors = []                                       # (point, outward direction per axis: -1, 0, +1)
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                anchors.append((np.where(np.array([sx, sy, sz]) < 0, lo, hi), np.array([sx, sy, sz], np.float64)))
    for axis in range(3):
        for sign in (-1, 1):
            q, d = mid.copy(), np.zeros(3)
            q[axis] = lo[axis] if sign < 0 else hi[axis]
            d[axis] = sign
            anchors.append((q, d))
    for axis in range(3):                              # ... and the EXTREME cloud points of each face, where the cloud is
        order = np.argsort(p64[:, axis], kind="stable")
        for sign, ext in ((-1, order[:EXTREME]), (1, order[-EXTREME:])):
            d = np.zeros(3)
            d[axis] = sign
            anchors.extend((p64[i], d) for i in ext)
    outside = [q + f * r_max * d for q, d in anchors for f in PUSH]
    # inside empty cells: random positions in the box, moved along the line to their nearest cloud point until they are f r from it
    h = header(pts, r_abs)
    occupied = np.zeros(h["ncells"], bool)
    occupied[cells(pts, h)] = True
    tree = spatial.cKDTree(p64)
    rs = np.random.RandomState(seed)
    inside = []
    for r in r_abs:
        for f in (0.9, 1.1):
            base = p64[rs.randint(0, len(p64), 4000)]      # anywhere in the box, and next to cloud points (a thin cloud in a big box)
            cand = np.concatenate([lo + rs.uniform(size=(4000, 3)) * (hi - lo), base + rs.normal(size=base.shape) * r])
            _, j = tree.query(cand)
            d = cand - p64[j]
            n = np.linalg.norm(d, axis=1)
            ok = n > 0
            q = (p64[j[ok]] + (f * r) * d[ok] / n[ok, None]).astype(np.float32)
            near, _ = tree.query(q.astype(np.float64))
            box = ((q >= lo) & (q <= hi)).all(axis=1)
            keep = box & ~occupied[cells(q, h)] & (near >= 0.97 * f * r) & (near <= 1.0000001 * f * r)
            inside.append(q[keep][:12])
    pos = np.ascontiguousarray(np.concatenate([np.asarray(outside, np.float64).astype(np.float32)] + inside))
    return pos, len(outside)


def _make(name):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.config import NestiConfig
    c = {"name": name}
    if name == "lattice_exact":
        c["pts"] = lattice_points()
        c["cfg"] = NestiConfig(patch_radius=[3.0 / 42.0, 5.0 / 42.0, 7.0 / 42.0])
        c["rows"] = _lattice_rows()
    elif name == "lattice_shifted":
        c["pts"] = lattice_points(0.25, (256.0, -512.0, 128.0))      # multiples of 0.25 below 2^10: exact in float32
        c["cfg"] = NestiConfig(patch_radius=[3.0 / 42.0, 5.0 / 42.0, 7.0 / 42.0])
        c["rows"] = _lattice_rows()
    elif name == "plate":
        rs = np.random.RandomState(201)
        c["pts"] = np.ascontiguousarray((rs.uniform(size=(60000, 3)) * np.array([1.0, 0.5, 0.02])).astype(np.float32))
        c["cfg"] = NestiConfig(patch_radius=[0.002, 0.004, 0.006], num_point=8)
        c["rows"] = np.arange(0, 60000, 151).astype(np.int64)
    elif name == "needle_x":
        rs = np.random.RandomState(202)
        x = np.sort(rs.uniform(size=5000))
        c["pts"] = np.ascontiguousarray(np.stack([x, np.zeros(5000), np.zeros(5000)], 1).astype(np.float32))
        c["cfg"] = NestiConfig(patch_radius=[0.002, 0.004, 0.007], num_point=32)
        c["rows"] = np.concatenate([[0, 1, 4998, 4999], np.arange(5, 5000, 13)]).astype(np.int64)
    elif name == "needle_diag":
        rs = np.random.RandomState(203)
        t = np.sort(rs.uniform(size=5000))
        c["pts"] = np.ascontiguousarray((t[:, None] * np.ones(3) + rs.normal(0.0, 1e-4, size=(5000, 3))).astype(np.float32))
        c["cfg"] = NestiConfig(patch_radius=[0.001, 0.002, 0.004], num_point=32)
        c["rows"] = np.concatenate([[0, 1, 4998, 4999], np.arange(5, 5000, 13)]).astype(np.int64)
    elif name == "offset":
        rs = np.random.RandomState(204)
        p = rs.uniform(size=(6000, 3)) * np.array([1.0, 1.0, 0.05]) + np.array([1000.0, -2000.0, 500.0])
        c["pts"] = np.ascontiguousarray(p.astype(np.float32))
        c["cfg"] = NestiConfig(num_point=64)
        c["rows"] = np.arange(0, 6000, 17).astype(np.int64)
    elif name == "duplicates":
        rs = np.random.RandomState(205)
        base = rs.uniform(size=(2000, 3))
        many = rs.uniform(0.3, 0.7, size=(1, 3))
        p = np.concatenate([np.repeat(base, 4, axis=0), np.repeat(many, 1500, axis=0)])
        order = rs.permutation(len(p))
        c["pts"] = np.ascontiguousarray(p[order].astype(np.float32))
        c["cfg"] = NestiConfig()
        heavy = np.flatnonzero(order >= 8000)            # the rows of the point that is there 1 500 times
        c["rows"] = np.unique(np.concatenate([heavy[:8], np.arange(0, len(p), 31)])).astype(np.int64)
        c["heavy"] = heavy
    else:
        raise KeyError(name)
    c["bbdiag"], c["r_abs"] = radii(c["pts"], c["cfg"])
    c["header"] = header(c["pts"], c["r_abs"])
    if name in WITH_POSITIONS:
        c["positions"], c["n_outside"] = _positions(c["pts"], c["r_abs"], 300 + CASES.index(name))
    return c


def case(name):
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def ball_sizes(name):
    """Ball sizes [len(rows), S] of a case's rows on the host, computed once: the int64 brute force on the lattices (independent of
    scipy), elsewhere scipy's ``query_ball_point`` as oracle/patches_ref.py asks it."""
    key = ("balls", name)
    if key not in _cache:
        c = case(name)
        if name.startswith("lattice"):
            # the shifted lattice is the integer one x 0.25: the same index differences, r^2 = 9, 25, 49 in lattice units
            _cache[key] = lattice_counts(c["rows"], (9, 25, 49))[0].astype(np.int32)
        else:
            from scipy import spatial
            tree = spatial.cKDTree(c["pts"], 10)
            _cache[key] = np.stack([tree.query_ball_point(c["pts"][c["rows"]], r, return_length=True) for r in c["r_abs"]], 1).astype(np.int32)
    return _cache[key]


def orient_input(name, max_points=12000):
    """(xyz, normals, R, K) of the orientation-graph test: the cloud (every k-th point of a large one: the bounding box, and with it the
    grid regime at R, stays), noisy normals of a constant ground truth, R = max(r_abs), K = 8."""
    key = ("orient", name)
    if key not in _cache:
        import _orient_fixture as OF
        c = case(name)
        step = -(-len(c["pts"]) // max_points)
        xyz = np.ascontiguousarray(c["pts"][::step])
        gt = np.tile(np.array([[0.0, 0.0, 1.0]]), (len(xyz), 1))
        _cache[key] = (xyz, OF.noisy_normals(gt, 400 + CASES.index(name)), max(c["r_abs"]), 8)
    return _cache[key]
