"""The fixture of the orientation tests (tests/test_orient.py, tests/test_gpu_orient.py) and the tests' OWN restatement of the
orientation pass on the CPU, written from its definition (DESIGN.md 2 "Orientation", include/nesti_hip.h) in numpy:

  eligible rows    all three normal components finite and one non-zero
  nbr(i)           the eligible j != i with float64 d2 = (dx dx + dy dy) + dz dz <= R R, the K smallest by (d2, j), in that order
  edge {a < b}     b in nbr(a) or a in nbr(b); id = a K + slot of b in nbr(a) if b in nbr(a), else b K + slot of a in nbr(b)
  per edge         d = (na.x nb.x + na.y nb.y) + na.z nb.z, q = |n|^2, f = d < 0, w = float32(max(0, 1 - (d d) / (qa qb))), all float64
  forest           Kruskal over the keys (bits of w) << 32 | id
  root of a tree   largest z (ties: smaller index), first non-zero of (nz, ny, nx) made positive; with a viewpoint v the smallest
                   float64 d2 to v, flipped iff n . (v - p) < 0
  flip(x)          flip(root) xor the xor of f over the tree path root -> x

numpy evaluates every product and sum of an expression on its own, which is the rounding the definition asks for.

Clouds come from ``synth.make_cloud``; the input normals are the analytic ones tilted by Gaussian noise, scaled to random lengths
in [0.3, 3] and multiplied by a random sign, all from seeded ``RandomState`` streams."""
import collections

import numpy as np

_cache = {}


def bbdiag(xyz):
    x = np.asarray(xyz, np.float64)
    return float(np.linalg.norm(x.max(0) - x.min(0)))


def noisy_normals(gt, seed, tilt=0.15, signs=False):
    """Analytic normals -> tilted (sigma ``tilt``), lengths in [0.3, 3], random sign; float32.  ``signs``: also the signs drawn."""
    rs = np.random.RandomState(seed)
    n = np.asarray(gt, np.float64) + rs.normal(0.0, tilt, size=gt.shape)
    n *= rs.uniform(0.3, 3.0, size=(len(gt), 1))
    s = rs.choice([-1.0, 1.0], size=(len(gt), 1))
    n = np.ascontiguousarray((n * s).astype(np.float32))
    return (n, s[:, 0]) if signs else n


def _ellipsoid(noise=0.0, tilt=0.15, seed=101, signs=False):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    xyz, gt = synth.make_cloud("ellipsoid", 3001, seed=11, noise=noise)
    return xyz, gt, noisy_normals(gt, seed, tilt, signs)


def _make(name):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    c = {"name": name, "K": 8, "viewpoint": None, "surfaces": 1, "gt": None}
    if name in ("ellipsoid3001", "ellipsoid3001_k16", "ellipsoid3001_k1"):
        c["xyz"], c["gt"], c["normals"] = _ellipsoid()
        c["K"] = {"ellipsoid3001": 8, "ellipsoid3001_k16": 16, "ellipsoid3001_k1": 1}[name]
        if name == "ellipsoid3001_k1":
            c["surfaces"] = None                      # the documented limit: the graph falls apart
    elif name == "ellipsoid3001_zero10":
        c["xyz"], c["gt"], n = _ellipsoid()
        n = n.copy()
        n[np.random.RandomState(102).uniform(size=len(n)) < 0.1] = 0.0       # the sentinel of a query without a neighbourhood
        c["normals"] = n
    elif name == "ellipsoid3001_noisy":
        # tilt 0.3: a handful of the tilted normals themselves point against the analytic ones, so the case carries the signs drawn
        c["xyz"], c["gt"], (c["normals"], c["signs"]) = _ellipsoid(noise=0.006, tilt=0.3, seed=103, signs=True)
    elif name == "torus4k_gradient":
        c["xyz"], c["gt"] = synth.make_cloud("torus", 4000, seed=12, density="gradient")
        c["normals"] = noisy_normals(c["gt"], 104)
    elif name == "two_spheres":
        p, g = synth.make_cloud("sphere", 1500, seed=13)
        q = (p.astype(np.float64) * 0.6 + np.array([3.0, 0.0, 0.2])).astype(np.float32)
        c["xyz"], c["gt"] = np.ascontiguousarray(np.concatenate([p, q])), np.concatenate([g, g])
        c["normals"] = noisy_normals(c["gt"], 105)
        c["surfaces"] = 2
    elif name == "helix2000":
        t = np.linspace(0.0, 12.0 * np.pi, 2000)
        c["xyz"] = np.ascontiguousarray(np.stack([np.cos(t), np.sin(t), 0.05 * t], 1).astype(np.float32))
        c["gt"] = np.stack([np.cos(t), np.sin(t), np.zeros_like(t)], 1).astype(np.float32)
        c["normals"] = noisy_normals(c["gt"], 106, tilt=0.05)
        c["K"], c["R"] = 2, 0.1
    elif name == "lattice":
        g = np.arange(12) * 0.25
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        c["xyz"] = np.ascontiguousarray(np.concatenate([p, p[:100]]).astype(np.float32))       # massive d2 ties, duplicates at d2 = 0
        c["normals"] = np.ascontiguousarray(np.random.RandomState(107).normal(size=c["xyz"].shape).astype(np.float32))
        c["K"], c["R"], c["surfaces"] = 6, 0.26, None
    else:
        raise KeyError(name)
    c.setdefault("R", 0.05 * bbdiag(c["xyz"]))
    return c


SANITY = ("ellipsoid3001", "ellipsoid3001_k16", "ellipsoid3001_zero10", "torus4k_gradient", "two_spheres")
TABLE = SANITY + ("ellipsoid3001_k1", "ellipsoid3001_noisy", "helix2000", "lattice")


def case(name):
    """One input of the table, computed once and never changed: {xyz, normals, gt, K, R, viewpoint, surfaces}."""
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def eligible(normals):
    n = np.asarray(normals, np.float32)
    return np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)


def neighbours(xyz, normals, R, K):
    """nbr [M,K] int32, -1 padded."""
    from scipy import spatial
    x = np.asarray(xyz, np.float32).astype(np.float64)
    M = len(x)
    el = eligible(normals)
    nbr = np.full((M, K), -1, np.int32)
    ids = np.nonzero(el)[0]
    if len(ids) == 0:
        return nbr
    tree = spatial.cKDTree(x[ids])
    balls = tree.query_ball_point(x[ids], R * 1.001 + 1e-300)
    r2 = R * R
    for row, ball in zip(ids, balls):
        j = ids[np.asarray(ball, np.int64)]
        j = j[j != row]
        d = x[j] - x[row]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 <= r2
        j, d2 = j[keep], d2[keep]
        o = np.lexsort((j, d2))[:K]
        nbr[row, :len(o)] = j[o]
    return nbr


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def graph(xyz, normals, R, K):
    """{nbr, u, v, wbits, flip, w}: u / v [M K] int32 by edge id (-1: no edge in the slot), wbits uint32, flip uint8, w float32."""
    nbr = neighbours(xyz, normals, R, K)
    M = len(nbr)
    i = np.repeat(np.arange(M), K)
    j = nbr.reshape(-1).astype(np.int64)
    valid = j >= 0
    members = [set(row[row >= 0].tolist()) for row in nbr]
    for e in np.nonzero(valid & (i > j))[0]:
        if i[e] in members[j[e]]:
            valid[e] = False                       # the pair lives in the slot of the larger index in the smaller one's list
    u = np.where(valid, np.minimum(i, j), -1).astype(np.int32)
    v = np.where(valid, np.maximum(i, j), -1).astype(np.int32)
    n = np.asarray(normals, np.float32).astype(np.float64)
    a, b = n[u[valid]], n[v[valid]]
    d = _dot(a, b)
    with np.errstate(all="ignore"):
        w = np.maximum(0.0, 1.0 - (d * d) / (_dot(a, a) * _dot(b, b))).astype(np.float32)
    wf = np.zeros(M * K, np.float32)
    wf[valid] = w
    flip = np.zeros(M * K, np.uint8)
    flip[valid] = d < 0
    return {"nbr": nbr, "u": u, "v": v, "w": wf, "wbits": wf.view(np.uint32).copy(), "flip": flip}


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def orient(xyz, normals, R, K, viewpoint=None, g=None, wbits=None):
    """The predicted result: {out, flipped [M] bool, tree [M K] uint8, stats, depth, g}.  ``wbits``: weights to order the edges by
    in place of the restatement's own (the GPU test passes the library's)."""
    xyz = np.asarray(xyz, np.float32)
    normals = np.asarray(normals, np.float32)
    M = len(xyz)
    g = g or graph(xyz, normals, R, K)
    wb = g["wbits"] if wbits is None else np.asarray(wbits, np.uint32)
    el = eligible(normals)
    ids = np.nonzero(g["u"] >= 0)[0]
    keys = (wb[ids].astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
    parent = list(range(M))
    adj = collections.defaultdict(list)
    tree = np.zeros(M * K, np.uint8)
    for e in ids[np.argsort(keys, kind="stable")]:
        a, b = int(g["u"][e]), int(g["v"][e])
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[ra] = rb
            tree[e] = 1
            f = int(g["flip"][e])
            adj[a].append((b, f))
            adj[b].append((a, f))
    comps = collections.defaultdict(list)
    for x in np.nonzero(el)[0]:
        comps[_find(parent, int(x))].append(int(x))
    x64, n64 = xyz.astype(np.float64), normals.astype(np.float64)
    flipped = np.zeros(M, bool)
    depth = 0
    for members in comps.values():
        m = np.asarray(members)                    # ascending: argmax / argmin take the smaller index on ties
        if viewpoint is None:
            root = int(m[np.argmax(xyz[m, 2])])
            lead = [c for c in (normals[root, 2], normals[root, 1], normals[root, 0]) if c != 0][0]
            rf = bool(lead < 0)
        else:
            dv = np.asarray(viewpoint, np.float64)[None, :] - x64[m]
            root = int(m[np.argmin(_dot(dv, dv))])
            dr = np.asarray(viewpoint, np.float64) - x64[root]
            rf = bool(_dot(n64[root][None], dr[None])[0] < 0)
        flipped[root] = rf
        seen = {root}
        queue = collections.deque([(root, 0)])
        while queue:
            a, da = queue.popleft()
            depth = max(depth, da)
            for b, f in adj[a]:
                if b not in seen:
                    seen.add(b)
                    flipped[b] = flipped[a] ^ bool(f)
                    queue.append((b, da + 1))
    out = normals.copy()
    bits = out.view(np.uint32)
    bits[flipped] ^= np.uint32(0x80000000)         # sign bits only
    stats = {"n_eligible": int(el.sum()), "n_components": len(comps), "n_flipped": int(flipped.sum()), "n_edges": int(len(ids))}
    return {"out": out, "flipped": flipped, "tree": tree, "stats": stats, "depth": depth, "g": g}


def orient_viewpoint(xyz, normals, viewpoint):
    """NESTI_ORIENT_VIEWPOINT: every eligible row flipped iff the float64 n . (v - p) < 0."""
    xyz = np.asarray(xyz, np.float32)
    normals = np.asarray(normals, np.float32)
    el = eligible(normals)
    dv = np.asarray(viewpoint, np.float64)[None, :] - xyz.astype(np.float64)
    with np.errstate(all="ignore"):
        flipped = el & (_dot(normals.astype(np.float64), dv) < 0)
    out = normals.copy()
    out.view(np.uint32)[flipped] ^= np.uint32(0x80000000)
    return {"out": out, "flipped": flipped,
            "stats": {"n_eligible": int(el.sum()), "n_components": 0, "n_flipped": int(flipped.sum()), "n_edges": 0}}


def predicted(name):
    """``orient`` of a table case with the restatement's own weights, computed once."""
    key = ("pred", name)
    if key not in _cache:
        c = case(name)
        _cache[key] = orient(c["xyz"], c["normals"], c["R"], c["K"], c["viewpoint"])
    return _cache[key]


def inward(out, gt, normals_in):
    """Rows of eligible input whose oriented normal points against the analytic one."""
    el = eligible(normals_in)
    return int((np.sum(out.astype(np.float64) * gt.astype(np.float64), axis=1)[el] < 0).sum())
