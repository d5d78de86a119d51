"""The fixture of the robust plane-fit tests (tests/test_robust.py, tests/test_gpu_robust.py): the tests' OWN restatement of
``nesti_robust_normals_nbr`` on the CPU, written from its definition (DESIGN.md 2 "Robust plane fit", include/nesti_hip.h) in numpy,
vectorised over rows, scalar by scalar in the stated order.  float64 throughout; numpy rounds every operation on its own, as the kernel
does.

  lists     the valid prefix of a row ends at its first entry outside [0, N); n = min(k, prefix); a non-finite centre has an empty
            prefix; d = float64(p) - float64(c); d2 = (dx dx + dy dy) + dz dz; r2 = max d2 over the prefix (NaN ignored, as fmax does)
  sums      slot i is added in lane i mod 64, a lane adds its slots in ascending order from +0.0; the 64 partial sums meet in the
            xor-butterfly 32, 16, ..., 1
  steps 1-5 of one iteration: bit for bit.  The two order statistics are elements of the sorted values (rank n // 2), never averages
  step 6    m, C in numpy, then the library's HOST entry ``nesti_sym3_eig`` -- the solver source the device compiles --, the
            normalisation, one rounding to float32 and the sign rule
  step 7    the failure rules; ``restate`` chains the iterations through the float32 normal alone
  plane     the same sums with weight 1 and the count for the mass: ``nesti_pca_normals_nbr``'s normal

It takes a list, so it needs no search of its own.  Host only, deterministic."""
import ctypes

import numpy as np

from _pca_fixture import sign_rule
from _select_fixture import within_deg  # noqa: F401  (the share within 10 degrees, in per cent: the tests' figure of merit)

WAVE = 64
_D = ctypes.POINTER(ctypes.c_double)
_lib = []


def sym3_eig(c6):
    """``nesti_sym3_eig`` of {xx, xy, xz, yy, yz, zz}: (w [3] ascending, vec [3,3], row k the eigenvector of w[k])."""
    if not _lib:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import _lib as L
        _lib.append(L.load())
    c = np.ascontiguousarray(c6, np.float64)
    w, v = np.zeros(3), np.zeros(9)
    assert _lib[0].nesti_sym3_eig(c.ctypes.data_as(_D), w.ctypes.data_as(_D), v.ctypes.data_as(_D)) == 0
    return w, v.reshape(3, 3)


def butterfly(part):
    """The xor-butterfly of 64 partial sums [..., 64]: offsets 32, ..., 1; lane 0's total."""
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off:
        part = part + part[..., lanes ^ off]
        off //= 2
    return part[..., 0]


def lane_totals(terms, used):
    """terms [M,k,T], used [M,k] -> [M,T]: the totals as the wave forms them (an unused slot is no addition)."""
    M, k, T = terms.shape
    trips = -(-k // WAVE)
    padded = np.zeros((M, trips * WAVE, T))
    padded[:, :k] = np.where(used[..., None], terms, 0.0)
    took = np.zeros((M, trips * WAVE), bool)
    took[:, :k] = used
    padded, took = padded.reshape(M, trips, WAVE, T), took.reshape(M, trips, WAVE)
    part = np.zeros((M, WAVE, T))
    with np.errstate(all="ignore"):
        for s in range(trips):
            part = np.where(took[:, s, :, None], part + padded[:, s], part)
        return np.stack([butterfly(part[..., c]) for c in range(T)], -1)


def rank_element(vals, used, n):
    """The element of 0-based rank n // 2 of the used values of every row, ascending; 0 for a row without values."""
    s = np.sort(np.where(used, vals, np.inf), axis=1)
    return np.where(n > 0, s[np.arange(len(s)), np.minimum(n // 2, s.shape[1] - 1)], 0.0)


def geometry(pts, centres, nbr, k):
    """The lists of one scale: n [M], used [M,k], D [M,k,3], d2 [M,k], r2 [M], the nine plane terms [M,k,9] (d, then the products
    xx xy xz yy yz zz of d) and wild [M] (a d2 of the prefix that is not finite)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    c64 = np.ascontiguousarray(centres, dtype=np.float32).astype(np.float64)
    nbr = np.asarray(nbr, np.int64)[:, :k]
    N = len(pts)
    bad = (nbr < 0) | (nbr >= N)
    n = np.where(bad.any(1), bad.argmax(1), nbr.shape[1])
    n = np.where(np.isfinite(c64).all(1), n, 0)
    used = np.arange(nbr.shape[1])[None, :] < n[:, None]
    with np.errstate(all="ignore"):
        D = pts.astype(np.float64)[np.clip(nbr, 0, N - 1)] - c64[:, None, :]
        x, y, z = D[..., 0], D[..., 1], D[..., 2]
        d2 = (x * x + y * y) + z * z
        r2 = np.fmax.reduce(np.where(used, d2, 0.0), axis=1, initial=0.0)
        terms = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], -1)
    wild = (used & ~np.isfinite(d2)).any(1)
    return {"n": n.astype(np.int32), "used": used, "D": D, "d2": d2, "r2": r2, "terms": terms, "wild": wild}


def solve(sums, mass, r2, rows):
    """Step 6 for the rows ``rows`` (a mask): the normal of the nine sums [M,9] of total mass [M] -> float32 [M,3] (0 elsewhere)."""
    out = np.zeros((len(mass), 3), np.float32)
    with np.errstate(all="ignore"):
        m = sums[:, :3] / mass[:, None]
        mm = np.stack([m[:, 0] * m[:, 0], m[:, 0] * m[:, 1], m[:, 0] * m[:, 2], m[:, 1] * m[:, 1], m[:, 1] * m[:, 2], m[:, 2] * m[:, 2]], -1)
        C = (sums[:, 3:] / mass[:, None] - mm) / r2[:, None]
        for q in np.flatnonzero(rows):
            v = sym3_eig(C[q])[1][0]
            ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            out[q] = sign_rule((v / ln).astype(np.float32))
    return out


def plane(geo):
    """``nesti_pca_normals_nbr``'s normal of the lists ``geometry`` returned: float32 [M,3]; n < 3 or r2 == 0: 0 0 0."""
    sums = lane_totals(geo["terms"], geo["used"])
    return solve(sums, geo["n"].astype(np.float64), geo["r2"], (geo["n"] >= 3) & (geo["r2"] > 0.0))


def eligible(g):
    """float32 [M,3] -> bool [M]: three finite components and one non-zero."""
    g = np.asarray(g, np.float32)
    return np.isfinite(g).all(1) & (g != 0).any(1)


def unit(g):
    """Step 1: the canonicalised float32 normals [M,3] -> v float64 [M,3]."""
    g = sign_rule(g).astype(np.float64)
    with np.errstate(all="ignore"):
        return g / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]


def weights(geo, g, sigma, falloff, floor):
    """Steps 1-4 from the float32 normals g [M,3]: (w [M,k], res [M,k], sig [M])."""
    sigma, falloff, floor = np.float64(sigma), np.float64(falloff), np.float64(floor)
    v, D, used, n = unit(g), geo["D"], geo["used"], geo["n"]
    with np.errstate(all="ignore"):
        h = (v[:, None, 0] * D[..., 0] + v[:, None, 1] * D[..., 1]) + v[:, None, 2] * D[..., 2]
        res = h - rank_element(h, used, n)[:, None]
        med = rank_element(np.abs(res), used, n)
        sig = np.maximum(sigma * med, floor * np.sqrt(geo["r2"]))
        x = res / sig[:, None]
        t = 1.0 / (1.0 + x * x)
        u = 1.0 - falloff * (geo["d2"] / geo["r2"][:, None])
        a = u * t
        return a * a, res, sig


def iterate_once(geo, g, live, sigma, falloff, floor):
    """One iteration from the float32 normals g [M,3] for the rows ``live`` -> dict of normals f32 [M,3] (the new normal where the
    iteration succeeded, g under the sign rule elsewhere), ok [M], moments f64 [M,10], inliers int32 [M]."""
    used = geo["used"]
    w, res, sig = weights(geo, g, sigma, falloff, floor)
    with np.errstate(all="ignore"):
        moments = lane_totals(np.concatenate([w[..., None], w[..., None] * geo["terms"]], -1), used)
        heavy = (used & (w > 0.0)).sum(1)
        inliers = (used & (np.abs(res) <= sig[:, None])).sum(1).astype(np.int32)
        can = live & (moments[:, 0] > 0.0) & (heavy >= 3)
    new = solve(moments[:, 1:], moments[:, 0], geo["r2"], can)
    ok = can & eligible(new)
    return {"normals": np.where(ok[:, None], new, sign_rule(g)), "ok": ok, "moments": np.where(ok[:, None], moments, 0.0),
            "inliers": np.where(ok, inliers, 0).astype(np.int32)}


def restate(pts, centres, nbr, k, iters=8, sigma=2.0, falloff=0.5, floor=0.01, init=None):
    """One scale of the entry: the ``k`` first entries of the lists ``nbr`` [M,K] of the float32 positions ``centres`` [M,3], ``init``
    float32 [M,3] or None -> dict of normals, plane f32 [M,3], support f32 [M], inliers, iters_done, count int32 [M], moments f64
    [M,10], radius f32 [M], and ``geo`` (``geometry``)."""
    geo = geometry(pts, centres, nbr, k)
    M = len(geo["n"])
    pl = plane(geo)
    g = pl if init is None else np.ascontiguousarray(init, np.float32).reshape(M, 3)
    live = (geo["n"] >= 3) & (geo["r2"] > 0.0) & ~geo["wild"] & eligible(g)
    cur = np.where(live[:, None], sign_rule(g), np.float32(0.0)).astype(np.float32)
    done, inliers, moments = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((M, 10))
    if iters == 0:
        with np.errstate(all="ignore"):
            cur = np.where(live[:, None], sign_rule(unit(np.where(live[:, None], g, np.float32(1.0))).astype(np.float32)), cur)
    going = live.copy()
    for _ in range(iters):
        if not going.any():
            break
        step = iterate_once(geo, np.where(going[:, None], cur, np.float32(1.0)), going, sigma, falloff, floor)
        ok = step["ok"]
        cur = np.where(ok[:, None], step["normals"], cur).astype(np.float32)
        moments = np.where(ok[:, None], step["moments"], moments)
        inliers = np.where(ok, step["inliers"], inliers).astype(np.int32)
        done = done + ok.astype(np.int32)
        going = going & ok
    with np.errstate(all="ignore"):
        radius = np.sqrt(geo["r2"]).astype(np.float32)
    return {"normals": cur, "plane": pl, "support": moments[:, 0].astype(np.float32), "inliers": inliers, "iters_done": done,
            "moments": moments, "radius": radius, "count": geo["n"], "geo": geo}


def near_edge(pts, radius):
    """The near-edge rows of the box of ``synth.make_cloud("box", ...)``, as scripts/hough_check.py defines them: closer to a box edge
    (the second-smallest of 1 - |coord|, clipped at 0) than their neighbourhood radius."""
    edge = np.sort(np.clip(1.0 - np.abs(np.asarray(pts, np.float64)), 0.0, None), axis=1)[:, 1]
    return edge < np.asarray(radius, np.float64)
