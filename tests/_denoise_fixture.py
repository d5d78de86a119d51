"""The fixture of the point-denoising tests (tests/test_denoise.py, tests/test_gpu_denoise.py): the tests' OWN restatement of one pass of
``nesti_denoise_points_nbr`` on the CPU, written from its definition (DESIGN.md 2 "Point denoising", include/nesti_hip.h) in numpy,
vectorised over rows, scalar by scalar in the stated order.  float64 throughout; numpy rounds every operation on its own, as the kernel
does.

  lists        the valid prefix of a row ends at its first entry outside [0, N); n = min(k, prefix); a non-finite centre position has
               an empty prefix; d = float64(p) - float64(c); d2 = (dx dx + dy dy) + dz dz; r2 = max d2 over the prefix; rad = sqrt(r2)
  eligibility  on the bits: three finite components, one of them non-zero
  centre       v = float64(n_c) / sqrt(q_c), component by component
  slot         dd = (cx jx + cy jy) + cz jz; ca = |dd| / sqrt(qc qj); t = (ca - cos_t) / (1 - cos_t); t > 0 or nothing; t = min(t, 1);
               u = 1 - (falloff d2) / r2 (1 where r2 = 0); h = (vx dx + vy dy) + vz dz; x = h / (sigma rad) (0 where r2 = 0);
               g = 1 / (1 + x x); a = (u t) g; W = a a; the slot adds W h to H, W to Wsum and 1 to the count
  sums         lane l = slot mod ``lanes`` adds its slots in ascending order from +0.0; the partial sums meet in the xor-butterfly
               lanes / 2, ..., 1 (``lanes`` = 64: the statement; 16 or 32: a lane group, for k <= lanes)
  result       delta = step (H / Wsum) where Wsum > 0 and delta is finite: float32(float64(p_c) + delta v) per component, the product
               and the sum rounded separately; the input row, and delta 0, otherwise

It takes a list, so it needs no search of its own.  Host only, deterministic."""
import numpy as np

WAVE = 64


def eligible(normals):
    """[..., 3] float32 -> bool [...]: three finite components and one non-zero, on the bits."""
    bits = np.ascontiguousarray(normals, dtype=np.float32).view(np.uint32)
    finite = (bits & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
    nonzero = (bits & np.uint32(0x7fffffff)) != 0
    return finite.all(-1) & nonzero.any(-1)


def prefixes(N, centres, nbr, k):
    """n [M]: min(k, valid prefix) of every row; 0 for a non-finite centre position."""
    nbr = np.asarray(nbr, np.int64)[:, :k]
    bad = (nbr < 0) | (nbr >= N)
    valid = np.where(bad.any(1), bad.argmax(1), nbr.shape[1])
    return np.where(np.isfinite(np.asarray(centres, np.float64)).all(1), valid, 0)


def butterfly(part):
    """The xor-butterfly of L partial sums [..., L]: offsets L / 2, ..., 1; lane 0's total."""
    L = part.shape[-1]
    lanes = np.arange(L)
    off = L // 2
    while off:
        part = part + part[..., lanes ^ off]
        off //= 2
    return part[..., 0]


def _sq(x, y, z):
    return (x * x + y * y) + z * z


def restate(pts, normals, centres, nbr, k, cos_t, falloff, sigma, step, lanes=WAVE):
    """One pass over the rows whose centres are the cloud points ``centres`` [M] (indices) with lists ``nbr`` [M,K] -> dict of
    points [M,3] f32, delta [M] f32, support [M] f32, count [M] int32."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    centres = np.asarray(centres, np.int64).reshape(-1)
    nbr = np.asarray(nbr, np.int64)
    N, M = len(pts), len(centres)
    assert normals.shape == (N, 3) and nbr.shape[0] == M and 1 <= k <= nbr.shape[1] and lanes in (16, 32, 64) and (lanes == WAVE or k <= lanes)
    cos_t, falloff, sigma, step = np.float64(cos_t), np.float64(falloff), np.float64(sigma), np.float64(step)
    out = {"points": pts[centres].copy(), "delta": np.zeros(M, np.float32), "support": np.zeros(M, np.float32),
           "count": np.zeros(M, np.int32)}
    if M == 0:
        return out
    p64, n64 = pts.astype(np.float64), normals.astype(np.float64)
    c64 = p64[centres]
    nc = n64[centres]                                                                           # [M,3]
    live = eligible(normals[centres])
    n = np.where(live, prefixes(N, c64, nbr, k), 0)
    J = np.clip(nbr[:, :k], 0, N - 1)                                                           # slots beyond the prefix are unused
    used = np.arange(k)[None, :] < n[:, None]
    with np.errstate(all="ignore"):
        D = p64[J] - c64[:, None, :]
        d2 = _sq(D[..., 0], D[..., 1], D[..., 2])
        r2 = np.where(used, d2, 0.0).max(1)
        rad = np.sqrt(r2)
        nj = n64[J]                                                                             # [M,k,3]
        qc = _sq(nc[:, 0], nc[:, 1], nc[:, 2])
        v = nc / np.sqrt(qc)[:, None]                                                           # [M,3], component by component
        qj = _sq(nj[..., 0], nj[..., 1], nj[..., 2])
        dd = (nc[:, None, 0] * nj[..., 0] + nc[:, None, 1] * nj[..., 1]) + nc[:, None, 2] * nj[..., 2]
        ca = np.abs(dd) / np.sqrt(qc[:, None] * qj)
        t = (ca - cos_t) / (np.float64(1.0) - cos_t)
        take = used & eligible(normals[J]) & (t > 0.0)
        t = np.minimum(t, 1.0)
        some = r2[:, None] > 0.0
        u = np.where(some, 1.0 - (falloff * d2) / r2[:, None], 1.0)
        h = (v[:, None, 0] * D[..., 0] + v[:, None, 1] * D[..., 1]) + v[:, None, 2] * D[..., 2]
        x = np.where(some, h / (sigma * rad)[:, None], 0.0)
        g = 1.0 / (1.0 + x * x)
        a = (u * t) * g
        W = a * a
        terms = np.stack([W * h, W], -1)                                                        # [M,k,2]
    terms = np.where(take[..., None], terms, 0.0)
    trips = -(-k // lanes)
    padded = np.zeros((M, trips * lanes, 2))
    padded[:, :k] = terms
    took = np.zeros((M, trips * lanes), bool)
    took[:, :k] = take
    padded, took = padded.reshape(M, trips, lanes, 2), took.reshape(M, trips, lanes)
    part = np.zeros((M, lanes, 2))
    for s in range(trips):                                                                      # lane l adds slots l, l + lanes, ... ascending;
        part = np.where(took[:, s, :, None], part + padded[:, s], part)                         # a slot that adds nothing is no addition
    H, Wsum = (butterfly(part[..., c]) for c in range(2))
    with np.errstate(all="ignore"):
        delta = step * (H / Wsum)
        good = (n > 0) & (Wsum > 0.0) & np.isfinite(delta)
        moved = (c64 + delta[:, None] * v).astype(np.float32)
    out["points"][good] = moved[good]
    out["delta"] = np.where(good, delta, 0.0).astype(np.float32)
    out["support"] = np.where(n > 0, Wsum, 0.0).astype(np.float32)
    out["count"] = np.where(n > 0, take.sum(1), 0).astype(np.int32)
    return out


def iterate(pts, normals, nbr_of, k, cos_t, falloff, sigma, step, iters, lanes=WAVE):
    """``iters`` passes over ALL cloud points with a FIXED normal field: every pass reads the previous one's positions and the lists
    ``nbr_of(points)`` [N,K >= k] of those positions; delta, support and count are the last pass's."""
    assert iters >= 1
    out = None
    cur = np.ascontiguousarray(pts, dtype=np.float32)
    for _ in range(iters):
        out = restate(cur, normals, np.arange(len(cur)), nbr_of(cur), k, cos_t, falloff, sigma, step, lanes)
        cur = out["points"]
    return out
