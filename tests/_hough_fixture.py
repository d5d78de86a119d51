"""The fixture of the Hough-transform tests (tests/test_hough.py, tests/test_gpu_hough.py): the tests' OWN restatement of the estimator
on the CPU, written from its definition (DESIGN.md 2 "Hough-transform normals", include/nesti_hip.h) in numpy, vectorised over rows and
triplets.  float64 throughout; numpy rounds every operation on its own, as the kernel does.

  lists     the valid prefix of a row ends at its first entry outside [0, N); n_s = min(k_s, prefix); a non-finite centre has an empty
            prefix; d = float64(p) - float64(c); r2_s = max (dx dx + dy dy) + dz dz over the prefix
  hash      the subsample key: the splitmix64 finaliser over seed ^ (q << 34) ^ (scale << 32) ^ index in np.uint64, upper 32 bits
  triplets  i0 = (h0 n) >> 32; j = (h1 (n - 1)) >> 32, i1 = j + (j >= i0); lo, hi = min, max; j = (h2 (n - 2)) >> 32, j += (j >= lo),
            i2 = j + (j >= hi)
  votes     hemi-octahedral bins per rotation, integer counts; the winner is the first largest count in (rho, bin) order
  normal    lane l = t mod 64 adds its triplets in ascending t; the 64 partial sums meet in the xor-butterfly 32, 16, ..., 1

It takes a list, so it needs no search of its own.  Host only, deterministic."""
import numpy as np

WAVE = 64
MAX_T, MAX_BINS, MAX_ROT = 4096, 16, 8
_U = np.uint64


def subsample_hash(seed, q, s, idx):
    """Upper 32 bits of the splitmix64 finaliser over (seed, q, s, idx); arrays broadcast, all np.uint64."""
    seed, q, s, idx = (np.asarray(v).astype(np.uint64) for v in (seed, q, s, idx))
    with np.errstate(over="ignore"):
        z = seed ^ (q << _U(34)) ^ (s << _U(32)) ^ idx
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        z = z ^ (z >> _U(31))
    return z >> _U(32)


def triplet_indices(seed, key, n, T):
    """(i0, i1, i2) [M,T] int64 of key rows ``key`` [M] over prefixes ``n`` [M] (>= 3)."""
    key = np.asarray(key).astype(np.uint64)[:, None]
    n = np.asarray(n).astype(np.uint64)[:, None]
    t3 = _U(3) * np.arange(T, dtype=np.uint64)[None, :]
    h0, h1, h2 = (subsample_hash(_U(seed), key, _U(0), t3 + _U(c)) for c in range(3))
    i0 = ((h0 * n) >> _U(32)).astype(np.int64)
    j = ((h1 * (n - _U(1))) >> _U(32)).astype(np.int64)
    i1 = j + (j >= i0)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    j = ((h2 * (n - _U(2))) >> _U(32)).astype(np.int64)
    j = j + (j >= lo)
    i2 = j + (j >= hi)
    return i0, i1, i2


def prefixes(N, centres, nbr, ks):
    """n [M,S]: min(k_s, valid prefix) of every row; 0 for a non-finite centre."""
    nbr = np.asarray(nbr, np.int64)
    bad = (nbr < 0) | (nbr >= N)
    valid = np.where(bad.any(1), bad.argmax(1), nbr.shape[1])
    valid = np.where(np.isfinite(np.asarray(centres, np.float64)).all(1), valid, 0)
    return np.minimum(np.asarray(ks, np.int64)[None, :], valid[:, None])


def sign_of(wx, wy, wz):
    """-1 where the first non-zero of (wz, wy, wx) is negative, else +1."""
    lead = np.where(wz != 0.0, wz, np.where(wy != 0.0, wy, wx))
    return np.where(lead < 0.0, -1.0, 1.0)


def bins_of(rot, u, B):
    """Step 3 under one rotation ``rot`` [9]: (bin [M,T] int64, sigma [M,T])."""
    ux, uy, uz = u
    wx = (rot[0] * ux + rot[1] * uy) + rot[2] * uz
    wy = (rot[3] * ux + rot[4] * uy) + rot[5] * uz
    wz = (rot[6] * ux + rot[7] * uy) + rot[8] * uz
    sg = sign_of(wx, wy, wz)
    wx, wy, wz = sg * wx, sg * wy, sg * wz
    m = (np.abs(wx) + np.abs(wy)) + wz
    a, b = wx / m, wy / m
    half = B / 2.0
    with np.errstate(invalid="ignore"):
        bi = np.clip(np.nan_to_num(np.floor(((a + b) + 1.0) * half)), 0, B - 1).astype(np.int64)
        bj = np.clip(np.nan_to_num(np.floor(((a - b) + 1.0) * half)), 0, B - 1).astype(np.int64)
    return bi * B + bj, sg


def wave_sum(part):
    """The xor-butterfly of 64 partial sums [..., 64]: offsets 32, 16, ..., 1; every lane ends with the total."""
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off:
        part = part + part[..., lanes ^ off]
        off //= 2
    return part[..., 0]


def restate(pts, centres, nbr, ks, T, B, R, rot, seed, row0=0):
    """The estimator over the lists ``nbr`` [M,K] of float32 ``centres`` [M,3] -> dict of normals [M,S,3] f32, conf [M,S] f32, votes
    [M,S,2] int32, radius [M,S] f32, count [M,S] int32."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    centres = np.ascontiguousarray(centres, dtype=np.float32).reshape(-1, 3)
    nbr = np.asarray(nbr, np.int64)
    rot = np.asarray(rot, np.float64).reshape(-1, 9)[:R]
    N, M, S = len(pts), len(centres), len(ks)
    c64 = centres.astype(np.float64)
    ns = prefixes(N, c64, nbr, ks)
    out = {"normals": np.zeros((M, S, 3), np.float32), "conf": np.zeros((M, S), np.float32), "votes": np.zeros((M, S, 2), np.int32),
           "radius": np.zeros((M, S), np.float32), "count": ns.astype(np.int32)}
    if M == 0:
        return out
    rows = np.arange(M)[:, None]
    with np.errstate(all="ignore"):
        D = pts.astype(np.float64)[np.clip(nbr, 0, N - 1)] - c64[:, None, :]                # [M,K,3]; slots beyond the prefix unused
    d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    slot = np.arange(nbr.shape[1])[None, :]
    key = row0 + np.arange(M)
    Tp = -(-T // WAVE) * WAVE
    for s in range(S):
        n = ns[:, s]
        out["radius"][:, s] = np.sqrt(np.where(slot < n[:, None], d2, 0.0).max(1)).astype(np.float32)
        live = n >= 3
        i0, i1, i2 = triplet_indices(seed, key, np.maximum(n, 3), T)
        with np.errstate(all="ignore"):
            d0, d1, dd2 = D[rows, np.minimum(i0, nbr.shape[1] - 1)], D[rows, np.minimum(i1, nbr.shape[1] - 1)], D[rows, np.minimum(i2, nbr.shape[1] - 1)]
            e1, e2 = d1 - d0, dd2 - d0
            vx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
            vy = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
            vz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
            l1 = (e1[..., 0] * e1[..., 0] + e1[..., 1] * e1[..., 1]) + e1[..., 2] * e1[..., 2]
            l2 = (e2[..., 0] * e2[..., 0] + e2[..., 1] * e2[..., 1]) + e2[..., 2] * e2[..., 2]
            qq = (vx * vx + vy * vy) + vz * vz
            ok = (qq > 2.0 ** -20 * (l1 * l2)) & live[:, None]
            ln = np.sqrt(qq)
            u = (vx / ln, vy / ln, vz / ln)
            counts = np.zeros((M, R, B * B), np.int64)
            binned, sigmas = [], []
            for r in range(R):
                b, sg = bins_of(rot[r], u, B)
                binned.append(b)
                sigmas.append(sg)
                np.add.at(counts[:, r, :], (np.broadcast_to(rows, b.shape)[ok], b[ok]), 1)
        valid = ok.sum(1)
        flat = counts.reshape(M, R * B * B)
        best = flat.argmax(1)                                   # the first largest: the smaller rho, then the smaller bin
        win = flat[np.arange(M), best]
        rho, wbin = best // (B * B), best % (B * B)
        b_star = np.stack(binned, 0)[rho, np.arange(M)]         # [M,T]
        s_star = np.stack(sigmas, 0)[rho, np.arange(M)]
        take = ok & (b_star == wbin[:, None])
        with np.errstate(all="ignore"):
            contrib = np.stack([np.where(take, s_star * c, 0.0) for c in u], -1)           # [M,T,3]
        padded = np.zeros((M, Tp, 3))
        padded[:, :T] = contrib
        trips = padded.reshape(M, Tp // WAVE, WAVE, 3)
        part = np.zeros((M, WAVE, 3))
        for k in range(trips.shape[1]):                         # lane l adds t = l, l + 64, ... in ascending order
            part = part + trips[:, k]
        X, Y, Z = (wave_sum(part[..., c]) for c in range(3))
        with np.errstate(all="ignore"):
            nn = (X * X + Y * Y) + Z * Z
            good = (win > 0) & (nn > 0.0) & np.isfinite(nn)
            ln = np.sqrt(nn)
            nrm = np.stack([X / ln, Y / ln, Z / ln], -1).astype(np.float32)
        lead = np.where(nrm[:, 2] != 0, nrm[:, 2], np.where(nrm[:, 1] != 0, nrm[:, 1], nrm[:, 0]))
        nrm = np.where((lead < 0)[:, None], -nrm, nrm) + np.float32(0.0)
        out["normals"][:, s] = np.where(good[:, None], nrm, np.float32(0.0))
        win = np.where(good, win, 0)
        with np.errstate(all="ignore"):
            out["conf"][:, s] = np.where(good, (win.astype(np.float64) / valid.astype(np.float64)), 0.0).astype(np.float32)
        out["votes"][:, s, 0], out["votes"][:, s, 1] = win, valid
    return out
