"""The fixture of the outlier-filter tests (tests/test_outliers.py, tests/test_gpu_outliers.py): the tests' OWN restatement of
``nesti_outlier_scores_nbr``, ``nesti_outlier_threshold``, ``nesti_outlier_compact`` and ``outliers.remove_outliers`` on the CPU, written
from their definition (DESIGN.md 2 "Outlier removal", include/nesti_hip.h) in numpy, scalar by scalar in the stated order.  float64
throughout; numpy rounds every operation on its own, as the kernels do.

  search     brute force: d = float64(p) - float64(c); d2 = (dx dx + dy dy) + dz dz; the K smallest (d2, index) pairs ascending; a NaN d2
             is never a neighbour; -1 beyond the count
  scores     P = min(k + 1, valid prefix) (the prefix ends at the first entry outside [0, N)); the first slot below P whose INDEX is the
             row's own is skipped, else the slots below min(k, P) are used; lane l = slot mod ``lanes`` adds sqrt(d2) of its used slots
             in ascending order from +0.0; the lanes meet in the xor-butterfly lanes / 2, ..., 1; mean = sum / n_other (+inf for 0);
             kth_d2 = max d2 used where n_other == k, else +inf; a NaN sum or a non-finite centre: the quiet NaN (n_other 0 for the centre)
  threshold  a non-finite score is absent (value +0, count 0); blocks of 256 by stride halving; thread t of the final 256 adds partials
             t, t + 256, ... to +0.0, then stride halving; mean = S / n; Q over (s - mean)^2 by the same tree; std = sqrt(Q / (n - 1))
  compact    kept iff finite and <= thr

Host only, deterministic."""
import numpy as np

WAVE, BLOCK = 64, 256


def d2_to(p64, c64):
    D = p64[None, :, :] - c64[:, None, :]
    return (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]


def knn_brute(pts, K, rows=None, chunk=512):
    """The K smallest (d2, index) pairs of the rows (default: all): idx [M,K] int32, -1 beyond the count of non-NaN d2."""
    p64 = np.ascontiguousarray(pts, dtype=np.float32).astype(np.float64)
    rows = np.arange(len(p64)) if rows is None else np.asarray(rows, np.int64)
    out = np.full((len(rows), K), -1, np.int32)
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        with np.errstate(all="ignore"):
            d2 = d2_to(p64, p64[r])
        order = np.argsort(d2, axis=1, kind="stable")[:, :K]                # stable: equal d2 by ascending index; NaN last
        ok = ~np.isnan(np.take_along_axis(d2, order, 1))
        out[a:a + chunk, :order.shape[1]] = np.where(ok, order, -1)
    return out


def butterfly(part):
    """The xor-butterfly of L partial sums [..., L]: offsets L / 2, ..., 1; lane 0's total."""
    L = part.shape[-1]
    lanes = np.arange(L)
    off = L // 2
    while off:
        part = part + part[..., lanes ^ off]
        off //= 2
    return part[..., 0]


def scores(pts, row0, nbr, k, lanes=WAVE):
    """Rows row0 .. row0 + M of the cloud over the lists ``nbr`` [M,K>k] -> dict of mean [M] f64, kth_d2 [M] f64, n_other [M] int32."""
    p64 = np.ascontiguousarray(pts, dtype=np.float32).astype(np.float64)
    nbr = np.asarray(nbr, np.int64)
    N, M = len(p64), len(nbr)
    assert 1 <= k < nbr.shape[1] and lanes in (16, 32, 64) and (lanes == WAVE or k + 1 <= lanes) and row0 >= 0 and row0 + M <= N
    own = row0 + np.arange(M)
    c64 = p64[own]
    lost = ~np.isfinite(c64).all(1)
    head = nbr[:, :k + 1]
    bad = (head < 0) | (head >= N)
    P = np.where(bad.any(1), bad.argmax(1), k + 1)
    P = np.where(lost, 0, P)
    slot = np.arange(k + 1)[None, :]
    is_own = (head == own[:, None]) & (slot < P[:, None])
    found = is_own.any(1)
    self_slot = np.where(found, is_own.argmax(1), -1)
    limit = np.where(found, P, np.minimum(k, P))
    used = (slot < limit[:, None]) & (slot != self_slot[:, None])
    n_other = used.sum(1).astype(np.int32)
    assert np.array_equal(n_other, np.where(found, P - 1, limit))
    J = np.clip(head, 0, N - 1)
    with np.errstate(all="ignore"):
        D = p64[J] - c64[:, None, :]
        d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
        term = np.sqrt(d2)
        trips = -(-(k + 1) // lanes)
        pad_t = np.zeros((M, trips * lanes))
        pad_u = np.zeros((M, trips * lanes), bool)
        pad_t[:, :k + 1] = term
        pad_u[:, :k + 1] = used
        pad_t, pad_u = pad_t.reshape(M, trips, lanes), pad_u.reshape(M, trips, lanes)
        part = np.zeros((M, lanes))
        for s in range(trips):                                                # lane l adds slots l, l + lanes, ... ascending
            part = np.where(pad_u[:, s], part + pad_t[:, s], part)
        total = butterfly(part)
        top = np.fmax.reduce(np.where(used, d2, 0.0), axis=1, initial=0.0)
        mean = np.where(n_other > 0, total / np.maximum(n_other, 1).astype(np.float64), np.inf)
    kth = np.where(n_other == k, top, np.inf)
    nan = lost | np.isnan(total)
    mean = np.where(nan, np.nan, mean)
    kth = np.where(nan, np.nan, kth)
    n_other = np.where(lost, 0, n_other).astype(np.int32)
    return {"mean": mean.astype(np.float64), "kth_d2": kth.astype(np.float64), "n_other": n_other}


def _halving(v):
    """[rows, 256] -> [rows]: v[t] = v[t] + v[t + s] for s = 128, 64, ..., 1."""
    v = v.copy()
    s = BLOCK // 2
    while s:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s //= 2
    return v[:, 0]


def tree_sum(vals):
    """The fixed tree of nesti_outlier_threshold over [M] values (absent ones already +0)."""
    vals = np.asarray(vals, np.float64)
    nb = -(-len(vals) // BLOCK)
    padded = np.zeros(nb * BLOCK)
    padded[:len(vals)] = vals
    partial = _halving(padded.reshape(nb, BLOCK))
    rounds = -(-nb // BLOCK)
    p2 = np.zeros(rounds * BLOCK)
    present = np.zeros(rounds * BLOCK, bool)
    p2[:nb] = partial
    present[:nb] = True
    p2, present = p2.reshape(rounds, BLOCK), present.reshape(rounds, BLOCK)
    acc = np.zeros(BLOCK)
    for r in range(rounds):                                                   # thread t: partials t, t + 256, ... ascending, to +0.0
        acc = np.where(present[r], acc + p2[r], acc)
    return _halving(acc[None, :])[0]


def threshold(sc, std_ratio):
    """[M] f64 scores -> stats [4] f64: n, mean, std, thr."""
    sc = np.asarray(sc, np.float64)
    present = np.isfinite(sc)
    n = int(present.sum())
    with np.errstate(all="ignore"):
        S = tree_sum(np.where(present, sc, 0.0))
        if n == 0:
            return np.array([0.0, 0.0, 0.0, np.inf])
        mean = S / np.float64(n)
        e = np.where(present, sc, mean) - mean
        Q = tree_sum(np.where(present, e * e, 0.0))
        std = np.sqrt(Q / np.float64(n - 1)) if n >= 2 else np.float64(0.0)
        scaled = np.float64(std_ratio) * std
        thr = mean + scaled
    return np.array([np.float64(n), mean, std, thr])


def compact(pts, sc, thr):
    """-> dict of xyz [n_kept,3] f32, kept_idx [n_kept] int32, new_of_old [N] int32, keep [N] uint8, n_kept."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    sc = np.asarray(sc, np.float64)
    with np.errstate(all="ignore"):
        keep = np.isfinite(sc) & (sc <= np.float64(thr))
    kept = np.flatnonzero(keep).astype(np.int32)
    new_of_old = np.full(len(sc), -1, np.int32)
    new_of_old[kept] = np.arange(len(kept), dtype=np.int32)
    return {"xyz": pts[kept], "kept_idx": kept, "new_of_old": new_of_old, "keep": keep.astype(np.uint8), "n_kept": len(kept)}


def remove(pts, mode="statistical", k=16, std_ratio=1.0, radius=None, min_neighbours=None, passes=1):
    """``outliers.remove_outliers`` restated with the brute-force search: dict of points, kept (int64), inlier, score, passes."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    N = len(pts)
    kk = k if mode == "statistical" else (k if min_neighbours is None else min_neighbours)
    cur, kept, score, log = pts, np.arange(N, dtype=np.int64), np.zeros(N), []
    for _ in range(passes):
        n = len(cur)
        if n == 0:
            break
        s = scores(cur, 0, knn_brute(cur, kk + 1), kk)
        if mode == "statistical":
            sc = s["mean"]
            st = threshold(sc, std_ratio)
            thr = st[3]
        else:
            sc = s["kth_d2"]
            thr = np.float64(radius) * np.float64(radius)
        c = compact(cur, sc, thr)
        score[kept] = sc
        if mode == "statistical":
            log.append({"n": int(st[0]), "mean": float(st[1]), "std": float(st[2]), "threshold": float(st[3]), "removed": n - c["n_kept"]})
        else:
            log.append({"n": n, "mean": None, "std": None, "threshold": float(thr), "removed": n - c["n_kept"]})
        kept = kept[c["kept_idx"].astype(np.int64)]
        cur = c["xyz"]
        if not len(cur):
            break
    inlier = np.zeros(N, bool)
    inlier[kept] = True
    return {"points": cur, "kept": kept, "inlier": inlier, "score": score, "passes": log}


# ---- the clouds of the filter tests -------------------------------------------------------------------------------------------------------
def noisy_cloud(shape, seed, n=2000, n_out=100):
    """``shape`` at ``n`` points (synth.make_cloud, no noise) plus ``n_out`` points drawn uniformly in its bounding box, shuffled
    (seeded): (pts [n + n_out,3] f32, injected [n + n_out] bool, clean [n,3] f32)."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    clean, _ = synth.make_cloud(shape, n=n, seed=seed)
    rs = np.random.RandomState(1000 + seed)
    lo, hi = clean.min(0), clean.max(0)
    extra = (lo + rs.rand(n_out, 3) * (hi - lo)).astype(np.float32)
    allp = np.concatenate([clean, extra])
    flag = np.concatenate([np.zeros(n, bool), np.ones(n_out, bool)])
    perm = rs.permutation(n + n_out)
    return np.ascontiguousarray(allp[perm]), flag[perm], clean


FILTER_CLOUDS = (("box", 1), ("torus", 2), ("ellipsoid", 1))


def scatter(rows, kept, n, fill=0):
    rows = np.asarray(rows)
    out = np.full((n,) + rows.shape[1:], fill, dtype=rows.dtype)
    out[np.asarray(kept, np.int64)] = rows
    return out
