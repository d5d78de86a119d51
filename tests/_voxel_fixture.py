"""The tests' numpy restatement of the voxel downsampling (csrc/voxel.hip; DESIGN.md 2 "Voxel downsampling"): ``np.float64``
operations, one rounding each; the sort is ``np.argsort(kind="stable")``; the sum is an explicit emulation of the 64-lane statement --
64 accumulators, then the xor butterfly --; the representative is the lexicographic minimum of (d2, index).  It predicts every output
bit of ``nesti_voxel_keys``, ``nesti_sort_pairs``, ``nesti_voxel_reduce`` and ``downsample.voxel_downsample``."""
import numpy as np

WAVE = 64


def grid_of(pts, voxel, origin=None):
    """(origin [3] f64, voxel [3] f64, dims [3] python ints, lost key, key bits) of a finite cloud."""
    pts = np.asarray(pts, np.float32)
    voxel = np.broadcast_to(np.asarray(voxel, np.float64), (3,)).copy()
    origin = pts.min(0).astype(np.float64) if origin is None else np.broadcast_to(np.asarray(origin, np.float64), (3,)).copy()
    top = np.floor((pts.max(0).astype(np.float64) - origin) / voxel)
    dims = [max(1, int(t) + 1) for t in top]
    lost = dims[0] * dims[1] * dims[2]
    assert lost < 1 << 62
    return origin, voxel, dims, lost, lost.bit_length()


def keys(pts, origin, voxel, dims):
    """key [N] uint64: (i_z dims_y + i_y) dims_x + i_x with i = floor(((double)p - origin) / voxel); the lost key dims_x dims_y dims_z
    for a row with a non-finite coordinate or a cell outside [0, dims)."""
    pts = np.asarray(pts, np.float32)
    origin, voxel = np.asarray(origin, np.float64), np.asarray(voxel, np.float64)
    lost = int(dims[0]) * int(dims[1]) * int(dims[2])
    with np.errstate(all="ignore"):
        d = pts.astype(np.float64) - origin
        t = d / voxel
        f = np.floor(t)
    ok = np.isfinite(pts).all(1) & ((f >= 0.0) & (f < 9223372036854775808.0)).all(1)
    i = np.zeros(f.shape, np.int64)
    i[ok] = f[ok].astype(np.int64)
    ok &= (i < np.asarray([int(x) for x in dims], np.int64)).all(1)
    i = i.astype(np.uint64)
    key = (i[:, 2] * np.uint64(dims[1]) + i[:, 1]) * np.uint64(dims[0]) + i[:, 0]
    key[~ok] = np.uint64(lost)
    return key


def sort_pairs(key, key_bits):
    """(sorted keys, idx int32): the stable argsort of the low ``key_bits`` bits; the keys are carried whole."""
    key = np.asarray(key, np.uint64)
    mask = np.uint64((1 << key_bits) - 1)
    idx = np.argsort(key & mask, kind="stable")
    return key[idx], idx.astype(np.int32)


def lane_sum(d, group=WAVE):
    """The sum of ``d`` [count] (or [count, C]) float64 in the order of the statement: slot s is added in lane s mod 64, a lane's slots
    ascending from +0.0, the lanes meet in the xor butterfly 32 .. 1.  ``group`` = 16 or 32: the emulation of a lane group that holds
    64 / group accumulators per lane, met as (a0 + a2) + (a1 + a3) (16) or a0 + a1 (32), then the butterfly group / 2 .. 1."""
    d = np.asarray(d, np.float64)
    tail = d.shape[1:]
    acc = np.zeros((WAVE,) + tail, np.float64)
    for s in range(len(d)):                                   # explicit: one addition per slot, in slot order
        acc[s % WAVE] = acc[s % WAVE] + d[s]
    if group == WAVE:
        v = acc
    elif group == 32:
        v = acc[:32] + acc[32:]
    else:
        assert group == 16
        a0, a1, a2, a3 = acc[:16], acc[16:32], acc[32:48], acc[48:]
        v = (a0 + a2) + (a1 + a3)
    off = len(v) // 2
    while off:
        v = v + v[np.arange(len(v)) ^ off]
        off //= 2
    return v[0]


def _lane_sums(d, begin, count):
    """``lane_sum`` of every run d[begin[v] : begin[v] + count[v]] ([*, 3]) at once: the runs of equal trip count share the additions."""
    out = np.zeros((len(begin), d.shape[1]), np.float64)
    trips = (count + WAVE - 1) // WAVE
    lanes = np.arange(WAVE)
    for t in np.unique(trips):
        sel = np.flatnonzero(trips == t)
        acc = np.zeros((len(sel), WAVE, d.shape[1]), np.float64)
        for j in range(int(t)):
            s = j * WAVE + lanes[None, :]                     # [1, 64] slots
            live = s < count[sel, None]
            rows = np.where(live, begin[sel, None] + s, 0)
            term = np.where(live[..., None], d[rows], 0.0)    # an idle lane adds +0.0: no bit changes (the accumulators are never -0)
            acc = acc + term
        off = WAVE // 2
        while off:
            acc = acc + acc[:, lanes ^ off]
            off //= 2
        out[sel] = acc[:, 0]
    return out


def reduce(pts, skeys, sidx, lost, origin):
    """The voxels of sorted (key, row) pairs -> dict of centroid [V,3] f32, rep [V] int32, count [V] int32, key [V] uint64,
    voxel_of [N] int32 and V."""
    pts = np.asarray(pts, np.float32)
    skeys, sidx = np.asarray(skeys, np.uint64), np.asarray(sidx, np.int64)
    origin = np.asarray(origin, np.float64)
    N = len(skeys)
    live = skeys != np.uint64(lost)
    head = live & np.concatenate([[True], skeys[1:] != skeys[:-1]])
    begin = np.flatnonzero(head)
    V = len(begin)
    n_live = int(live.sum())
    count = np.diff(np.concatenate([begin, [n_live]])).astype(np.int64)
    voxel_of = np.full(N, -1, np.int32)
    voxel_of[sidx[live]] = (np.cumsum(head) - 1)[live].astype(np.int32)
    with np.errstate(all="ignore"):
        d = pts[sidx].astype(np.float64) - origin             # in sorted order; the lost rows are never read
    d[~live] = 0.0
    S = _lane_sums(d, begin, count)
    m = S / count[:, None].astype(np.float64)
    centroid = (origin + m).astype(np.float32)
    rep = np.zeros(V, np.int32)
    e = d[:n_live] - np.repeat(m, count, axis=0)
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    for v in range(V):                                        # the rows of a voxel ascend in index: the first minimum is the lowest index
        rep[v] = sidx[begin[v] + int(np.argmin(d2[begin[v]:begin[v] + count[v]]))]
    return {"centroid": centroid.reshape(-1, 3), "rep": rep, "count": count.astype(np.int32), "key": skeys[begin], "voxel_of": voxel_of, "V": V}


def downsample(pts, voxel, mode="centroid", origin=None):
    """``downsample.voxel_downsample`` restated: the same dict."""
    pts = np.ascontiguousarray(pts, np.float32)
    origin, voxel, dims, lost, bits = grid_of(pts, voxel, origin)
    key = keys(pts, origin, voxel, dims)
    sk, si = sort_pairs(key, bits)
    r = reduce(pts, sk, si, lost, origin)
    rep = r["rep"].astype(np.int64)
    k = r["key"]
    dx, dy = np.uint64(dims[0]), np.uint64(dims[1])
    cell = np.stack([k % dx, (k // dx) % dy, k // (dx * dy)], axis=1).astype(np.int64).reshape(-1, 3)
    return {"points": r["centroid"] if mode == "centroid" else pts[rep], "centroid": r["centroid"], "rep": rep, "count": r["count"], "key": k,
            "cell": cell, "voxel_of": r["voxel_of"].astype(np.int64), "origin": origin, "voxel": voxel, "dims": np.asarray(dims, np.int64)}
