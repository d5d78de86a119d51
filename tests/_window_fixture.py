"""The fixture of the image-window tests (tests/test_window.py, tests/test_gpu_window.py): the tests' OWN restatement of
``nesti_depth_window_knn`` on the CPU, written from its definition (include/nesti_hip.h, DESIGN.md 2 "Image-window neighbourhoods") in
numpy float64, over the depth fixture's scene and restatement (tests/_depth_fixture.py).

  centre       cloud row i (an index is clamped into the cloud); its pixel p = pix[i], v0 = p // W, u0 = p % W; a p outside [0, H W)
               or a centre that is not finite has count 0 and proven 0
  candidates   the pixels of [u0 - R, u0 + R] x [v0 - R, v0 + R] inside the image whose rank entry j lies in [0, N)
  list         ``_knn_fixture``'s d2 -- (dx dx + dy dy) + dz dz of float64 differences, numpy rounds each operation on its own --, a NaN
               d2 dropped, order = np.lexsort((j, d2)), the first K; -1 / +inf beyond count = min(K, candidates)
  proof        per side with image beyond it: e = (u0 - R) - 0.5 | (u0 + R) + 0.5 (v likewise), a = (e - cx) / fx (cy, fy),
               m_r = T[r, axis] - a * T[r, 2], rel_r = c_r - T[r, 3], s = (m_0 rel_0 + m_1 rel_1) + m_2 rel_2,
               dist = |s| / sqrt(1 + a a); bound = the smallest; no such side: proven; else
               b = max(0, bound (1 - 2^-21) - 2^-21 ((|c_0| + |c_1|) + |c_2|)), proven = count == K and d2[K - 1] < b b

Host only, deterministic; what a test shares is computed once and never changed."""
import numpy as np

import _depth_fixture as D

WINDOW_MAX_R = 15
PAIRS = ((2, 8), (3, 16), (5, 32), (7, 64), (7, 100))      # (R, K); the last: a window too small for K on purpose
INT_MAX = 0x7FFFFFFF
_cache = {}


def frame(kind, crop=None):
    """The depth fixture's frame -- ``'u16'`` without a pose, ``'f32'`` with ``rigid_pose(5)`` -- as (depth, camera dict, the dict of
    ``_depth_fixture.back_project``), computed once.  ``crop`` = (v0, v1, u0, u1): that part of the image, the principal point moved
    with it."""
    key = (kind, crop)
    if key not in _cache:
        depth = D.scene(kind)
        cam = D.camera(kind, pose=D.rigid_pose(5) if kind == "f32" else None)
        if crop is not None:
            v0, v1, u0, u1 = crop
            depth = np.ascontiguousarray(depth[v0:v1, u0:u1])
            cam.update(cx=cam["cx"] - u0, cy=cam["cy"] - v0)
        _cache[key] = (depth, cam, D.back_project(depth, cam))
    return _cache[key]


def _side(c, T, axis, e, c0, f):
    a = (e - c0) / f
    m = [T[r, axis] - a * T[r, 2] for r in range(3)]
    rel = [c[:, r] - T[r, 3] for r in range(3)]
    s = (m[0] * rel[0] + m[1] * rel[1]) + m[2] * rel[2]
    return np.abs(s) / np.sqrt(1.0 + a * a)


def window_knn(xyz, pix, rank, H, W, cam, R, K, rows=None):
    """-> (idx [M,K] int32, d2 [M,K] float64, count [M] int32, proven [M] int32) of the cloud rows ``rows`` (default: all), from the
    float32 cloud ``xyz`` [N,3], ``pix`` [N], ``rank`` [H W] and the camera dict ``cam`` (fx, fy, cx, cy, pose)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    p64 = xyz.astype(np.float64)
    pix, rank = np.asarray(pix, np.int64), np.asarray(rank, np.int64)
    N = len(xyz)
    rows = np.arange(N) if rows is None else np.clip(np.asarray(rows, np.int64), 0, N - 1)
    M = len(rows)
    c = p64[rows]
    p = pix[rows]
    ok = (p >= 0) & (p < H * W) & np.isfinite(c).all(axis=1)
    ps = np.where(ok, p, 0)
    v0, u0 = ps // W, ps % W
    off = np.arange(-R, R + 1)
    dv, du = (g.reshape(-1) for g in np.meshgrid(off, off, indexing="ij"))
    vv, uu = v0[:, None] + dv[None, :], u0[:, None] + du[None, :]
    inside = (vv >= 0) & (vv < H) & (uu >= 0) & (uu < W)
    j = rank[np.clip(vv, 0, H - 1) * W + np.clip(uu, 0, W - 1)]
    valid = inside & (j >= 0) & (j < N) & ok[:, None]
    js = np.where(valid, j, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p64[js] - c[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    valid &= ~np.isnan(d2)
    d2 = np.where(valid, d2, np.inf)
    js = np.where(valid, js, INT_MAX)
    order = np.lexsort((js, d2), axis=-1)
    d2 = np.take_along_axis(d2, order, axis=-1)
    js = np.take_along_axis(js, order, axis=-1)
    cands = valid.sum(axis=1)
    count = np.minimum(K, cands).astype(np.int32)
    idx = np.full((M, K), -1, np.int32)
    d2o = np.full((M, K), np.inf, np.float64)
    w = min(K, js.shape[1])
    keep = np.arange(w)[None, :] < count[:, None]
    idx[:, :w] = np.where(keep, js[:, :w], -1)
    d2o[:, :w] = np.where(keep, d2[:, :w], np.inf)
    # ---- the proof -----------------------------------------------------------------------------------------------------------------
    T = np.asarray(cam["pose"], np.float64) if cam.get("pose") is not None else np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    bound = np.full(M, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for has, axis, e, c0, f in ((u0 - R > 0, 0, (u0 - R).astype(np.float64) - 0.5, cx, fx),
                                    (u0 + R < W - 1, 0, (u0 + R).astype(np.float64) + 0.5, cx, fx),
                                    (v0 - R > 0, 1, (v0 - R).astype(np.float64) - 0.5, cy, fy),
                                    (v0 + R < H - 1, 1, (v0 + R).astype(np.float64) + 0.5, cy, fy)):
            bound = np.where(has, np.minimum(bound, _side(c, T, axis, e, c0, f)), bound)
        covered = np.isinf(bound)
        b = np.maximum(0.0, np.where(covered, 0.0, bound) * (1.0 - 2.0 ** -21) - 2.0 ** -21 * ((np.abs(c[:, 0]) + np.abs(c[:, 1])) + np.abs(c[:, 2])))
        proven = np.where(covered, True, (count == K) & (d2o[:, K - 1] < b * b)) & ok
    return idx, d2o, count, proven.astype(np.int32)


def restated(kind, R, K, crop=None, stride=None):
    """``window_knn`` over ``frame(kind, crop)``, all rows or the rows on ``stride``; computed once."""
    key = ("w", kind, R, K, crop, stride)
    if key not in _cache:
        depth, cam, b = frame(kind, crop)
        rows = None if stride is None else D.back_project(depth, cam, stride)["qidx"]
        H, W = depth.shape
        _cache[key] = window_knn(b["xyz"], b["pix"], b["rank"], H, W, cam, R, K, rows)
    return _cache[key]
