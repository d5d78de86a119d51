"""Outlier removal before estimation on the GPU (``csrc/outlier.hip``; DESIGN.md 2 "Outlier removal"): the statistical filter -- a point
leaves when the mean distance to its ``k`` nearest other points exceeds the cloud's mean of that figure by ``std_ratio`` standard
deviations (Rusu et al. 2008) -- and the radius filter -- a point leaves when fewer than ``min_neighbours`` other points lie within
``radius``.  Both are one pass over the sorted lists of ``nesti_knn``, the statistics and an ordered compaction on the device.  Every
estimator takes the filter as ``outliers=`` (``pca.pca_normals``, ``quadric.quadric_fit``, ``hough.hough_normals``,
``robust.robust_normals``, ``select.select_normals``, ``NormalEstimator.estimate`` / ``estimate_depth``; ``--outliers`` on the command
line): it then runs on the filtered cloud and its per-row results come back with the rows of the input, the removed ones holding a fill.
The conventions are the library's own (no parity with any published code is claimed).  There is no CPU fallback."""
import collections
import math

import numpy as np

from . import _lib
from ._args import int_in as _int_in, number as _number
from .stages import FILLS, inverse, take_result, take_rows

MODES = ("statistical", "radius")
DEFAULT_K, DEFAULT_STD_RATIO, DEFAULT_PASSES = 16, 1.0, 1
MAX_K = _lib.KNN_MAX_K - 1             # nesti_outlier_scores_nbr: 1 <= k < K <= NESTI_KNN_MAX_K
MAX_PASSES = 8
KEYS = ("mode", "k", "std_ratio", "radius", "min_neighbours", "passes")

# mode; k (statistical: the neighbours of the mean; radius: what min_neighbours defaults to); std_ratio (statistical); radius and
# min_neighbours (radius mode, else None); passes
Params = collections.namedtuple("Params", KEYS)


def check_k(k):
    """A count of OTHER points in 1 .. 255 as an int; ``ValueError`` otherwise."""
    return _int_in("k", k, 1, MAX_K)


def check_std_ratio(std_ratio):
    """``std_ratio`` finite and >= 0 as a float; ``ValueError`` otherwise."""
    f = _number("std_ratio", std_ratio)
    if f < 0.0:
        raise ValueError("std_ratio must be >= 0: got %r" % (std_ratio,))
    return f


def check_threshold(thr):
    """A host threshold of ``nesti_outlier_compact``, finite and >= 0, as a float; ``ValueError`` otherwise."""
    f = _number("thr", thr)
    if f < 0.0:
        raise ValueError("thr must be >= 0: got %r" % (thr,))
    return f


def check_params(mode="statistical", k=DEFAULT_K, std_ratio=DEFAULT_STD_RATIO, radius=None, min_neighbours=None, passes=DEFAULT_PASSES):
    """The one place where the ranges are checked -> ``Params``; ``ValueError`` otherwise.  ``mode`` 'statistical': ``k`` in 1 .. 255,
    ``std_ratio`` finite and >= 0; ``radius`` and ``min_neighbours`` must be None.  ``mode`` 'radius': ``radius`` finite and > 0 (in the
    cloud's units) whose square is finite, ``min_neighbours`` in 1 .. 255 (None: ``k``).  ``passes`` in 1 .. 8."""
    if mode not in MODES:
        raise ValueError("mode must be 'statistical' or 'radius': got %r" % (mode,))
    k = check_k(k)
    std_ratio = check_std_ratio(std_ratio)
    passes = _int_in("passes", passes, 1, MAX_PASSES)
    if mode == "statistical":
        if radius is not None or min_neighbours is not None:
            raise ValueError("radius and min_neighbours belong to mode='radius'")
        return Params(mode, k, std_ratio, None, None, passes)
    if radius is None:
        raise ValueError("mode='radius' needs a radius (in the cloud's units)")
    radius = _number("radius", radius)
    if not radius > 0.0 or not math.isfinite(radius * radius):
        raise ValueError("radius must be > 0 and its square finite: got %r" % (radius,))
    min_neighbours = k if min_neighbours is None else _int_in("min_neighbours", min_neighbours, 1, MAX_K)
    return Params(mode, k, std_ratio, radius, min_neighbours, passes)


def as_params(outliers):
    """``outliers=`` of the estimators -> ``Params`` or None: None (off), ``'statistical'`` (the defaults) or a dict of the keyword
    arguments of ``check_params``.  ``ValueError`` otherwise -- for ``'radius'`` alone too: that mode needs its radius."""
    if outliers is None:
        return None
    if isinstance(outliers, Params):
        return check_params(*outliers)
    if isinstance(outliers, str):
        if outliers == "statistical":
            return check_params()
        if outliers == "radius":
            raise ValueError("outliers='radius' needs its radius: pass a dict, e.g. {'mode': 'radius', 'radius': r}")
        raise ValueError("outliers must be None, 'statistical' or a dict of %s: got %r" % (", ".join(KEYS), outliers))
    if isinstance(outliers, dict):
        extra = sorted(set(outliers) - set(KEYS), key=repr)
        if extra:
            raise ValueError("outliers: unknown key%s %s (%s)" % ("s" if len(extra) > 1 else "", ", ".join(map(repr, extra)), ", ".join(KEYS)))
        return check_params(**outliers)
    raise ValueError("outliers must be None, 'statistical' or a dict of %s: got %r" % (", ".join(KEYS), outliers))


def refuse_pidx(pidx):
    """``outliers=`` with ``pidx=``: ``ValueError`` -- left for later."""
    if pidx is not None:
        raise ValueError("outliers with pidx is not served yet: the filter renumbers the cloud, and a pidx entry that names a removed "
                         "point would have no row to stand for; filter first (outliers.remove_outliers) and index the kept cloud")


def check_cloud(pts):
    """``pts`` as a contiguous float32 [N,3] numpy array; ``ValueError`` for another shape."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("pts must be [N, 3]: got %s" % (pts.shape,))
    return pts


def outlier_cloud(cloud, params, stream=None):
    """The device form: filter ALL points of a prepared ``provider.CloudPatches`` (no ``pidx``, no ``queries``; ``radius_grid=False``
    serves).  Every pass searches the current cloud at K = k + 1, scores it (``CloudPatches.outlier_scores``), takes the threshold --
    ``CloudPatches.outlier_threshold`` over the mean distances, or ``radius * radius`` against the squared distance to the
    ``min_neighbours``-th other point -- and compacts (``CloudPatches.outlier_compact``); the next pass runs on the compacted cloud and
    the index maps are composed.  Each pass synchronises once, to read ``n_kept`` (and the pass's statistics) back; the kept rows cross
    to the host where another pass follows, whose search grid is sized from their bounding box.  Returns a dict of device tensors

      points  [n_kept,3] f32   the kept rows, bit for bit, in the cloud's order
      kept    [n_kept]   int64 their indices in the cloud, ascending
      inlier  [N]        bool
      score   [N]        f64   the score (mean distance; radius mode: squared distance to the k-th) from the pass that last saw the row

    and ``passes``: per pass a dict of ``n`` (the scores that took part in the statistics; radius mode: the rows of the pass), ``mean``,
    ``std`` (radius mode: None), ``threshold`` and ``removed``.  The kept set is a pure function of (cloud, parameters)."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    params = as_params(params)
    if params is None:
        raise ValueError("outlier_cloud: params must be given")
    if cloud.pidx is not None or cloud.queries is not None:
        raise ValueError("outlier_cloud: the filter runs over all points of a cloud: no pidx, no queries")
    statistical = params.mode == "statistical"
    k = params.k if statistical else params.min_neighbours
    N = cloud.n_points
    dev = cloud.device
    cur, kept, score, log = cloud, None, None, []
    with torch.cuda.device(dev):
        points = cloud.cloud
        for p in range(params.passes):
            n = cur.n_points
            if n == 0:
                break
            st = cur._stream(stream)
            mean, kth_d2, _ = cur.outlier_scores(0, n, k, stream=st)
            if statistical:
                sc = mean
                stats = cur.outlier_threshold(sc, params.std_ratio, stream=st)
                xyz, kept_idx, _, _, n_kept = cur.outlier_compact(sc, stats[3:], stream=st)
            else:
                sc = kth_d2
                thr = float(np.float64(params.radius) * np.float64(params.radius))
                stats = None
                xyz, kept_idx, _, _, n_kept = cur.outlier_compact(sc, thr, stream=st)
            with torch.cuda.stream(st):
                # the pass's one readback (synchronises): n_kept, behind the statistics where there are any
                back = (n_kept.double() if stats is None else torch.cat([stats, n_kept.double()])).cpu()
                m = int(back[-1])
                if score is None:
                    score = sc
                else:
                    score[kept] = sc
                local = kept_idx[:m].long()
                kept = local if kept is None else kept[local]
                points = xyz[:m]
            if statistical:
                log.append({"n": int(back[0]), "mean": float(back[1]), "std": float(back[2]), "threshold": float(back[3]), "removed": n - m})
            else:
                log.append({"n": n, "mean": None, "std": None, "threshold": thr, "removed": n - m})
            if p + 1 < params.passes and m:
                cur = CloudPatches(points.cpu().numpy(), NestiConfig(), device=dev, radius_grid=False)
            elif not m:
                break
        if kept is None:                                                     # an empty cloud
            kept = torch.zeros(0, dtype=torch.int64, device=dev)
            score = torch.zeros(0, dtype=torch.float64, device=dev)
        inlier = torch.zeros(N, dtype=torch.bool, device=dev)
        inlier[kept] = True
    return {"points": points, "kept": kept, "inlier": inlier, "score": score, "passes": log}


def remove_outliers(pts, mode="statistical", k=DEFAULT_K, std_ratio=DEFAULT_STD_RATIO, radius=None, min_neighbours=None,
                    passes=DEFAULT_PASSES, device="cuda:0"):
    """Remove the outliers of a cloud: numpy in, a dict of numpy arrays out (synchronises).

      points  [n_kept,3] f32   the kept rows, bit for bit, in the input's order
      kept    [n_kept]   int64 their indices in ``pts``, ascending
      inlier  [N]        bool
      score   [N]        f64   from the pass that last saw the row: the mean distance to the ``k`` nearest other points (+inf: there are
                               none); in radius mode the squared distance to the ``min_neighbours``-th other point (+inf: fewer exist)
      passes  a list, per pass a dict of ``n``, ``mean``, ``std``, ``threshold`` and ``removed``

    ``mode='statistical'``: a row stays iff its score is at most ``mean + std_ratio * std`` of the scores of its pass (``k`` in 1 .. 255,
    ``std_ratio`` >= 0; the std is the sample's, n - 1).  ``mode='radius'``: a row stays iff at least ``min_neighbours`` (1 .. 255; None:
    ``k``) other points lie within ``radius`` (closed).  ``passes`` (1 .. 8): each further pass searches the compacted cloud again -- a
    cluster of outliers that shielded each other in one pass may fall in the next.  Duplicates are other points at distance 0.  The kept
    set is a pure function of (cloud, parameters).  Raises ``ValueError`` for parameters outside their ranges and for a cloud that is
    not [N,3] or not finite."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    params = check_params(mode, k, std_ratio, radius, min_neighbours, passes)
    pts = check_cloud(pts)
    if not len(pts):                                                         # nothing to filter, and no bounding box to prepare
        return {"points": pts, "kept": np.zeros(0, np.int64), "inlier": np.zeros(0, bool), "score": np.zeros(0, np.float64), "passes": []}
    cloud = CloudPatches(pts, NestiConfig(), device=device, radius_grid=False)
    res = outlier_cloud(cloud, params)
    with torch.cuda.device(cloud.device):
        torch.cuda.current_stream(cloud.device).synchronize()
    return {"points": res["points"].cpu().numpy().reshape(-1, 3), "kept": res["kept"].cpu().numpy(), "inlier": res["inlier"].cpu().numpy(),
            "score": res["score"].cpu().numpy(), "passes": res["passes"]}


# ---- filtered rows back to the rows of the input ------------------------------------------------------------------------------------------
def scatter_rows(rows, kept_idx, n, fill=0, stream=None):
    """Device: ``rows`` [M] or [M,C] (float32 or int32, C <= 8) of the kept points -> a tensor [n] / [n,C] whose row ``kept_idx[i]`` is
    ``rows[i]`` and whose other rows hold ``fill``: ``nesti_image_scatter`` over an image of H = 1, W = n (``depth.scatter_to_image``).
    ``kept_idx`` [M] int32 on the rows' device, its entries distinct; n <= 2^26.  Asynchronous on ``stream``."""
    from .depth import scatter_to_image
    return scatter_to_image(rows, kept_idx, 1, int(n), fill, stream=stream)[0]


def scatter_host(rows, kept, n, fill=0):
    """Host: numpy ``rows`` [M, ...] of the kept points -> [n, ...] with ``rows[i]`` at row ``kept[i]`` and ``fill`` elsewhere, for the
    results an estimator has already brought to the host."""
    return take_rows(rows, inverse(kept, n), fill)


def scatter_result(res, kept, n, rows=None):
    """A result dict of numpy arrays over the kept points -> over the ``n`` rows of the input: every array whose first dimension is the
    kept count (``rows``: that count, default ``len(kept)``) is scattered, with 0 -- ``expert``: -1 (``FILLS``) -- in the removed rows;
    everything else (``orient`` statistics, scalars) passes through."""
    return take_result(res, inverse(kept, n), len(kept) if rows is None else rows)
