"""Scale-selected plane-fit normals on the GPU (``csrc/select.hip``; DESIGN.md 2 "Scale-selected plane fit"): the plane fit of
``pca.pca_normals(knn=...)`` at every neighbour count of a ladder, and per row the choice of one of them -- the candidate of smallest
surface variation ``e0 / (e0 + e1 + e2)``, Pauly, Keiser and Gross's multi-scale surface variation (2003) read as a selector, standing
in for the bias / variance trade of Mitra and Nguyen (2003).  No single neighbourhood size is right for every point: a small one
follows the noise, a large one rounds off creases; here every row names its own.  It needs no model and no weights.  The conventions
are the library's own: no parity with any published selector is claimed.  There is no CPU fallback."""
import math

import numpy as np

from . import _lib
from .pca import ORIENT_MODES, orient_rows

DEFAULT_LADDER = (12, 16, 24, 32, 48, 64, 96, 128, 192, 256)


def check_ladder(ladder):
    """``ladder`` -- an int or a strictly ascending sequence of 1 .. ``_lib.SELECT_MAX_L`` ints in 1 .. ``_lib.KNN_MAX_K`` -- as a tuple
    of ints; ``ValueError`` otherwise."""
    from .knn import check_k
    if isinstance(ladder, (int, np.integer)) and not isinstance(ladder, bool):
        return (check_k(ladder),)
    if isinstance(ladder, (str, bytes)):
        raise ValueError("ladder must be an int or a sequence of ints: got %r" % (ladder,))
    try:
        ks = tuple(ladder)
    except TypeError:
        raise ValueError("ladder must be an int or a sequence of ints: got %r" % (ladder,))
    if not 1 <= len(ks) <= _lib.SELECT_MAX_L:
        raise ValueError("ladder must hold 1 .. %d neighbour counts: got %d" % (_lib.SELECT_MAX_L, len(ks)))
    ks = tuple(check_k(k) for k in ks)
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("ladder must be strictly ascending: got %r" % (ks,))
    return ks


def check_slack(slack):
    """``slack`` as a finite float >= 0; ``ValueError`` otherwise."""
    try:
        f = float(slack)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(slack, bool) or not (math.isfinite(f) and f >= 0.0):
        raise ValueError("slack must be a finite number >= 0: got %r" % (slack,))
    return f


def selected_variation(variation_all, sel):
    """``variation_all[i, sel[i]]`` as float32 [M], 0 where ``sel[i]`` is -1."""
    variation_all, sel = np.asarray(variation_all, np.float32), np.asarray(sel)
    out = np.zeros(len(sel), np.float32)
    has = sel >= 0
    out[has] = variation_all[np.flatnonzero(has), sel[has]]
    return out


def select_cloud(cloud, ladder=DEFAULT_LADDER, slack=0.0, orient=None, viewpoint=None, orient_k=8, smooth=None, lists=None):
    """``select_normals`` for a prepared ``provider.CloudPatches`` (all of its patch rows; ``radius_grid=False`` will do): one search at
    ``ladder[-1]``, one selected fit over its lists, the optional smoothing over the same lists where they reach its ``k``, the optional
    orientation; synchronises.  ``lists`` -- a contiguous int32 [patch_count, K >= ladder[-1]] device tensor of sorted neighbour lists
    (``depth.window_knn``) -- is used instead of the search."""
    import torch
    from . import orient as _orient
    from . import smooth as _smooth
    ladder, slack = check_ladder(ladder), check_slack(slack)
    if orient not in ORIENT_MODES:
        raise ValueError("orient must be None, 'mst' or 'viewpoint'")
    sm = _smooth.as_params(smooth)
    if sm is not None:
        _smooth.refuse_subset(cloud.pidx, cloud.queries)
    names = ("normals", "eig", "sel", "k", "radius", "variation_all", "normals_all", "eig_all", "radius_all", "n_ball")
    with torch.cuda.device(cloud.device):
        if lists is None:
            lists = cloud.knn(0, cloud.patch_count, ladder[-1])[0]
        out = dict(zip(names, cloud.pca_select(0, cloud.patch_count, ladder, slack, nbr=lists)))
        normals = out["normals"]
        if sm is not None:
            normals, out["smooth_support"], out["smooth_count"] = _smooth.smooth_cloud(cloud, normals, sm,
                                                                                       nbr=lists if lists.shape[1] >= sm.k else None)
            out["normals"] = normals
        stats = None
        if orient is not None and cloud.patch_count:
            # the radius rule of the k-NN fits: the selected radii vary per row and are not a safe grid cell
            stats = orient_rows(cloud, normals, 0, orient, viewpoint, orient_k, radius=max(cloud.r_abs))
        torch.cuda.current_stream(cloud.device).synchronize()
    res = {key: t.cpu().numpy() for key, t in out.items()}
    res["variation"] = selected_variation(res["variation_all"], res["sel"])
    res["orient"] = None if orient is None else (_orient.stats_dict(stats) if stats is not None else dict.fromkeys(_orient.STAT_NAMES, 0))
    return res


def select_normals(pts, ladder=DEFAULT_LADDER, slack=0.0, pidx=None, queries=None, orient=None, viewpoint=None, orient_k=8, smooth=None,
                   device="cuda:0", outliers=None, downsample=None, denoise=None):
    """Scale-selected plane-fit normals of a cloud: numpy in, a dict of numpy arrays out (synchronises).  Queries are all points, the
    points ``pidx`` or the positions ``queries`` [M,3] (mutually exclusive), as for ``pca.pca_normals``.  ``ladder`` -- an int or a
    strictly ascending sequence of at most 32 ints in 1 .. 256 -- names the candidates: candidate c is the plane fit over the
    ``ladder[c]`` nearest cloud points of the query (one exact search at ``ladder[-1]``), bit for bit ``pca_normals(knn=ladder[c])``.

      normals        [M,3]    the normal of the selected candidate, after the optional smoothing and orientation
      k              [M]      int32, the neighbours the selected candidate used (``min(ladder[sel], N)``)
      sel            [M]      int32, the selected index into ``ladder``; -1: no candidate could be fitted, the row is 0 0 0
      radius         [M]      the distance to the farthest neighbour of the selected candidate
      eig            [M,3]    its eigenvalues in units of that radius squared, ascending
      variation      [M]      its surface variation ``e0 / (e0 + e1 + e2)``
      variation_all  [M,L]    the score of every candidate, 0 where it could not be fitted
      normals_all    [M,L,3]  every candidate, unoriented: the first non-zero of (n_z, n_y, n_x) is positive
      eig_all        [M,L,3]
      radius_all     [M,L]
      n_ball         [M,L]    int32, the neighbour counts (``min(ladder[c], N)``)
      orient         the stats dict of ``orient.orient_normals``, or None

    The score is computed in float64 from the float32 eigenvalues as written: ``v_c = e0 / ((e0 + e1) + e2)``; a candidate is eligible
    iff it has 3 neighbours or more, a radius above 0 and a sum of eigenvalues above 0.  With ``v_min`` the smallest score of a row the
    selected candidate is the LARGEST eligible one with ``v_c <= v_min + v_min * slack``: ``slack = 0`` is the arg-min with ties to the
    larger count; a larger ``slack`` (finite, >= 0) prefers larger neighbourhoods, which helps noisy smooth surfaces and hurts creases
    (DESIGN.md).  ``smooth`` and ``orient`` are as for ``pca.pca_normals(knn=...)``: the smoothing reuses the searched lists where
    ``ladder[-1]`` reaches its ``k`` and needs all points; ``'mst'`` uses the default configuration's largest patch radius.

    Raises ``ValueError`` -- before any GPU work -- for a bad ``ladder`` or ``slack``, for ``pidx`` together with ``queries``, for a bad
    ``orient`` or ``smooth`` and for ``smooth`` with ``pidx`` or ``queries``.

    ``downsample``, ``outliers``, ``denoise`` -- the preprocessing chain (``stages``: the arguments, their order, the keys they add,
    the way back to the rows of ``pts`` and what ``queries`` changes) -- run in front of the estimator; ``pidx`` with any is refused."""
    from . import smooth as _smooth, stages
    from .config import NestiConfig
    params = stages.check(downsample, outliers, denoise, pidx)
    ladder, slack = check_ladder(ladder), check_slack(slack)
    if smooth is not None:
        _smooth.as_params(smooth)
        _smooth.refuse_subset(pidx, queries)
    if orient not in ORIENT_MODES:
        raise ValueError("orient must be None, 'mst' or 'viewpoint'")
    if pidx is not None and queries is not None:
        raise ValueError("pidx and queries are mutually exclusive: a query is a cloud point (pidx) or a position (queries)")
    if orient is not None:
        from .orient import _check_args
        _check_args(1.0, orient_k, viewpoint, orient)
    from .provider import CloudPatches
    chain = stages.run(pts, params, queries, device)
    cloud = CloudPatches(np.asarray(chain.points, dtype=np.float32), NestiConfig(), device=device, pidx=pidx, queries=queries, radius_grid=False)
    return chain.back(select_cloud(cloud, ladder, slack, orient, viewpoint, orient_k, smooth))
