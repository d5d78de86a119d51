"""Plane-fit (PCA) normals and surface variation at every patch scale on the GPU (``csrc/pca.hip``; DESIGN.md 2 "Plane-fit normals"):
the classical estimator -- the first row of the paper's comparison tables, and the frame of the reference dataset's ``use_pca`` step
(``utils/pcpnet_dataset.py:357-377``).  It needs no model and no weights: per query and patch radius, the plane fitted to the full
ball; the normal is the eigenvector of the smallest eigenvalue of the ball's covariance and the three eigenvalues give the surface
variation ``w0 / (w0 + w1 + w2)``.  There is no CPU fallback."""
import numpy as np

from . import _lib
from .config import NestiConfig

ORIENT_MODES = (None, "mst", "viewpoint")


def check_scale(scale, n_scales):
    """``scale`` in [-S, S) -> its non-negative index; ``ValueError`` otherwise."""
    if int(scale) != scale or not -n_scales <= int(scale) < n_scales:
        raise ValueError("scale must be in [-%d, %d): got %r" % (n_scales, n_scales, scale))
    return int(scale) % n_scales


def variation(eig):
    """Surface variation ``w0 / (w0 + w1 + w2)`` of eigenvalues [..., 3] (float32 in, float32 out), 0 where the sum is 0."""
    eig = np.asarray(eig, np.float32)
    total = eig.sum(axis=-1, dtype=np.float32)
    return np.divide(eig[..., 0], total, out=np.zeros_like(total), where=total != 0)


def orient_rows(cloud, normals, scale, mode, viewpoint=None, k=8, radius=None):
    """Orient the rows ``normals`` [patch_count, 3] (contiguous, on the cloud's device) of a prepared cloud IN PLACE with
    ``orient.orient_device``, the way ``NormalEstimator.orient`` does: positions are the cloud, ``cloud[pidx]`` or the (harmless) query
    positions (``CloudPatches.centre_positions``); the radius is ``r_abs[scale]``, or ``radius`` where given (the k-NN fits, whose
    scales are no radii).  Only sign bits change, sentinel rows stay 0 0 0.  Returns the int32[4] stats tensor."""
    import torch
    from . import orient as _orient
    r = float(cloud.r_abs[scale]) if radius is None else float(radius)
    return _orient.orient_device(cloud.centre_positions(), normals, r, k, viewpoint, mode, torch.cuda.current_stream(cloud.device))


def fit_cloud(cloud, ball, nbr, names, scale, orient, viewpoint, orient_k, knn, after=None, smooth=None, lists=None):
    """What ``pca_cloud`` and ``quadric.quadric_cloud`` share: fit all patch rows of a prepared cloud with the method ``ball`` -- over
    the neighbour counts ``knn`` with the method ``nbr`` --, take the normals of ``scale``, orient them, synchronise.  ``names``: the
    dict keys of the ball method's outputs, normals first and counts last (a k-NN method returns ``radius`` before the counts).
    ``after(out, s, before)`` runs behind the orientation step on the dict of device tensors, ``out["normals"]`` among them, with the
    scale's index and the normals from before the pass (None where none ran), and may add tensors.  ``ball=None``: an estimator that
    exists over neighbour lists only (``hough.hough_cloud``), for which ``knn`` must be given.  ``smooth`` (``smooth.as_params``: None,
    a number of passes or a dict) smooths the scale's normals over all points between those two steps -- ``normals_all`` stays as
    fitted -- and adds ``smooth_support`` and ``smooth_count``; a k-NN fit whose lists hold at least ``k`` entries is given the lists
    of ONE search (``nbr`` then takes them as its ``nbr=`` keyword) which the passes reuse, a prefix of a sorted list being the k-NN
    list; otherwise the passes search once for themselves.  ``lists`` -- a contiguous int32 [patch_count, K >= max(knn)] device tensor of
    sorted neighbour lists (``depth.window_knn``) -- is used instead of the fit's own search, and by the passes where K reaches their
    ``k``; it needs ``knn``.  Returns the dict as numpy arrays, with ``orient``."""
    import torch
    from . import orient as _orient
    if ball is None and knn is None:
        raise ValueError("this estimator exists over neighbour lists only: knn must be given")
    if lists is not None and knn is None:
        raise ValueError("lists are neighbour lists: knn must be given")
    ks = None
    if knn is not None:
        from .knn import check_ks
        ks = check_ks(knn)
        names = names[:-1] + ("radius",) + names[-1:]
    s = check_scale(scale, cloud.cfg.n_scales if ks is None else len(ks))
    if orient not in ORIENT_MODES:
        raise ValueError("orient must be None, 'mst' or 'viewpoint'")
    from . import smooth as _smooth
    sm = _smooth.as_params(smooth)
    if sm is not None:
        _smooth.refuse_subset(cloud.pidx, cloud.queries)
    with torch.cuda.device(cloud.device):
        if ks is None:
            out = dict(zip(names, ball(0, cloud.patch_count)))
        elif lists is not None:
            if lists.dim() != 2 or lists.shape[1] < ks[-1]:
                raise ValueError("lists: an int32 [patch_count, K >= %d] tensor" % ks[-1])
            out = dict(zip(names, nbr(0, cloud.patch_count, ks, nbr=lists)))
            if sm is not None and lists.shape[1] < sm.k:
                lists = None                                   # too short for the passes: they search for themselves
        elif sm is not None and ks[-1] >= sm.k:
            lists = cloud.knn(0, cloud.patch_count, ks[-1])[0]
            out = dict(zip(names, nbr(0, cloud.patch_count, ks, nbr=lists)))
        else:
            out = dict(zip(names, nbr(0, cloud.patch_count, ks)))
        normals = out["normals"] = out[names[0]][:, s, :].contiguous()
        if sm is not None:
            normals, out["smooth_support"], out["smooth_count"] = _smooth.smooth_cloud(cloud, normals, sm, nbr=lists)
            out["normals"] = normals
        before = stats = None
        if orient is not None and cloud.patch_count:
            before = normals.clone() if after else None
            stats = orient_rows(cloud, normals, s, orient, viewpoint, orient_k, radius=None if ks is None else max(cloud.r_abs))
        if after:
            after(out, s, before)
        torch.cuda.current_stream(cloud.device).synchronize()
    res = {key: t.cpu().numpy() for key, t in out.items()}
    res["orient"] = None if orient is None else (_orient.stats_dict(stats) if stats is not None else dict.fromkeys(_orient.STAT_NAMES, 0))
    return res


def pca_cloud(cloud, scale=-1, orient=None, viewpoint=None, orient_k=8, knn=None, smooth=None, lists=None):
    """``pca_normals`` for a prepared ``provider.CloudPatches`` (all of its patch rows); synchronises.  ``knn``: neighbour counts
    instead of the cloud's radii (``scale`` then indexes them, and the dict gains ``radius``).  ``smooth``, ``lists``: see ``fit_cloud``."""
    res = fit_cloud(cloud, cloud.pca, cloud.pca_knn, ("normals_all", "eig", "n_ball"), scale, orient, viewpoint, orient_k, knn,
                    smooth=smooth, lists=lists)
    res["variation"] = variation(res["eig"])
    return res


def check_knn_args(knn, cfg):
    """``knn=`` of ``pca_normals`` / ``quadric.quadric_fit`` -> (ks or None, the configuration to prepare the cloud with).  ``ValueError``
    for a bad ``knn`` and for ``knn`` together with a ``cfg``: the scales of a k-NN fit are neighbour counts, a configuration's radii
    would mean nothing."""
    if knn is None:
        return None, cfg or NestiConfig()
    from .knn import check_ks
    ks = check_ks(knn)
    if cfg is not None:
        raise ValueError("knn and cfg are mutually exclusive: the scales of a k-NN fit are the neighbour counts, not cfg.patch_radius")
    return ks, NestiConfig()


def prepare_cloud(pts, cfg, pidx, queries, scale, orient, viewpoint, orient_k, device, knn, smooth=None):
    """The "numpy in" front of ``pca_normals`` and ``quadric.quadric_fit``: every argument check, then the ``CloudPatches``.  Returns the
    arguments of ``pca_cloud`` / ``quadric.quadric_cloud`` (``smooth``, checked here, is not among them)."""
    ks, cfg = check_knn_args(knn, cfg)
    if smooth is not None:
        from . import smooth as _smooth
        _smooth.as_params(smooth)
        _smooth.refuse_subset(pidx, queries)
    check_scale(scale, cfg.n_scales if ks is None else len(ks))
    if orient not in ORIENT_MODES:
        raise ValueError("orient must be None, 'mst' or 'viewpoint'")
    if pidx is not None and queries is not None:
        raise ValueError("pidx and queries are mutually exclusive: a query is a cloud point (pidx) or a position (queries)")
    if orient is not None:
        from .orient import _check_args
        _check_args(1.0, orient_k, viewpoint, orient)
    from .provider import CloudPatches
    # the k-NN fits never read the radius grid (the orientation pass builds its own): a cloud without extent is served too
    cloud = CloudPatches(np.asarray(pts, dtype=np.float32), cfg, device=device, pidx=pidx, queries=queries, radius_grid=ks is None)
    return cloud, scale, orient, viewpoint, orient_k, ks


def pca_normals(pts, cfg=None, pidx=None, queries=None, scale=-1, orient=None, viewpoint=None, orient_k=8, device="cuda:0", knn=None,
                smooth=None, outliers=None, downsample=None, denoise=None):
    """Plane-fit normals of a cloud: numpy in, a dict of numpy arrays out (synchronises).  Queries are all points, the points
    ``pidx`` or the positions ``queries`` [M,3] (mutually exclusive), as for ``NormalEstimator.estimate``; the radii are
    ``cfg.patch_radius`` times the cloud's bounding-box diagonal.

      normals      [M,3]    the normals at ``scale`` (default -1: the largest), after the optional orientation
      normals_all  [M,S,3]  every scale, unoriented: the first non-zero of (n_z, n_y, n_x) is positive
      eig          [M,S,3]  eigenvalues of the ball's covariance in units of r^2, ascending
      variation    [M,S]    w0 / (w0 + w1 + w2), 0 where the sum is 0
      n_ball       [M,S]    points in the ball (the full ball: not capped at ``cfg.num_point``, not subsampled)
      orient       the stats dict of ``orient.orient_normals``, or None

    A scale whose ball holds fewer than 3 points has normal 0 0 0 and eigenvalues 0 0 0; the orientation leaves such rows alone.
    ``orient='mst' | 'viewpoint'`` orients the rows of ``scale`` with radius ``r_abs[scale]`` (only sign bits change).

    ``knn`` -- an int or an ascending sequence of at most 4 ints in 1 .. 256 -- replaces the balls by the nearest neighbours
    (DESIGN.md 2 "k-nearest neighbourhoods"): scale s is the ``knn[s]`` nearest cloud points of the query, itself included where it is
    a cloud point; ``scale`` indexes ``knn``; ``n_ball`` holds the counts (``min(knn[s], N)``); the dict gains ``radius`` [M,S] float32,
    the distance to the farthest neighbour, and ``eig`` is in units of that radius squared.  No row is a sentinel for want of
    neighbours unless the cloud has fewer than 3 points (or the neighbours all coincide with the query).  A row's bits do not depend
    on batching or on the search grid.  With ``orient='mst'`` the orientation graph's radius is the default configuration's largest
    patch radius, as on the network path: the k-NN radii vary per row and are not a safe grid cell; ``'viewpoint'`` needs no radius.

    ``smooth`` -- None, a number of passes or a dict of ``k``, ``iters``, ``angle``, ``falloff`` (``smooth.smooth_normals``) -- smooths
    ``normals`` over all points before the orientation (DESIGN.md 2 "Normal smoothing"); ``normals_all`` stays as fitted and the dict
    gains ``smooth_support`` [M] float32 and ``smooth_count`` [M] int32 of the last pass.  It needs all points.

    Raises ``ValueError`` for a ``scale`` outside [-S, S), for ``pidx`` together with ``queries``, for a bad ``knn``, for ``knn``
    together with ``cfg`` (whose radii would mean nothing), for a bad ``smooth`` and for ``smooth`` with ``pidx`` or ``queries`` (the
    rows' neighbours would have no normal).

    ``downsample``, ``outliers``, ``denoise`` -- the preprocessing chain (``stages``: the arguments, their order, the keys they add,
    the way back to the rows of ``pts`` and what ``queries`` changes) -- run in front of the estimator; ``pidx`` with any is refused."""
    from . import stages
    chain = stages.run(pts, stages.check(downsample, outliers, denoise, pidx), queries, device)
    cloud = prepare_cloud(chain.points, cfg, pidx, queries, scale, orient, viewpoint, orient_k, device, knn, smooth)
    return chain.back(pca_cloud(*cloud, smooth=smooth))
