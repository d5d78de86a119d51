"""Robust plane-fit normals over the nearest neighbours on the GPU (``csrc/robust.hip``; DESIGN.md 2 "Robust plane fit"): an
M-estimator of the plane through a neighbourhood, solved by iteratively re-weighted least squares -- after Mederos et al. (2003),
Fleishman et al. (2005) and the RIMLS of Oztireli et al. (2009).  Residuals to the current plane down-weight the points of the other face
of a crease, so the fit leans to one face where the plane fit and the quadric fit average both; the normal stays continuous, with no bins
and no triplets, so it loses little on noisy smooth surfaces where the Hough transform pays for its bins.  With ``init=`` the same call
refines any other estimator's normals against the points.  It needs no model and no weights.  The conventions are the library's own (no
parity with any published code is claimed).  There is no ball variant and no CPU fallback."""
import numpy as np

from . import _lib
from ._args import number as _number
from .pca import fit_cloud, prepare_cloud

DEFAULT_KNN, DEFAULT_ITERS, DEFAULT_SIGMA, DEFAULT_FALLOFF, DEFAULT_FLOOR = 100, 8, 2.0, 0.5, 0.01
SIGMA_MAX, FLOOR_MIN = 1e6, 1e-6


def check_params(iters=DEFAULT_ITERS, sigma=DEFAULT_SIGMA, falloff=DEFAULT_FALLOFF, floor=DEFAULT_FLOOR):
    """(iters, sigma, falloff, floor) as an int and three floats within the limits of include/nesti_hip.h; ``ValueError`` otherwise."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= int(iters) <= _lib.ROBUST_MAX_ITERS:
        raise ValueError("iters must be an integer in 0 .. %d: got %r" % (_lib.ROBUST_MAX_ITERS, iters))
    sigma, falloff, floor = _number("sigma", sigma), _number("falloff", falloff), _number("floor", floor)
    if not 0.0 < sigma <= SIGMA_MAX:
        raise ValueError("sigma must be in (0, %g]: got %r" % (SIGMA_MAX, sigma))
    if not 0.0 <= falloff <= 1.0:
        raise ValueError("falloff must be in [0, 1]: got %r" % (falloff,))
    if not FLOOR_MIN <= floor <= 1.0:
        raise ValueError("floor must be in [%g, 1]: got %r" % (FLOOR_MIN, floor))
    return int(iters), sigma, falloff, floor


def check_init(init, rows, n_scales):
    """``init`` -- None, [rows,3] (one start normal per row, used at every scale) or [rows,S,3] -- as a contiguous float32 numpy array
    [rows,S,3] or None; ``ValueError`` otherwise.  The values are not looked at: a row that is 0 0 0 or not finite comes back 0 0 0."""
    if init is None:
        return None
    try:
        a = np.asarray(init, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("init must be an array of start normals [M,3] or [M,S,3]")
    if a.shape == (rows, 3):
        a = np.broadcast_to(a[:, None, :], (rows, n_scales, 3))
    if a.shape != (rows, n_scales, 3):
        raise ValueError("init must be [M,3] or [M,S,3] with M = %d rows and S = %d scales: got %s" % (rows, n_scales, np.shape(init)))
    return np.ascontiguousarray(a)


def _need_knn(knn):
    if knn is None:
        raise ValueError("the robust plane fit exists over neighbour lists only (there is no ball variant): knn must be given")


def robust_cloud(cloud, knn=DEFAULT_KNN, scale=-1, iters=DEFAULT_ITERS, sigma=DEFAULT_SIGMA, falloff=DEFAULT_FALLOFF, floor=DEFAULT_FLOOR,
                 init=None, orient=None, viewpoint=None, orient_k=8, smooth=None, lists=None):
    """``robust_normals`` for a prepared ``provider.CloudPatches`` (all of its patch rows); synchronises.  ``smooth``, ``lists``: see
    ``pca.fit_cloud``."""
    import torch
    from .knn import check_ks
    _need_knn(knn)
    iters, sigma, falloff, floor = check_params(iters, sigma, falloff, floor)
    start = check_init(init, cloud.patch_count, len(check_ks(knn)))
    if start is not None:
        start = torch.from_numpy(start).to(cloud.device)

    def nbr(first, count, ks, nbr=None):
        return cloud.robust_knn(first, count, ks, iters, sigma, falloff, floor, init=None if start is None else start[first:first + count],
                                nbr=nbr)

    res = fit_cloud(cloud, None, nbr, ("normals_all", "plane_all", "support", "inliers", "iters_done", "moments", "n_ball"), scale, orient,
                    viewpoint, orient_k, knn, smooth=smooth, lists=lists)
    del res["moments"]
    return res


def robust_normals(pts, knn=DEFAULT_KNN, pidx=None, queries=None, scale=-1, iters=DEFAULT_ITERS, sigma=DEFAULT_SIGMA,
                   falloff=DEFAULT_FALLOFF, floor=DEFAULT_FLOOR, init=None, orient=None, viewpoint=None, orient_k=8, smooth=None,
                   device="cuda:0", outliers=None, downsample=None, denoise=None):
    """Robust plane-fit normals of a cloud: numpy in, a dict of numpy arrays out (synchronises).  Queries are all points, the points
    ``pidx`` or the positions ``queries`` [M,3] (mutually exclusive), as for ``pca.pca_normals``.  ``knn`` -- an int or an ascending
    sequence of at most 4 ints in 1 .. 256 -- names the neighbourhoods: scale s is the ``knn[s]`` nearest cloud points of the query
    (one exact search at ``max(knn)``).

      normals      [M,3]    the normals at ``scale`` (default -1: the largest), after the optional smoothing and orientation
      normals_all  [M,S,3]  every scale, unoriented: the first non-zero of (n_z, n_y, n_x) is positive
      plane_all    [M,S,3]  the plane fit of the same neighbourhoods: the bits of ``pca.pca_normals(knn=...)``
      support      [M,S]    the sum of the weights of the last iteration
      inliers      [M,S]    int32, the neighbours whose residual lies within the scale of the residuals in that iteration
      iters_done   [M,S]    int32, the iterations done
      radius       [M,S]    the distance to the farthest neighbour of the scale
      n_ball       [M,S]    int32, the neighbour counts (``min(knn[s], N)``)
      orient       the stats dict of ``orient.orient_normals``, or None

    Each of the ``iters`` (0 .. 64) iterations measures the neighbours' heights over the plane of the current normal through their
    median height, takes ``sig = max(sigma * median |residual|, floor * radius)`` as the scale of the residuals, weighs a neighbour by
    ``(u t)^2`` with ``t = 1 / (1 + (residual / sig)^2)`` (Geman-McClure) and ``u = 1 - falloff * (distance / radius)^2``, and fits the
    plane to the weighted neighbours.  The first normal is the plane fit's, or ``init`` -- [M,3], used at every scale, or [M,S,3]: the
    normals of any other estimator, which the iterations then refine against the points; their sign does not matter, and a row that is
    0 0 0 or not finite comes back 0 0 0.  ``sigma`` in (0, 1e6], ``falloff`` in [0, 1], ``floor`` in [1e-6, 1].  A scale with fewer
    than 3 neighbours, or whose neighbours all coincide with the query, is 0 0 0.  ``iters=T`` equals ``T`` calls with ``iters=1``
    chained through ``init``, bit for bit.  ``smooth`` and ``orient`` are as for ``pca.pca_normals(knn=...)``.

    Raises ``ValueError`` -- before any GPU work -- for ``knn=None`` (there is no ball variant), for parameters outside their ranges,
    for an ``init`` of another shape, for a ``scale`` outside [-S, S), for ``pidx`` together with ``queries``, for a bad ``orient`` or
    ``smooth`` and for ``smooth`` with ``pidx`` or ``queries``.

    ``downsample``, ``outliers``, ``denoise`` -- the preprocessing chain (``stages``: the arguments, their order, the keys they add,
    the way back to the rows of ``pts`` and what ``queries`` changes) -- run in front of the estimator; ``pidx`` with any is refused."""
    from . import stages
    from .knn import check_ks
    params = stages.check(downsample, outliers, denoise, pidx)
    _need_knn(knn)
    check_params(iters, sigma, falloff, floor)
    if pidx is not None and queries is not None:
        raise ValueError("pidx and queries are mutually exclusive: a query is a cloud point (pidx) or a position (queries)")
    rows = len(pidx) if pidx is not None else len(queries) if queries is not None else len(pts)
    init = check_init(init, rows, len(check_ks(knn)))
    chain = stages.run(pts, params, queries, device)
    cloud, scale, orient, viewpoint, orient_k, ks = prepare_cloud(chain.points, None, pidx, queries, scale, orient, viewpoint, orient_k, device,
                                                                  knn, smooth)
    return chain.back(robust_cloud(cloud, ks, scale, iters, sigma, falloff, floor, chain.take(init), orient, viewpoint, orient_k, smooth=smooth))
