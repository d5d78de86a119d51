"""Feature-preserving normal smoothing over the nearest neighbours on the GPU (``csrc/smooth.hip``; DESIGN.md 2 "Normal smoothing"):
the step after estimation -- a bilateral filter of normals after Jones et al. 2004, Sun et al. 2007 and the anisotropic normal smoothing
of Huang et al.'s edge-aware resampling.  A row's normal becomes the weighted mean of its neighbours' normals; the weight is 0 where a
neighbour's normal leaves a cone of ``angle`` degrees round the row's own, so rows agree along a face and not across a crease.  It runs
after any estimator (``smooth=`` of ``pca.pca_normals``, ``quadric.quadric_fit``, ``hough.hough_normals`` and
``NormalEstimator.estimate``; ``--smooth`` on the command line), before the orientation.  It filters normals: positions never move.
The conventions are the library's own.  There is no CPU fallback."""
import collections
import math

import numpy as np

from . import _lib
from ._args import int_in as _int_in

DEFAULT_K, DEFAULT_ITERS, DEFAULT_ANGLE, DEFAULT_FALLOFF = 16, 2, 45.0, 0.75
MAX_ITERS = 64
MAX_COS = 0.999999                     # nesti_smooth_normals_nbr: cos_t in [0, MAX_COS]

# k, iters, angle (degrees), falloff, and cos_t = cos(angle), computed once on the host
Params = collections.namedtuple("Params", "k iters angle falloff cos_t")


def _float_in(name, v, lo, hi, what):
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(v, bool) or not (math.isfinite(f) and lo <= f <= hi):
        raise ValueError("%s must be a finite number in %s: got %r" % (name, what, v))
    return f


def check_pass(k, cos_t, falloff):
    """(k, cos_t, falloff) of one pass within the limits of include/nesti_hip.h; ``ValueError`` otherwise."""
    return (_int_in("k", k, 1, _lib.KNN_MAX_K), _float_in("cos_t", cos_t, 0.0, MAX_COS, "[0, %r]" % MAX_COS),
            _float_in("falloff", falloff, 0.0, 1.0, "[0, 1]"))


def check_params(k=DEFAULT_K, iters=DEFAULT_ITERS, angle=DEFAULT_ANGLE, falloff=DEFAULT_FALLOFF):
    """The one place where the ranges are checked: ``k`` in 1 .. 256, ``iters`` in 1 .. 64, ``angle`` in (0, 90] degrees, ``falloff``
    in [0, 1] -> ``Params``; ``ValueError`` otherwise."""
    iters = _int_in("iters", iters, 1, MAX_ITERS)
    angle = _float_in("angle", angle, 0.0, 90.0, "(0, 90] degrees")
    if not angle > 0.0:
        raise ValueError("angle must be a finite number in (0, 90] degrees: got %r" % (angle,))
    cos_t = min(max(math.cos(math.radians(angle)), 0.0), MAX_COS)     # an angle below 0.081 degrees is served at the entry's limit
    k, cos_t, falloff = check_pass(k, cos_t, falloff)
    return Params(k, iters, angle, falloff, cos_t)


def as_params(smooth):
    """``smooth=`` of the estimators -> ``Params`` or None: None (off), an int (that many passes, the other defaults) or a dict of the
    keyword arguments ``k``, ``iters``, ``angle``, ``falloff``.  ``ValueError`` otherwise."""
    if smooth is None:
        return None
    if isinstance(smooth, Params):
        return check_params(smooth.k, smooth.iters, smooth.angle, smooth.falloff)
    if isinstance(smooth, dict):
        extra = sorted(set(smooth) - {"k", "iters", "angle", "falloff"})
        if extra:
            raise ValueError("smooth: unknown key%s %s (k, iters, angle, falloff)" % ("s" if len(extra) > 1 else "", ", ".join(map(repr, extra))))
        return check_params(**smooth)
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)):
        raise ValueError("smooth must be None, a number of passes or a dict of k, iters, angle, falloff: got %r" % (smooth,))
    return check_params(iters=smooth)


def refuse_subset(pidx, queries):
    """``smooth=`` needs a normal for every cloud point: ``ValueError`` with ``pidx`` or ``queries``."""
    if pidx is not None or queries is not None:
        raise ValueError("smooth needs all points: with pidx or queries the rows' neighbours would have no normal")


def smooth_cloud(cloud, normals_dev, params, nbr=None, stream=None):
    """``params.iters`` passes over ALL points of a prepared ``provider.CloudPatches`` (no ``pidx``, no ``queries``): ``normals_dev``
    [n_points,3] f32 on the cloud's device is read, never written; the passes ping-pong between two buffers of their own.  The lists
    are searched once at K = ``params.k`` unless ``nbr`` [n_points, K >= k] (sorted lists, int32, device) is given -- a prefix of a
    sorted list is the k-NN list.  Returns device tensors ``(normals [n_points,3], support [n_points], count [n_points])``, the last
    two from the last pass.  Does not synchronise."""
    params = as_params(params)
    if params is None:
        raise ValueError("smooth_cloud: params must be given")
    if cloud.pidx is not None or cloud.queries is not None:
        refuse_subset(cloud.pidx, cloud.queries)
    n = cloud.n_points
    if nbr is None:
        nbr = cloud.knn(0, n, params.k, stream=stream)[0]
    out = None
    cur = normals_dev
    for _ in range(params.iters):
        out = cloud.smooth_knn(cur, 0, n, params.k, params.cos_t, params.falloff, nbr=nbr, stream=stream)
        cur = out[0]
    return out


def smooth_normals(pts, normals, k=DEFAULT_K, iters=DEFAULT_ITERS, angle=DEFAULT_ANGLE, falloff=DEFAULT_FALLOFF, nbr=None, device="cuda:0"):
    """Smooth the normals of a cloud: numpy in, a dict of numpy arrays out (synchronises).  ``normals`` [N,3] holds one normal per
    point, oriented or not, of any length; a row that is 0 0 0 or not finite takes no part and is returned as it came.

      normals  [N,3] f32    unit normals on the input's side of the surface (``out . in >= 0``)
      support  [N]   f32    the sum of the weights of the last pass
      count    [N]   int32  the neighbours that had a weight in the last pass, the point itself included (1: nothing agreed)

    ``iters`` (1 .. 64) passes over the ``k`` (1 .. 256) nearest neighbours; a neighbour's weight is ``u^2 t^2`` with ``t`` falling
    linearly in the cosine from 1 (parallel) to 0 at ``angle`` degrees (in (0, 90]) and ``u = 1 - falloff d^2 / r^2`` over the
    neighbourhood's radius ``r`` (``falloff`` in [0, 1]).  ``nbr`` [N,K >= k]: sorted lists of the caller's instead of the one search.
    Creases are kept; many passes staircase curved surfaces.  Raises ``ValueError`` for arguments outside their ranges."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    params = check_params(k, iters, angle, falloff)
    pts = np.asarray(pts, dtype=np.float32)
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3 or normals.shape != pts.shape:
        raise ValueError("pts and normals must both be [N, 3]: got %s and %s" % (pts.shape, normals.shape))
    cloud = CloudPatches(pts, NestiConfig(), device=device, radius_grid=False)
    with torch.cuda.device(cloud.device):
        if nbr is not None:
            nbr = torch.as_tensor(np.ascontiguousarray(nbr, dtype=np.int32), device=cloud.device)
        out = smooth_cloud(cloud, torch.from_numpy(normals).to(cloud.device), params, nbr=nbr)
        torch.cuda.current_stream(cloud.device).synchronize()
    return dict(zip(("normals", "support", "count"), (t.cpu().numpy() for t in out)))
