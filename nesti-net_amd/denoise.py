"""Point denoising over the nearest neighbours on the GPU (``csrc/denoise.hip``; DESIGN.md 2 "Point denoising"): the step between outlier
removal and estimation -- the bilateral point filter of Fleishman, Drori and Cohen-Or 2003 and Digne and de Franchis 2017, the projection
step of Huang et al.'s edge-aware resampling.  A point moves along its own normal by the weighted mean of its neighbours' heights over
its tangent plane; a neighbour's weight is 0 where its normal leaves a cone of ``angle`` degrees round the point's own and falls with its
height, so faces are flattened and creases are not rounded off.  Every model-free estimator takes the filter as ``denoise=``
(``pca.pca_normals``, ``quadric.quadric_fit``, ``hough.hough_normals``, ``select.select_normals``, ``robust.robust_normals``;
``--denoise`` on the command line).  The conventions are the library's own.  There is no CPU fallback."""
import collections
import math

import numpy as np

from . import _lib
from .smooth import MAX_COS, _float_in, _int_in

DEFAULT_K, DEFAULT_ITERS, DEFAULT_ANGLE, DEFAULT_FALLOFF, DEFAULT_SIGMA, DEFAULT_STEP = 16, 2, 45.0, 0.75, 0.5, 1.0
MAX_ITERS = 64
MAX_SIGMA = 1e6                        # nesti_denoise_points_nbr: sigma in (0, MAX_SIGMA]; at the bound the height weight is 1 to rounding
KEYS = ("k", "iters", "angle", "falloff", "sigma", "step", "normal_k")

# k, iters, angle (degrees), falloff, sigma, step, normal_k (the neighbours of the plane-fit normals), and cos_t = cos(angle)
Params = collections.namedtuple("Params", KEYS + ("cos_t",))


def _open_in(name, v, hi, what):
    f = _float_in(name, v, 0.0, hi, what)
    if not f > 0.0:
        raise ValueError("%s must be a finite number in %s: got %r" % (name, what, v))
    return f


def check_pass(k, cos_t, falloff, sigma, step):
    """(k, cos_t, falloff, sigma, step) of one pass within the limits of include/nesti_hip.h; ``ValueError`` otherwise."""
    return (_int_in("k", k, 1, _lib.KNN_MAX_K), _float_in("cos_t", cos_t, 0.0, MAX_COS, "[0, %r]" % MAX_COS),
            _float_in("falloff", falloff, 0.0, 1.0, "[0, 1]"), _open_in("sigma", sigma, MAX_SIGMA, "(0, %g]" % MAX_SIGMA),
            _open_in("step", step, 1.0, "(0, 1]"))


def check_params(k=DEFAULT_K, iters=DEFAULT_ITERS, angle=DEFAULT_ANGLE, falloff=DEFAULT_FALLOFF, sigma=DEFAULT_SIGMA, step=DEFAULT_STEP,
                 normal_k=None):
    """The one place where the ranges are checked: ``k`` in 1 .. 256, ``iters`` in 1 .. 64, ``angle`` in (0, 90] degrees, ``falloff``
    in [0, 1], ``sigma`` in (0, 1e6], ``step`` in (0, 1], ``normal_k`` in 1 .. 256 (None: ``min(2 k, 256)``) -> ``Params``;
    ``ValueError`` otherwise."""
    iters = _int_in("iters", iters, 1, MAX_ITERS)
    angle = _float_in("angle", angle, 0.0, 90.0, "(0, 90] degrees")
    if not angle > 0.0:
        raise ValueError("angle must be a finite number in (0, 90] degrees: got %r" % (angle,))
    cos_t = min(max(math.cos(math.radians(angle)), 0.0), MAX_COS)     # an angle below 0.081 degrees is served at the entry's limit
    k, cos_t, falloff, sigma, step = check_pass(k, cos_t, falloff, sigma, step)
    normal_k = min(2 * k, _lib.KNN_MAX_K) if normal_k is None else _int_in("normal_k", normal_k, 1, _lib.KNN_MAX_K)
    return Params(k, iters, angle, falloff, sigma, step, normal_k, cos_t)


def as_params(denoise):
    """``denoise=`` of the estimators -> ``Params`` or None: None or False (off), True (the defaults) or a dict of the keyword
    arguments ``k``, ``iters``, ``angle``, ``falloff``, ``sigma``, ``step``, ``normal_k``.  ``ValueError`` otherwise."""
    if denoise is None or denoise is False:
        return None
    if denoise is True:
        return check_params()
    if isinstance(denoise, Params):
        return check_params(*denoise[:len(KEYS)])
    if isinstance(denoise, dict):
        extra = sorted(set(denoise) - set(KEYS), key=repr)
        if extra:
            raise ValueError("denoise: unknown key%s %s (%s)" % ("s" if len(extra) > 1 else "", ", ".join(map(repr, extra)), ", ".join(KEYS)))
        return check_params(**denoise)
    raise ValueError("denoise must be None, True or a dict of %s: got %r" % (", ".join(KEYS), denoise))


def refuse_pidx(pidx):
    """``denoise=`` with ``pidx=``: ``ValueError`` -- the filter moves all points, and the rows of a subset would not be the rows of
    ``points``; denoise first (``denoise_points``) and index the result."""
    if pidx is not None:
        raise ValueError("denoise with pidx is not served: the filter moves all points of the cloud and the result's points would not "
                         "have the rows of pidx; denoise first (denoise.denoise_points) and index the denoised cloud")


def denoise_cloud(cloud, normals_dev, params, stream=None):
    """``params.iters`` Jacobi passes over ALL points of a prepared ``provider.CloudPatches`` (no ``pidx``, no ``queries``;
    ``radius_grid=False`` serves).  Every pass works on the CURRENT positions: it searches lists of ``max(k, normal_k)`` on them,
    fits plane normals over their first ``normal_k`` entries (``CloudPatches.pca_knn``) -- or, with ``normals_dev`` [n_points,3] f32 on
    the cloud's device, holds that field fixed for every pass, e.g. Hough normals after smoothing, which keep creases -- and moves
    every point over the first ``k`` entries (``CloudPatches.denoise_knn``).  The cloud's own buffer is never written; a pass after the
    first prepares the moved points as a cloud of their own, which takes them through the host once (the search grid is sized from
    their bounding box).  Returns a dict of device tensors

      points   [n_points,3] f32   the final positions
      delta    [n_points]   f32   the length of the displacement from the input row to the final row
      support  [n_points]   f32   the sum of the weights of the last pass
      count    [n_points]   int32 the neighbours that had a weight in the last pass
      moved    []           int64 the rows whose bits changed

    Synchronises between passes (the host copy), not after the last."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    params = as_params(params)
    if params is None:
        raise ValueError("denoise_cloud: params must be given")
    if cloud.pidx is not None or cloud.queries is not None:
        raise ValueError("denoise_cloud: the filter runs over all points of a cloud: no pidx, no queries")
    n = cloud.n_points
    dev = cloud.device
    if normals_dev is not None and (not isinstance(normals_dev, torch.Tensor) or normals_dev.dtype != torch.float32
                                    or tuple(normals_dev.shape) != (n, 3) or not normals_dev.is_contiguous() or normals_dev.device != dev):
        raise ValueError("normals: a contiguous float32 [n_points, 3] tensor on %s" % dev)
    K = max(params.k, params.normal_k) if normals_dev is None else params.k
    cur = cloud
    with torch.cuda.device(dev):
        for it in range(params.iters):
            st = cur._stream(stream)
            nbr = cur.knn(0, n, K, stream=st)[0]
            normals = normals_dev if normals_dev is not None else cur.pca_knn(0, n, (params.normal_k,), nbr=nbr, stream=st)[0][:, 0, :].contiguous()
            points, _, support, count = cur.denoise_knn(normals, 0, n, params.k, params.cos_t, params.falloff, params.sigma, params.step,
                                                        nbr=nbr, stream=st)
            if it + 1 < params.iters:
                with torch.cuda.stream(st):
                    cur = CloudPatches(points.cpu().numpy(), NestiConfig(), device=dev, radius_grid=False)
        with torch.cuda.stream(cloud._stream(stream)):
            diff = points.double() - cloud.cloud.double()
            delta = (diff * diff).sum(1).sqrt().float()
            moved = (points.view(torch.int32) != cloud.cloud.view(torch.int32)).any(1).sum()
    return {"points": points, "delta": delta, "support": support, "count": count, "moved": moved}


def denoise_points(pts, k=DEFAULT_K, iters=DEFAULT_ITERS, angle=DEFAULT_ANGLE, falloff=DEFAULT_FALLOFF, sigma=DEFAULT_SIGMA,
                   step=DEFAULT_STEP, normals=None, normal_k=None, device="cuda:0"):
    """Denoise the positions of a cloud: numpy in, a dict out (synchronises).

      points   [N,3] f32    the denoised positions, row for row
      delta    [N]   f32    the length of the displacement from the input row to the final row
      support  [N]   f32    the sum of the weights of the last pass
      count    [N]   int32  the neighbours that had a weight in the last pass, the point itself included
      moved    int          the rows whose bits changed

    ``iters`` (1 .. 64) Jacobi passes over the ``k`` (1 .. 256) nearest neighbours of the CURRENT positions.  In a pass a point moves
    along its normal by ``step`` (in (0, 1]) times the weighted mean of its neighbours' heights ``h`` over its tangent plane; a
    neighbour's weight is ``(u t g)^2`` with ``t`` falling linearly in the cosine between the normals from 1 (parallel) to 0 at
    ``angle`` degrees (in (0, 90]), ``u = 1 - falloff d^2 / r^2`` over the neighbourhood's radius ``r`` (``falloff`` in [0, 1]) and
    ``g = 1 / (1 + (h / (sigma r))^2)`` (``sigma`` in (0, 1e6]: the height scale in radii; 1e6 switches the height weight off).  The
    normals are plane fits over the ``normal_k`` (default ``2 k``) nearest neighbours, fitted again in every pass -- or the field
    ``normals`` [N,3] (any sign, any length; a row that is 0 0 0 or not finite does not move and weighs nothing), held fixed for
    every pass.  A point never moves tangentially; thin features shrink and too many passes drift.  Raises ``ValueError``
    for arguments outside their ranges and for a cloud that is not [N,3] or not finite."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    params = check_params(k, iters, angle, falloff, sigma, step, normal_k)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("pts must be [N, 3]: got %s" % (pts.shape,))
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != pts.shape:
            raise ValueError("pts and normals must both be [N, 3]: got %s and %s" % (pts.shape, normals.shape))
    if not len(pts):                                                         # nothing to move, and no bounding box to prepare
        return {"points": pts, "delta": np.zeros(0, np.float32), "support": np.zeros(0, np.float32), "count": np.zeros(0, np.int32),
                "moved": 0}
    cloud = CloudPatches(pts, NestiConfig(), device=device, radius_grid=False)
    with torch.cuda.device(cloud.device):
        res = denoise_cloud(cloud, None if normals is None else torch.from_numpy(normals).to(cloud.device), params)
        torch.cuda.current_stream(cloud.device).synchronize()
    out = {key: res[key].cpu().numpy() for key in ("points", "delta", "support", "count")}
    out["moved"] = int(res["moved"])
    return out
