"""Voxel-grid downsampling before estimation on the GPU (``csrc/voxel.hip``; DESIGN.md 2 "Voxel downsampling"): one point per occupied
cell of a regular grid -- the centroid of the cell's points, or the point nearest it.  A key per row, a stable device-wide radix sort of
(key, row) pairs and a reduction of the sorted runs, all on the device.  The five numpy-in model-free estimators take it as
``downsample=`` (``pca.pca_normals``, ``quadric.quadric_fit``, ``hough.hough_normals``, ``robust.robust_normals``,
``select.select_normals``; ``--voxel_size`` on the command line): the estimator -- and ``outliers=``, which comes second -- then runs on
the downsampled cloud and its per-row results come back with the rows of the input, every row holding the result of its voxel.
Voxels come in key order (z-major), not input order; a centroid is not an input point, so nothing per-point is carried except through
``rep``; the grid's origin is the cloud's minimum corner unless ``origin=`` is given, so one far point moves every voxel -- filter
strays first (``outliers.remove_outliers``) or pass ``origin=``.  The conventions are the library's own (no parity with PCL's
VoxelGrid or Open3D's voxel_down_sample is claimed).  There is no CPU fallback."""
import collections

import numpy as np

from . import outliers as _outliers
from ._args import int_in as _int_in
from .stages import take_result, take_rows

MODES = ("centroid", "nearest")
KEYS = ("voxel", "mode", "origin")
MAX_CELLS = 1 << 62                    # nesti_voxel_keys: the number of cells stays below it

# voxel: three floats (the cloud's units); mode; origin: three floats or None (the cloud's minimum corner)
Params = collections.namedtuple("Params", KEYS)


def _triple(name, v, positive):
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        a = np.asarray(float("nan"))
    if isinstance(v, (bool, str)) or a.shape not in ((), (3,)) or not np.isfinite(a).all() or (positive and not (a > 0).all()):
        raise ValueError("%s must be a finite%s number or three of them: got %r" % (name, " positive" if positive else "", v))
    return tuple(float(x) for x in np.broadcast_to(a, (3,)))


def check_voxel(voxel):
    """``voxel`` -- a finite positive number or three of them -- as three floats; ``ValueError`` otherwise."""
    return _triple("voxel", voxel, True)


def check_origin(origin):
    """``origin`` -- three finite numbers (or one, for all axes) -- as three floats; ``ValueError`` otherwise."""
    return _triple("origin", origin, False)


def check_key_bits(key_bits):
    """The low bits a sort looks at, 1 .. 64, as an int; ``ValueError`` otherwise."""
    return _int_in("key_bits", key_bits, 1, 64)


def check_grid(origin, voxel, dims):
    """(origin, voxel, dims) of ``nesti_voxel_keys`` as three tuples; ``ValueError`` for a non-finite origin, a voxel size that is not
    finite and positive, a ``dims`` entry below 1 or a number of cells of 2^62 or more."""
    origin, voxel = check_origin(origin), check_voxel(voxel)
    try:
        dims = tuple(int(d) for d in dims)
    except (TypeError, ValueError):
        dims = ()
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError("dims must be three integers >= 1: got %r" % (dims,))
    if dims[0] * dims[1] * dims[2] >= MAX_CELLS:
        raise ValueError("dims %r: the number of cells must be below 2^62" % (dims,))
    return origin, voxel, dims


def check_params(voxel, mode="centroid", origin=None):
    """The one place where the ranges are checked -> ``Params``; ``ValueError`` otherwise.  ``voxel``: a finite positive number or three
    of them, in the cloud's units.  ``mode`` 'centroid' (the points are the cells' centroids) or 'nearest' (the cloud's own row nearest
    each centroid, bit for bit).  ``origin``: None (the cloud's minimum corner) or three finite numbers."""
    voxel = check_voxel(voxel)
    if mode not in MODES:
        raise ValueError("mode must be 'centroid' or 'nearest': got %r" % (mode,))
    return Params(voxel, mode, None if origin is None else check_origin(origin))


def as_params(downsample):
    """``downsample=`` of the estimators -> ``Params`` or None: None (off), a number or three (the voxel size, mode 'centroid') or a dict
    of the keyword arguments of ``check_params``.  ``ValueError`` otherwise."""
    if downsample is None:
        return None
    if isinstance(downsample, Params):
        return check_params(*downsample)
    if isinstance(downsample, dict):
        extra = sorted(set(downsample) - set(KEYS), key=repr)
        if extra:
            raise ValueError("downsample: unknown key%s %s (%s)" % ("s" if len(extra) > 1 else "", ", ".join(map(repr, extra)), ", ".join(KEYS)))
        if "voxel" not in downsample:
            raise ValueError("downsample: a dict needs 'voxel', the voxel size")
        return check_params(**downsample)
    if isinstance(downsample, (bool, str)):
        raise ValueError("downsample must be None, a voxel size or a dict of %s: got %r" % (", ".join(KEYS), downsample))
    return check_params(downsample)


def refuse_pidx(pidx):
    """``downsample=`` with ``pidx=``: ``ValueError`` -- left for later."""
    if pidx is not None:
        raise ValueError("downsample with pidx is not served yet: the voxel grid renumbers the cloud, and a pidx entry names a point "
                         "that no longer exists as a row; downsample first (downsample.voxel_downsample) and index the result")


def grid_of(lo, hi, params):
    """The grid of a cloud whose float32 corners are ``lo`` and ``hi``: (origin, voxel, dims, lost_key, key_bits).  ``origin`` is
    ``params.origin`` or ``lo``; the dims are computed in fp64 exactly as the kernel computes a cell,
    ``floor(((double)hi_a - origin_a) / voxel_a) + 1`` (at least 1); ``lost_key`` is their product, the key of a row outside the grid,
    and ``key_bits`` its bit length: what the sort has to look at.  ``ValueError`` naming the voxel size where the product reaches 2^62."""
    origin = tuple(float(np.float64(x)) for x in lo) if params.origin is None else params.origin
    dims = []
    with np.errstate(over="ignore"):
        for a in range(3):
            t = np.floor((np.float64(np.float32(hi[a])) - np.float64(origin[a])) / np.float64(params.voxel[a]))
            dims.append(int(t) + 1 if np.isfinite(t) else MAX_CELLS)
    dims = tuple(max(1, d) for d in dims)
    lost = dims[0] * dims[1] * dims[2]
    if lost >= MAX_CELLS:
        raise ValueError("voxel size %s is too small for this cloud: the grid would have %s cells (dims %s), 2^62 or more"
                         % (list(params.voxel), "%.3g" % float(lost), list(dims)))
    return origin, params.voxel, dims, lost, lost.bit_length()


def cells_of(key, dims):
    """``key`` [V] uint64 -> ``cell`` [V,3] int64, the (i_x, i_y, i_z) of ``key = (i_z dims_y + i_y) dims_x + i_x``."""
    key = np.asarray(key, np.uint64)
    dx, dy = np.uint64(dims[0]), np.uint64(dims[1])
    return np.stack([key % dx, (key // dx) % dy, key // (dx * dy)], axis=1).astype(np.int64).reshape(-1, 3)


def voxel_cloud(cloud, params, stream=None):
    """The device form: downsample ALL points of a prepared ``provider.CloudPatches`` (no ``pidx``, no ``queries``;
    ``radius_grid=False`` serves): ``CloudPatches.voxel_keys``, ``sort_pairs`` and ``voxel_reduce`` on one stream, then ONE readback
    (synchronises), of V.  Returns a dict of device tensors

      points    [V,3] f32    ``centroid``, or in mode 'nearest' the cloud's rows ``rep``, bit for bit
      centroid  [V,3] f32
      rep       [V]   int64  the row nearest its voxel's fp64 centroid, the lower index on a tie
      count     [V]   int32
      key       [V]   int64  the uint64 bits; ascending
      voxel_of  [N]   int64  the voxel of every row (-1: outside a caller's grid)

    and ``origin``, ``voxel``, ``dims`` (tuples), ``lost_key``, ``key_bits`` and ``n_voxels`` (ints).  Every byte is a pure function
    of (cloud, parameters)."""
    import torch
    params = as_params(params)
    if params is None:
        raise ValueError("voxel_cloud: params must be given")
    if cloud.pidx is not None or cloud.queries is not None:
        raise ValueError("voxel_cloud: the grid runs over all points of a cloud: no pidx, no queries")
    if not cloud.n_points:
        raise ValueError("voxel_cloud: an empty cloud")
    origin, voxel, dims, lost, key_bits = grid_of(cloud.host_pts.min(0), cloud.host_pts.max(0), params)
    st = cloud._stream(stream)
    keys = cloud.voxel_keys(origin, voxel, dims, stream=st)
    skeys, sidx = cloud.sort_pairs(keys, key_bits, stream=st)
    centroid, rep, count, key, voxel_of, n_voxels = cloud.voxel_reduce(skeys, sidx, lost, origin, stream=st)
    with torch.cuda.device(cloud.device), torch.cuda.stream(st):
        V = int(n_voxels.cpu()[0])                                           # the one readback (synchronises)
        rep = rep[:V].long()
        centroid = centroid[:V]
        points = centroid if params.mode == "centroid" else cloud.cloud[rep]
        res = {"points": points, "centroid": centroid, "rep": rep, "count": count[:V], "key": key[:V], "voxel_of": voxel_of.long()}
    res.update(origin=origin, voxel=voxel, dims=dims, lost_key=lost, key_bits=key_bits, n_voxels=V)
    return res


def voxel_downsample(pts, voxel, mode="centroid", origin=None, device="cuda:0"):
    """Downsample a cloud on a voxel grid: numpy in, a dict of numpy arrays out (synchronises).

      points    [V,3] f32    one per occupied cell, cells in ascending key order (z-major): ``centroid`` or, in mode 'nearest',
                             ``pts[rep]`` bit for bit
      centroid  [V,3] f32    origin + (the fp64 sum of p - origin over the cell's rows, in a fixed order) / count, rounded once
      rep       [V]   int64  the row nearest the fp64 centroid; the lower index on a tie
      count     [V]   int32
      key       [V]   uint64 (i_z dims_y + i_y) dims_x + i_x
      cell      [V,3] int64  (i_x, i_y, i_z)
      voxel_of  [N]   int64  the voxel of every row of ``pts`` (-1: a row outside the grid of a caller's ``origin``)
      origin, voxel [3] f64 and dims [3] int64

    ``voxel``: a finite positive number or three, in the cloud's units; cell i_a of a coordinate is ``floor((p_a - origin_a) /
    voxel_a)`` in fp64.  ``origin=None``: the cloud's minimum corner; with a caller's origin the rows below it are lost.  An empty
    cloud gives empty arrays.  Every byte is a pure function of (cloud, parameters).  Raises ``ValueError`` for parameters outside
    their ranges, for a voxel so small that the grid would have 2^62 cells or more, and for a cloud that is not [N,3] or not finite."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    params = check_params(voxel, mode, origin)
    pts = _outliers.check_cloud(pts)
    if not len(pts):
        org = (0.0, 0.0, 0.0) if params.origin is None else params.origin
        return {"points": pts, "centroid": pts.copy(), "rep": np.zeros(0, np.int64), "count": np.zeros(0, np.int32),
                "key": np.zeros(0, np.uint64), "cell": np.zeros((0, 3), np.int64), "voxel_of": np.zeros(0, np.int64),
                "origin": np.asarray(org, np.float64), "voxel": np.asarray(params.voxel, np.float64), "dims": np.ones(3, np.int64)}
    bad = np.flatnonzero(~np.isfinite(pts).all(axis=1))
    if len(bad):
        raise ValueError("cloud row %d is not finite: %s" % (bad[0], pts[bad[0]].tolist()))
    grid_of(pts.min(0), pts.max(0), params)                                  # a voxel too small for the cloud is refused before any device work
    cloud = CloudPatches(pts, NestiConfig(), device=device, radius_grid=False)
    res = voxel_cloud(cloud, params)
    with torch.cuda.device(cloud.device):
        torch.cuda.current_stream(cloud.device).synchronize()
    key = res["key"].cpu().numpy().view(np.uint64)
    return {"points": res["points"].cpu().numpy().reshape(-1, 3), "centroid": res["centroid"].cpu().numpy().reshape(-1, 3),
            "rep": res["rep"].cpu().numpy(), "count": res["count"].cpu().numpy(), "key": key, "cell": cells_of(key, res["dims"]),
            "voxel_of": res["voxel_of"].cpu().numpy(), "origin": np.asarray(res["origin"], np.float64),
            "voxel": np.asarray(res["voxel"], np.float64), "dims": np.asarray(res["dims"], np.int64)}


# ---- the voxels' rows back to the rows of the input ----------------------------------------------------------------------------------------
def gather_host(rows, voxel_of, fill=0):
    """Host: numpy ``rows`` [V, ...] of the voxels -> [N, ...] with ``rows[voxel_of[i]]`` at row i and ``fill`` where ``voxel_of`` is -1."""
    return take_rows(rows, voxel_of, fill)


def gather_result(res, voxel_of, rows):
    """A result dict of numpy arrays over the ``rows`` voxels -> over the rows of the input: every array whose first dimension is
    ``rows`` is gathered through ``voxel_of``, with 0 -- ``expert``: -1 -- in the lost rows; everything else passes through."""
    return take_result(res, voxel_of, rows)
