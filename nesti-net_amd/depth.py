"""Depth images in, normal images out (``csrc/depth.hip``; DESIGN.md 2 "Depth images"): the two ends of the reference's Kinect route --
``MATLAB/ScanNet_depth2xyz.m`` before the network, ``MATLAB/ScanNet_world2cam_normals.m`` after it -- on the GPU.

The conventions are the library's own (include/nesti_hip.h): pixel coordinates are 0-BASED, ``u`` = column, ``v`` = row (the MATLAB
files are 1-based: a caller with MATLAB-convention intrinsics passes ``cx - 1``, ``cy - 1``); the pose is a proper rigid transform,
translation included; where several rows project onto one pixel the nearest wins.  There is no CPU fallback."""
import ctypes
import dataclasses
import math

import numpy as np

from . import _lib


@dataclasses.dataclass
class Camera:
    """Pinhole intrinsics, the depth unit and range, and an optional pose (3 x 4 or 4 x 4, row-major ``[R | t]``): camera -> world for
    :func:`depth_to_cloud`, world -> camera for :func:`project_to_image` (:meth:`inverse` turns one into the other)."""
    fx: float
    fy: float
    cx: float
    cy: float
    depth_scale: float = 1.0
    z_near: float = 0.0
    z_far: float = math.inf
    pose: object = None

    def pose34(self):
        """The pose as a float64 [3,4] array, or None.  ``ValueError`` for another shape or a bottom row that is not 0 0 0 1."""
        if self.pose is None:
            return None
        T = np.asarray(self.pose, np.float64)
        if T.shape == (4, 4):
            if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
                raise ValueError("a 4 x 4 pose must end in the row 0 0 0 1")
            T = T[:3]
        if T.shape != (3, 4):
            raise ValueError("the pose must be 3 x 4 or 4 x 4, not %s" % (T.shape,))
        return np.ascontiguousarray(T)

    def to_c(self):
        c = _lib.CCamera()
        for name in ("fx", "fy", "cx", "cy", "depth_scale", "z_near", "z_far"):
            setattr(c, name, float(getattr(self, name)))
        T = self.pose34()
        c.has_pose = int(T is not None)
        if T is not None:
            c.pose[:] = T.reshape(-1).tolist()
        return c

    @classmethod
    def from_c(cls, c):
        pose = np.array(c.pose[:], np.float64).reshape(3, 4) if c.has_pose else None
        return cls(c.fx, c.fy, c.cx, c.cy, c.depth_scale, c.z_near, c.z_far, pose)

    @property
    def centre(self):
        """The camera centre in the coordinates of the cloud :func:`depth_to_cloud` produces: the pose's translation column, or the
        origin.  The viewpoint of ``orient='viewpoint'``."""
        T = self.pose34()
        return np.zeros(3) if T is None else T[:, 3].copy()

    def inverse(self):
        """The same camera with the inverse rigid pose (R^T, -R^T t), computed in float64."""
        T = self.pose34()
        if T is None:
            return dataclasses.replace(self)
        R, t = T[:, :3], T[:, 3]
        return dataclasses.replace(self, pose=np.concatenate([R.T, -(R.T @ t)[:, None]], axis=1))


@dataclasses.dataclass
class DepthCloud:
    """What :func:`depth_to_cloud` returns.  Device tensors, rows in row-major pixel order: ``xyz`` [n_valid,3] f32, ``pix`` [n_valid]
    int32 (pixel index ``v W + u``), ``rank`` [H W] int32 (cloud row of a pixel or -1), ``qidx`` [n_queries] int32 (cloud rows of the
    valid pixels on the stride); ``viewpoint``: the camera centre, three floats on the host; ``camera``: the :class:`Camera` itself."""
    xyz: object
    pix: object
    rank: object
    qidx: object
    n_valid: int
    n_queries: int
    H: int
    W: int
    stride: int
    viewpoint: object
    camera: object = None             # the Camera of the back-projection: what :func:`window_knn` proves its lists with


def _upload_depth(depth, dev):
    """depth [H,W] uint16 / float32 (numpy or torch) -> (contiguous device tensor, NESTI_DEPTH_*).  uint16 travels as its int16 bits."""
    import torch
    if hasattr(depth, "data_ptr"):
        if depth.dim() != 2:
            raise ValueError("depth must be [H, W]")
        if depth.dtype == torch.float32:
            return depth.to(dev).contiguous(), _lib.DEPTH_F32
        if depth.dtype == torch.uint16:
            return depth.contiguous().view(torch.int16).to(dev), _lib.DEPTH_U16
        raise ValueError("depth must be uint16 or float32, not %s" % depth.dtype)
    d = np.asarray(depth)
    if d.ndim != 2:
        raise ValueError("depth must be [H, W]")
    if d.dtype == np.float32:
        return torch.from_numpy(np.ascontiguousarray(d)).to(dev), _lib.DEPTH_F32
    if d.dtype == np.uint16:
        return torch.from_numpy(np.ascontiguousarray(d).view(np.int16)).to(dev), _lib.DEPTH_U16
    raise ValueError("depth must be uint16 or float32, not %s" % d.dtype)


def _check_image(H, W):
    if H <= 0 or W <= 0 or H * W > _lib.DEPTH_MAX_PIXELS:
        raise ValueError("the image must have 1 .. 2^26 pixels, not %d x %d" % (H, W))


def depth_to_cloud(depth, camera, stride=1, device="cuda:0", stream=None):
    """Back-project ``depth`` [H,W] (uint16 or float32; numpy or torch) through ``camera`` (``nesti_depth_to_cloud``) -> :class:`DepthCloud`.
    A pixel is valid iff ``z = raw * depth_scale`` is finite, > 0 and inside ``[z_near, z_far]``.  ONE readback (the two counts, which
    size everything that follows); it synchronises ``stream``."""
    import torch
    if int(stride) < 1:
        raise ValueError("stride must be >= 1")
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.NestiError("depth_to_cloud needs a GPU: there is no CPU fallback")
    dev = torch.device(device)
    cam = camera.to_c()
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        d, dtype = _upload_depth(depth, dev)
        H, W = int(d.shape[0]), int(d.shape[1])
        _check_image(H, W)
        n = H * W
        s = int(stride)
        xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
        pix = torch.empty((n,), dtype=torch.int32, device=dev)
        rank = torch.empty((n,), dtype=torch.int32, device=dev)
        qidx = torch.empty((((H + s - 1) // s) * ((W + s - 1) // s),), dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.nesti_depth_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
        _lib.check(lib.nesti_depth_to_cloud(_lib.ptr(d), dtype, H, W, ctypes.byref(cam), s, _lib.ptr(xyz), _lib.ptr(pix), _lib.ptr(rank),
                                            _lib.ptr(qidx), _lib.ptr(counts), _lib.ptr(ws), ws.numel(),
                                            ctypes.c_void_p(st.cuda_stream)), "nesti_depth_to_cloud")
        n_valid, n_queries = (int(v) for v in counts.cpu().tolist())          # the one readback
    return DepthCloud(xyz[:n_valid], pix[:n_valid], rank, qidx[:n_queries], n_valid, n_queries, H, W, s, camera.centre, camera)


def _fill_words(fill, C, torch_dtype):
    """``fill`` (a scalar or C values) as C 4-byte words of the rows' element type."""
    import torch
    np_dtype = np.float32 if torch_dtype == torch.float32 else np.int32
    f = np.asarray(fill, np_dtype).reshape(-1)
    if f.size == 1:
        f = np.repeat(f, C)
    if f.shape != (C,):
        raise ValueError("fill must be a scalar or %d values" % C)
    return np.ascontiguousarray(f)


def _rows_2d(rows):
    import torch
    if rows.dtype not in (torch.float32, torch.int32):
        raise ValueError("rows must be float32 or int32")
    if rows.dim() not in (1, 2):
        raise ValueError("rows must be [M] or [M, C]")
    r = rows[:, None] if rows.dim() == 1 else rows
    if not 1 <= r.shape[1] <= 8:
        raise ValueError("rows must have 1 .. 8 columns")
    return r.contiguous()


def scatter_to_image(rows, pix, H, W, fill=0, stream=None):
    """``rows`` [M] or [M,C] (float32 or int32 device tensor, C <= 8) written at the pixels ``pix`` [M] of a new [H,W] / [H,W,C] image of
    ``fill`` (``nesti_image_scatter``).  A ``pix`` entry outside the image is skipped.  Nothing synchronises."""
    import torch
    lib = _lib.load()
    _check_image(H, W)
    if not rows.is_cuda:
        raise _lib.NestiError("scatter_to_image needs device tensors: there is no CPU fallback")
    dev = rows.device
    flat = rows.dim() == 1
    r = _rows_2d(rows)
    M, C = int(r.shape[0]), int(r.shape[1])
    if pix.shape != (M,) or pix.dtype != torch.int32 or pix.device != dev:
        raise ValueError("pix must be int32 [M] on the device of rows")
    f = _fill_words(fill, C, r.dtype)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        image = torch.empty((H, W) if flat else (H, W, C), dtype=r.dtype, device=dev)
        p = pix.contiguous()
        _lib.check(lib.nesti_image_scatter(_lib.ptr(r) if M else None, _lib.ptr(p) if M else None, M, C, H, W, _lib.ptr(f),
                                           _lib.ptr(image), ctypes.c_void_p(st.cuda_stream)), "nesti_image_scatter")
    return image


def project_to_image(xyz, values, camera, H, W, fill=0, stream=None):
    """Project a cloud that did not come from :func:`depth_to_cloud` into an image (``nesti_project_to_image``): ``xyz`` [M,3] f32 and
    ``values`` [M] / [M,C] (float32 or int32, C <= 8) device tensors; ``camera.pose`` is WORLD -> CAMERA here (``Camera.inverse``).
    Per pixel the nearest row wins, among equals the smaller row index.  Returns (image [H,W] / [H,W,C], index_image [H,W] int32: the
    winning row or -1).  Nothing synchronises."""
    import torch
    lib = _lib.load()
    _check_image(H, W)
    if not (xyz.is_cuda and values.is_cuda and xyz.device == values.device):
        raise _lib.NestiError("project_to_image needs device tensors on one GPU: there is no CPU fallback")
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be float32 [M, 3]")
    dev = xyz.device
    flat = values.dim() == 1
    v = _rows_2d(values)
    M, C = int(v.shape[0]), int(v.shape[1])
    if xyz.shape[0] != M:
        raise ValueError("xyz and values differ in length")
    f = _fill_words(fill, C, v.dtype)
    cam = camera.to_c()
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        x = xyz.contiguous()
        image = torch.empty((H, W) if flat else (H, W, C), dtype=v.dtype, device=dev)
        index = torch.empty((H, W), dtype=torch.int32, device=dev)
        ws = torch.empty(lib.nesti_depth_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
        _lib.check(lib.nesti_project_to_image(_lib.ptr(x) if M else None, _lib.ptr(v) if M else None, M, C, H, W, ctypes.byref(cam),
                                              _lib.ptr(f), _lib.ptr(image), _lib.ptr(index), _lib.ptr(ws), ws.numel(),
                                              ctypes.c_void_p(st.cuda_stream)), "nesti_project_to_image")
    return image, index


# ---- image-window neighbour lists and model-free normals (csrc/window.hip; DESIGN.md 2 "Image-window neighbourhoods") ---------------
WINDOW_FACTOR = 1.5
ESTIMATORS = ("pca", "quadric", "hough", "robust", "select")


def default_window(k):
    """The half-width R of the pixel window for ``k`` neighbours: ``ceil(WINDOW_FACTOR * sqrt(k / pi))``, within 1 ..
    ``_lib.WINDOW_MAX_R``.  On a surface seen face-on the ``k`` nearest points fill a disc of ``sqrt(k / pi)`` pixels radius; the factor
    1.5 leaves the room the proof needs on tilted surfaces.  Measured on the 96 x 128 test scene (the restatement of
    tests/_window_fixture.py predicts the flags bit for bit; profiles/window_check.json has the 480 x 640 frame): with the factor 1.5 the
    window proves 98.5 / 97.4 / 95.4 / 94.2 / 92.6 / 90.6 % of the rows at k = 8 / 16 / 32 / 64 / 128 / 256; with a window as wide as
    the disc itself (factor 1) 94.6 / 93.4 / 86.8 / 61.1 / 40.8 / 28.5 %; with the factor 2, 99.4 / 99.0 / 98.6 / 98.5 / 97.9 / 94.0 %
    at 1.8 x the candidates.  The rows left over sit at depth discontinuities and on steep surfaces.  The choice moves the share of
    rows the exact mode re-searches, never a result."""
    from .knn import check_k
    return max(1, min(_lib.WINDOW_MAX_R, int(math.ceil(WINDOW_FACTOR * math.sqrt(check_k(k) / math.pi)))))


def check_window(window, k):
    """``window`` -- ``'auto'`` (:func:`default_window`) or an int in 1 .. ``_lib.WINDOW_MAX_R`` -- as the half-width R; ``ValueError``
    otherwise."""
    if isinstance(window, str) and window == "auto":
        return default_window(k)
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= int(window) <= _lib.WINDOW_MAX_R:
        raise ValueError("window must be 'auto' or an integer in 1 .. %d: got %r" % (_lib.WINDOW_MAX_R, window))
    return int(window)


def window_knn(dc, k, window="auto", exact=True, rows=None, stream=None, cloud=None):
    """The ``k`` nearest cloud points of the rows of a :class:`DepthCloud` among the points of a (2 R + 1)^2 pixel window round each
    row's pixel (``nesti_depth_window_knn``): all rows, or the cloud rows ``rows`` (int32 [M] on the device: ``dc.qidx`` for a strided
    frame).  Device tensors ``(idx [M,k] int32, d2 [M,k] float64, n [M] int32, proven [M] int32)``; ``proven`` is 1 where the window's
    list is PROVEN to be the exact k-NN list over the whole cloud, bit for bit ``knn.knn``'s row.  ``window``: ``'auto'``
    (:func:`default_window`) or R in 1 .. 15.

    ``exact=True``: the unproven rows are compacted (one readback: their number), searched by ``CloudPatches.knn_rows`` over a
    search-only grid -- built only when there is such a row; ``cloud``: a prepared ``CloudPatches`` of ``dc.xyz`` to search with instead
    of one made here, which passes the cloud through the host -- and written back.  The result then equals ``knn.knn`` on every row;
    ``proven`` is returned as it came from the window.  ``exact=False``: the window's lists as they are, nothing read back.

    The proof presumes an untouched cloud: ``dc`` as :func:`depth_to_cloud` returned it, under a rigid pose."""
    import torch
    from .knn import check_k
    k = check_k(k)
    R = check_window(window, k)
    if dc.camera is None:
        raise ValueError("window_knn: the DepthCloud carries no camera (depth_to_cloud sets it)")
    lib = _lib.load()
    dev = dc.xyz.device
    N = int(dc.n_valid)
    if rows is not None and (not hasattr(rows, "data_ptr") or rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != dev):
        raise ValueError("rows: an int32 [M] tensor on %s" % dev)
    M = N if rows is None else int(rows.shape[0])
    cam = dc.camera.to_c()
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        idx = torch.empty((M, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((M, k), dtype=torch.float64, device=dev)
        n = torch.empty((M,), dtype=torch.int32, device=dev)
        proven = torch.empty((M,), dtype=torch.int32, device=dev)
        if M == 0 or N == 0:
            return idx, d2, n, proven
        xyz, pix, rank = dc.xyz.contiguous(), dc.pix.contiguous(), dc.rank.contiguous()
        q = None if rows is None else rows.contiguous()
        _lib.check(lib.nesti_depth_window_knn(_lib.ptr(xyz), N, _lib.ptr(pix), _lib.ptr(rank), dc.H, dc.W, ctypes.byref(cam), _lib.ptr(q), M, 0,
                                              R, k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(n), _lib.ptr(proven),
                                              ctypes.c_void_p(st.cuda_stream)), "nesti_depth_window_knn")
        if exact:
            open_rows = torch.nonzero(proven == 0).reshape(-1)              # the one readback: their number
            if open_rows.numel():
                if cloud is None:
                    from .config import NestiConfig
                    from .provider import CloudPatches
                    cloud = CloudPatches(xyz.cpu().numpy(), NestiConfig(), device=dev, radius_grid=False)
                which = open_rows.to(torch.int32) if q is None else q[open_rows].contiguous()
                e_idx, e_d2, e_n = cloud.knn_rows(which, k, stream=st)
                idx.index_copy_(0, open_rows, e_idx)
                d2.index_copy_(0, open_rows, e_d2)
                n.index_copy_(0, open_rows, e_n)
    return idx, d2, n, proven


def _fit_by_name(estimator):
    from . import hough, pca, quadric, robust, select
    return {"pca": pca.pca_cloud, "quadric": quadric.quadric_cloud, "hough": hough.hough_cloud, "robust": robust.robust_cloud,
            "select": select.select_cloud}[estimator]


def check_normals_args(estimator, knn, ladder, scale, stride, orient, smooth):
    """The argument checks of :func:`depth_normals` that need no GPU -> (neighbour counts, the largest count to search at, the smoothing
    parameters or None); ``ValueError`` otherwise."""
    from . import smooth as _smooth
    from .knn import check_ks
    from .pca import ORIENT_MODES, check_scale
    if estimator not in ESTIMATORS:
        raise ValueError("estimator must be one of %s: got %r" % (", ".join(ESTIMATORS), estimator))
    if int(stride) < 1:
        raise ValueError("stride must be >= 1")
    if orient not in ORIENT_MODES:
        raise ValueError("orient must be None, 'mst' or 'viewpoint'")
    if estimator == "select":
        from .select import DEFAULT_LADDER, check_ladder
        ks = check_ladder(DEFAULT_LADDER if ladder is None else ladder)
    else:
        if ladder is not None:
            raise ValueError("ladder belongs to estimator='select'")
        ks = check_ks(knn)
        check_scale(scale, len(ks))
    sm = _smooth.as_params(smooth)
    if sm is not None and int(stride) != 1:
        raise ValueError("smooth needs stride == 1: on a strided frame the rows' neighbours would have no normal")
    return ks, max(ks[-1], sm.k if sm is not None else 0), sm


def depth_normals(depth, camera, estimator="pca", knn=(32,), scale=-1, window="auto", exact=True, stride=1, orient="viewpoint",
                  orient_k=8, smooth=None, device="cuda:0", **params):
    """Depth frame in, MODEL-FREE normal image out: back-project ``depth`` [H,W] (uint16 or float32) through ``camera``
    (:func:`depth_to_cloud`), search ONCE over the pixel windows (:func:`window_knn`) at the largest neighbour count -- ``max(knn)``, or
    the smoothing's ``k`` where that is larger --, run ``estimator`` and the optional smoothing over those lists, orient, scatter.

    ``estimator``: ``'pca'`` (plane fit), ``'quadric'``, ``'hough'``, ``'robust'`` -- over the neighbour counts ``knn`` (an int or up to
    four ascending ints), ``scale`` indexing them -- or ``'select'`` (the scale-selected plane fit; ``ladder=`` instead of ``knn=``);
    ``params`` are the estimator's own keywords (``triplets``, ``iters``, ``slack``, ...).  ``stride`` > 1 estimates at the valid pixels
    on the stride only; the neighbourhoods still come from every valid pixel.  ``orient``: ``'viewpoint'`` (the camera centre),
    ``'mst'`` or None.  ``smooth`` (``smooth.as_params``) needs ``stride == 1``.  ``exact=True``: every row's list is the exact k-NN list
    (the rows the window cannot prove are searched on the grid), so the result equals the estimator's own ``*_normals(xyz, knn=...)``
    bit for bit; ``exact=False``: the window's lists as they are -- at a depth discontinuity a row may then miss a nearer point of a
    far-away pixel.

    Returns a dict of numpy arrays (synchronises): the estimator's usual arrays per estimated pixel (``normals`` [M,3] among them),
    ``xyz`` [M,3], ``pix`` [M], ``normal_map`` [H,W,3] f32 (fill 0 0 0), for the quadric fit ``curv_map`` [H,W,2] (fill 0 0), ``window``
    (R), ``window_proven`` [M] bool and ``window_exact_rows`` (the rows re-searched; 0 with ``exact=False``).  A frame without a valid
    pixel gives all-fill maps and empty rows.  Raises ``ValueError`` for a bad ``estimator``, ``knn``, ``window``, ``scale`` or
    ``orient`` and for ``smooth`` with ``stride > 1``."""
    import torch
    from .config import NestiConfig
    from .provider import CloudPatches
    ladder = params.pop("ladder", None)
    ks, kmax, sm = check_normals_args(estimator, knn, ladder, scale, stride, orient, smooth)
    R = check_window(window, kmax)
    dc = depth_to_cloud(depth, camera, stride=stride, device=device)
    H, W, dev = dc.H, dc.W, dc.xyz.device
    sparse = dc.stride > 1
    rows = dc.n_queries if sparse else dc.n_valid
    with torch.cuda.device(dev):
        if rows == 0:
            res = {"normals": np.zeros((0, 3), np.float32)}
            xyz, pix = dc.xyz[:0], dc.pix[:0]
            proven = np.zeros(0, bool)
            n_exact = 0
            if estimator == "quadric":
                res["curv"] = np.zeros((0, 2), np.float32)
        else:
            cloud = CloudPatches(dc.xyz.cpu().numpy(), NestiConfig(), device=dev, pidx=dc.qidx.cpu().numpy() if sparse else None,
                                 radius_grid=False)
            lists, _, _, proven = window_knn(dc, kmax, R, exact, rows=dc.qidx if sparse else None, cloud=cloud)
            proven = proven.cpu().numpy().astype(bool)
            n_exact = int((~proven).sum()) if exact else 0
            common = dict(orient=orient, viewpoint=dc.viewpoint, orient_k=orient_k, smooth=sm, lists=lists)
            if estimator == "select":
                res = _fit_by_name(estimator)(cloud, ks, **common, **params)
            else:
                res = _fit_by_name(estimator)(cloud, knn=ks, scale=scale, **common, **params)
            sel = dc.qidx.long() if sparse else None
            xyz = dc.xyz[sel] if sparse else dc.xyz
            pix = dc.pix[sel].contiguous() if sparse else dc.pix
        res["normal_map"] = scatter_to_image(torch.from_numpy(res["normals"]).to(dev), pix, H, W, 0.0).cpu().numpy()
        if estimator == "quadric":
            res["curv_map"] = scatter_to_image(torch.from_numpy(res["curv"]).to(dev), pix, H, W, 0.0).cpu().numpy()
        res.update(xyz=xyz.cpu().numpy(), pix=pix.cpu().numpy(), window=R, window_proven=proven, window_exact_rows=n_exact)
    return res


# ---- the command line's per-frame files ---------------------------------------------------------------------------------------------
def read_camera(path):
    """``<name>.camera``: one text line ``fx fy cx cy depth_scale`` -> :class:`Camera` (no pose).  ``ValueError`` for a short file or a
    number that is not finite."""
    with open(path) as f:
        words = f.read().split()
    if len(words) < 5:
        raise ValueError("%s: expected 'fx fy cx cy depth_scale', found %d numbers" % (path, len(words)))
    try:
        v = [float(w) for w in words[:5]]
    except ValueError:
        raise ValueError("%s: not a number among %s" % (path, words[:5]))
    if not all(math.isfinite(x) for x in v):
        raise ValueError("%s: the camera's numbers must be finite, got %s" % (path, v))
    return Camera(*v)


def read_cam2world(path):
    """``<name>.cam2world``: 4 x 4 text, camera -> world -> float64 [4,4].  ``ValueError`` for fewer than 16 numbers, a number that is
    not finite, or a bottom row that is not 0 0 0 1."""
    with open(path) as f:
        words = f.read().split()
    if len(words) != 16:
        raise ValueError("%s: expected 4 x 4 numbers, found %d" % (path, len(words)))
    try:
        T = np.array([float(w) for w in words], np.float64).reshape(4, 4)
    except ValueError:
        raise ValueError("%s: not a number in the matrix" % path)
    if not np.isfinite(T).all():
        raise ValueError("%s: the pose must be finite" % path)
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("%s: the last row of a rigid pose is 0 0 0 1" % path)
    return T


def read_depth(path):
    """``<name>.depth.npy``: [H,W] uint16 or float32."""
    d = np.load(path)
    if d.ndim != 2 or d.dtype not in (np.uint16, np.float32):
        raise ValueError("%s: expected a [H,W] uint16 or float32 array, found %s %s" % (path, d.dtype, d.shape))
    return d
