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
    valid pixels on the stride); ``viewpoint``: the camera centre, three floats on the host."""
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
    return DepthCloud(xyz[:n_valid], pix[:n_valid], rank, qidx[:n_queries], n_valid, n_queries, H, W, s, camera.centre)


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
