"""Consistent orientation of estimated normals on the GPU (``csrc/orient.hip``; DESIGN.md 2 "Orientation"): Hoppe's spanning-tree
propagation made unique, or the single-viewpoint rule.  Nesti-Net's loss is unoriented, so the signs of ``.normals`` rows are
whatever the routed expert produced; the consumer of a consistent sign is the reference's "RMS oriented"
(``utils/evaluate.py:151``), Poisson reconstruction, shading.  There is no CPU fallback.

Sharded callers (``dist.estimate_sharded``) orient the gathered result: ``orient_normals(positions, normals, r_abs[-1])``."""
import ctypes

import numpy as np

from . import _lib

MODES = {"mst": _lib.ORIENT_MST, "viewpoint": _lib.ORIENT_VIEWPOINT}
STAT_NAMES = ("n_eligible", "n_components", "n_flipped", "n_edges")


def _check_args(radius, k, viewpoint, mode):
    if mode not in MODES:
        raise ValueError("mode must be 'mst' or 'viewpoint', not %r" % (mode,))
    if not 1 <= int(k) <= 16:
        raise ValueError("k must be in [1, 16]")
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0")
    if viewpoint is not None:
        viewpoint = np.asarray(viewpoint, np.float64).reshape(-1)
        if viewpoint.shape != (3,) or not np.isfinite(viewpoint).all():
            raise ValueError("viewpoint must be three finite numbers")
    elif mode == "viewpoint":
        raise ValueError("mode 'viewpoint' needs a viewpoint")
    return viewpoint


def orient_device(xyz, normals, radius, k=8, viewpoint=None, mode="mst", stream=None, tree_edge_out=None):
    """``nesti_orient_normals`` on device tensors: ``xyz`` [M,3] and ``normals`` [M,3] contiguous float32 on one GPU; ``normals`` is
    oriented IN PLACE on ``stream`` (default: the current one).  Returns the stats as an int32[4] device tensor (``STAT_NAMES``);
    nothing synchronises.  Positions of eligible rows must be finite (``orient_normals`` checks that)."""
    import torch
    viewpoint = _check_args(radius, k, viewpoint, mode)
    lib = _lib.load()
    if not (xyz.is_cuda and normals.is_cuda and xyz.device == normals.device):
        raise _lib.NestiError("orient_device needs both tensors on one GPU: there is no CPU fallback")
    for t in (xyz, normals):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError("xyz and normals must be contiguous float32 [M, 3]")
    M = xyz.shape[0]
    if normals.shape[0] != M:
        raise ValueError("xyz and normals differ in length")
    dev = xyz.device
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        if M == 0:
            return stats
        gws = torch.empty(lib.nesti_patches_workspace_bytes(M), dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.nesti_orient_workspace_bytes(M, int(k)), dtype=torch.uint8, device=dev)
        vp = (ctypes.c_double * 3)(*viewpoint) if viewpoint is not None else None
        _lib.check(lib.nesti_orient_normals(_lib.ptr(xyz), M, _lib.ptr(normals), MODES[mode], ctypes.c_double(radius), int(k), vp,
                                            _lib.ptr(gws), gws.numel(), _lib.ptr(ws), ws.numel(), _lib.ptr(tree_edge_out),
                                            _lib.ptr(stats), ctypes.c_void_p(stream.cuda_stream)), "nesti_orient_normals")
    return stats


def harmless_positions(xyz):
    """Device tensor [M,3] with every non-finite row replaced by the first finite one (no synchronisation).  For rows whose normal is
    ineligible anyway -- the sentinel rows of position queries -- which then only feed the search grid's bounding box."""
    import torch
    finite = torch.isfinite(xyz).all(dim=1)
    first = torch.argmax(finite.to(torch.int32))
    fill = torch.where(finite[first], xyz[first], torch.zeros_like(xyz[first]))
    return torch.where(finite[:, None], xyz, fill[None, :]).contiguous()


def stats_dict(stats):
    """The int32[4] tensor of ``orient_device`` as a dict (synchronises on the copy)."""
    return dict(zip(STAT_NAMES, (int(v) for v in stats.cpu().tolist())))


def orient_normals(xyz, normals, radius, k=8, viewpoint=None, mode="mst", device="cuda:0", stream=None):
    """Orient ``normals`` [M,3] at positions ``xyz`` [M,3] (numpy arrays or torch tensors) -> (oriented normals of the kind that came
    in, stats dict).  Only sign bits change: a row comes back as itself or negated; rows whose normal is not finite or is
    (0, 0, 0) -- the sentinel of a query without a neighbourhood -- come back untouched and are nobody's neighbour.

    ``mode='mst'``: neighbours are the ``k`` (1 .. 16) nearest inside ``radius``; signs propagate along the minimum spanning forest
    of the 1 - cos^2 weights from each tree's root -- the vertex with the largest z, made to point up, or with ``viewpoint`` the
    vertex nearest to it, made to face it.  Every tree is oriented on its own: ``stats['n_components']`` tells how many there are.
    ``mode='viewpoint'``: every row is made to face ``viewpoint`` (a single-sensor scan).

    Raises ``ValueError`` for a non-finite position on an eligible row, ``NestiError`` without the library or a GPU."""
    import torch
    _check_args(radius, k, viewpoint, mode)
    as_numpy = not hasattr(normals, "data_ptr")
    x = np.asarray(xyz, np.float32) if not hasattr(xyz, "data_ptr") else xyz.detach().to(torch.float32).cpu().numpy()
    n = np.asarray(normals, np.float32) if as_numpy else normals.detach().to(torch.float32).cpu().numpy()
    if x.ndim != 2 or x.shape[1] != 3 or n.shape != x.shape:
        raise ValueError("xyz and normals must both be [M, 3]")
    eligible = np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
    finite = np.isfinite(x).all(axis=1)
    if (eligible & ~finite).any():
        raise ValueError("position %d is not finite but its normal is eligible for orientation" % int(np.nonzero(eligible & ~finite)[0][0]))
    if not finite.all():
        # ineligible rows take part in nothing but the search grid's bounding box: give them a harmless position
        x = x.copy()
        x[~finite] = x[finite][0] if finite.any() else 0.0
    _lib.load()                                        # NestiError if the library is missing
    if not torch.cuda.is_available():
        raise _lib.NestiError("orient_normals needs a GPU: there is no CPU fallback")
    dev = normals.device if (not as_numpy and normals.is_cuda) else torch.device(device)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        nd = torch.from_numpy(np.ascontiguousarray(n)).to(dev)
        stats = orient_device(xd, nd, float(radius), k, viewpoint, mode, st)
        st.synchronize()
        out = nd.cpu().numpy() if as_numpy else nd.to(normals.device)
    return out, stats_dict(stats)
