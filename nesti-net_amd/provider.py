"""Host-side mirror of the reference's data seam.

``provider.get_data_loader(...)`` (``utils/provider.py:319-429``) returns
``(DataLoader, PointcloudPatchDataset)`` whose batches are
``([b,S*P,3] f32, [b,3,3], [b,S] f64)``.  :func:`get_data_loader` here has the same
keyword arguments for the inference configuration (``test_n_est_w_experts.py:109-116``)
and yields the same tuple, but the patches are produced by the HIP ball-query kernel
(``nesti_patches_build``) from a cloud resident in HBM instead of one Python
``__getitem__`` per point.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import knn as _knn
from . import orient as _orient
from .config import NestiConfig


def load_xyz(path):
    """``np.loadtxt(point_filename).astype('float32')`` with the ``.npy`` cache the reference
    writes next to the file (``utils/pcpnet_dataset.py:249-251``, ``:13-14``)."""
    npy = path + ".npy"
    if os.path.exists(npy) and os.path.getmtime(npy) >= os.path.getmtime(path):
        return np.load(npy)
    pts = np.loadtxt(path).astype("float32")
    if pts.ndim == 1:
        pts = pts.reshape(1, -1)
    pts = np.ascontiguousarray(pts[:, :3])
    try:
        np.save(npy, pts)
    except OSError:
        pass   # read-only dataset dir: the cache is an optimisation only
    return pts


def load_qxyz(path):
    """``<shape>.qxyz``: the query positions of a shape, a text file of M rows x 3 read like ``.xyz`` (no cache file)."""
    q = np.loadtxt(path).astype("float32")
    if q.ndim == 1:
        q = q.reshape(1, -1) if q.size else q.reshape(0, 3)
    return np.ascontiguousarray(q[:, :3])


def check_queries(queries):
    """``queries`` as a contiguous float32 [M,3] host array, or a float32 [M,3] torch tensor left where it is.  ``ValueError``
    for another shape, and for a host array with a non-finite entry (the first bad row is named): a position without
    coordinates is a mistake of the caller.  The kernels themselves serve any bit pattern (such a query has empty balls)."""
    if isinstance(queries, torch.Tensor):
        if queries.dim() != 2 or queries.shape[1] != 3:
            raise ValueError("queries must be [M,3]: got %s" % (tuple(queries.shape),))
        return queries.to(torch.float32)
    q = np.asarray(queries)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("queries must be [M,3]: got %s" % (q.shape,))
    q = np.ascontiguousarray(q, dtype=np.float32)
    bad = np.flatnonzero(~np.isfinite(q).all(axis=1))
    if len(bad):
        raise ValueError("queries row %d is not finite: %s" % (bad[0], q[bad[0]].tolist()))
    return q


def check_out(out, specs, device, what=""):
    """``out=`` of a method that writes a tuple of tensors: ``specs`` is that tuple as ``(shape, dtype)`` pairs.  None -> fresh tensors
    on ``device``; otherwise the caller's own as a tuple, each contiguous, of its shape and dtype and on ``device`` -- ``ValueError``
    naming ``what`` (the tuple in words) if not."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dt, device=device) for shape, dt in specs)
    out = tuple(out)
    if len(out) != len(specs) or any(tuple(t.shape) != tuple(shape) or t.dtype != dt or not t.is_contiguous() or t.device != device
                                     for t, (shape, dt) in zip(out, specs)):
        raise ValueError("out: contiguous %s on %s" % (what, device))
    return out


class CloudPatches:
    """One shape: the cloud in HBM + its uniform search grid (replaces ``load_shape`` /
    ``cKDTree``, ``utils/pcpnet_dataset.py:13-39``).  ``build(rows)`` extracts patches.

    ``queries`` ([M,3], converted to float32; mutually exclusive with ``pidx``): the patch centres are these POSITIONS instead
    of cloud points -- a downsampled copy, mesh vertices, voxel centres, another sweep -- while the neighbourhoods come from
    this cloud and ``r_abs`` from ITS bounding box.  Patch row i is ``queries[i]``; a position whose balls are all empty gets
    the sentinel outputs.

    ``radius_grid=False`` skips the radius grid: only :meth:`knn`, :meth:`knn_rows`, :meth:`pca_knn`, :meth:`quadric_knn`, :meth:`hough_knn`,
    :meth:`pca_select`, :meth:`smooth_knn`, :meth:`denoise_knn`, the outlier filter's :meth:`outlier_scores`, :meth:`outlier_threshold` and
    :meth:`outlier_compact` and the voxel grid's :meth:`voxel_keys`, :meth:`sort_pairs` and :meth:`voxel_reduce` may then be called."""

    def __init__(self, pts, cfg: NestiConfig, device="cuda:0", seed=3627473, pidx=None, queries=None, radius_grid=True):
        if pidx is not None and queries is not None:
            raise ValueError("pidx and queries are mutually exclusive: a query is a cloud point (pidx) or a position (queries)")
        if queries is not None:
            queries = check_queries(queries)
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        bad = np.flatnonzero(~np.isfinite(pts).all(axis=1)) if pts.ndim == 2 else []
        if len(bad):      # one infinite coordinate makes bbdiag, and with it every radius, infinite: no grid can be built for it
            raise ValueError("cloud row %d is not finite: %s" % (bad[0], pts[bad[0]].tolist()))
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.NestiError("CloudPatches needs a GPU: libnesti_hip.so has no CPU path")
        self.cfg, self.device, self.seed = cfg, torch.device(device), int(seed)
        self.host_pts = pts                   # kept for the opt-in reference-order subsample (pipeline.py: subsample='reference')
        self.n_points = pts.shape[0]
        # utils/pcpnet_dataset.py:281-282 -- float64 Python arithmetic on the host, like the reference
        self.bbdiag = float(np.linalg.norm(pts.max(0) - pts.min(0), 2))
        self.r_abs = [self.bbdiag * rad for rad in cfg.patch_radius]
        self.cloud = torch.from_numpy(pts).to(self.device)
        if pidx is not None:
            pidx = np.asarray(pidx).astype(np.int64).reshape(-1)
            if len(pidx) and (pidx.min() < 0 or pidx.max() >= self.n_points):      # a bad .pidx file must not read out of bounds
                raise ValueError("pidx entries must lie in [0, %d): got [%d, %d]" % (self.n_points, pidx.min(), pidx.max()))
        self.pidx = None if pidx is None else torch.as_tensor(pidx, dtype=torch.int32, device=self.device)
        self.patch_count = self.n_points if pidx is None else len(pidx)     # :276-279
        self.queries = None
        if queries is not None:
            self.queries = (queries if isinstance(queries, torch.Tensor) else torch.from_numpy(queries)).to(self.device).contiguous()
            self.patch_count = self.queries.shape[0]
        nbytes = self.lib.nesti_patches_workspace_bytes(self.n_points)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._c = cfg.to_c()
        self._r = (ctypes.c_double * len(self.r_abs))(*self.r_abs)
        # radius_grid=False: a cloud prepared for the k-NN entries alone (knn.knn), which build their own search grid and serve a cloud
        # without extent -- a single point, say -- whose radii are 0 and whose radius grid cannot be built
        self._has_radius_grid = bool(radius_grid)
        self._extent = pts.max(0).astype(np.float64) - pts.min(0) if len(pts) else np.zeros(3)
        self._knn_grids = {}                  # search-only grids of the k-NN entries: key -> (workspace, build event); knn_grid
        if radius_grid:
            self.build_grid()

    def _stream(self, stream):
        """``stream``, or the current stream of the cloud's device."""
        return stream if stream is not None else torch.cuda.current_stream(self.device)

    def _rows(self, first, count):
        """(at, queries) of patch rows [first, first + count), validated: ``at`` -- the queries are positions; ``queries`` -- their
        [count,3] positions, the [count] indices of ``pidx``, or None (row i is cloud point first + i)."""
        if first < 0 or count < 0 or first + count > self.patch_count:
            raise ValueError("patch rows [%d, %d) outside [0, %d)" % (first, first + count, self.patch_count))
        if self.queries is not None:
            return True, self.queries[first:first + count]
        return False, (self.pidx[first:first + count].contiguous() if self.pidx is not None else None)

    def _call(self, name, at, q, count, first, args, stream, ball=True, seed=(), keyed=False):
        """One entry over patch rows: ``name``, or ``name + "_at"`` where the queries are positions, called on the cloud's device and
        checked under that name.  The two argument layouts of include/nesti_hip.h: a ball entry (``ball``) takes the configuration,
        the radii, ``query_row0`` in both forms (after ``seed`` where it has one) and, behind its own ``args``, the radius grid; a
        k-NN or list-fit entry takes ``query_row0`` in the index form only -- in both forms where its hash is keyed by the row
        (``keyed``: the Hough entries).  The stream comes last."""
        entry = name + "_at" if at else name
        head = (_lib.ptr(self.cloud), self.n_points, _lib.ptr(q), count)
        row0 = (ctypes.c_int(first),)
        if ball:
            head = (ctypes.byref(self._c),) + head + (self._r,) + seed + row0
            args = tuple(args) + (_lib.ptr(self._ws), self._ws.numel())
        elif not at or keyed:
            head += row0
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, entry)(*head, *args, ctypes.c_void_p(stream.cuda_stream)), entry)

    def centre_positions(self):
        """The [patch_count, 3] positions of the patch rows (device): the query positions made harmless for an orientation pass
        (``orient.harmless_positions``: a non-finite position has no neighbourhood, its row is the sentinel), ``cloud[pidx]``, or the
        cloud itself."""
        if self.queries is not None:
            return _orient.harmless_positions(self.queries)
        if self.pidx is not None:
            return self.cloud[self.pidx.long()].contiguous()
        return self.cloud

    def build_grid(self, stream=None):
        """(Re)build the uniform search grid on the device -- the cKDTree construction of the
        reference (``utils/pcpnet_dataset.py:37``).  Asynchronous on ``stream``."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nesti_patches_grid(ctypes.byref(self._c), _lib.ptr(self.cloud), self.n_points, self._r,
                                                   _lib.ptr(self._ws), self._ws.numel(), ctypes.c_void_p(self._stream(stream).cuda_stream)),
                       "nesti_patches_grid")

    def _patch_out(self, count, out, want_idx):
        """(points [count,S*P,3] f32, n_eff [count,S] int32) -- the two of ``out`` as they are, where given -- and nbr [count,S*P]
        int32 or None."""
        S, P = self.cfg.n_scales, self.cfg.num_point
        points, n_eff = out if out is not None else check_out(None, (((count, S * P, 3), torch.float32), ((count, S), torch.int32)), self.device)
        return points, n_eff, (torch.empty((count, S * P), dtype=torch.int32, device=self.device) if want_idx else None)

    def build(self, first, count, want_idx=False, out=None, stream=None):
        """Patches for local patch rows [first, first+count) (file order, or ``pidx`` order when
        sparse -- ``utils/pcpnet_dataset.py:292-295``).

        Returns points [count,S*P,3] f32, n_eff [count,S] int32 (+ nbr_idx [count,S*P], n_ball
        [count,S] when ``want_idx``).  The subsample key uses the global row ``first + i`` so
        results do not depend on batching."""
        at, q = self._rows(first, count)
        points, n_eff, nbr = self._patch_out(count, out, want_idx)
        n_ball = torch.empty((count, self.cfg.n_scales), dtype=torch.int32, device=self.device) if want_idx else None
        self._call("nesti_patches_query", at, q, count, first, [_lib.ptr(t) for t in (points, n_eff, nbr, n_ball)], self._stream(stream),
                   seed=(ctypes.c_uint64(self.seed),))
        if want_idx:
            return points, n_eff, nbr, n_ball
        return points, n_eff

    # ---- the reference's own subsample order on the GPU (utils/pcpnet_dataset.py:304, 320-321; patches.hip: patches_ref_kernel) ----
    def ensure_tree_order(self):
        """cKDTree's visiting order as a sort key: ``scipy.spatial.cKDTree(pts, 10)`` exactly as the reference builds it
        (``utils/pcpnet_dataset.py:37``); ``query_ball_point`` returns a ball in ascending position in ``tree.indices``
        (tests/test_refreplay.py), so the kernel only needs ``rank[i]`` = that position and ``order`` = ``tree.indices``."""
        if getattr(self, "_tree_rank", None) is None:
            from scipy import spatial
            tree = spatial.cKDTree(self.host_pts, 10)
            order = np.ascontiguousarray(tree.indices, dtype=np.int32)
            rank = np.empty(self.n_points, np.int32)
            rank[order] = np.arange(self.n_points, dtype=np.int32)
            self._ref_tree = tree            # the host path (refsample.ReferencePatchSampler) uses the same tree
            self._tree_order = torch.from_numpy(order).to(self.device)
            self._tree_rank = torch.from_numpy(rank).to(self.device)
        return self._tree_rank, self._tree_order

    def _index_queries_only(self, what):
        """The reference-order entries exist to diff against a reference run, which has only index queries."""
        if self.queries is not None:
            raise _lib.NestiError("%s: the reference's subsample order is defined for index queries only; a cloud with position "
                                  "queries uses subsample='hash'" % what)

    def count_balls(self, first, count, stream=None):
        """Ball sizes [count, S] int32 (device) of patch rows [first, first + count): what the reference's random stream needs
        (``nesti_patches_count``)."""
        self._index_queries_only("count_balls")
        at, q = self._rows(first, count)
        n_ball = torch.empty((count, self.cfg.n_scales), dtype=torch.int32, device=self.device)
        self._call("nesti_patches_count", at, q, count, first, [_lib.ptr(n_ball)], self._stream(stream))
        return n_ball

    def pca(self, first, count, out=None, stream=None):
        """Plane-fit normals of patch rows [first, first + count) at every scale (``nesti_pca_normals`` / ``nesti_pca_normals_at``;
        DESIGN.md 2 "Plane-fit normals"): device tensors ``(normals [count,S,3] f32, eig [count,S,3] f32, n_ball [count,S] int32)``,
        or the three of ``out``.  Serves all points, ``pidx`` and ``queries``; asynchronous on ``stream``.  A scale whose ball holds
        fewer than 3 points has normal 0 0 0 and eigenvalues 0 0 0.  For this grid a row's bits do not depend on the batching."""
        S = self.cfg.n_scales
        at, q = self._rows(first, count)
        out = check_out(out, (((count, S, 3), torch.float32), ((count, S, 3), torch.float32), ((count, S), torch.int32)), self.device,
                        "(normals [count,S,3] f32, eig [count,S,3] f32, n_ball [count,S] int32)")
        self._call("nesti_pca_normals", at, q, count, first, [_lib.ptr(t) for t in out], self._stream(stream))
        return out

    def quadric(self, first, count, out=None, stream=None):
        """Quadric-fit normals and principal curvatures of patch rows [first, first + count) at every scale (``nesti_quadric_fit`` /
        ``nesti_quadric_fit_at``; DESIGN.md 2 "Quadric fit"): device tensors ``(normals [count,S,3] f32, curv [count,S,2] f32 (k_max,
        k_min; absolute units), plane [count,S,3] f32 (the bits of ``pca``'s normals), n_ball [count,S] int32)``, or the four of ``out``.
        Serves all points, ``pidx`` and ``queries``; asynchronous on ``stream``.  A failed fit (fewer than 6 points in the ball, no plane
        normal, a singular system) has normal 0 0 0 and curvatures 0 0.  For this grid a row's bits do not depend on the batching."""
        S = self.cfg.n_scales
        at, q = self._rows(first, count)
        out = check_out(out, (((count, S, 3), torch.float32), ((count, S, 2), torch.float32), ((count, S, 3), torch.float32),
                              ((count, S), torch.int32)), self.device,
                        "(normals [count,S,3] f32, curv [count,S,2] f32, plane [count,S,3] f32, n_ball [count,S] int32)")
        self._call("nesti_quadric_fit", at, q, count, first, [_lib.ptr(t) for t in out], self._stream(stream))
        return out

    # ---- k-nearest neighbourhoods (csrc/knn.hip; DESIGN.md 2 "k-nearest neighbourhoods") ----------------------------------------
    KNN_GRIDS_KEPT = 4                        # search-only grids kept per cloud, each the size of the radius grid's workspace

    def knn_grid(self, grid, k, stream):
        """The grid workspace of a k-NN search: ``grid`` None -> the search-only grid of ``knn.default_radius(N, k, extent)``, built
        with the one-scale ``nesti_patches_grid`` on first use; ``"radius"`` -> the patch grid of this cloud (left untouched); a
        positive float -> a grid of that pseudo-radius.  Built grids are kept by pseudo-radius, the ``KNN_GRIDS_KEPT`` most recently
        used; an older one is dropped (its memory is held until the work queued on ``stream`` so far is done; a caller that
        searches one cloud from several streams over more grids than that orders them itself).  A grid is built on ``stream``; a later call on another stream waits for that build.  The choice moves the time of a
        search, never its result."""
        if isinstance(grid, str):
            if grid != "radius":
                raise ValueError("grid must be None, 'radius' or a positive pseudo-radius: got %r" % (grid,))
            if not self._has_radius_grid:
                raise ValueError("grid='radius': this cloud was prepared without its radius grid")
            return self._ws
        if grid is None:
            radius = _knn.default_radius(self.n_points, _knn.check_k(k), self._extent)
        else:
            radius = float(grid)
            if not (radius > 0.0 and np.isfinite(radius)):
                raise ValueError("grid must be None, 'radius' or a positive pseudo-radius: got %r" % (grid,))
        if radius in self._knn_grids:
            ws, built = self._knn_grids.pop(radius)
        else:
            while len(self._knn_grids) >= self.KNN_GRIDS_KEPT:
                old_ws, _ = self._knn_grids.pop(next(iter(self._knn_grids)))      # the least recently used
                old_ws.record_stream(stream)
            ws = torch.empty(self._ws.numel(), dtype=torch.uint8, device=self.device)
            one = NestiConfig.for_model("ss_norm_est").to_c()      # a one-scale config: the grid reads n_scales and the radius
            with torch.cuda.device(self.device):
                _lib.check(self.lib.nesti_patches_grid(ctypes.byref(one), _lib.ptr(self.cloud), self.n_points, (ctypes.c_double * 1)(radius),
                                                       _lib.ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream)), "nesti_patches_grid")
            built = torch.cuda.Event()
            built.record(stream)
        self._knn_grids[radius] = (ws, built)                                     # most recently used last
        stream.wait_event(built)
        return ws

    def knn(self, first, count, k, grid=None, stream=None):
        """The ``k`` nearest cloud points of patch rows [first, first + count) (``nesti_knn`` / ``nesti_knn_at``): device tensors
        ``(idx [count,k] int32, d2 [count,k] float64, n [count] int32)``; -1 / +inf beyond ``n = min(k, N)``.  Exact and independent of
        ``grid`` (:meth:`knn_grid`).  Serves all points, ``pidx`` and ``queries``; asynchronous on ``stream``."""
        k = _knn.check_k(k)
        at, q = self._rows(first, count)
        st = self._stream(stream)
        ws = self.knn_grid(grid, k, st)
        out = check_out(None, (((count, k), torch.int32), ((count, k), torch.float64), ((count,), torch.int32)), self.device)
        if count:                         # 0 rows: a no-op; an empty tensor has no address to pass
            self._call("nesti_knn", at, q, count, first, [k] + [_lib.ptr(t) for t in out] + [_lib.ptr(ws), ws.numel()], st, ball=False)
        return out

    def knn_rows(self, rows, k, grid=None, stream=None):
        """:meth:`knn` for the cloud points ``rows`` (a contiguous int32 [count] tensor on the cloud's device, whatever ``pidx`` or
        ``queries`` the cloud was prepared with): what ``depth.window_knn`` hands its unproven rows to.  An index is clamped into the
        cloud, as by ``nesti_knn``."""
        k = _knn.check_k(k)
        if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous()
                or rows.device != self.device):
            raise ValueError("rows: a contiguous int32 [count] tensor on %s" % self.device)
        count = int(rows.shape[0])
        st = self._stream(stream)
        out = check_out(None, (((count, k), torch.int32), ((count, k), torch.float64), ((count,), torch.int32)), self.device)
        if count:                         # 0 rows: no grid is built
            ws = self.knn_grid(grid, k, st)
            self._call("nesti_knn", False, rows, count, 0, [k] + [_lib.ptr(t) for t in out] + [_lib.ptr(ws), ws.numel()], st, ball=False)
        return out

    def _fit_nbr(self, name, first, count, ks, grid, nbr, widths, stream, params=(), keyed=False):
        """One list-fit entry over the rows' sorted neighbour lists -- ``nbr`` [count, K], or one search at K = max(ks): outputs of
        ``widths`` (a width w: f32 [count,S,w]; a pair (tail, dtype): [count,S] + tail) + radius + count.  ``params``: the entry's own
        arguments between the scales and the outputs; ``keyed``: see :meth:`_call`."""
        ks = _knn.check_ks(ks)
        st = self._stream(stream)
        if nbr is None:
            nbr = self.knn(first, count, ks[-1], grid=grid, stream=st)[0]
        at, q = self._rows(first, count)
        S = len(ks)
        if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != count or not nbr.is_contiguous() or nbr.device != self.device:
            raise ValueError("nbr: a contiguous int32 [count, K] tensor on %s" % self.device)
        specs = tuple(((count, S) + tuple(w[0]), w[1]) if isinstance(w, tuple) else ((count, S, w), torch.float32) for w in widths)
        out = check_out(None, specs + (((count, S), torch.float32), ((count, S), torch.int32)), self.device)
        if count:                         # 0 rows: a no-op; an empty list has no address to pass
            self._call(name, at, q, count, first,
                       [_lib.ptr(nbr), int(nbr.shape[1]), (ctypes.c_int32 * S)(*ks), S] + list(params) + [_lib.ptr(t) for t in out],
                       st, ball=False, keyed=keyed)
        return out

    def pca_knn(self, first, count, ks, grid=None, nbr=None, stream=None):
        """Plane-fit normals of patch rows [first, first + count) over their nearest neighbours: scale s is the first ``ks[s]``
        entries of ONE sorted list (one search at K = max(ks), then ``nesti_pca_normals_nbr``).  Device tensors ``(normals [count,S,3]
        f32, eig [count,S,3] f32 in units of the neighbourhood's own radius squared, radius [count,S] f32, n [count,S] int32)``.
        ``nbr`` [count,K] int32: the caller's own lists instead of a search (untrusted: a row ends at its first entry outside the
        cloud).  A row's bits are a pure function of (cloud, centre, ks): independent of batching, streams, ``grid`` and grid build.
        Serves all points, ``pidx`` and ``queries``; asynchronous on ``stream``."""
        return self._fit_nbr("nesti_pca_normals_nbr", first, count, ks, grid, nbr, (3, 3), stream)

    def pca_select(self, first, count, ladder, slack=0.0, nbr=None, grid=None, stream=None):
        """The scale-selected plane fit of patch rows [first, first + count) (``nesti_pca_select_nbr`` / ``_at``; DESIGN.md 2
        "Scale-selected plane fit"): the plane fit of :meth:`pca_knn` at every neighbour count of ``ladder`` (1 .. 32 strictly ascending
        counts in 1 .. 256) over ONE sorted list (one search at K = ladder[-1]), and per row the candidate of smallest surface variation
        -- the largest one within ``v_min (1 + slack)``.  Device tensors ``(normals [count,3] f32, eig [count,3] f32, sel [count] int32
        (the index into the ladder, -1: no candidate could be fitted and the row is 0), k [count] int32 (the neighbours used), radius
        [count] f32, variation_all [count,L] f32, normals_all [count,L,3] f32, eig_all [count,L,3] f32, radius_all [count,L] f32,
        count_all [count,L] int32)``; candidate c of the ``*_all`` tensors holds the bits of ``pca_knn`` at ``ks=(ladder[c],)``.
        ``nbr`` [count,K >= ladder[-1]] int32: the caller's own lists instead of the search (untrusted, as for :meth:`pca_knn`).
        Serves all points, ``pidx`` and ``queries``; asynchronous on ``stream``."""
        from . import select as _select
        ladder, slack = _select.check_ladder(ladder), _select.check_slack(slack)
        st = self._stream(stream)
        if nbr is None:
            nbr = self.knn(first, count, ladder[-1], grid=grid, stream=st)[0]
        at, q = self._rows(first, count)
        L = len(ladder)
        if (nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != count or nbr.shape[1] < ladder[-1] or not nbr.is_contiguous()
                or nbr.device != self.device):
            raise ValueError("nbr: a contiguous int32 [count, K >= ladder[-1]] tensor on %s" % self.device)
        f32, i32 = torch.float32, torch.int32
        out = check_out(None, (((count, 3), f32), ((count, 3), f32), ((count,), i32), ((count,), i32), ((count,), f32),
                               ((count, L), f32), ((count, L, 3), f32), ((count, L, 3), f32), ((count, L), f32), ((count, L), i32)),
                        self.device)
        if count:                         # 0 rows: a no-op; an empty list has no address to pass
            self._call("nesti_pca_select_nbr", at, q, count, first,
                       [_lib.ptr(nbr), int(nbr.shape[1]), (ctypes.c_int32 * L)(*ladder), L, ctypes.c_double(slack)]
                       + [_lib.ptr(t) for t in out], st, ball=False)
        return out

    def quadric_knn(self, first, count, ks, grid=None, nbr=None, stream=None):
        """Quadric-fit normals and principal curvatures of patch rows [first, first + count) over their nearest neighbours, as
        :meth:`pca_knn`: device tensors ``(normals [count,S,3] f32, curv [count,S,2] f32 (k_max, k_min; absolute units), plane
        [count,S,3] f32 (the bits of ``pca_knn``'s normals), radius [count,S] f32, n [count,S] int32)``."""
        return self._fit_nbr("nesti_quadric_fit_nbr", first, count, ks, grid, nbr, (3, 2, 3), stream)

    def hough_knn(self, first, count, ks, triplets, bins, rotations, seed, grid=None, nbr=None, stream=None):
        """Hough-transform normals of patch rows [first, first + count) over their nearest neighbours (``nesti_hough_normals_nbr`` /
        ``_at``; DESIGN.md 2 "Hough-transform normals"), as :meth:`pca_knn`: one search at K = max(ks), then ``triplets`` hashed
        planes per row and scale voting in ``rotations`` rotated ``bins`` x ``bins`` accumulators (``hough.ROTATIONS``).  Device
        tensors ``(normals [count,S,3] f32, conf [count,S] f32, votes [count,S,2] int32 (winning bin, valid triplets), radius
        [count,S] f32, n [count,S] int32)``.  The hash is keyed by the patch row ``first + i``, so a row's bits do not depend on the
        batching."""
        from . import hough as _hough
        T, B, R, seed = _hough.check_params(triplets, bins, rotations, seed)
        rot = _hough.rotation_table(R)
        params = [T, B, R, rot.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_uint64(seed)]
        return self._fit_nbr("nesti_hough_normals_nbr", first, count, ks, grid, nbr, (3, ((), torch.float32), ((2,), torch.int32)),
                             stream, params=params, keyed=True)

    def robust_knn(self, first, count, ks, iters, sigma, falloff, floor, init=None, nbr=None, grid=None, stream=None):
        """Robust plane-fit normals of patch rows [first, first + count) over their nearest neighbours (``nesti_robust_normals_nbr`` /
        ``_at``; DESIGN.md 2 "Robust plane fit"), as :meth:`pca_knn`: one search at K = max(ks), then ``iters`` re-weighted plane fits
        per row and scale from the plane fit's normal -- or from ``init`` [count,S,3] f32 on the device, the start normals of the rows
        (any sign; a row that is 0 0 0 or not finite comes back 0 0 0).  Device tensors ``(normals [count,S,3] f32, plane [count,S,3]
        f32 (the bits of ``pca_knn``'s normals), support [count,S] f32, inliers [count,S] int32, iters_done [count,S] int32, moments
        [count,S,10] f64 (the ten weighted sums of the last iteration), radius [count,S] f32, n [count,S] int32)``."""
        from . import robust as _robust
        iters, sigma, falloff, floor = _robust.check_params(iters, sigma, falloff, floor)
        S = len(_knn.check_ks(ks))
        if init is not None and (not isinstance(init, torch.Tensor) or init.dtype != torch.float32 or tuple(init.shape) != (count, S, 3)
                                 or not init.is_contiguous() or init.device != self.device):
            raise ValueError("init: a contiguous float32 [count, S, 3] tensor on %s" % self.device)
        params = [iters, ctypes.c_double(sigma), ctypes.c_double(falloff), ctypes.c_double(floor), None if init is None else _lib.ptr(init)]
        return self._fit_nbr("nesti_robust_normals_nbr", first, count, ks, grid, nbr,
                             (3, 3, ((), torch.float32), ((), torch.int32), ((), torch.int32), ((10,), torch.float64)), stream, params=params)

    def smooth_knn(self, normals, first, count, k, cos_t, falloff, nbr=None, grid=None, stream=None):
        """One pass of feature-preserving normal smoothing over patch rows [first, first + count) (``nesti_smooth_normals_nbr``;
        DESIGN.md 2 "Normal smoothing"): ``normals`` [n_points,3] f32 on the device holds a normal for every cloud point; a row's
        normal becomes the weighted mean of the normals of its ``k`` nearest cloud points, the weight 0 where the (unoriented) angle
        to the row's own normal reaches acos(``cos_t``) and falling with the distance by ``falloff``.  Device tensors ``(normals
        [count,3] f32, support [count] f32 (the sum of the weights), count [count] int32 (the neighbours that had one))``.  ``nbr``
        [count,K >= k] int32: the caller's own lists instead of a search at K = k (untrusted, as for :meth:`pca_knn`).  The pass is a
        Jacobi step: the returned normals are a fresh tensor, never ``normals``.  Serves all points and ``pidx``; a cloud built with
        ``queries=`` raises ``ValueError`` (a position has no normal of its own).  Asynchronous on ``stream``."""
        from . import smooth as _smooth
        if self.queries is not None:
            raise ValueError("smooth_knn: a cloud with position queries cannot be smoothed: a position has no normal of its own")
        k, cos_t, falloff = _smooth.check_pass(k, cos_t, falloff)
        if (not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (self.n_points, 3)
                or not normals.is_contiguous() or normals.device != self.device):
            raise ValueError("normals: a contiguous float32 [n_points, 3] tensor on %s" % self.device)
        st = self._stream(stream)
        if nbr is None:
            nbr = self.knn(first, count, k, grid=grid, stream=st)[0]
        at, q = self._rows(first, count)
        if (nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != count or nbr.shape[1] < k or not nbr.is_contiguous()
                or nbr.device != self.device):
            raise ValueError("nbr: a contiguous int32 [count, K >= k] tensor on %s" % self.device)
        out = check_out(None, (((count, 3), torch.float32), ((count,), torch.float32), ((count,), torch.int32)), self.device)
        if count:                         # 0 rows: a no-op; an empty list has no address to pass
            with torch.cuda.device(self.device):
                _lib.check(self.lib.nesti_smooth_normals_nbr(
                    _lib.ptr(self.cloud), self.n_points, _lib.ptr(normals), _lib.ptr(q), count, first, _lib.ptr(nbr), int(nbr.shape[1]), k,
                    cos_t, falloff, *[_lib.ptr(t) for t in out], ctypes.c_void_p(st.cuda_stream)), "nesti_smooth_normals_nbr")
        return out

    def denoise_knn(self, normals, first, count, k, cos_t, falloff, sigma, step, nbr=None, grid=None, stream=None):
        """One pass of point denoising over patch rows [first, first + count) (``nesti_denoise_points_nbr``; DESIGN.md 2 "Point
        denoising"): ``normals`` [n_points,3] f32 on the device holds a normal for every cloud point; a row's point moves along its
        own normal by ``step`` times the weighted mean of the heights of its ``k`` nearest cloud points over its tangent plane, the
        weight 0 where the (unoriented) angle between the normals reaches acos(``cos_t``), falling with the distance by ``falloff``
        and with the height over ``sigma`` neighbourhood radii.  Device tensors ``(points [count,3] f32, delta [count] f32 (the signed
        displacement along the row's normal), support [count] f32 (the sum of the weights), count [count] int32 (the neighbours that
        had one))``.  ``nbr`` [count,K >= k] int32: the caller's own lists instead of a search at K = k (untrusted, as for
        :meth:`pca_knn`).  The pass is a Jacobi step: the returned points are a fresh tensor, never the cloud.  Serves all points and
        ``pidx``; a cloud built with ``queries=`` raises ``ValueError`` (a position that is not a cloud point has nothing to move).
        Asynchronous on ``stream``."""
        from . import denoise as _denoise
        if self.queries is not None:
            raise ValueError("denoise_knn: a cloud with position queries cannot be denoised: a position that is not a cloud point has "
                             "nothing to move")
        k, cos_t, falloff, sigma, step = _denoise.check_pass(k, cos_t, falloff, sigma, step)
        if (not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (self.n_points, 3)
                or not normals.is_contiguous() or normals.device != self.device):
            raise ValueError("normals: a contiguous float32 [n_points, 3] tensor on %s" % self.device)
        st = self._stream(stream)
        if nbr is None:
            nbr = self.knn(first, count, k, grid=grid, stream=st)[0]
        at, q = self._rows(first, count)
        if (nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != count or nbr.shape[1] < k or not nbr.is_contiguous()
                or nbr.device != self.device):
            raise ValueError("nbr: a contiguous int32 [count, K >= k] tensor on %s" % self.device)
        out = check_out(None, (((count, 3), torch.float32), ((count,), torch.float32), ((count,), torch.float32), ((count,), torch.int32)),
                        self.device)
        if count:                         # 0 rows: a no-op; an empty list has no address to pass
            with torch.cuda.device(self.device):
                _lib.check(self.lib.nesti_denoise_points_nbr(
                    _lib.ptr(self.cloud), self.n_points, _lib.ptr(normals), _lib.ptr(q), count, first, _lib.ptr(nbr), int(nbr.shape[1]), k,
                    cos_t, falloff, sigma, step, *[_lib.ptr(t) for t in out], ctypes.c_void_p(st.cuda_stream)), "nesti_denoise_points_nbr")
        return out

    # ---- outlier removal (csrc/outlier.hip; DESIGN.md 2 "Outlier removal"; outliers.py) -----------------------------------------------
    def _outlier_ws(self, rows):
        """The workspace of ``nesti_outlier_threshold`` / ``nesti_outlier_compact`` for ``rows`` rows: a fresh tensor per call, so calls
        on several streams never share one."""
        return torch.empty(max(1, self.lib.nesti_outlier_workspace_bytes(max(1, int(rows)))), dtype=torch.uint8, device=self.device)

    def outlier_scores(self, first, count, k, nbr=None, grid=None, stream=None):
        """The outlier scores of cloud rows [first, first + count) (``nesti_outlier_scores_nbr``) over their ``k`` (1 .. 255) nearest
        OTHER points: device tensors ``(mean [count] f64 -- the mean distance to them, +inf where there are none --, kth_d2 [count] f64
        -- the squared distance to the k-th, +inf where fewer exist --, n_other [count] int32)``.  One search at K = k + 1 (a row is its
        own first neighbour; the slot that holds its own INDEX is the one skipped) unless ``nbr`` [count, K > k] int32 is given: the
        caller's own sorted lists (untrusted, as for :meth:`pca_knn`).  A row's bits are a pure function of (cloud, row, k).  All points
        only: a cloud built with ``pidx=`` or ``queries=`` raises ``ValueError``.  Asynchronous on ``stream``."""
        from . import outliers as _outliers
        if self.pidx is not None or self.queries is not None:
            raise ValueError("outlier_scores: the rows are the cloud's own points; a cloud built with pidx or queries is not served")
        k = _outliers.check_k(k)
        self._rows(first, count)
        st = self._stream(stream)
        if nbr is None:
            nbr = self.knn(first, count, k + 1, grid=grid, stream=st)[0]
        if (not isinstance(nbr, torch.Tensor) or nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != count or nbr.shape[1] <= k
                or not nbr.is_contiguous() or nbr.device != self.device):
            raise ValueError("nbr: a contiguous int32 [count, K > k] tensor on %s" % self.device)
        out = check_out(None, (((count,), torch.float64), ((count,), torch.float64), ((count,), torch.int32)), self.device)
        if count:                         # 0 rows: a no-op; an empty list has no address to pass
            with torch.cuda.device(self.device):
                _lib.check(self.lib.nesti_outlier_scores_nbr(_lib.ptr(self.cloud), self.n_points, first, count, _lib.ptr(nbr),
                                                             int(nbr.shape[1]), k, *[_lib.ptr(t) for t in out],
                                                             ctypes.c_void_p(st.cuda_stream)), "nesti_outlier_scores_nbr")
        return out

    def outlier_threshold(self, scores, std_ratio, stream=None):
        """The statistics of a score array on the device (``nesti_outlier_threshold``): ``scores`` [M] f64 -> ``stats`` [4] f64 = (n,
        mean, std, thr = mean + std_ratio std) over the finite scores, in a fixed order of additions; n = 0 gives (0, 0, 0, +inf).
        Nothing is read back.  Asynchronous on ``stream``."""
        from . import outliers as _outliers
        std_ratio = _outliers.check_std_ratio(std_ratio)
        if (not isinstance(scores, torch.Tensor) or scores.dtype != torch.float64 or scores.dim() != 1 or not scores.is_contiguous()
                or scores.device != self.device):
            raise ValueError("scores: a contiguous float64 [M] tensor on %s" % self.device)
        st = self._stream(stream)
        M = int(scores.shape[0])
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            stats = torch.empty(4, dtype=torch.float64, device=self.device)
            if not M:                     # the entry is a no-op for 0 rows: the statistics of no score at all
                stats.copy_(torch.tensor([0.0, 0.0, 0.0, float("inf")], dtype=torch.float64))
            else:
                ws = self._outlier_ws(M)
                _lib.check(self.lib.nesti_outlier_threshold(_lib.ptr(scores), M, std_ratio, _lib.ptr(stats), _lib.ptr(ws), ws.numel(),
                                                            ctypes.c_void_p(st.cuda_stream)), "nesti_outlier_threshold")
                ws.record_stream(st)
        return stats

    def outlier_compact(self, scores, thr, stream=None):
        """Keep the rows of the cloud whose score is finite and <= ``thr`` (``nesti_outlier_compact``): ``scores`` [n_points] f64 on the
        device; ``thr`` a host number (finite, >= 0) or a device tensor whose FIRST element is the threshold (``stats[3:]`` of
        :meth:`outlier_threshold`).  Device tensors ``(xyz [n_points,3] f32 -- its first n_kept rows are the kept points, bit for bit, in
        the cloud's order --, kept_idx [n_points] int32 -- its first n_kept entries, ascending --, new_of_old [n_points] int32 (-1: removed),
        keep [n_points] uint8, n_kept [1] int32)``.  Nothing is read back: the caller reads ``n_kept`` and slices.  Asynchronous."""
        N = self.n_points
        if (not isinstance(scores, torch.Tensor) or scores.dtype != torch.float64 or tuple(scores.shape) != (N,) or not scores.is_contiguous()
                or scores.device != self.device):
            raise ValueError("scores: a contiguous float64 [n_points] tensor on %s" % self.device)
        thr_dev, thr_host = None, 0.0
        if isinstance(thr, torch.Tensor):
            if thr.dtype != torch.float64 or thr.numel() < 1 or not thr.is_contiguous() or thr.device != self.device:
                raise ValueError("thr: a number, or a contiguous float64 tensor on %s whose first element is the threshold" % self.device)
            thr_dev = thr
        else:
            from . import outliers as _outliers
            thr_host = _outliers.check_threshold(thr)
        st = self._stream(stream)
        out = check_out(None, (((N, 3), torch.float32), ((N,), torch.int32), ((N,), torch.int32), ((N,), torch.uint8), ((1,), torch.int32)),
                        self.device)
        if N == 0:
            out[4].zero_()
            return out
        with torch.cuda.device(self.device):
            ws = self._outlier_ws(N)
            _lib.check(self.lib.nesti_outlier_compact(_lib.ptr(self.cloud), N, _lib.ptr(scores), _lib.ptr(thr_dev), thr_host,
                                                      *[_lib.ptr(t) for t in out], _lib.ptr(ws), ws.numel(),
                                                      ctypes.c_void_p(st.cuda_stream)), "nesti_outlier_compact")
            ws.record_stream(st)
        return out

    # ---- voxel-grid downsampling (csrc/voxel.hip; DESIGN.md 2 "Voxel downsampling"; downsample.py) ---------------------------------------
    # Keys cross as int64 tensors that hold the uint64 bits (torch has no arithmetic on uint64; a voxel key is below 2^62 anyway).
    VOXEL_OUTPUTS = ("centroid", "rep", "count", "key", "voxel_of")

    def _voxel_ws(self, rows):
        """The workspace of ``nesti_sort_pairs`` / ``nesti_voxel_reduce`` for ``rows`` rows: a fresh tensor per call, so calls on
        several streams never share one."""
        return torch.empty(max(1, self.lib.nesti_voxel_workspace_bytes(max(1, int(rows)))), dtype=torch.uint8, device=self.device)

    def _check_keys(self, keys, what):
        if (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_contiguous()
                or keys.device != self.device):
            raise ValueError("%s: a contiguous int64 [n] tensor (the uint64 bits) on %s" % (what, self.device))

    def voxel_keys(self, origin, voxel, dims, stream=None):
        """The voxel key of every cloud row (``nesti_voxel_keys``): ``origin`` and ``voxel`` three host floats, ``dims`` three host
        ints (``downsample.grid_of``).  A device tensor [n_points] int64 holding the uint64 keys ``(i_z dims_y + i_y) dims_x + i_x``;
        a row outside the grid has the lost key ``dims_x dims_y dims_z``.  Asynchronous on ``stream``."""
        from . import downsample as _downsample
        origin, voxel, dims = _downsample.check_grid(origin, voxel, dims)
        st = self._stream(stream)
        N = self.n_points
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            keys = torch.empty(N, dtype=torch.int64, device=self.device)
            if N:
                _lib.check(self.lib.nesti_voxel_keys(_lib.ptr(self.cloud), N, (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*voxel),
                                                     (ctypes.c_int64 * 3)(*dims), _lib.ptr(keys), ctypes.c_void_p(st.cuda_stream)),
                           "nesti_voxel_keys")
        return keys

    def sort_pairs(self, keys, key_bits, stream=None):
        """A stable sort of ``keys`` [n] int64 (the uint64 bits; any n, not only the cloud's) by their low ``key_bits`` (1 .. 64) bits
        (``nesti_sort_pairs``): device tensors ``(sorted_keys [n] int64, idx [n] int32)`` with ``sorted_keys = keys[idx]`` and ``idx`` the
        stable argsort of ``keys & mask``.  ``keys`` is left as it is.  Asynchronous on ``stream``."""
        from . import downsample as _downsample
        key_bits = _downsample.check_key_bits(key_bits)
        self._check_keys(keys, "keys")
        st = self._stream(stream)
        n = int(keys.shape[0])
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            out = check_out(None, (((n,), torch.int64), ((n,), torch.int32)), self.device)
            if n:
                ws = self._voxel_ws(n)
                _lib.check(self.lib.nesti_sort_pairs(_lib.ptr(keys), n, key_bits, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(ws), ws.numel(),
                                                     ctypes.c_void_p(st.cuda_stream)), "nesti_sort_pairs")
                ws.record_stream(st)
        return out

    def voxel_reduce(self, sorted_keys, sorted_idx, lost_key, origin, outputs=VOXEL_OUTPUTS, stream=None):
        """The voxels of the cloud from its sorted keys (``nesti_voxel_reduce``): ``sorted_keys`` / ``sorted_idx`` [n_points] as
        :meth:`sort_pairs` returns them for :meth:`voxel_keys`, ``lost_key`` = ``dims_x dims_y dims_z``, ``origin`` as for the keys.
        Device tensors ``(centroid [n_points,3] f32, rep [n_points] int32, count [n_points] int32, key [n_points] int64, voxel_of
        [n_points] int32 (-1: a lost row), n_voxels [1] int32)``: the first V = n_voxels rows of the first four are written, voxels in
        ascending key order.  An output not named in ``outputs`` is not computed and comes back as None.  Nothing is read back: the
        caller reads ``n_voxels`` and slices.  Asynchronous on ``stream``."""
        from . import downsample as _downsample
        N = self.n_points
        self._check_keys(sorted_keys, "sorted_keys")
        if (tuple(sorted_keys.shape) != (N,) or not isinstance(sorted_idx, torch.Tensor) or sorted_idx.dtype != torch.int32
                or tuple(sorted_idx.shape) != (N,) or not sorted_idx.is_contiguous() or sorted_idx.device != self.device):
            raise ValueError("sorted_keys int64 [n_points] and sorted_idx int32 [n_points], contiguous on %s" % self.device)
        extra = sorted(set(outputs) - set(self.VOXEL_OUTPUTS))
        if extra:
            raise ValueError("outputs: unknown name %r (%s)" % (extra[0], ", ".join(self.VOXEL_OUTPUTS)))
        lost_key = int(lost_key)
        if not 0 < lost_key < 1 << 62:
            raise ValueError("lost_key must be the number of cells, in 1 .. 2^62 - 1: got %r" % (lost_key,))
        origin = _downsample.check_origin(origin)
        st = self._stream(stream)
        specs = {"centroid": ((N, 3), torch.float32), "rep": ((N,), torch.int32), "count": ((N,), torch.int32), "key": ((N,), torch.int64),
                 "voxel_of": ((N,), torch.int32)}
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            out = [torch.empty(specs[name][0], dtype=specs[name][1], device=self.device) if name in outputs else None
                   for name in self.VOXEL_OUTPUTS]
            n_voxels = torch.zeros(1, dtype=torch.int32, device=self.device)
            if N:
                ws = self._voxel_ws(N)
                _lib.check(self.lib.nesti_voxel_reduce(_lib.ptr(self.cloud), N, _lib.ptr(sorted_keys), _lib.ptr(sorted_idx),
                                                       ctypes.c_uint64(lost_key), (ctypes.c_double * 3)(*origin),
                                                       *[_lib.ptr(t) for t in out], _lib.ptr(n_voxels), _lib.ptr(ws), ws.numel(),
                                                       ctypes.c_void_p(st.cuda_stream)), "nesti_voxel_reduce")
                ws.record_stream(st)
        return tuple(out) + (n_voxels,)

    def build_reference_order(self, first, count, picks, pick_offsets, want_idx=False, out=None, stream=None):
        """Patch tensors of rows [first, first + count) exactly as the reference's ``PointcloudPatchDataset.__getitem__`` builds
        them (``nesti_patches_query_ref``): balls in cKDTree's visiting order, over-full balls thinned by ``picks`` (uint16 device
        tensor, any 2-byte dtype) at ``pick_offsets`` [count * S] int64 (device; -1 = the ball holds <= P points) -- the table
        ``refsample.RefStream.picks`` replays from the ball sizes of :meth:`count_balls`."""
        self._index_queries_only("build_reference_order")
        at, q = self._rows(first, count)
        rank, order = self.ensure_tree_order()
        points, n_eff, nbr = self._patch_out(count, out, want_idx)
        if pick_offsets.dtype != torch.int64 or pick_offsets.numel() < count * self.cfg.n_scales or picks.element_size() != 2:
            raise ValueError("picks: 2-byte elements, pick_offsets: int64 [count * S]")
        self._call("nesti_patches_query_ref", at, q, count, first,
                   [_lib.ptr(rank), _lib.ptr(order), _lib.ptr(picks) if picks.numel() else None, _lib.ptr(pick_offsets), _lib.ptr(points),
                    _lib.ptr(n_eff), _lib.ptr(nbr)], self._stream(stream))
        if want_idx:
            return points, n_eff, nbr
        return points, n_eff


class PointcloudPatchDataset:
    """Shape list + per-shape patch counts, like the reference class of the same name
    (``utils/pcpnet_dataset.py:179-282``), for the inference configuration only."""

    def __init__(self, root, shape_list_filename, cfg: NestiConfig, seed=3627473, sparse_patches=False,
                 device="cuda:0", cache_capacity=100, query_positions=False):
        self.root, self.cfg, self.seed, self.device = root, cfg, seed, device
        self.sparse_patches = bool(sparse_patches)
        # query_positions: the rows of <shape>.qxyz (M rows x 3, read like .xyz) are the queries instead of cloud points
        self.query_positions = bool(query_positions)
        if self.sparse_patches and self.query_positions:
            raise ValueError("sparse_patches and query_positions are mutually exclusive")
        with open(os.path.join(root, shape_list_filename)) as f:
            self.shape_names = [x.strip() for x in f.readlines()]
        self.shape_names = list(filter(None, self.shape_names))       # :221-224
        self.shape_patch_count = []
        self._cache, self._cache_cap, self._tick = {}, cache_capacity, 0
        for ind in range(len(self.shape_names)):
            self.shape_patch_count.append(self.get_shape(ind).patch_count)

    def get_shape(self, ind):
        """LRU of loaded shapes (``Cache``, ``utils/pcpnet_dataset.py:151-176``)."""
        self._tick += 1
        if ind not in self._cache:
            if len(self._cache) >= self._cache_cap:
                old = min(self._cache, key=lambda k: self._cache[k][1])
                del self._cache[old]
            name = self.shape_names[ind]
            pts = load_xyz(os.path.join(self.root, name + ".xyz"))
            pidx = None
            if self.sparse_patches:
                pidx = np.loadtxt(os.path.join(self.root, name + ".pidx")).astype("int")   # :267-270
            queries = load_qxyz(os.path.join(self.root, name + ".qxyz")) if self.query_positions else None
            self._cache[ind] = [CloudPatches(pts, self.cfg, self.device, self.seed, pidx, queries=queries), self._tick]
        self._cache[ind][1] = self._tick
        return self._cache[ind][0]

    def __len__(self):
        return sum(self.shape_patch_count)


class _Loader:
    """Iterates all patches of all shapes in order (``SequentialPointcloudPatchSampler``,
    ``utils/pcpnet_dataset.py:41-55``) in batches of ``batch_size``; a batch may span shapes."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, int(batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds, B = self.dataset, self.batch_size
        pend_p, pend_n, have = [], [], 0
        for ind in range(len(ds.shape_names)):
            shape, done = ds.get_shape(ind), 0
            while done < shape.patch_count:
                take = min(B - have, shape.patch_count - done)
                p, n = shape.build(done, take)
                pend_p.append(p)
                pend_n.append(n)
                have += take
                done += take
                if have == B:
                    yield self._emit(pend_p, pend_n)
                    pend_p, pend_n, have = [], [], 0
        if have:
            yield self._emit(pend_p, pend_n)

    @staticmethod
    def _emit(ps, ns):
        p = ps[0] if len(ps) == 1 else torch.cat(ps)
        n = ns[0] if len(ns) == 1 else torch.cat(ns)
        trans = torch.eye(3, device=p.device).expand(p.shape[0], 3, 3)     # use_pca=False (:377)
        return p, trans, n


def get_data_loader(dataset_name, batchSize, indir, patch_radius, points_per_patch, outputs=(), patch_point_count_std=0,
                    seed=3627473, identical_epochs=False, use_pca=False, patch_center="point", point_tuple=1,
                    cache_capacity=100, patch_sample_order="full", workers=0, dataset_type="test", sparse_patches=False,
                    cfg: NestiConfig = None, device="cuda:0", query_positions=False):
    """Keyword-compatible with ``utils/provider.py:319-429`` for the inference settings of
    ``test_n_est_w_experts.py:109-116``; anything outside that configuration raises, as it is
    outside the hot path."""
    if outputs not in ((), [], None) or use_pca or patch_center != "point" or point_tuple != 1 \
            or patch_point_count_std != 0 or identical_epochs or patch_sample_order != "full":
        raise ValueError("only the inference configuration of test_n_est_w_experts.py:109-116 is supported")
    cfg = cfg or NestiConfig()
    cfg = NestiConfig(**{**cfg.__dict__, "patch_radius": list(patch_radius), "num_point": int(points_per_patch)})
    listfile = os.path.relpath(dataset_name, indir) if os.path.isabs(dataset_name) else dataset_name
    ds = PointcloudPatchDataset(indir, listfile, cfg, seed=seed, sparse_patches=sparse_patches, device=device,
                                cache_capacity=cache_capacity, query_positions=query_positions)
    return _Loader(ds, batchSize), ds
