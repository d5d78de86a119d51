"""Exact k-nearest-neighbour search on the GPU (``csrc/knn.hip``; DESIGN.md 2 "k-nearest neighbourhoods"): the neighbourhood that
adapts to the density of a cloud, where a fixed radius starves its sparse part.  ``pca.pca_normals(..., knn=...)`` and
``quadric.quadric_fit(..., knn=...)`` fit over these lists; :func:`knn` returns the lists themselves.  There is no CPU fallback."""
import numpy as np

from . import _lib
from .config import MAX_SCALES, NestiConfig


def check_k(k):
    """A neighbour count in 1 .. ``_lib.KNN_MAX_K`` as an int; ``ValueError`` otherwise."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _lib.KNN_MAX_K:
        raise ValueError("k must be an integer in 1 .. %d: got %r" % (_lib.KNN_MAX_K, k))
    return int(k)


def check_ks(knn):
    """``knn`` -- an int or an ascending sequence of at most ``MAX_SCALES`` ints in 1 .. ``_lib.KNN_MAX_K`` -- as a tuple of ints;
    ``ValueError`` otherwise."""
    if isinstance(knn, (int, np.integer)) and not isinstance(knn, bool):
        return (check_k(knn),)
    try:
        ks = tuple(knn)
    except TypeError:
        raise ValueError("knn must be an int or a sequence of ints: got %r" % (knn,))
    if not 1 <= len(ks) <= MAX_SCALES:
        raise ValueError("knn must hold 1 .. %d neighbour counts: got %d" % (MAX_SCALES, len(ks)))
    ks = tuple(check_k(k) for k in ks)
    if any(b < a for a, b in zip(ks, ks[1:])):
        raise ValueError("knn must be ascending: got %r" % (ks,))
    return ks


def default_radius(n_points, k, extent):
    """The pseudo-radius of the search-only grid ``provider.CloudPatches`` builds for a k-NN search: the cell edge at which a 3 x 3 x 3
    cell block holds about ``k`` points of a SURFACE-like cloud.  With (a, b, c) the bounding box's extents the surface is taken as
    half the box's own, A = a b + b c + c a (a sphere of diameter D: 3 D^2 against pi D^2; a flat plate: exactly its area), of which a
    block three cells wide sees (3 cell)^2:  9 cell^2 N / A = k.  A degenerate box (a needle, a point) gives 0 and is lifted to
    1e-6 of the diagonal, or to 1: ``nesti_patches_grid`` then limits the grid to 128 cells an axis on its own.  The choice moves the
    time of a search, never its result.  Timed on the 100k bench cloud against cells half and twice as wide (profiles/knn_check.json):
    the fastest of the three at k = 64 and k = 256, 19 % behind cells twice as wide at k = 16."""
    a, b, c = (float(v) for v in extent)
    area = a * b + b * c + c * a
    diag = float(np.sqrt(a * a + b * b + c * c))
    r = float(np.sqrt(k * area / (9.0 * max(1, n_points))))
    r = max(r, 1e-6 * diag)
    return r if r > 0.0 and np.isfinite(r) else 1.0


def knn(pts, k, pidx=None, queries=None, device="cuda:0"):
    """The ``k`` nearest cloud points of every query: numpy in, a dict of numpy arrays out (synchronises).  Queries are all points,
    the points ``pidx`` or the positions ``queries`` [M,3] (mutually exclusive), as for ``pca.pca_normals``.

      idx    [M,k] int32    cloud indices, ascending in (d2, index); -1 beyond ``count``
      d2     [M,k] float64  (dx dx + dy dy) + dz dz of float64 differences, each operation rounded on its own; +inf beyond ``count``
      count  [M]   int32    min(k, N)

    Exact, over the whole cloud, with no radius bound; a cloud point queried by index is its own first neighbour.  Raises
    ``ValueError`` for ``k`` outside 1 .. 256 and for ``pidx`` together with ``queries``."""
    k = check_k(k)
    if pidx is not None and queries is not None:
        raise ValueError("pidx and queries are mutually exclusive: a query is a cloud point (pidx) or a position (queries)")
    import torch
    from .provider import CloudPatches
    cloud = CloudPatches(np.asarray(pts, dtype=np.float32), NestiConfig(), device=device, pidx=pidx, queries=queries,
                         radius_grid=False)
    with torch.cuda.device(cloud.device):
        idx, d2, count = cloud.knn(0, cloud.patch_count, k)
        torch.cuda.current_stream(cloud.device).synchronize()
    return {"idx": idx.cpu().numpy(), "d2": d2.cpu().numpy(), "count": count.cpu().numpy()}
