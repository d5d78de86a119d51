"""Hough-transform normals over the nearest neighbours on the GPU (``csrc/hough.hip``; DESIGN.md 2 "Hough-transform normals"): the
sharp-feature estimator after Boulch and Marlet, "Fast and Robust Normal Estimation for Point Clouds with Sharp Features" (SGP 2012) --
the classical sharp-feature baseline of the PCPNet / HoughCNN / Nesti-Net comparisons.  Planes through hashed triplets of a neighbourhood
vote for their normal in an accumulator over the hemisphere and the fullest bin names the normal: where the plane fit and the quadric
fit average across a crease, the vote picks one of its faces.  It needs no model and no weights.  The conventions are the library's own
(no parity with the authors' code is claimed).  There is no ball variant and no CPU fallback."""
import numpy as np

from . import _lib
from ._args import int_in as _int_in
from .pca import fit_cloud, prepare_cloud

# The rotation table of the accumulator: 8 orthonormal 3 x 3 matrices, row 0 the identity, generated once (QR of seeded normal draws)
# and committed as literals -- nothing is generated at run time, so the written files are a function of the inputs alone.
ROTATIONS = (
    ((1.0, 0.0, 0.0),
     (0.0, 1.0, 0.0),
     (0.0, 0.0, 1.0)),
    ((-0.08543944056991792, -0.5569953015974398, 0.8261091550112953),
     (-0.7201181119433049, -0.5384957971658133, -0.43755248974947525),
     (0.6885709889665039, -0.6322804049099828, -0.35509362528854077)),
    ((0.10230478253380926, -0.558961043214852, -0.8228586048883939),
     (0.7358920165477449, 0.5991122803144707, -0.3154796594991324),
     (0.669325534737771, -0.5732600001260854, 0.4726270208139155)),
    ((-0.892074993289744, 0.3637590249475112, -0.2681074003386313),
     (0.22849657809526247, 0.8749749089954211, 0.42685855084232494),
     (0.3898608984572047, 0.31952821533894304, -0.8636609285225604)),
    ((-0.14493813037098047, 0.7997824716073935, 0.5825297730366524),
     (0.43667700030026424, -0.4766012540087398, 0.7629970131567091),
     (0.8878660573382272, 0.3649647144408145, -0.28016891590575627)),
    ((0.7879219688746104, 0.3137200364510988, 0.529866690492881),
     (-0.49635586843267626, -0.18568297641746448, 0.8480287047861029),
     (0.3644308203722639, -0.9311828880503941, 0.009413084772069726)),
    ((0.6931492144712459, -0.17874529086074709, 0.6982795195858188),
     (0.7206461861611215, 0.19148098463968818, -0.6663363316620563),
     (-0.014602768550003515, 0.9650829775291463, 0.2615370062422381)),
    ((0.13975388150075396, -0.9830285858222444, 0.1188429722860871),
     (0.6287594103035006, 0.18081940359321685, 0.7562843031816723),
     (-0.7649382044062563, -0.03097002971441625, 0.6433586874358819)),
)

DEFAULT_KNN, DEFAULT_TRIPLETS, DEFAULT_BINS, DEFAULT_ROTATIONS = 100, 1000, 16, 5


def check_params(triplets, bins, rotations, seed):
    """(T, B, R, seed) as ints within the limits of include/nesti_hip.h; ``ValueError`` otherwise."""
    return (_int_in("triplets", triplets, 1, _lib.HOUGH_MAX_T), _int_in("bins", bins, 2, _lib.HOUGH_MAX_BINS),
            _int_in("rotations", rotations, 1, min(_lib.HOUGH_MAX_ROT, len(ROTATIONS))), _int_in("seed", seed, 0, 2 ** 64 - 1))


def rotation_table(rotations):
    """The first ``rotations`` matrices of ``ROTATIONS`` as float64 [R, 9], row-major: the ``rot`` argument of the C entries."""
    return np.ascontiguousarray(np.array(ROTATIONS[:rotations], dtype=np.float64).reshape(rotations, 9))


def _need_knn(knn):
    if knn is None:
        raise ValueError("the Hough estimator exists over neighbour lists only (there is no ball variant): knn must be given")


def hough_cloud(cloud, knn=DEFAULT_KNN, scale=-1, triplets=DEFAULT_TRIPLETS, bins=DEFAULT_BINS, rotations=DEFAULT_ROTATIONS, seed=0,
                orient=None, viewpoint=None, orient_k=8, smooth=None, lists=None):
    """``hough_normals`` for a prepared ``provider.CloudPatches`` (all of its patch rows); synchronises.  ``smooth``, ``lists``: see
    ``pca.fit_cloud``."""
    _need_knn(knn)
    T, B, R, seed = check_params(triplets, bins, rotations, seed)

    def nbr(first, count, ks, nbr=None):
        return cloud.hough_knn(first, count, ks, T, B, R, seed, nbr=nbr)

    return fit_cloud(cloud, None, nbr, ("normals_all", "conf", "votes", "n_ball"), scale, orient, viewpoint, orient_k, knn, smooth=smooth,
                     lists=lists)


def hough_normals(pts, knn=DEFAULT_KNN, pidx=None, queries=None, scale=-1, triplets=DEFAULT_TRIPLETS, bins=DEFAULT_BINS,
                  rotations=DEFAULT_ROTATIONS, seed=0, orient=None, viewpoint=None, orient_k=8, device="cuda:0", cfg=None, smooth=None,
                  outliers=None, downsample=None, denoise=None):
    """Hough-transform normals of a cloud: numpy in, a dict of numpy arrays out (synchronises).  Queries are all points, the points
    ``pidx`` or the positions ``queries`` [M,3] (mutually exclusive), as for ``pca.pca_normals``.  ``knn`` -- an int or an ascending
    sequence of at most 4 ints in 1 .. 256 -- names the neighbourhoods: scale s is the ``knn[s]`` nearest cloud points of the query
    (one exact search at ``max(knn)``).

      normals      [M,3]    the normals at ``scale`` (default -1: the largest), after the optional orientation
      normals_all  [M,S,3]  every scale, unoriented: the first non-zero of (n_z, n_y, n_x) is positive
      conf         [M,S]    the winning bin's share of the valid triplets, in (0, 1]; 0 for a sentinel row
      votes        [M,S,2]  int32 (votes of the winning bin, valid triplets)
      radius       [M,S]    the distance to the farthest neighbour of the scale
      n_ball       [M,S]    the neighbour counts (``min(knn[s], N)``)
      orient       the stats dict of ``orient.orient_normals``, or None

    ``triplets`` (1 .. 4096) planes are drawn per row and scale by a hash of (``seed``, patch row, triplet), so a row's bits depend
    neither on batching nor on the search grid; each votes in ``rotations`` (1 .. 8) rotated copies (``ROTATIONS``) of a hemi-octahedral
    accumulator of ``bins`` x ``bins`` (2 .. 16) cells.  A scale with fewer than 3 neighbours, or whose triplets are all degenerate
    (coincident or collinear neighbours), has normal 0 0 0, ``conf`` 0 and votes (0, valid); the orientation leaves such rows alone.
    ``orient`` is as for ``pca.pca_normals(..., knn=...)``.

    ``smooth`` -- as for ``pca.pca_normals`` -- smooths ``normals`` over all points before the orientation, over the lists of the
    estimator's own search where ``max(knn)`` reaches the smoothing's ``k``: the vote keeps a crease, the smoothing takes the bins'
    noise off the faces.  The dict gains ``smooth_support`` and ``smooth_count``.

    Raises ``ValueError`` for ``knn=None`` (there is no ball variant), for a ``cfg`` (the scales are neighbour counts: a
    configuration's radii would mean nothing), for parameters outside their ranges, for a ``scale`` outside [-S, S), for ``pidx``
    together with ``queries``, for a bad ``smooth`` and for ``smooth`` with ``pidx`` or ``queries``.

    ``downsample``, ``outliers``, ``denoise`` -- the preprocessing chain (``stages``: the arguments, their order, the keys they add,
    the way back to the rows of ``pts`` and what ``queries`` changes) -- run in front of the estimator; ``pidx`` with any is refused."""
    from . import stages
    params = stages.check(downsample, outliers, denoise, pidx)
    _need_knn(knn)
    check_params(triplets, bins, rotations, seed)
    chain = stages.run(pts, params, queries, device)
    cloud, scale, orient, viewpoint, orient_k, ks = prepare_cloud(chain.points, cfg, pidx, queries, scale, orient, viewpoint, orient_k, device,
                                                                  knn, smooth)
    return chain.back(hough_cloud(cloud, ks, scale, triplets, bins, rotations, seed, orient, viewpoint, orient_k, smooth=smooth))
