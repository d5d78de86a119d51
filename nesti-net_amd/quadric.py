"""Quadric-fit normals and principal curvatures at every patch scale on the GPU (``csrc/quadric.hip``; DESIGN.md 2 "Quadric fit"): the
osculating-jet estimator of Cazals and Pouget at degree 2 -- the second row of the paper's comparison tables, and the source of the
per-point principal curvatures the reference's data layer reads from ``<shape>.curv`` (``utils/pcpnet_dataset.py:260-263``).  It needs no
model and no weights: per query and patch radius, a height function ``h = a . (1, u, v, u^2, u v, v^2)`` fitted to the full ball in the
frame of the plane fit; the normal is the fitted surface's at the query and the curvatures are the eigenvalues of its shape operator.
There is no CPU fallback."""
import numpy as np

from .pca import fit_cloud, prepare_cloud


def mean_gauss(curv):
    """(H, K) = ((k_max + k_min) / 2, k_max k_min) of curvatures [..., 2] (float32 in, float32 out)."""
    curv = np.asarray(curv, np.float32)
    return (curv[..., 0] + curv[..., 1]) * np.float32(0.5), curv[..., 0] * curv[..., 1]


def quadric_cloud(cloud, scale=-1, orient=None, viewpoint=None, orient_k=8, knn=None, smooth=None, lists=None):
    """``quadric_fit`` for a prepared ``provider.CloudPatches`` (all of its patch rows); synchronises.  ``knn``: neighbour counts
    instead of the cloud's radii (``scale`` then indexes them, and the dict gains ``radius``).  ``smooth``, ``lists``: see ``pca.fit_cloud``; the
    curvatures are untouched by the smoothing and still flip with the orientation."""
    import torch

    def curvatures(out, s, before):
        out["curv"] = out["curv_all"][:, s, :].contiguous()
        if before is not None:
            # the flip rule: the pass changes sign bits only, and a row whose normal it turned has curvatures (-k_min, -k_max)
            flipped = (before.view(torch.int32) != out["normals"].view(torch.int32)).any(dim=1, keepdim=True)
            out["curv"] = torch.where(flipped, -out["curv"].flip(1), out["curv"])

    return fit_cloud(cloud, cloud.quadric, cloud.quadric_knn, ("normals_all", "curv_all", "plane_all", "n_ball"), scale, orient, viewpoint,
                     orient_k, knn, after=curvatures, smooth=smooth, lists=lists)


def quadric_fit(pts, cfg=None, pidx=None, queries=None, scale=-1, orient=None, viewpoint=None, orient_k=8, device="cuda:0", knn=None,
                smooth=None, outliers=None, downsample=None, denoise=None):
    """Quadric-fit normals and principal curvatures of a cloud: numpy in, a dict of numpy arrays out (synchronises).  Queries are all
    points, the points ``pidx`` or the positions ``queries`` [M,3] (mutually exclusive), as for ``pca.pca_normals``; the radii are
    ``cfg.patch_radius`` times the cloud's bounding-box diagonal.

      normals      [M,3]    the fitted surface's normal at ``scale`` (default -1: the largest), after the optional orientation
      curv         [M,2]    (k_max, k_min) at ``scale``, in absolute units (1 / length: a PCPNet ``.curv`` row), positive where the
                            surface bends toward ``normals``; after the optional orientation
      normals_all  [M,S,3]  every scale, unoriented: on the side of the plane-fit normal
      curv_all     [M,S,2]  every scale, signs referring to ``normals_all``
      plane_all    [M,S,3]  the plane-fit normals the frames were built from: ``pca_normals``' ``normals_all``
      n_ball       [M,S]    points in the ball (the full ball: not capped at ``cfg.num_point``, not subsampled)
      orient       the stats dict of ``orient.orient_normals``, or None

    A failed fit -- fewer than 6 points in the ball, no plane normal, or a singular system (collinear points, say) -- has normal 0 0 0
    and curvatures 0 0; the orientation leaves such rows alone.  ``orient='mst' | 'viewpoint'`` orients the rows of ``scale`` with
    radius ``r_abs[scale]``; where it turns a normal the row's curvatures become ``(-k_min, -k_max)``.

    ``knn`` -- an int or an ascending sequence of at most 4 ints in 1 .. 256 -- replaces the balls by the nearest neighbours, as for
    ``pca.pca_normals``: scale s is fitted to the ``knn[s]`` nearest cloud points, scaled by the distance to the farthest of them;
    ``scale`` indexes ``knn``; ``n_ball`` holds the counts and the dict gains ``radius`` [M,S] float32.  ``plane_all`` is
    ``pca_normals(..., knn=knn)``'s ``normals_all``, bit for bit.  With ``orient='mst'`` the orientation graph's radius is the default
    configuration's largest patch radius (the k-NN radii vary per row and are not a safe grid cell); ``'viewpoint'`` needs no radius;
    the curvature flip is the same.

    ``smooth`` -- as for ``pca.pca_normals`` -- smooths ``normals`` over all points before the orientation; ``curv`` is untouched by
    it (the curvatures are the fit's) and still flips with the orientation; the dict gains ``smooth_support`` and ``smooth_count``.

    Raises ``ValueError`` for a ``scale`` outside [-S, S), for ``pidx`` together with ``queries``, for a bad ``knn``, for ``knn``
    together with ``cfg`` (whose radii would mean nothing), for a bad ``smooth`` and for ``smooth`` with ``pidx`` or ``queries``.

    ``downsample``, ``outliers``, ``denoise`` -- the preprocessing chain (``stages``: the arguments, their order, the keys they add,
    the way back to the rows of ``pts`` and what ``queries`` changes) -- run in front of the estimator; ``pidx`` with any is refused."""
    from . import stages
    chain = stages.run(pts, stages.check(downsample, outliers, denoise, pidx), queries, device)
    cloud = prepare_cloud(chain.points, cfg, pidx, queries, scale, orient, viewpoint, orient_k, device, knn, smooth)
    return chain.back(quadric_cloud(*cloud, smooth=smooth))
