"""The preprocessing chain in front of the estimators (DESIGN.md 2 "The preprocessing chain"): voxel downsampling, outlier removal and
point denoising, in that fixed order, and the one way back to the rows of the input.  This module is the only place that knows the
order and the way back; ``pca.pca_normals``, ``quadric.quadric_fit``, ``hough.hough_normals``, ``robust.robust_normals``,
``select.select_normals``, ``NormalEstimator.estimate`` (the filter alone) and the command line all go through it.

``downsample`` -- None, a voxel size (a number or three, in the cloud's units) or a dict of ``voxel``, ``mode``, ``origin``
(``downsample.voxel_downsample``; DESIGN.md 2 "Voxel downsampling") -- downsamples the cloud on a voxel grid first: ``outliers``
(which comes second, the statistical filter being a density test and the grid what makes density uniform), ``denoise``, the estimator,
its smoothing and its orientation run on the voxels' points, every per-row array comes back with the rows of ``pts`` -- row i holds the
result of its voxel --, and the dict gains ``voxel_of`` [N] int64, ``voxel_points`` [V,3] f32 and ``voxel_count`` [V] int32.

``outliers`` -- None, ``'statistical'`` or a dict of ``mode``, ``k``, ``std_ratio``, ``radius``, ``min_neighbours``, ``passes``
(``outliers.remove_outliers``; DESIGN.md 2 "Outlier removal") -- filters the cloud next: ``denoise``, the estimator, its smoothing and
its orientation run on the kept points, every per-row array comes back with the rows of ``pts`` (0 -- ``expert``: -1 -- in the removed
ones), and the dict gains ``inlier`` [N] bool, ``outlier_score`` [N] f64 and ``outlier_passes``.

``denoise`` -- None, True (the defaults) or a dict of ``k``, ``iters``, ``angle``, ``falloff``, ``sigma``, ``step``, ``normal_k``
(``denoise.denoise_points``; DESIGN.md 2 "Point denoising") -- denoises the positions last, before the estimator, whose smoothing and
orientation then run over the denoised positions.  Rows stay one-to-one and the dict gains ``points`` [N,3] f32 and ``denoise_delta``
[N] f32 (0 in rows that ``outliers`` removed).

``pidx`` with any of the three is refused.  With ``queries`` the estimator's rows are positions: the cloud goes through the chain, the
queries are left alone and NOTHING is mapped back -- the keys a stage adds then keep the rows of the cloud that stage ran on
(``inlier`` has the voxels' rows under ``downsample``, ``points`` the kept rows under ``outliers``)."""
import collections

import numpy as np

Stages = collections.namedtuple("Stages", "downsample outliers denoise")      # the checked Params of each stage, or None
FILLS = {"expert": -1}                 # every other per-row array is filled with 0


def take_rows(rows, src, fill=0):
    """The one gather: numpy ``rows`` [M, ...] -> [len(src), ...] with ``rows[src[i]]`` at row i and ``fill`` where ``src`` is -1."""
    rows = np.asarray(rows)
    src = np.asarray(src, np.int64)
    live = src >= 0
    if live.all():
        return rows[src]
    if not len(rows):
        return np.full((len(src),) + rows.shape[1:], fill, dtype=rows.dtype)
    out = rows[np.where(live, src, 0)]         # one indexed read and a few filled rows: no boolean-mask copies of whole arrays
    out[~live] = fill
    return out


def take_result(res, src, rows):
    """A result dict over ``rows`` rows -> over the rows of ``src``: every numpy array whose first dimension is ``rows`` is taken
    through ``src`` (``take_rows``) with 0 -- ``expert``: -1 -- where ``src`` is -1; everything else (``orient`` statistics, scalars)
    passes through as the same object."""
    out = {}
    for key, v in res.items():
        per_row = isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == rows
        out[key] = take_rows(v, src, FILLS.get(key, 0)) if per_row else v
    return out


def inverse(kept, n):
    """``kept`` [M] (distinct rows of a cloud of ``n``) -> [n] int64: the position of row i in ``kept``, -1 where it is not there."""
    kept = np.asarray(kept, np.int64)
    inv = np.full(int(n), -1, np.int64)
    inv[kept] = np.arange(len(kept))
    return inv


def check(downsample, outliers, denoise, pidx):
    """The three stage arguments of an estimator -> ``Stages`` of checked ``Params``, or None where no stage is given.  Raises every
    ``ValueError`` of the three ``as_params`` and ``refuse_pidx``, before any work: denoise, then downsample, then outliers."""
    from . import denoise as _denoise, downsample as _downsample, outliers as _outliers
    params = {}
    for name, mod, arg in (("denoise", _denoise, denoise), ("downsample", _downsample, downsample), ("outliers", _outliers, outliers)):
        params[name] = mod.as_params(arg)
        if params[name] is not None:
            mod.refuse_pidx(pidx)
    return Stages(**params) if any(p is not None for p in params.values()) else None


class Chain:
    """What ``run`` returns: ``points`` (the cloud the estimator is to run on; the caller's own object where no stage ran), ``n`` (the
    rows of the input), ``src`` [n] int64 (input row i takes its result from estimator row ``src[i]``, -1: the fill -- ``voxel_of``
    composed with the inverse of ``kept``; the identity where no stage renumbers), ``kept`` (the filter's kept rows of the cloud it ran
    on, or None) and ``keys`` (what the stages add to a result)."""

    def __init__(self, pts, mapped):
        self.points, self.mapped, self.keys, self.kept = pts, mapped, {}, None
        self._src = self._at = None            # None: the identity

    @property
    def n(self):
        return len(self.points) if self._src is None else len(self._src)

    @property
    def src(self):
        return np.arange(self.n, dtype=np.int64) if self._src is None else self._src

    def _renumber(self, points, src, at):
        """A stage that renumbers: ``src`` [rows before] -> the row after (-1: none), ``at`` [rows after] -> a row before."""
        self.points = points
        self._src = src if self._src is None else take_rows(src, self._src, -1)
        self._at = at if self._at is None else self._at[at]

    def to_input(self, rows, fill=0):
        """Rows of the estimator's cloud as it stands -> the rows of the input; left alone with ``queries`` or where nothing renumbered."""
        return take_rows(rows, self._src, fill) if self.mapped and self._src is not None else rows

    def take(self, arg):
        """A per-point argument of the estimator (``init=`` of the robust fit) at the estimator's rows: taken at ``rep``, then at
        ``kept``; left alone with ``queries`` and where it is None."""
        return arg if arg is None or not self.mapped or self._at is None else np.asarray(arg)[self._at]

    def back(self, res):
        """An estimator's result dict -> over the rows of the input, in one gather through ``src`` (``take_result``; nothing with
        ``queries``), with the stage keys added."""
        if self.mapped and self._src is not None:
            res = take_result(res, self._src, len(self.points))
        res.update(self.keys)
        return res


def run(pts, params, queries=None, device="cuda:0", report=None):
    """Run the stages of ``params`` (``check``) on the host cloud ``pts``: ``voxel_downsample``, ``remove_outliers``,
    ``denoise_points``, each only where given -> ``Chain``.  ``params=None``: the identity, no primitive is called.
    ``report(stage, out, chain)`` (optional) is called behind each primitive with its name ('downsample', 'outliers', 'denoise'), its
    result and the chain as it stood BEFORE the stage (``chain.to_input`` maps the rows the stage ran on).  ``ValueError`` for a cloud
    that is not [N,3], for an empty cloud or a grid that catches no point under ``downsample``, and for a filter that keeps no point."""
    chain = Chain(pts, queries is None)
    if params is None:
        return chain
    from . import denoise as _denoise, downsample as _downsample, outliers as _outliers
    report = report or (lambda stage, out, chain: None)
    chain.points = _outliers.check_cloud(pts)
    added = []
    if params.downsample is not None:
        if not chain.n:
            raise ValueError("downsample: an empty cloud")
        vd = _downsample.voxel_downsample(chain.points, *params.downsample, device=device)
        report("downsample", vd, chain)
        if not len(vd["rep"]):
            raise ValueError("downsample: none of the %d points lies in the grid of origin %s" % (chain.n, list(vd["origin"])))
        added.append({"voxel_of": vd["voxel_of"], "voxel_points": vd["points"], "voxel_count": vd["count"]})
        chain._renumber(vd["points"], vd["voxel_of"], vd["rep"])
    if params.outliers is not None:
        rows = len(chain.points)
        f = _outliers.remove_outliers(chain.points, *params.outliers, device=device)
        report("outliers", f, chain)
        if not len(f["kept"]):
            raise ValueError("outliers: the filter kept none of the %d points" % rows)
        added.append({"inlier": chain.to_input(f["inlier"]), "outlier_score": chain.to_input(f["score"]), "outlier_passes": f["passes"]})
        chain.kept = f["kept"]
        chain._renumber(f["points"], inverse(f["kept"], rows), f["kept"])
    if params.denoise is not None:
        p = params.denoise
        d = _denoise.denoise_points(chain.points, p.k, p.iters, p.angle, p.falloff, p.sigma, p.step, None, p.normal_k, device=device)
        report("denoise", d, chain)
        added.append({"points": chain.to_input(d["points"]), "denoise_delta": chain.to_input(d["delta"])})
        chain.points = d["points"]
    for keys in reversed(added):               # the order the keys have always had: denoise, outliers, downsample
        chain.keys.update(keys)
    return chain
