"""The fixture of the scale-count tests (tests/test_fit_scales.py, tests/test_gpu_fit_scales.py): the clouds, rows, radii and neighbour
counts at which the model-free fits are run with 1, 2 and 4 scales, and their restatements by tests/_pca_fixture.py,
tests/_quadric_fixture.py, tests/_knn_fixture.py and tests/_hough_fixture.py -- nothing here restates an estimator again.

  ellipsoid    synth.make_cloud("ellipsoid", 4000, seed=7), rows 0::16 (250).  At 0.01 x bbdiag the balls hold 1 - 6 points: sentinel
               rows, failed fits and live rows interleave inside the four lanes that solve the four scales of one row
  torus_clean  synth.make_cloud("torus", 12000, seed=7), rows 0::48 (250).  Balls of 17 - 679 points, curvatures of both signs
  SCALE_SETS   the relative radii of every ball case: four scales on both clouds, two scales out of order, one scale, four scales
               with a repeated radius out of order
  KS_SETS      the neighbour counts of every list case on both clouds: four full trips per lane at 256 = NESTI_KNN_MAX_K, a partial
               last trip at 200, one scale

Host only, deterministic; what a test shares is computed once and never changed."""
import numpy as np

import _knn_fixture as kx
import _pca_fixture as fx
import _quadric_fixture as qx

A4 = [0.01, 0.03, 0.05, 0.08]
T4 = [0.03, 0.045, 0.06, 0.1]
SCALE_SETS = {"ellipsoid_4": ("ellipsoid", A4),
              "torus_4": ("torus_clean", T4),
              "torus_2_out_of_order": ("torus_clean", [0.1, 0.03]),
              "torus_1": ("torus_clean", [0.06]),
              "ellipsoid_4_repeated": ("ellipsoid", [0.05, 0.05, 0.01, 0.03])}
FULL_SET = {"ellipsoid": "ellipsoid_4", "torus_clean": "torus_4"}     # the four-scale set a cloud's sub-configurations are drawn from
SUB_CONFIGS = ((0,), (1,), (2,), (3,), (0, 2), (3, 1), (0, 1, 2))      # columns of the four-scale set run as a configuration of their own
KS_SETS = ((8, 16, 64, 256), (16, 200), (24,))
CLOUDS = ("ellipsoid", "torus_clean")
HOUGH_KS_SETS = ((3, 9, 17, 40), (17, 40))
HOUGH_K, HOUGH_T, HOUGH_B, HOUGH_R, HOUGH_SEED = 40, (65, 200), 16, 3, 9

_cache = {}


def cloud(name):
    """{pts, gt, rows} of a cloud, computed once."""
    if ("cloud", name) not in _cache:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import synth
        if name == "ellipsoid":
            pts, gt = synth.make_cloud("ellipsoid", 4000, seed=7)
            rows = np.arange(0, len(pts), 16)
        elif name == "torus_clean":
            pts, gt = synth.make_cloud("torus", 12000, seed=7)
            rows = np.arange(0, len(pts), 48)
        else:
            raise KeyError(name)
        _cache[("cloud", name)] = {"name": name, "pts": pts, "gt": gt, "rows": rows}
    return _cache[("cloud", name)]


def config(radii):
    """A configuration whose only job is to carry ``radii``: the fits read n_scales and nothing else of it."""
    from nesti_net_amd.config import NestiConfig
    return NestiConfig(patch_radius=list(radii))


def scale_set(key):
    """{cloud, pts, gt, rows, radii (relative), cfg, r_abs} of a ball case."""
    if ("set", key) not in _cache:
        name, radii = SCALE_SETS[key]
        c = dict(cloud(name))
        c["cloud"], c["radii"], c["cfg"] = name, list(radii), config(radii)
        c["r_abs"] = fx.radii(c["pts"], c["cfg"])
        _cache[("set", key)] = c
    return _cache[("set", key)]


def plane_balls(key):
    """``_pca_fixture.restate`` of a ball case, computed once."""
    if ("plane", key) not in _cache:
        c = scale_set(key)
        _cache[("plane", key)] = fx.restate(c["pts"], c["pts"][c["rows"]], c["r_abs"])
    return _cache[("plane", key)]


def quadric_balls(key, n0):
    """``_quadric_fixture.restate`` of a ball case from the plane normals ``n0`` [M,S,3] (the GPU's plane_out, or the restatement's)."""
    c = scale_set(key)
    return qx.restate(c["pts"], c["pts"][c["rows"]], c["r_abs"], n0)


def lists(name):
    """The 256 nearest neighbours of a cloud's rows by brute force: (idx, d2, count), computed once."""
    c = cloud(name)
    return kx.searched(("fit_scales", name), c["pts"], c["pts"][c["rows"]], kx.KNN_MAX_K)


def plane_lists(name, ks):
    """``_knn_fixture.plane_lists`` of a list case, computed once."""
    if ("plane_lists", name, ks) not in _cache:
        c = cloud(name)
        _cache[("plane_lists", name, ks)] = kx.plane_lists(c["pts"], c["pts"][c["rows"]], lists(name)[0], ks)
    return _cache[("plane_lists", name, ks)]


def quadric_lists(name, ks, n0):
    """``_knn_fixture.quadric_lists`` of a list case from the plane normals ``n0`` [M,S,3]."""
    c = cloud(name)
    return kx.quadric_lists(c["pts"], c["pts"][c["rows"]], lists(name)[0], ks, n0)


def plane_bound(ref):
    """(bound, live) of the direction rule of tests/test_gpu_pca.py over a plane restatement: 2^-22 + 16 n eps / (w1 - w0) per (row,
    scale) pair, inf where the gap is 0; live = n >= 3.  A live pair is ill-conditioned iff not bound <= 1e-3."""
    n = ref["n_ball"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = 2.0 ** -22 + 16 * n * fx.EPS / (ref["w"][..., 1] - ref["w"][..., 0])
    return bound, ref["n_ball"] >= 3


def quadric_ill(ref):
    """(ill, fit) masks of the rule of tests/test_gpu_quadric.py over a quadric restatement: fit = n >= 6, ill = fit and not B <= 1e-6."""
    fit = ref["n_ball"] >= 6
    with np.errstate(invalid="ignore"):
        return fit & ~(qx.bound_B(ref) <= 1e-6), fit


def box():
    """The 300-point box of tests/test_gpu_hough.py."""
    if "box" not in _cache:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import synth
        _cache["box"] = synth.make_cloud("box", n=300, seed=3)[0]
    return _cache["box"]
