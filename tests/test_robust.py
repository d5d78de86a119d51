"""The robust plane fit without a GPU: the tests' restatement (tests/_robust_fixture.py) against a plain float64 formulation, its sign
invariance, its order statistics, ``iters = 0``, what it buys at a crease, and the refusals of the Python layer and the command line
that come before any device call."""
import numpy as np
import pytest

import _knn_fixture as kx
import _robust_fixture as rx

EPS = 2.0 ** -53
K = 32
_cache = {}


def _box():
    """``synth.make_cloud("box", n=2000, seed=3, noise=0.002)`` with its exact sorted lists at K = 32; computed once."""
    if "box" not in _cache:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import synth
        pts, gt = synth.make_cloud("box", n=2000, seed=3, noise=0.002)
        _cache["box"] = {"pts": pts, "gt": gt, "nbr": kx.search(pts, pts, K)[0]}
    return _cache["box"]


def _plain_iteration(D, g, sigma, falloff, floor):
    """One iteration for one row in plain float64 numpy: sorted medians, ``np.sum`` and ``numpy.linalg.eigh`` -> (normal float64 [3],
    the eigenvalues of the weighted covariance in r^2 units)."""
    g = np.asarray(g, np.float64)
    v = g / np.linalg.norm(g)
    d2 = (D * D).sum(1)
    r2 = d2.max()
    h = D @ v
    res = h - np.sort(h)[len(h) // 2]
    med = np.sort(np.abs(res))[len(h) // 2]
    sig = max(sigma * med, floor * np.sqrt(r2))
    w = ((1.0 - falloff * d2 / r2) / (1.0 + (res / sig) ** 2)) ** 2
    m = (w[:, None] * D).sum(0) / w.sum()
    C = ((w[:, None, None] * D[:, :, None] * D[:, None, :]).sum(0) / w.sum() - m[:, None] * m[None, :]) / r2
    ew, V = np.linalg.eigh(0.5 * (C + C.T))
    return V[:, 0], ew


def test_fixture_against_a_plain_float64_formulation():
    """One iteration from the plane fit's normal on the rows of the noisy box, creases included.  The two formulations differ in the order
    of their sums and in their eigen-solvers: with n the neighbour count, w the plain formulation's eigenvalues in r^2 units and eps =
    2^-53, |sin(angle)| <= 2^-22 + 16 n eps / (w1 - w0) -- the f32 rounding of a unit vector, and Davis-Kahan with ||E|| <= 4 n eps for
    each of the two summations (a weighted term is at most w_i r^2, so the sums of magnitudes are at most sw r^2: the bound of
    tests/test_gpu_pca.py carries over with the sum of the weights for the count).  Rows with a bound above 1e-3 are ill-conditioned and
    left out; there must be none here."""
    b = _box()
    rows = np.arange(0, 2000, 5)
    ref = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=1)
    assert (ref["iters_done"] == 1).all() and (ref["count"] == K).all()
    p64 = b["pts"].astype(np.float64)
    worst = 0.0
    for i, q in enumerate(rows):
        D = p64[b["nbr"][q]] - p64[q]
        v, ew = _plain_iteration(D, ref["plane"][i], 2.0, 0.5, 0.01)
        bound = 2.0 ** -22 + 16 * K * EPS / (ew[1] - ew[0])
        assert bound <= 1e-3, (q, ew)
        a = ref["normals"][i].astype(np.float64)
        sin = np.linalg.norm(np.cross(a, v)) / (np.linalg.norm(a) * np.linalg.norm(v))
        worst = max(worst, sin / bound)
        assert sin <= bound, (q, sin, bound)
    print("largest sin / bound over %d rows: %.3g" % (len(rows), worst))
    # the robust normal is a unit vector under the sign rule
    n = ref["normals"]
    lead = np.where(n[:, 2] != 0, n[:, 2], np.where(n[:, 1] != 0, n[:, 1], n[:, 0]))
    assert (lead > 0).all() and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22


def test_an_iteration_does_not_see_the_sign_of_its_start():
    b = _box()
    rows = np.arange(0, 2000, 40)
    rs = np.random.RandomState(5)
    init = rs.normal(size=(len(rows), 3)).astype(np.float32) * np.float32(3.0)          # any direction, any length
    for iters in (0, 1, 3):
        plus = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=iters, init=init)
        minus = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=iters, init=-init)
        for key in ("normals", "support", "inliers", "iters_done", "moments"):
            assert np.array_equal(np.ascontiguousarray(plus[key]).view(np.uint8), np.ascontiguousarray(minus[key]).view(np.uint8)), (iters, key)
        assert (plus["iters_done"] == iters).all()


def test_the_order_statistics_are_elements_of_rank_n_over_2():
    used = np.array([[True] * 5 + [False] * 3, [True] * 6 + [False] * 2, [True] * 8, [False] * 8, [True] * 1 + [False] * 7])
    vals = np.array([[5.0, 1.0, 4.0, 2.0, 3.0, -9.0, -9.0, -9.0],          # odd n = 5: rank 2 -> 3
                     [6.0, 1.0, 5.0, 2.0, 4.0, 3.0, -9.0, -9.0],           # even n = 6: rank 3 -> 4, the upper of the two middle elements
                     [2.0, 2.0, 1.0, 2.0, 7.0, 2.0, 2.0, 0.0],             # ties: rank 4 of 0 1 2 2 2 2 2 7 -> 2
                     [1.0] * 8,                                            # no values
                     [-3.5, 0, 0, 0, 0, 0, 0, 0]])                         # n = 1: rank 0
    n = used.sum(1)
    assert rx.rank_element(vals, used, n).tolist() == [3.0, 4.0, 2.0, 0.0, -3.5]
    # in an iteration: six coplanar points and two above; the even count takes an element, so c is a height that occurs
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0.5], [0, 2, 0.25], [2, 2, 0], [2, 1, 0]], np.float32)
    nbr = np.tile(np.arange(8), (1, 1))
    geo = rx.geometry(pts, pts[:1], nbr, 8)
    g = np.array([[0, 0, 1]], np.float32)
    w, res, sig = rx.weights(geo, g, 2.0, 0.5, 0.01)
    assert sorted(res[0].tolist()) == [0.0] * 6 + [0.25, 0.5]               # c = 0: rank 4 of 0 0 0 0 0 0 .25 .5
    assert sig[0] == 0.01 * np.sqrt(8.0)                                    # med = 0: the floor carries the scale
    assert np.array_equal(w[0] == w[0].max(), (geo["d2"][0] == 0))          # the centre itself weighs most


def test_iters_0_is_the_start_normal_renormalised():
    b = _box()
    rows = np.arange(0, 2000, 100)
    init = np.random.RandomState(6).normal(size=(len(rows), 3)).astype(np.float32) * np.float32(0.01)
    init[3] = 0.0
    init[4, 1] = np.nan
    out = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=0, init=init)
    live = np.ones(len(rows), bool)
    live[[3, 4]] = False
    want = init[live].astype(np.float64)
    want = want / np.linalg.norm(want, axis=1, keepdims=True)
    got = out["normals"][live].astype(np.float64)
    assert np.abs(np.abs((got * want).sum(1)) - 1).max() <= 2.0 ** -22 and np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 2.0 ** -22
    assert not out["normals"][~live].view(np.uint32).any() and not out["iters_done"].any() and not out["support"].any()
    assert not out["moments"].any() and not out["inliers"].any() and (out["count"] == K).all()
    plain = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=0)
    assert np.abs(np.abs((plain["normals"].astype(np.float64) * plain["plane"].astype(np.float64)).sum(1)) - 1).max() <= 2.0 ** -22


def test_chained_single_iterations_equal_one_call():
    b = _box()
    rows = np.arange(0, 2000, 50)
    whole = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=3)
    cur = None
    for _ in range(3):
        step = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], K, iters=1, init=cur)
        cur = step["normals"]
    for key in ("normals", "support", "inliers", "moments"):
        assert np.array_equal(np.ascontiguousarray(whole[key]).view(np.uint8), np.ascontiguousarray(step[key]).view(np.uint8)), key
    # falloff = 1 over three neighbours: the farthest weighs 0, fewer than 3 slots have a weight, the first iteration fails
    three = rx.restate(b["pts"], b["pts"][rows], b["nbr"][rows], 3, iters=4, falloff=1.0)
    assert not three["iters_done"].any() and not three["support"].any()
    assert np.array_equal(three["normals"].view(np.uint32), three["plane"].view(np.uint32)) and (three["plane"] != 0).any(1).all()


def test_the_robust_fit_leans_to_a_face_at_a_crease():
    """Near-edge rows of the 2 000-point box at noise 0.002, k = 32, defaults: the share within 10 degrees of the analytic normal is at
    least 20 points above the plane fit's (a float64 trial of the algorithm gave 69.2 % against 34.6 % on 1 103 rows; the margin leaves
    14 points for the differences between that trial and the exact arithmetic)."""
    b = _box()
    out = rx.restate(b["pts"], b["pts"], b["nbr"], K)
    near = rx.near_edge(b["pts"], out["radius"])
    robust, plane = rx.within_deg(out["normals"][near], b["gt"][near]), rx.within_deg(out["plane"][near], b["gt"][near])
    away = (rx.within_deg(out["normals"][~near], b["gt"][~near]), rx.within_deg(out["plane"][~near], b["gt"][~near]))
    print("near-edge rows: %d; within 10 degrees: robust %.1f %%, plane %.1f %%; the other rows: %.1f %%, %.1f %%"
          % (near.sum(), robust, plane, away[0], away[1]))
    assert (out["iters_done"] == 8).all() and near.sum() > 800
    assert robust >= plane + 20.0


def test_check_params():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import robust
    assert robust.check_params() == (8, 2.0, 0.5, 0.01)
    assert robust.check_params(0, 1e6, 0, 1e-6) == (0, 1e6, 0.0, 1e-6) and robust.check_params(np.int32(64), 1e-9, 1, 1) == (64, 1e-9, 1.0, 1.0)
    for bad in (-1, 65, 1.5, True, None, "8"):
        with pytest.raises(ValueError, match="iters"):
            robust.check_params(iters=bad)
    for bad in (0.0, -2.0, 1.0000001e6, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="sigma"):
            robust.check_params(sigma=bad)
    for bad in (-1e-9, 1.0000001, float("nan"), None):
        with pytest.raises(ValueError, match="falloff"):
            robust.check_params(falloff=bad)
    for bad in (0.0, 0.9e-6, 1.5, float("nan"), -0.01):
        with pytest.raises(ValueError, match="floor"):
            robust.check_params(floor=bad)


def test_python_layer_refuses_before_any_device_call():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import robust
    pts = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="knn must be given"):
        robust.robust_normals(pts, knn=None)
    for kw, word in (({"knn": 0}, "k"), ({"knn": 257}, "k"), ({"knn": (8, 4)}, "ascending"), ({"knn": (1, 2, 3, 4, 5)}, "neighbour counts"),
                     ({"iters": 65}, "iters"), ({"sigma": 0}, "sigma"), ({"falloff": 2}, "falloff"), ({"floor": 0}, "floor"),
                     ({"scale": 1}, "scale"), ({"knn": (4, 8), "scale": -3}, "scale"),
                     ({"init": np.zeros((9, 3), np.float32)}, "init"), ({"init": np.zeros((10, 2, 3), np.float32)}, "init"),
                     ({"init": np.zeros((10, 4), np.float32)}, "init"), ({"init": "north"}, "init"),
                     ({"pidx": [0, 1], "init": np.zeros((10, 3), np.float32)}, "init"),
                     ({"pidx": [0, 1], "queries": np.zeros((2, 3), np.float32)}, "mutually exclusive"),
                     ({"orient": "up"}, "orient"), ({"orient": "viewpoint"}, "viewpoint"),
                     ({"smooth": 0}, "iters"), ({"smooth": 1, "pidx": [0, 1]}, "smooth"),
                     ({"smooth": 1, "queries": np.zeros((2, 3), np.float32)}, "smooth")):
        with pytest.raises(ValueError, match=word):
            robust.robust_normals(pts, **kw)
    a = robust.check_init(np.ones((10, 3)), 10, 2)
    assert a.shape == (10, 2, 3) and a.dtype == np.float32 and a.flags.c_contiguous and robust.check_init(None, 10, 2) is None


@pytest.mark.parametrize("extra, word", [(["--depth_images", "1"], "--depth_images 1"), (["--reproducible", "1"], "--reproducible 1"),
                                         (["--subsample", "reference"], "--subsample reference"),
                                         (["--subsample", "reference_host"], "--subsample reference_host")])
def test_command_line_refusals(extra, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--estimator", "robust", "--knn", "32", "--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)] + extra)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--estimator robust does not take " + word in err
    assert not (tmp_path / "out").exists()                      # refused while parsing: nothing was created


def test_command_line_flags(capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    f = cli.build_parser().parse_args([])
    assert (f.estimator, f.robust_scale, f.robust_iters, f.robust_sigma, f.robust_falloff, f.robust_floor) == ("net", -1, 8, 2.0, 0.5, 0.01)
    base = ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)]
    for argv, word in ((["--estimator", "robust"], "--estimator robust needs --knn"),
                       (["--robust_scale", "0"], "--robust_scale belongs to --estimator robust"),
                       (["--estimator", "pca", "--robust_iters", "2"], "--robust_iters belongs to --estimator robust"),
                       (["--estimator", "hough", "--knn", "32", "--robust_sigma", "3"], "--robust_sigma belongs to --estimator robust"),
                       (["--robust_falloff", "0.25"], "--robust_falloff belongs to --estimator robust"),
                       (["--robust_floor", "0.1"], "--robust_floor belongs to --estimator robust"),
                       (["--estimator", "robust", "--knn", "32", "--robust_iters", "65"], "--estimator robust: iters"),
                       (["--estimator", "robust", "--knn", "32", "--robust_sigma", "0"], "--estimator robust: sigma"),
                       (["--estimator", "robust", "--knn", "32", "--robust_falloff", "1.5"], "--estimator robust: falloff"),
                       (["--estimator", "robust", "--knn", "32", "--robust_floor", "0"], "--estimator robust: floor"),
                       (["--estimator", "robust", "--knn", "32", "--patch_radius", "0.05"], "--patch_radius belongs to"),
                       (["--estimator", "robust", "--knn_ladder", "auto"], "--knn_ladder belongs to --estimator pca")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + base)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not (tmp_path / "out").exists()
