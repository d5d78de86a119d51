"""The outlier filter without a GPU: every refusal of ``nesti_outlier_scores_nbr``, ``nesti_outlier_threshold`` and
``nesti_outlier_compact`` through ctypes (each returns before any device call), the range checks of the Python layer, the ``--outliers``
parser errors, and the tests' restatement (tests/_outliers_fixture.py): its statistics against plain numpy, a lane group against the
64-lane statement, and the property that makes the filter worth having -- on the clouds of the GPU test, proven here."""
import ctypes

import numpy as np
import pytest

import _outliers_fixture as ox


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------

def _refused(lib, entry, rc, word):
    msg = lib.nesti_last_error() or b""
    assert rc != 0 and word.encode() in msg and msg.startswith((entry + ":").encode()), (entry, rc, msg, word)


def test_refusals_need_no_device():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    dummy = np.zeros(8, np.float64)                                          # never dereferenced: the checks come first
    p = ctypes.c_void_p(dummy.ctypes.data)
    N, M, K = 1000, 100, 64
    ws = lib.nesti_outlier_workspace_bytes(N)
    assert lib.nesti_outlier_workspace_bytes(0) == 0 and lib.nesti_outlier_workspace_bytes(-1) == 0
    assert ws > 0 and ws % 256 == 0 and lib.nesti_outlier_workspace_bytes(1) > 0
    assert lib.nesti_outlier_workspace_bytes(1 << 20) > ws

    def scores(cloud=p, n=N, row0=0, m=M, nbr=p, K=K, k=16):
        return lib.nesti_outlier_scores_nbr(cloud, n, row0, m, nbr, K, k, p, p, p, None)

    e = "nesti_outlier_scores_nbr"
    _refused(lib, e, scores(cloud=None), "null")
    _refused(lib, e, scores(nbr=None), "null")
    _refused(lib, e, scores(n=0), "empty cloud")
    _refused(lib, e, scores(n=-4), "empty cloud")
    _refused(lib, e, scores(K=0), "K must be in 1 .. 256")
    _refused(lib, e, scores(K=257), "K must be in 1 .. 256")
    for K_, k in ((K, 0), (K, -1), (K, K), (K, K + 1), (1, 1), (256, 256)):
        _refused(lib, e, scores(K=K_, k=k), "k must be in 1 .. K - 1")
    _refused(lib, e, scores(m=-1), "M must be")
    _refused(lib, e, scores(row0=-1), "query_row0")
    _refused(lib, e, scores(row0=N - M + 1), "exceed the cloud")
    assert scores(m=0, K=2, k=1) == 0 and scores(m=0, row0=N, K=256, k=255) == 0         # M = 0 is a no-op at the ends of the ranges
    _refused(lib, e, scores(m=0, k=K), "k must be")                                       # ... and an argument error is still one

    def threshold(sc=p, m=M, ratio=1.0, stats=p, w=p, nbytes=ws):
        return lib.nesti_outlier_threshold(sc, m, ratio, stats, w, nbytes, None)

    e = "nesti_outlier_threshold"
    _refused(lib, e, threshold(sc=None), "null")
    _refused(lib, e, threshold(stats=None), "null")
    _refused(lib, e, threshold(w=None), "null")
    _refused(lib, e, threshold(m=-1), "M must be")
    for r in (-1e-9, -1.0, np.nan, np.inf, -np.inf):
        _refused(lib, e, threshold(ratio=r), "std_ratio must be finite and >= 0")
    _refused(lib, e, threshold(m=N, nbytes=ws - 1), "workspace too small")
    _refused(lib, e, threshold(m=1, nbytes=0), "workspace too small")
    assert threshold(m=0, ratio=0.0, nbytes=0) == 0
    _refused(lib, e, threshold(m=0, ratio=np.nan), "std_ratio")

    def compact(cloud=p, n=N, sc=p, thr_dev=None, thr=1.0, xyz=p, n_kept=p, w=p, nbytes=ws):
        return lib.nesti_outlier_compact(cloud, n, sc, thr_dev, thr, xyz, p, p, p, n_kept, w, nbytes, None)

    e = "nesti_outlier_compact"
    _refused(lib, e, compact(sc=None), "null")
    _refused(lib, e, compact(n_kept=None), "null")
    _refused(lib, e, compact(w=None), "null")
    _refused(lib, e, compact(cloud=None), "null")                             # the points are asked for, the cloud is missing
    _refused(lib, e, compact(n=0), "empty cloud")
    _refused(lib, e, compact(n=-1), "empty cloud")
    for t in (-1e-9, np.nan, np.inf, -np.inf):
        _refused(lib, e, compact(thr=t), "thr must be finite and >= 0")
    _refused(lib, e, compact(nbytes=ws - 1), "workspace too small")
    _refused(lib, e, compact(thr_dev=p, thr=np.nan, nbytes=ws - 1), "workspace too small")   # a device threshold: the host value is not read
    for bad in (-1, 1, 8, 48, 128):
        assert lib.nesti_debug_outlier_lanes(bad) != 0 and b"nesti_debug_outlier_lanes: lanes must be 0, 16, 32 or 64" in lib.nesti_last_error()
    for lanes in (16, 32, 64, 0):
        assert lib.nesti_debug_outlier_lanes(lanes) == 0


# ---- 2. the Python layer ---------------------------------------------------------------------------------------------------------------

def test_python_layer_validates():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough, outliers, pca, quadric, robust, select
    p = outliers.check_params()
    assert p == ("statistical", 16, 1.0, None, None, 1) and outliers.as_params(None) is None and outliers.as_params("statistical") == p
    assert outliers.as_params(p) == p and outliers.as_params({"k": 8, "std_ratio": 2, "passes": 3}) == ("statistical", 8, 2.0, None, None, 3)
    r = outliers.as_params({"mode": "radius", "radius": 0.05})
    assert r == ("radius", 16, 1.0, 0.05, 16, 1) and outliers.as_params({"mode": "radius", "radius": 1, "min_neighbours": 3}).min_neighbours == 3
    assert outliers.check_params(k=255).k == 255 and outliers.check_params(std_ratio=0).std_ratio == 0.0 and outliers.check_params(passes=8).passes == 8
    for kw, word in (({"k": 0}, "k must"), ({"k": 256}, "k must"), ({"k": 2.5}, "k must"), ({"k": True}, "k must"),
                     ({"std_ratio": -0.1}, "std_ratio"), ({"std_ratio": float("nan")}, "std_ratio"), ({"std_ratio": float("inf")}, "std_ratio"),
                     ({"std_ratio": "wide"}, "std_ratio"), ({"passes": 0}, "passes"), ({"passes": 9}, "passes"), ({"passes": 1.0}, "passes"),
                     ({"mode": "median"}, "mode must be"), ({"radius": 0.1}, "belong to mode='radius'"),
                     ({"min_neighbours": 4}, "belong to mode='radius'"), ({"mode": "radius"}, "needs a radius"),
                     ({"mode": "radius", "radius": 0.0}, "radius must be"), ({"mode": "radius", "radius": -1.0}, "radius must be"),
                     ({"mode": "radius", "radius": float("inf")}, "radius must be"), ({"mode": "radius", "radius": 1e200}, "radius must be"),
                     ({"mode": "radius", "radius": 0.1, "min_neighbours": 0}, "min_neighbours"),
                     ({"mode": "radius", "radius": 0.1, "min_neighbours": 256}, "min_neighbours")):
        with pytest.raises(ValueError, match=word):
            outliers.check_params(**kw)
        with pytest.raises(ValueError, match=word):
            outliers.as_params(kw)
        with pytest.raises(ValueError, match=word):
            outliers.remove_outliers(np.zeros((10, 3), np.float32), **kw)
    for bad, word in (("radius", "needs its radius"), ("median", "outliers must be"), (3, "outliers must be"), (True, "outliers must be"),
                      ({"iters": 2}, "unknown key")):
        with pytest.raises(ValueError, match=word):
            outliers.as_params(bad)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        outliers.remove_outliers(np.zeros((10, 2), np.float32))
    for t in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="thr must be"):
            outliers.check_threshold(t)
    # outliers= of the estimators: the ranges and the pidx refusal come before anything is prepared
    pts = np.zeros((10, 3), np.float32)
    for fit, kw in ((pca.pca_normals, {}), (pca.pca_normals, {"knn": 8}), (quadric.quadric_fit, {}), (hough.hough_normals, {"knn": 8}),
                    (robust.robust_normals, {"knn": 8}), (select.select_normals, {})):
        with pytest.raises(ValueError, match="outliers with pidx is not served yet"):
            fit(pts, pidx=[0, 1], outliers="statistical", **kw)
        with pytest.raises(ValueError, match="k must"):
            fit(pts, outliers={"k": 0}, **kw)
        with pytest.raises(ValueError, match="needs its radius"):
            fit(pts, outliers="radius", **kw)
    # the host scatter: rows back to the rows of the input
    res = {"normals": np.ones((3, 2), np.float32), "expert": np.array([4, 5, 6], np.int32), "orient": {"n_flipped": 1}, "scalar": 3}
    back = outliers.scatter_result(res, np.array([0, 2, 5]), 6)
    assert back["normals"].dtype == np.float32 and back["normals"].tolist() == [[1, 1], [0, 0], [1, 1], [0, 0], [0, 0], [1, 1]]
    assert back["expert"].tolist() == [4, -1, 5, -1, -1, 6] and back["orient"] == {"n_flipped": 1} and back["scalar"] == 3


# ---- 3. the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, word", [
    (["--outliers", "statistical", "--sparse_patches", "1"], "--outliers does not go with --sparse_patches 1"),
    (["--outliers", "statistical", "--subsample", "reference"], "--outliers does not go with --subsample reference"),
    (["--estimator", "pca", "--outliers", "radius", "--outlier_radius", "0.1", "--sparse_patches", "1"], "--outliers does not go with --sparse_patches 1"),
    (["--outliers", "statistical", "--depth_images", "1", "--depth_stride", "2"], "--outliers does not go with --depth_stride 2"),
    (["--outliers", "radius"], "--outliers radius needs --outlier_radius R"),
    (["--outliers", "statistical", "--outlier_radius", "0.1"], "--outlier_radius belongs to --outliers radius"),
    (["--outliers", "radius", "--outlier_radius", "0.1", "--outlier_std", "2"], "--outlier_std belongs to --outliers statistical"),
    (["--outliers", "median"], "invalid choice"),
    (["--outlier_k", "8"], "--outlier_k belongs to --outliers"),
    (["--outlier_std", "2"], "--outlier_std belongs to --outliers"),
    (["--estimator", "quadric", "--outlier_passes", "2"], "--outlier_passes belongs to --outliers"),
    (["--outlier_radius", "0.1"], "--outlier_radius belongs to --outliers"),
    (["--outliers", "statistical", "--outlier_k", "0"], "k must be an integer in 1 .. 255"),
    (["--outliers", "statistical", "--outlier_k", "256"], "k must be an integer in 1 .. 255"),
    (["--outliers", "statistical", "--outlier_std", "-1"], "std_ratio must be >= 0"),
    (["--outliers", "statistical", "--outlier_passes", "9"], "passes must be an integer in 1 .. 8"),
    (["--outliers", "radius", "--outlier_radius", "0"], "radius must be > 0"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and not (tmp_path / "out").exists()       # refused while parsing: nothing was created


# ---- 4. the restatement ------------------------------------------------------------------------------------------------------------------

def test_statistics_against_plain_numpy():
    """The fixed tree of ``threshold`` against ``numpy.mean`` / ``numpy.std(ddof=1)``: 1e-12 relative, over sizes at the block borders and
    with absent scores."""
    rs = np.random.RandomState(3)
    for M in (1, 2, 255, 256, 257, 5000, 65537):
        sc = rs.uniform(0.01, 2.0, M)
        hole = rs.rand(M) < 0.1
        if M > 2:
            sc[hole] = np.where(rs.rand(int(hole.sum())) < 0.5, np.nan, np.inf)
        live = sc[np.isfinite(sc)]
        for ratio in (0.0, 1.0, 2.5):
            n, mean, std, thr = ox.threshold(sc, ratio)
            assert n == len(live)
            assert abs(mean - live.mean()) <= 1e-12 * abs(live.mean())
            want = live.std(ddof=1) if len(live) >= 2 else 0.0
            assert abs(std - want) <= 1e-12 * max(want, 1e-300)
            assert abs(thr - (live.mean() + ratio * want)) <= 1e-12 * abs(thr)
    assert ox.threshold(np.array([np.nan, np.inf, -np.inf]), 1.0).tolist() == [0.0, 0.0, 0.0, np.inf]
    assert ox.threshold(np.array([np.nan, 0.25]), 3.0).tolist() == [1.0, 0.25, 0.0, 0.25]


def test_scores_against_plain_numpy_and_a_lane_group_gives_the_bytes_of_the_wave():
    """The mean of the restatement against a plain sorted-distance mean (1e-12 relative), kth_d2 exactly; k + 1 <= 16 / 32 in a lane
    group of 16 / 32 gives the bytes of the 64-lane statement; duplicates are other points at distance 0."""
    pts, _, _ = ox.noisy_cloud("box", 1, n=400, n_out=20)
    pts[7] = pts[3]
    pts[9] = pts[3]                                                         # a triple: 3, 7, 9
    nbr = ox.knn_brute(pts, 64)
    p64 = pts.astype(np.float64)
    for k in (1, 2, 15, 16, 31, 63):
        s = ox.scores(pts, 0, nbr, k)
        d = np.sqrt(((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(d, np.inf)
        d.sort(1)
        assert np.allclose(s["mean"], d[:, :k].mean(1), rtol=1e-12, atol=0)
        assert np.allclose(np.sqrt(s["kth_d2"]), d[:, k - 1], rtol=1e-12, atol=0) and (s["n_other"] == k).all()
        for lanes in (16, 32):
            if k + 1 <= lanes:
                g = ox.scores(pts, 0, nbr, k, lanes=lanes)
                assert all(np.array_equal(s[key].view(np.uint8), g[key].view(np.uint8)) for key in s), (k, lanes)
    s2 = ox.scores(pts, 0, nbr, 2)
    for row in (3, 7, 9):                                                    # the two other copies: distance 0, whatever their index
        assert s2["mean"][row] == 0.0 and s2["kth_d2"][row] == 0.0
    # rows in two batches
    a, b = ox.scores(pts, 0, nbr[:137], 16), ox.scores(pts, 137, nbr[137:], 16)
    whole = ox.scores(pts, 0, nbr, 16)
    assert all(np.array_equal(np.concatenate([a[key], b[key]]), whole[key]) for key in whole)


@pytest.mark.parametrize("shape, seed", ox.FILTER_CLOUDS)
def test_far_points_leave_and_the_surface_stays(shape, seed):
    """The clouds of tests/test_gpu_outliers.py (2000 surface points + 100 drawn uniformly in the bounding box, shuffled), k = 16,
    std_ratio = 1, one pass, on the restatement alone: every injected point farther from the clean surface -- from its nearest clean
    sample, which is at least as far as the surface itself, so no fewer points are asked for -- than 4 x the median nearest-neighbour
    spacing of the clean points is removed, and at most 8 % of the clean rows are.  The GPU test inherits this through byte equality."""
    pts, injected, clean = ox.noisy_cloud(shape, seed)
    res = ox.remove(pts, "statistical", 16, 1.0, passes=1)
    c64 = clean.astype(np.float64)
    d = np.sqrt(((c64[:, None, :] - c64[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    spacing = float(np.median(d.min(1)))
    off = np.sqrt(((pts[injected].astype(np.float64)[:, None, :] - c64[None, :, :]) ** 2).sum(-1)).min(1)
    far = off > 4.0 * spacing
    removed = ~res["inlier"]
    lost = removed[~injected].mean()
    print("%s seed %d: spacing %.4g, %d of %d injected are far, %d of them removed; clean rows removed %.2f %%; threshold %.6g"
          % (shape, seed, spacing, int(far.sum()), int(injected.sum()), int(removed[injected][far].sum()), 100.0 * lost,
             res["passes"][0]["threshold"]))
    assert far.sum() >= 20                                                   # the condition is not vacuous: a fifth of the injected points
    assert removed[injected][far].all()
    assert lost <= 0.08
    assert res["passes"][0]["removed"] == int(removed.sum()) and np.array_equal(res["kept"], np.flatnonzero(res["inlier"]))
    assert np.array_equal(res["points"].view(np.uint32), pts[res["kept"]].view(np.uint32))
    # a second pass only removes more, and sees the compacted cloud
    two = ox.remove(pts, "statistical", 16, 1.0, passes=2)
    assert two["passes"][0] == res["passes"][0] and not (two["inlier"] & ~res["inlier"]).any()
    assert two["passes"][1]["n"] == len(res["kept"])
