"""Point denoising without a GPU: every refusal of ``nesti_denoise_points_nbr`` through ctypes (each returns before any device call),
the range checks of the Python layer, the ``denoise=`` and ``--denoise`` refusals, and the properties of the tests' restatement
(tests/_denoise_fixture.py) that follow from the statement: a plane is a fixed point, noise along the normal is replaced by the
neighbourhood's mean, ``step`` scales the displacement, the signs of the normals do not matter, rows that cannot move are copied bit for
bit, a neighbour beyond the cone or without a normal adds nothing, and a lane group gives the bytes of the 64-lane statement."""
import ctypes
import math

import numpy as np
import pytest

import _denoise_fixture as dx
import _knn_fixture as kx

COS45 = math.cos(math.radians(45.0))
ENTRY = "nesti_denoise_points_nbr"
KEYS = ("points", "delta", "support", "count")


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------

def _refused(lib, rc, word):
    msg = lib.nesti_last_error() or b""
    assert rc != 0 and word.encode() in msg and msg.startswith((ENTRY + ":").encode()), (rc, msg, word)


def test_refusals_need_no_device():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    N, M, K = 1000, 100, 64
    block = np.zeros(3 * N + 3 * M + 8, np.float32)                          # never dereferenced: the checks come first
    at = lambda floats: ctypes.c_void_p(block.ctypes.data + 4 * floats)      # noqa: E731
    p, o = at(0), at(3 * N)                                                  # the cloud (and every input); the outputs, behind its last row

    def call(cloud=p, n=N, nin=p, q=p, m=M, row0=0, nbr=p, K=K, k=16, cos_t=COS45, falloff=0.75, sigma=0.5, step=1.0, pout=o):
        return getattr(lib, ENTRY)(cloud, n, nin, q, m, row0, nbr, K, k, cos_t, falloff, sigma, step, pout, o, o, o, None)

    # the errors of nesti_smooth_normals_nbr
    _refused(lib, call(cloud=None), "null")
    _refused(lib, call(nbr=None), "null")
    _refused(lib, call(n=0), "empty cloud")
    _refused(lib, call(K=0), "K must be in 1 .. 256")
    _refused(lib, call(K=257), "K must be in 1 .. 256")
    _refused(lib, call(m=-1), "M must be")
    _refused(lib, call(row0=-1), "query_row0")
    _refused(lib, call(q=None, row0=N - M + 1), "exceed the cloud")
    _refused(lib, call(nin=None), "null normals_in_dev")
    for k in (0, -1, K + 1):
        _refused(lib, call(k=k), "k must be in 1 .. K")
    for c in (-1e-9, 1.0, 0.9999991, np.nan, np.inf, -np.inf):
        _refused(lib, call(cos_t=c), "cos_t must be finite and in [0, 0.999999]")
    for f in (-0.01, 1.01, np.nan, np.inf):
        _refused(lib, call(falloff=f), "falloff must be finite and in [0, 1]")
    # the pass's own
    for s in (0.0, -0.5, 1000000.0000001, np.nan, np.inf, -np.inf):
        _refused(lib, call(sigma=s), "sigma must be finite and in (0, 1e6]")
    for s in (0.0, -0.5, 1.0000000001, np.nan, np.inf):
        _refused(lib, call(step=s), "step must be finite and in (0, 1]")
    for where in (p, at(3), at(3 * (N - 1)), at(3 * N - 1)):                 # the cloud itself, its second row, its last row, its last float
        _refused(lib, call(pout=where), "points_out_dev must not lie inside the cloud")
    _refused(lib, call(cloud=at(3), pout=p), "points_out_dev must not lie inside the cloud")      # the cloud begins inside the output
    # M = 0 is a no-op at the ends of every range, and an argument error is still one
    assert call(q=None, m=0, k=1, cos_t=0.0, falloff=0.0, sigma=1e-300, step=1e-300) == 0
    assert call(q=None, m=0, k=K, cos_t=0.999999, falloff=1.0, sigma=1e6, step=1.0) == 0
    assert call(q=None, m=0, row0=N, K=256, k=256, pout=None) == 0
    _refused(lib, call(q=None, m=0, sigma=np.nan), "sigma")
    _refused(lib, call(q=None, m=0, pout=p), "must not lie inside the cloud")
    # the lane-group selector of the measurements: 0, 16, 32, 64 and nothing else
    for bad in (-1, 1, 8, 48, 128):
        assert lib.nesti_debug_denoise_lanes(bad) != 0 and b"nesti_debug_denoise_lanes: lanes must be 0, 16, 32 or 64" in lib.nesti_last_error()
    for lanes in (16, 32, 64, 0):
        assert lib.nesti_debug_denoise_lanes(lanes) == 0


# ---- 2. the Python layer ---------------------------------------------------------------------------------------------------------------

def test_python_layer_validates():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import denoise, hough, pca, quadric, robust, select
    p = denoise.check_params()
    assert (p.k, p.iters, p.angle, p.falloff, p.sigma, p.step, p.normal_k) == (16, 2, 45.0, 0.75, 0.5, 1.0, 32) and p.cos_t == COS45
    assert denoise.check_params(k=200).normal_k == 256 and denoise.check_params(k=8, normal_k=5).normal_k == 5
    assert denoise.check_params(angle=1e-3).cos_t == denoise.MAX_COS and denoise.check_params(sigma=1e6).sigma == 1e6
    assert denoise.as_params(None) is None and denoise.as_params(False) is None and denoise.as_params(True) == p
    assert denoise.as_params({"k": 8, "sigma": 0.25}) == denoise.check_params(k=8, sigma=0.25) and denoise.as_params(p) == p
    for kw, word in (({"k": 0}, "k must"), ({"k": 257}, "k must"), ({"k": 2.5}, "k must"), ({"iters": 0}, "iters"), ({"iters": 65}, "iters"),
                     ({"iters": True}, "iters"), ({"angle": 0.0}, "angle"), ({"angle": 90.5}, "angle"), ({"angle": float("nan")}, "angle"),
                     ({"falloff": -0.1}, "falloff"), ({"falloff": 1.5}, "falloff"), ({"sigma": 0.0}, "sigma"), ({"sigma": -1.0}, "sigma"),
                     ({"sigma": 1.1e6}, "sigma"), ({"sigma": float("nan")}, "sigma"), ({"sigma": "wide"}, "sigma"), ({"step": 0.0}, "step"),
                     ({"step": 1.5}, "step"), ({"step": float("inf")}, "step"), ({"normal_k": 0}, "normal_k"), ({"normal_k": 257}, "normal_k")):
        with pytest.raises(ValueError, match=word):
            denoise.check_params(**kw)
        with pytest.raises(ValueError, match=word):
            denoise.as_params(kw)
        with pytest.raises(ValueError, match=word):
            denoise.denoise_points(np.zeros((10, 3), np.float32), **kw)
    for bad, word in ((2, "denoise must be"), ("on", "denoise must be"), (2.0, "denoise must be"), ({"passes": 2}, "unknown key")):
        with pytest.raises(ValueError, match=word):
            denoise.as_params(bad)
    for args, word in (((16, -0.1, 0.5, 0.5, 1.0), "cos_t"), ((16, 0.5, 1.1, 0.5, 1.0), "falloff"), ((16, 0.5, 0.5, 0.0, 1.0), "sigma"),
                       ((16, 0.5, 0.5, 0.5, 0.0), "step"), ((0, 0.5, 0.5, 0.5, 1.0), "k must")):
        with pytest.raises(ValueError, match=word):
            denoise.check_pass(*args)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        denoise.denoise_points(np.zeros((10, 2), np.float32))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        denoise.denoise_points(np.zeros((10, 3), np.float32), normals=np.zeros((9, 3), np.float32))
    empty = denoise.denoise_points(np.zeros((0, 3), np.float32))
    assert empty["points"].shape == (0, 3) and empty["moved"] == 0
    # denoise= of the five estimators: checked before anything is prepared; pidx is refused
    pts = np.zeros((10, 3), np.float32)
    for fit, kw in ((pca.pca_normals, {}), (pca.pca_normals, {"knn": 8}), (quadric.quadric_fit, {}), (hough.hough_normals, {"knn": 8}),
                    (select.select_normals, {}), (robust.robust_normals, {"knn": 8})):
        for extra in ({}, {"outliers": "statistical"}, {"downsample": 0.5}):
            with pytest.raises(ValueError, match="denoise with pidx is not served"):
                fit(pts, pidx=[0, 1], denoise=True, **extra, **kw)
            with pytest.raises(ValueError, match="sigma"):
                fit(pts, denoise={"sigma": 0.0}, **extra, **kw)
            with pytest.raises(ValueError, match="unknown key 'passes'"):
                fit(pts, denoise={"passes": 2}, **extra, **kw)
            with pytest.raises(ValueError, match="denoise must be"):
                fit(pts, denoise=3, **extra, **kw)


# ---- 3. the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, word", [
    (["--denoise", "2"], "--denoise does not go with --estimator net"),
    (["--estimator", "pca", "--denoise", "2", "--sparse_patches", "1"], "--denoise does not go with --sparse_patches 1"),
    (["--estimator", "pca", "--denoise", "2", "--query_positions", "1"], "--denoise does not go with --query_positions 1"),
    (["--denoise", "2", "--depth_images", "1"], "--denoise does not go with --depth_images 1"),
    (["--estimator", "pca", "--denoise", "2", "--subsample", "reference"], "--denoise does not go with --subsample reference"),
    (["--estimator", "pca", "--denoise", "2", "--subsample", "reference_host"], "--denoise does not go with --subsample reference_host"),
    (["--estimator", "quadric", "--denoise", "2", "--reproducible", "1"], "--denoise does not go with --reproducible 1"),
    (["--estimator", "pca", "--denoise_k", "8"], "--denoise_k belongs to --denoise ITERS"),
    (["--denoise_angle", "30"], "--denoise_angle belongs to --denoise ITERS"),
    (["--estimator", "hough", "--knn", "64", "--denoise_falloff", "0.5"], "--denoise_falloff belongs to --denoise ITERS"),
    (["--estimator", "pca", "--denoise_sigma", "0.25"], "--denoise_sigma belongs to --denoise ITERS"),
    (["--estimator", "pca", "--denoise_step", "0.5"], "--denoise_step belongs to --denoise ITERS"),
    (["--estimator", "pca", "--denoise", "65"], "iters must be an integer in 1 .. 64"),
    (["--estimator", "pca", "--denoise", "-1"], "iters must be an integer in 1 .. 64"),
    (["--estimator", "pca", "--denoise", "2", "--denoise_k", "0"], "k must be an integer in 1 .. 256"),
    (["--estimator", "pca", "--denoise", "2", "--denoise_angle", "120"], "angle must be"),
    (["--estimator", "pca", "--denoise", "2", "--denoise_falloff", "2"], "falloff must be"),
    (["--estimator", "pca", "--denoise", "2", "--denoise_sigma", "0"], "sigma must be"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--denoise", "2", "--denoise_step", "1.5"], "step must be"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and not (tmp_path / "out").exists()       # refused while parsing: nothing was created


# ---- 4. the restatement ------------------------------------------------------------------------------------------------------------------

def _lattice(side=12, z=1.0):
    """A ``side`` x ``side`` lattice in the plane z = ``z`` (no coordinate is -0), its normals 0 0 1 and its 9-NN lists."""
    g = np.arange(side, dtype=np.float64) * 0.125
    pts = np.stack([np.repeat(g, side), np.tile(g, side), np.full(side * side, z)], 1).astype(np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(pts), 1))
    return pts, nrm, kx.search(pts, pts, 9)[0]


def test_a_plane_is_a_fixed_point():
    """Every height is exactly 0: H = 0, delta = 0, and p + 0 v = p."""
    pts, nrm, nbr = _lattice()
    for sigma, step in ((0.5, 1.0), (1e6, 0.3), (0.05, 1.0)):
        res = dx.restate(pts, nrm, np.arange(len(pts)), nbr, 9, COS45, 0.75, sigma, step)
        assert _same_bytes(res["points"], pts) and (res["delta"] == 0).all()
        assert (res["count"] == 9).all() and (res["support"] > 0).all()


def test_noise_along_the_normal_becomes_the_mean_of_the_list():
    """The lattice at z = 1 with seeded noise in z alone, exact normals, cos_t = 0, falloff = 0, sigma = 1e6, step = 1: t = u = 1 and
    g = 1 / (1 + x x) with x x <= 1e-12, so W differs from 1 by 2e-12 at most and the weighted mean height from the plain one by
    1e-12 of a height: the new z is the mean of the list's z to the one float32 rounding of the result (an ulp of 1.19e-7 at z = 1;
    the bound is 2 ulp).  x and y never change: v_x = v_y = 0 and p + delta 0 = p."""
    pts, nrm, nbr = _lattice()
    rs = np.random.RandomState(5)
    pts[:, 2] += rs.normal(0.0, 0.01, len(pts)).astype(np.float32)
    res = dx.restate(pts, nrm, np.arange(len(pts)), nbr, 9, 0.0, 0.0, 1e6, 1.0)
    mean = pts[:, 2].astype(np.float64)[nbr].mean(1)
    ulp = np.spacing(np.float32(1.0)).astype(np.float64)
    err = np.abs(res["points"][:, 2].astype(np.float64) - mean)
    print("largest |z - mean| in ulp of float32 at 1: %.3f" % (err.max() / ulp))
    assert err.max() <= 2 * ulp
    assert _same_bytes(res["points"][:, :2], pts[:, :2]) and (res["count"] == 9).all()
    assert np.abs(res["delta"].astype(np.float64) - (mean - pts[:, 2])).max() <= 2 * ulp
    # step = 0.5: half the displacement; a power of two scales the float64 delta and its float32 rounding exactly
    half = dx.restate(pts, nrm, np.arange(len(pts)), nbr, 9, 0.0, 0.0, 1e6, 0.5)
    assert np.array_equal(half["delta"], np.float32(0.5) * res["delta"]) and (res["delta"] != 0).any()
    assert _same_bytes(half["support"], res["support"]) and _same_bytes(half["count"], res["count"])
    # a step that is no power of two: to the roundings of the product and of the float32 result
    third = dx.restate(pts, nrm, np.arange(len(pts)), nbr, 9, 0.0, 0.0, 1e6, 0.3)
    assert np.abs(third["delta"].astype(np.float64) - 0.3 * res["delta"].astype(np.float64)).max() <= 1e-9


def _noisy_box(n=600, seed=5):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    pts, nrm = synth.make_cloud("box", n=n, seed=seed, noise=0.004)
    rs = np.random.RandomState(9)
    given = (nrm.astype(np.float64) + rs.normal(0.0, 0.1, nrm.shape)) * rs.uniform(0.5, 2.0, len(nrm))[:, None]
    return pts, given.astype(np.float32), kx.search(pts, pts, 40)[0]


def test_the_signs_of_the_normals_do_not_matter():
    """Every slot's terms are even in the sign of n_j; h, H and delta are odd in the sign of n_c, and so is v: the output position has
    the same bits under any flips, delta changes sign with the centre's normal only, support and count do not change."""
    pts, given, nbr = _noisy_box()
    rows = np.arange(len(pts))
    for k, sigma in ((16, 0.5), (40, 0.05)):
        ref = dx.restate(pts, given, rows, nbr, k, COS45, 0.75, sigma, 1.0)
        assert (ref["delta"] != 0).sum() > len(pts) // 2
        for seed in (1, 2):
            flip = np.random.RandomState(seed).rand(len(pts)) < 0.5
            got = dx.restate(pts, np.where(flip[:, None], -given, given), rows, nbr, k, COS45, 0.75, sigma, 1.0)
            for key in ("points", "support", "count"):
                assert _same_bytes(got[key], ref[key]), key
            assert np.array_equal(got["delta"], np.where(flip, -ref["delta"], ref["delta"]))


def test_rows_that_cannot_move_are_copied():
    """A centre whose normal is not eligible, a row with an empty list and a centre that is not finite: the three floats of the input,
    bit for bit, and delta, support and count 0 -- while their neighbours go on."""
    pts, given, nbr = _noisy_box()
    pts, given, nbr = pts.copy(), given.copy(), nbr.copy()
    given[3] = 0.0
    given[7] = [np.nan, 0.5, 0.5]
    given[12] = [0.0, -0.0, -0.0]
    given[20, 1] = np.inf
    given[11] = [-0.0, 0.0, 1.5]                                             # eligible
    nbr[30, 0] = -1                                                          # an empty prefix
    nbr[31, 0] = len(pts)
    pts[40] = [np.nan, 0.0, 0.0]                                             # centres that are not finite
    pts[41, 2] = -np.inf
    pts[42] = np.array([0x7fc12345, 0x3f800000, 0xff800000], np.uint32).view(np.float32)
    res = dx.restate(pts, given, np.arange(len(pts)), nbr, 16, COS45, 0.75, 0.5, 1.0)
    for row in (3, 7, 12, 20, 30, 31, 40, 41, 42):
        assert _same_bytes(res["points"][row], pts[row]) and res["delta"][row] == 0 and res["support"][row] == 0 and res["count"][row] == 0, row
    assert res["count"][11] >= 1 and (res["count"] > 0).sum() == len(pts) - 9
    assert (res["delta"] != 0).sum() > len(pts) // 2


def test_a_neighbour_beyond_the_cone_or_without_a_normal_adds_nothing():
    """One row of four slots -- the centre, two neighbours in its plane's cone and one whose normal is perpendicular.  The row equals the
    same row with that neighbour's normal 0 0 0 (not eligible), count is 3, and delta is the scalar sum of the three other slots in
    the butterfly's order, ((p0 + 0) + (p1 + p3)): the perpendicular neighbour's height, far the largest, is nowhere in it."""
    pts = np.array([[0, 0, 0], [0.5, 0, 0.01], [0, 0.5, 1.0], [-1, 0, -0.02], [9, 9, 9]], np.float32)
    nrm = np.array([[0, 0, 2], [0.1, 0, 1], [1, 0, 0], [0, -0.2, -1], [0, 0, 1]], np.float32)
    nbr = np.array([[0, 1, 2, 3]])
    cos_t, falloff, sigma, step = COS45, 0.75, 0.5, 0.3
    res = dx.restate(pts, nrm, [0], nbr, 4, cos_t, falloff, sigma, step)
    dead = nrm.copy()
    dead[2] = 0.0
    gone = dx.restate(pts, dead, [0], nbr, 4, cos_t, falloff, sigma, step)
    for key in KEYS:
        assert _same_bytes(res[key], gone[key]), key
    assert res["count"][0] == 3
    p, n = pts.astype(np.float64), nrm.astype(np.float64)
    r2 = max(float(((p[j] - p[0]) ** 2).sum()) for j in (0, 1, 2, 3))        # the perpendicular neighbour still counts for the radius
    rad = math.sqrt(r2)
    qc = float((n[0] * n[0]).sum())
    terms = {}
    for slot, j in ((0, 0), (1, 1), (3, 3)):
        d = p[j] - p[0]
        d2 = float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        qj = float((n[j, 0] * n[j, 0] + n[j, 1] * n[j, 1]) + n[j, 2] * n[j, 2])
        ca = abs(float((n[0, 0] * n[j, 0] + n[0, 1] * n[j, 1]) + n[0, 2] * n[j, 2])) / math.sqrt(qc * qj)
        t = min((ca - cos_t) / (1.0 - cos_t), 1.0)
        u = 1.0 - (falloff * d2) / r2
        h = float(d[2])                                                      # v = 0 0 1
        x = h / (sigma * rad)
        a = (u * t) * (1.0 / (1.0 + x * x))
        terms[slot] = (a * a * h, a * a)
    H = (terms[0][0] + 0.0) + (terms[1][0] + terms[3][0])
    W = (terms[0][1] + 0.0) + (terms[1][1] + terms[3][1])
    assert res["delta"][0] == np.float32(step * (H / W)) and res["support"][0] == np.float32(W)
    assert res["points"][0, 2] == np.float32(step * (H / W)) and abs(res["delta"][0]) < 0.01


def test_a_lane_group_gives_the_bytes_of_the_wave():
    """For k <= 16 the sums of a 16-lane (and a 32-lane) group equal the 64-lane statement's on the bytes: the missing lanes' partial
    sums are +0.0 and adding them is exact."""
    pts, given, nbr = _noisy_box()
    given[5] = 0.0
    given[9, 1] = np.nan
    rows = np.arange(len(pts))
    for k in (1, 2, 7, 15, 16, 17, 32):
        for cos_t, falloff, sigma in ((0.0, 1.0, 1e6), (COS45, 0.75, 0.5), (0.999, 0.0, 0.05)):
            wave = dx.restate(pts, given, rows, nbr, k, cos_t, falloff, sigma, 1.0)
            for lanes in (16, 32):
                if k <= lanes:
                    group = dx.restate(pts, given, rows, nbr, k, cos_t, falloff, sigma, 1.0, lanes=lanes)
                    for key in KEYS:
                        assert _same_bytes(wave[key], group[key]), (key, k, lanes)
