"""Normal smoothing without a GPU: every refusal of ``nesti_smooth_normals_nbr`` through ctypes (each returns before any device call),
the range checks of the Python layer, the ``--smooth`` parser errors, and the properties of the tests' restatement
(tests/_smooth_fixture.py): creases are fixed points, noise on a smooth surface is halved, a row never leaves its own half-space, and a
16-lane grouping of the sums gives the bytes of the 64-lane statement."""
import ctypes
import math

import numpy as np
import pytest

import _knn_fixture as kx
import _smooth_fixture as sx

COS45 = math.cos(math.radians(45.0))
ENTRY = "nesti_smooth_normals_nbr"


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------

def _refused(lib, rc, word):
    msg = lib.nesti_last_error() or b""
    assert rc != 0 and word.encode() in msg and msg.startswith((ENTRY + ":").encode()), (rc, msg, word)


def test_refusals_need_no_device():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    dummy, other = np.zeros(8, np.float32), np.zeros(8, np.float32)         # never dereferenced: the checks come first
    p, o = ctypes.c_void_p(dummy.ctypes.data), ctypes.c_void_p(other.ctypes.data)
    N, M, K = 1000, 100, 64

    def call(cloud=p, n=N, nin=p, q=p, m=M, row0=0, nbr=p, K=K, k=16, cos_t=COS45, falloff=0.75, nout=o):
        return getattr(lib, ENTRY)(cloud, n, nin, q, m, row0, nbr, K, k, cos_t, falloff, nout, o, o, None)

    # the errors of nesti_pca_normals_nbr
    _refused(lib, call(cloud=None), "null")
    _refused(lib, call(nbr=None), "null")
    _refused(lib, call(n=0), "empty cloud")
    _refused(lib, call(K=0), "K must be in 1 .. 256")
    _refused(lib, call(K=257), "K must be in 1 .. 256")
    _refused(lib, call(m=-1), "M must be")
    _refused(lib, call(row0=-1), "query_row0")
    _refused(lib, call(q=None, row0=N - M + 1), "exceed the cloud")
    # the pass's own
    _refused(lib, call(nin=None), "null normals_in_dev")
    for k in (0, -1, K + 1):
        _refused(lib, call(k=k), "k must be in 1 .. K")
    for c in (-1e-9, 1.0, 0.9999991, np.nan, np.inf, -np.inf):
        _refused(lib, call(cos_t=c), "cos_t must be finite and in [0, 0.999999]")
    for f in (-0.01, 1.01, np.nan, np.inf):
        _refused(lib, call(falloff=f), "falloff must be finite and in [0, 1]")
    _refused(lib, call(nout=p), "normals_out_dev must not be normals_in_dev")
    # M = 0 is a no-op at the ends of every range, and an argument error is still one
    assert call(q=None, m=0, k=1, cos_t=0.0, falloff=0.0) == 0 and call(q=None, m=0, k=K, cos_t=0.999999, falloff=1.0) == 0
    assert call(q=None, m=0, row0=N, K=256, k=256, nout=None) == 0
    _refused(lib, call(q=None, m=0, cos_t=np.nan), "cos_t")
    _refused(lib, call(q=None, m=0, nout=p), "must not be normals_in_dev")
    # the lane-group selector of the measurements: 0, 16, 32, 64 and nothing else
    for bad in (-1, 1, 8, 48, 128):
        assert lib.nesti_debug_smooth_lanes(bad) != 0 and b"nesti_debug_smooth_lanes: lanes must be 0, 16, 32 or 64" in lib.nesti_last_error()
    for lanes in (16, 32, 64, 0):
        assert lib.nesti_debug_smooth_lanes(lanes) == 0


# ---- 2. the Python layer ---------------------------------------------------------------------------------------------------------------

def test_python_layer_validates():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough, pca, quadric, smooth
    p = smooth.check_params()
    assert (p.k, p.iters, p.angle, p.falloff) == (16, 2, 45.0, 0.75) and p.cos_t == COS45
    assert smooth.check_params(angle=90.0).cos_t == math.cos(math.radians(90.0)) and 0.0 <= smooth.check_params(angle=90.0).cos_t < 1e-16
    assert smooth.check_params(angle=1e-3).cos_t == smooth.MAX_COS
    assert smooth.as_params(None) is None and smooth.as_params(3) == p._replace(iters=3)
    assert smooth.as_params({"k": 8, "angle": 30.0}) == smooth.check_params(k=8, angle=30.0)
    for kw, word in (({"k": 0}, "k must"), ({"k": 257}, "k must"), ({"k": 2.5}, "k must"), ({"iters": 0}, "iters"), ({"iters": 65}, "iters"),
                     ({"iters": True}, "iters"), ({"angle": 0.0}, "angle"), ({"angle": -5.0}, "angle"), ({"angle": 90.5}, "angle"),
                     ({"angle": float("nan")}, "angle"), ({"angle": "wide"}, "angle"), ({"falloff": -0.1}, "falloff"),
                     ({"falloff": 1.5}, "falloff"), ({"falloff": float("inf")}, "falloff")):
        with pytest.raises(ValueError, match=word):
            smooth.check_params(**kw)
        with pytest.raises(ValueError, match=word):
            smooth.as_params(kw)
        with pytest.raises(ValueError, match=word):
            smooth.smooth_normals(np.zeros((10, 3), np.float32), np.zeros((10, 3), np.float32), **kw)
    for bad, word in ((0, "iters"), (65, "iters"), (2.0, "smooth must be"), ("2", "smooth must be"), (True, "smooth must be"),
                      ({"passes": 2}, "unknown key")):
        with pytest.raises(ValueError, match=word):
            smooth.as_params(bad)
    for c, f, word in ((-0.1, 0.5, "cos_t"), (1.0, 0.5, "cos_t"), (float("nan"), 0.5, "cos_t"), (0.5, 1.1, "falloff")):
        with pytest.raises(ValueError, match=word):
            smooth.check_pass(16, c, f)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        smooth.smooth_normals(np.zeros((10, 3), np.float32), np.zeros((9, 3), np.float32))
    # smooth= needs a normal at every point, and its ranges are checked before anything is prepared
    pts = np.zeros((10, 3), np.float32)
    for fit, kw in ((pca.pca_normals, {}), (pca.pca_normals, {"knn": 8}), (quadric.quadric_fit, {}), (hough.hough_normals, {"knn": 8})):
        with pytest.raises(ValueError, match="smooth needs all points"):
            fit(pts, pidx=[0, 1], smooth=2, **kw)
        with pytest.raises(ValueError, match="smooth needs all points"):
            fit(pts, queries=np.zeros((2, 3), np.float32), smooth={"iters": 1}, **kw)
        with pytest.raises(ValueError, match="iters"):
            fit(pts, smooth=0, **kw)
        with pytest.raises(ValueError, match="angle"):
            fit(pts, smooth={"angle": 91.0}, **kw)


# ---- 3. the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, word", [
    (["--smooth", "2", "--sparse_patches", "1"], "--smooth does not go with --sparse_patches 1: not all rows have normals"),
    (["--smooth", "2", "--query_positions", "1"], "--smooth does not go with --query_positions 1: not all rows have normals"),
    (["--smooth", "2", "--depth_images", "1"], "--smooth does not go with --depth_images 1"),
    (["--estimator", "pca", "--smooth", "1", "--sparse_patches", "1"], "--smooth does not go with --sparse_patches 1"),
    (["--estimator", "hough", "--knn", "64", "--smooth", "1", "--query_positions", "1"], "--smooth does not go with --query_positions 1"),
    (["--smooth_k", "8"], "--smooth_k belongs to --smooth ITERS"),
    (["--smooth_angle", "30"], "--smooth_angle belongs to --smooth ITERS"),
    (["--estimator", "quadric", "--smooth_falloff", "0.5"], "--smooth_falloff belongs to --smooth ITERS"),
    (["--smooth", "65"], "iters must be an integer in 1 .. 64"),
    (["--smooth", "-1"], "iters must be an integer in 1 .. 64"),
    (["--smooth", "2", "--smooth_k", "0"], "k must be an integer in 1 .. 256"),
    (["--smooth", "2", "--smooth_angle", "0"], "angle must be"),
    (["--smooth", "2", "--smooth_angle", "120"], "angle must be"),
    (["--smooth", "2", "--smooth_falloff", "2"], "falloff must be"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and not (tmp_path / "out").exists()       # refused while parsing: nothing was created


# ---- 4. the restatement ------------------------------------------------------------------------------------------------------------------

def _cloud(shape, n=2000, seed=5):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    pts, nrm = synth.make_cloud(shape, n=n, seed=seed)
    return pts, nrm, kx.search(pts, pts, 16)[0]


def _rms_angle(a, b):
    """The RMS of the unoriented angle between the rows of a and b, in degrees."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    c = np.abs((a * b).sum(1)) / np.sqrt((a * a).sum(1) * (b * b).sum(1))
    return float(np.degrees(np.sqrt((np.arccos(np.minimum(c, 1.0)) ** 2).mean())))


def test_creases_are_fixed_points():
    """box, n = 2000, seed 5: the analytic normals under random signs, k = 16, 45 degrees, falloff 0.75, 3 passes.  A neighbour on the
    other face of a crease is perpendicular and has no weight, a neighbour on the same face is the same axis: the output equals the
    input exactly (by value: written zeros are +0)."""
    pts, nrm, nbr = _cloud("box")
    signs = np.where(np.random.RandomState(11).rand(len(pts)) < 0.5, -1.0, 1.0)
    given = (nrm * signs[:, None]).astype(np.float32)
    res = sx.iterate(pts, given, np.arange(len(pts)), nbr, 16, COS45, 0.75, 3)
    assert np.array_equal(res["normals"], given)
    assert (res["count"] >= 1).all() and (res["count"] <= 16).all() and (res["count"] < 16).any()      # rows at a crease lost neighbours
    assert np.array_equal(res["support"] > 0, np.ones(len(pts), bool))


def _noisy_sphere():
    pts, nrm, nbr = _cloud("sphere")
    rs = np.random.RandomState(7)
    noisy = nrm.astype(np.float64) + rs.normal(0.0, np.radians(10.0) / np.sqrt(2.0), nrm.shape)      # about 10 degrees RMS
    noisy /= np.linalg.norm(noisy, axis=1, keepdims=True)
    noisy *= np.where(rs.rand(len(pts)) < 0.5, -1.0, 1.0)[:, None] * rs.uniform(0.5, 2.0, len(pts))[:, None]
    return pts, nrm, nbr, noisy.astype(np.float32)


def test_noise_on_a_sphere_is_halved_and_rows_keep_their_side():
    """sphere, n = 2000, seed 5: the analytic normals perturbed by about 10 degrees RMS (RandomState(7)), under random signs and with
    lengths in 0.5 .. 2; one pass at the defaults (k = 16, 45 degrees, falloff 0.75) brings the unoriented RMS angle to the analytic
    normals below half the input's, the output is of unit length, and no row leaves its own half-space (out . in >= 0).

    Measured with this restatement: 10.04 degrees -> 4.11 degrees."""
    pts, nrm, nbr, noisy = _noisy_sphere()
    res = sx.restate(pts, noisy, np.arange(len(pts)), nbr, 16, COS45, 0.75)
    before, after = _rms_angle(noisy, nrm), _rms_angle(res["normals"], nrm)
    print("unoriented RMS angle: %.2f degrees -> %.2f degrees" % (before, after))
    assert 8.0 < before < 12.0 and after < 0.5 * before
    out = res["normals"].astype(np.float64)
    assert np.abs(np.sqrt((out * out).sum(1)) - 1.0).max() < 1e-6
    assert ((out * noisy.astype(np.float64)).sum(1) >= 0.0).all()
    assert (res["count"] >= 1).all() and (res["support"] >= 1.0).all()       # the row itself: t = 1, u = 1
    # ... and over more passes, on the box under the same treatment, where creases cut the neighbourhoods
    bpts, bnrm, bnbr = _cloud("box")
    rs = np.random.RandomState(3)
    given = (bnrm + rs.normal(0.0, 0.1, bnrm.shape)) * np.where(rs.rand(len(bpts)) < 0.5, -1.0, 1.0)[:, None]
    cur = given.astype(np.float32)
    for _ in range(3):
        nxt = sx.restate(bpts, cur, np.arange(len(bpts)), bnbr, 16, COS45, 0.75)["normals"]
        assert ((nxt.astype(np.float64) * cur.astype(np.float64)).sum(1) >= 0.0).all()
        cur = nxt


def test_a_lane_group_gives_the_bytes_of_the_wave():
    """For k <= 16 the sums of a 16-lane (and a 32-lane) group equal the 64-lane statement's on the bytes: the missing lanes' partial
    sums are +0.0, adding them is exact, and written zeros are +0."""
    pts, nrm, nbr, noisy = _noisy_sphere()
    noisy[5] = 0.0                                                           # ineligible rows take no part
    noisy[9, 1] = np.nan
    noisy[12] = [-0.0, 0.0, -1.0]
    bpts, bnrm, bnbr = _cloud("box")
    axis = (bnrm * np.where(np.random.RandomState(2).rand(len(bpts)) < 0.5, -1.0, 1.0)[:, None]).astype(np.float32)   # sums with zero components
    for cloud, normals, lists in ((pts, noisy, nbr), (bpts, axis, bnbr)):
        for k in (1, 2, 7, 15, 16):
            for cos_t, falloff in ((0.0, 1.0), (COS45, 0.75), (0.999, 0.0)):
                wave = sx.restate(cloud, normals, np.arange(len(cloud)), lists, k, cos_t, falloff)
                for lanes in (16, 32):
                    group = sx.restate(cloud, normals, np.arange(len(cloud)), lists, k, cos_t, falloff, lanes=lanes)
                    for key in wave:
                        assert np.array_equal(wave[key].view(np.uint8), group[key].view(np.uint8)), (key, k, lanes)
    wide = sx.restate(pts, noisy, np.arange(len(pts)), kx.search(pts, pts, 32)[0], 32, COS45, 0.75)
    group = sx.restate(pts, noisy, np.arange(len(pts)), kx.search(pts, pts, 32)[0], 32, COS45, 0.75, lanes=32)
    assert all(np.array_equal(wide[key].view(np.uint8), group[key].view(np.uint8)) for key in wide)
    for row in (5, 9):                                                       # an ineligible row comes back bit for bit, alone
        assert np.array_equal(wide["normals"][row].view(np.uint32), noisy[row].view(np.uint32)) and wide["count"][row] == 0 and wide["support"][row] == 0
    assert wide["count"][12] >= 1
