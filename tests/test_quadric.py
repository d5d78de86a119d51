"""The quadric fit without a GPU: the solve behind ``nesti_quadric_solve`` (csrc/quadric_solve.h, the arithmetic the kernel runs) against
numpy, its flip property, the tests' numpy restatement against the unit sphere, and the refusals of the Python layer and the command
line that come before any device call.

Bounds, with eps = 2^-53, N the 6 x 6 matrix of the moments and a numpy's solution:
  coefficients  ||a_lib - a|| <= 4 * 6 * eps * kappa_2(N) * ||a||: two backward-stable solves of a 6 x 6 system, each within
                ~6 eps kappa ||a|| of the exact solution
  curvatures    |k_lib - k| <= 2^-23 |k| + 8 (1 + ||a||) B with B that bound on a -- the rule of tests/test_gpu_quadric.py in the
                units of the fit (r = 1): the curvatures are Lipschitz in a with a constant below 8 (1 + ||a||)"""
import ctypes

import numpy as np
import pytest

import _pca_fixture as fx
import _quadric_fixture as qx

EPS = 2.0 ** -53
_D = ctypes.POINTER(ctypes.c_double)


def _lib():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    return _lib.load()


def _solve(m):
    m = np.ascontiguousarray(m, np.float64)
    a, k, ok = np.full(6, 7.0), np.full(2, 7.0), ctypes.c_int(-1)
    assert _lib().nesti_quadric_solve(m.ctypes.data_as(_D), a.ctypes.data_as(_D), k.ctypes.data_as(_D), ctypes.byref(ok)) == 0
    return a, k, ok.value


def _samples(rs, n):
    """n random (u, v, h) inside the unit ball: a random quadric height function plus noise, tilted."""
    u, v = rs.uniform(-0.7, 0.7, n), rs.uniform(-0.7, 0.7, n)
    c = rs.normal(size=6) * np.array([0.05, 0.3, 0.3, 0.5, 0.5, 0.5])
    h = np.clip(qx.monomials(u, v) @ c + rs.normal(scale=0.02, size=n), -0.7, 0.7)
    return u, v, h


def test_solver_against_numpy():
    rs = np.random.RandomState(3)
    worst_a = worst_k = 0.0
    i = 0
    while i < 2000:
        n = int(rs.choice([6, 7, 8, 12, 40, 300]))
        m = qx.moments(*_samples(rs, n))
        N, b = qx.normal_matrix(m)
        kappa = np.linalg.cond(N)
        if not kappa < 1e10:           # well-posed vectors only: six or seven random points can come close to a conic
            continue
        i += 1
        a, k, ok = _solve(m)
        assert ok == 1, (i, n, kappa)
        ref = np.linalg.solve(N, b)
        na = np.linalg.norm(ref)
        bound_a = 4 * 6 * EPS * kappa * na
        assert np.linalg.norm(a - ref) <= bound_a, (i, n, kappa)
        # the curvatures of numpy's solution by the textbook route: eigenvalues of I^-1 II
        g = ref[1:3]
        w = np.sqrt(1 + g @ g)
        first = np.eye(2) + np.outer(g, g)
        second = np.array([[2 * ref[3], ref[4]], [ref[4], 2 * ref[5]]]) / w
        kr = np.sort(np.linalg.eigvals(np.linalg.inv(first) @ second).real)[::-1]
        bound_k = 2.0 ** -23 * np.abs(kr) + 8 * (1 + na) * bound_a
        assert (np.abs(k - kr) <= bound_k).all() and k[0] >= k[1], (i, k, kr)
        worst_a = max(worst_a, np.linalg.norm(a - ref) / bound_a)
        worst_k = max(worst_k, (np.abs(k - kr) / bound_k).max())
    print("largest error over bound: coefficients %.3g, curvatures %.3g" % (worst_a, worst_k))


def test_solver_fails_on_rank_deficient_and_nan_moments():
    rs = np.random.RandomState(4)
    u, v, h = _samples(rs, 50)
    cases = {"all v = 0": qx.moments(u, np.zeros(50), h), "five points": qx.moments(u[:5], v[:5], h[:5]),
             "collinear": qx.moments(u, 2 * u, h), "no points": np.zeros(21)}
    good = qx.moments(u, v, h)
    assert _solve(good)[2] == 1
    for i in (0, 4, 12, 17):
        bad = good.copy()
        bad[i] = np.nan
        cases["NaN at %d" % i] = bad
    cases["all NaN"] = np.full(21, np.nan)
    cases["inf"] = np.where(np.arange(21) == 3, np.inf, good)
    for name, m in cases.items():
        a, k, ok = _solve(m)
        assert ok == 0 and not a.any() and not k.any(), name        # a failed fit: finite (zero) outputs


def test_flip_property_of_the_solver():
    """Negating the moments that are odd in (u, h) gives a -> (-a0, a1, -a2, -a3, a4, -a5) and k -> (-k_min, -k_max), exactly."""
    rs = np.random.RandomState(5)
    # u -> -u, h -> -h: sum u^p v^q changes sign for odd p; sum h u^p v^q for even p
    sign = np.array([-1.0 if p % 2 else 1.0 for deg in range(5) for p in (deg - q for q in range(deg + 1))]
                    + [-1.0 if p % 2 == 0 else 1.0 for p in qx.PU])
    for _ in range(200):
        u, v, h = _samples(rs, int(rs.choice([6, 9, 50])))
        m = qx.moments(u, v, h)
        assert np.array_equal(m * sign, qx.moments(-u, v, -h))
        a, k, ok = _solve(m)
        a2, k2, ok2 = _solve(m * sign)
        assert ok == ok2
        assert np.array_equal(a2, a * np.array([-1, 1, -1, -1, 1, -1.0])) and np.array_equal(k2, -k[::-1])


def test_solver_refuses_null_pointers():
    lib = _lib()
    m, a, k, ok = np.zeros(21), np.zeros(6), np.zeros(2), ctypes.c_int(0)
    args = [m.ctypes.data_as(_D), a.ctypes.data_as(_D), k.ctypes.data_as(_D), ctypes.byref(ok)]
    for i in range(4):
        assert lib.nesti_quadric_solve(*[None if j == i else x for j, x in enumerate(args)]) == 1
        assert b"null" in lib.nesti_last_error()


def test_restatement_finds_the_sphere_curvatures():
    """The restatement itself on the 20 000-point unit sphere at radius 0.1 bbdiag, fed the plane-fit restatement's normals: with the
    curvatures referred to the outward normal both are negative and |k + 1| stays below 2 x 0.033, the spread measured when the
    estimator was defined (this test prints 0.0323 for k_max and 0.0325 for k_min over its 256 rows; the degree-2 bias of balls of ~600 points, not rounding)."""
    c = qx.cloud("sphere_big")
    rows, r = c["rows"], [c["r_abs"][1]]
    n0 = fx.predicted("sphere_big")["normals"][:len(rows), 1:2]
    res = qx.restate(c["pts"], c["pts"][rows], r, n0)
    assert res["ok"].all()
    out = (res["normals"][:, 0].astype(np.float64) * c["gt"][rows]).sum(1) > 0
    k = np.where(out[:, None], res["curv"][:, 0], -res["curv"][:, 0, ::-1]).astype(np.float64)
    spread = np.abs(k + 1.0).max(axis=0)
    print("unit sphere, r = %.4g: k_max in [%.4f, %.4f], k_min in [%.4f, %.4f]; largest |k + 1| %.4f (k_max), %.4f (k_min); RMS angle of "
          "nu %.3f degrees, of n0 %.3f" % (r[0], k[:, 0].min(), k[:, 0].max(), k[:, 1].min(), k[:, 1].max(), spread[0], spread[1],
                                           fx.angle_rms_deg(res["normals"][:, 0], c["gt"][rows]), fx.angle_rms_deg(n0[:, 0], c["gt"][rows])))
    assert (k < 0).all() and (k[:, 0] >= k[:, 1]).all()
    assert spread.max() <= 2 * 0.033


def test_python_layer_refuses_before_any_device_call():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import quadric
    pts = np.zeros((10, 3), np.float32)
    for bad in (3, -4, 17, 0.5):
        with pytest.raises(ValueError, match="scale"):
            quadric.quadric_fit(pts, scale=bad)
    with pytest.raises(ValueError, match="mutually exclusive"):
        quadric.quadric_fit(pts, pidx=[0, 1], queries=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="orient"):
        quadric.quadric_fit(pts, orient="up")
    with pytest.raises(ValueError, match="viewpoint"):
        quadric.quadric_fit(pts, orient="viewpoint")
    H, K = quadric.mean_gauss(np.array([[2, 1], [-1, -3], [0, 0]], np.float32))
    assert H.dtype == np.float32 and H.tolist() == [1.5, -2.0, 0.0] and K.tolist() == [2.0, 3.0, 0.0]


@pytest.mark.parametrize("extra, word", [(["--depth_images", "1"], "--depth_images 1"), (["--reproducible", "1"], "--reproducible 1"),
                                         (["--subsample", "reference"], "--subsample reference"),
                                         (["--subsample", "reference_host"], "--subsample reference_host")])
def test_command_line_refusals(extra, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--estimator", "quadric", "--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)] + extra)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--estimator quadric does not take " + word in err
    assert not (tmp_path / "out").exists()                      # refused while parsing: nothing was created


def test_command_line_flags(capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    f = cli.build_parser().parse_args(["--estimator", "quadric"])
    assert f.estimator == "quadric" and f.quadric_scale == -1 and cli.build_parser().parse_args([]).quadric_scale == -1
    for argv, message in ((["--quadric_scale", "0"], "--quadric_scale belongs to --estimator quadric"),
                          (["--estimator", "pca", "--quadric_scale", "0"], "--quadric_scale belongs to --estimator quadric"),
                          (["--estimator", "quadric", "--pca_scale", "0"], "--pca_scale belongs to --estimator pca")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + ["--results_path", str(tmp_path / "out")])
        assert e.value.code == 2 and message in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
