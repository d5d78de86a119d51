"""k-nearest neighbourhoods without a GPU: the tests' restatement of the search (tests/_knn_fixture.py) against scipy's cKDTree on a
tie-free cloud, the search kernel's stop rule with its margin emulated on the grids of tests/_grid_fixture.py, every refusal of the six
C entries through ctypes (each returns before any device call), the validation of ``ks`` / ``knn=`` in the Python layer, and the
``--knn`` parser errors."""
import ctypes

import numpy as np
import pytest

import _knn_fixture as kx


def test_restatement_against_ckdtree():
    """A random cloud has no two equal distances (asserted), so the (d2, index) order is the distance order and cKDTree's answer is the
    restatement's: indices equal, distances to a few ulp (the tree takes a square root).  Also the padding for K > N."""
    from scipy import spatial
    rs = np.random.RandomState(11)
    pts = rs.uniform(size=(3000, 3)).astype(np.float32)
    q = np.concatenate([pts[::7], rs.uniform(-0.5, 1.5, size=(100, 3)).astype(np.float32)])
    idx, d2, count = kx.search(pts, q, 33)
    assert (np.diff(d2, axis=1) > 0).all() and (count == 33).all()          # tie-free, ascending
    dist, want = spatial.cKDTree(pts.astype(np.float64)).query(q.astype(np.float64), k=33)
    assert np.array_equal(idx, want.astype(np.int32))
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-14, atol=0)
    assert np.array_equal(idx[:len(pts[::7]), 0], np.arange(0, 3000, 7))    # a cloud point is its own first neighbour
    idx, d2, count = kx.search(pts[:5], np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32), 8)
    assert count.tolist() == [5, 0, 0] and (idx[0, 5:] == -1).all() and np.isinf(d2[0, 5:]).all() and (idx[1:] == -1).all()
    ties = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0], [-1, 0, 0]], np.float32)
    assert kx.search(ties, np.zeros((1, 3), np.float32), 5)[0].tolist() == [[2, 3, 0, 1, 4]]      # ties by index


@pytest.mark.parametrize("name", ["lattice_shifted", "needle_diag", "offset", "duplicates"])
def test_stop_rule_with_its_margin(name):
    """``emulate_walk`` -- the kernel's shell walk, strict stop rule and margin in its own fp64 operations -- returns the brute force's
    indices and d2 bits at K = 1 and K = 128 over three grids: the case's radius grid, the default k-NN grid and one cell.  Ties at the
    K-th distance (lattice, duplicates), coordinates near 2 000 (offset), answers across empty cells and positions outside the
    bounding box (needle_diag), and a position 10^6 away, which stops only when the block covers the grid."""
    import _grid_fixture as gx
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import knn
    c = gx.case(name)
    pts = c["pts"]
    centres = [pts[c["rows"][::3]], np.array([[1e6, 1e6, 1e6], [np.nan, 0, 0]], np.float32)]
    if "positions" in c:
        centres.append(c["positions"])
    centres = np.concatenate(centres)
    ref = kx.search(pts, centres, 128)
    extent = pts.max(0).astype(np.float64) - pts.min(0)
    grids = {"radius": c["header"], "default": gx.header(pts, [knn.default_radius(len(pts), 128, extent)]),
             "one cell": gx.header(pts, [2.0 * c["bbdiag"]])}
    assert grids["one cell"]["dims"] == [1, 1, 1]
    for label, h in grids.items():
        for K in (1, 128):
            idx, d2, deepest = kx.emulate_walk(pts, centres, K, h)
            assert np.array_equal(idx, ref[0][:, :K]), (name, label, K)
            assert np.array_equal(d2.view(np.uint64), ref[1][:, :K].view(np.uint64)), (name, label, K)
            assert deepest == max(h["dims"]) - 1 or label == "one cell"        # the far position walked the whole grid


def _lib_and_dummy():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    dummy = np.zeros(8, np.float32)                     # never dereferenced: the checks come first
    return lib, _lib, ctypes.c_void_p(dummy.ctypes.data), dummy


def _refused(lib, rc, word):
    msg = lib.nesti_last_error() or b""
    assert rc != 0 and word.encode() in msg, (rc, msg, word)


def test_search_refusals_need_no_device():
    lib, _lib, p, _keep = _lib_and_dummy()
    N, M, K = 1000, 100, 16
    gws = lib.nesti_patches_workspace_bytes(N)

    def idx(cloud=p, n=N, q=p, m=M, row0=0, k=K, nbr=p, g=p, gb=gws):
        return lib.nesti_knn(cloud, n, q, m, row0, k, nbr, p, p, g, gb, None)

    def at(cloud=p, n=N, q=p, m=M, row0=0, k=K, nbr=p, g=p, gb=gws):
        return lib.nesti_knn_at(cloud, n, q, m, k, nbr, p, p, g, gb, None)

    for call, name in ((idx, "nesti_knn:"), (at, "nesti_knn_at:")):
        _refused(lib, call(cloud=None), "null")
        _refused(lib, call(nbr=None), "null")
        _refused(lib, call(g=None), "null")
        _refused(lib, call(n=0), "empty cloud")
        _refused(lib, call(n=-3), "empty cloud")
        _refused(lib, call(k=0), "K must be in 1 .. 256")
        _refused(lib, call(k=257), "K must be in 1 .. 256")
        _refused(lib, call(m=-1), "M must be")
        _refused(lib, call(gb=gws - 1), "workspace too small")
        assert lib.nesti_last_error().startswith(name.encode())            # under the entry's name
        assert call(m=0) == 0                                               # a no-op ...
        _refused(lib, call(m=0, k=0), "K must be")                          # ... and an argument error is still one
    _refused(lib, idx(row0=-1), "query_row0")
    _refused(lib, idx(q=None, row0=N - M + 1), "exceed the cloud")
    _refused(lib, at(q=None), "null query_xyz_dev")


@pytest.mark.parametrize("fit", ["nesti_pca_normals_nbr", "nesti_quadric_fit_nbr"])
def test_list_fit_refusals_need_no_device(fit):
    lib, _lib, p, _keep = _lib_and_dummy()
    N, M, K = 1000, 100, 64
    outs = (p,) * (4 if "pca" in fit else 5)
    good = (8, 32, 64)

    def ks_arr(ks):
        return None if ks is None else (ctypes.c_int32 * max(1, len(ks)))(*ks)

    def idx(cloud=p, n=N, q=p, m=M, row0=0, nbr=p, k=K, ks=good, s=None):
        return getattr(lib, fit)(cloud, n, q, m, row0, nbr, k, ks_arr(ks), len(ks) if s is None else s, *outs, None)

    def at(cloud=p, n=N, q=p, m=M, row0=0, nbr=p, k=K, ks=good, s=None):
        return getattr(lib, fit + "_at")(cloud, n, q, m, nbr, k, ks_arr(ks), len(ks) if s is None else s, *outs, None)

    for call, name in ((idx, fit + ":"), (at, fit + "_at:")):
        _refused(lib, call(cloud=None), "null")
        _refused(lib, call(nbr=None), "null")
        _refused(lib, call(ks=None, s=3), "null")
        _refused(lib, call(n=0), "empty cloud")
        _refused(lib, call(k=0), "K must be in 1 .. 256")
        _refused(lib, call(k=257), "K must be in 1 .. 256")
        _refused(lib, call(s=0), "n_scales")
        _refused(lib, call(ks=(1, 2, 3, 4, 5)), "n_scales")
        _refused(lib, call(ks=(0, 8)), "ks must be ascending")
        _refused(lib, call(ks=(32, 8)), "ks must be ascending")
        _refused(lib, call(ks=(8, 65)), "ks must be ascending")
        _refused(lib, call(m=-1), "M must be")
        assert lib.nesti_last_error().startswith(name.encode())
        assert call(m=0) == 0
        _refused(lib, call(m=0, ks=(9, 8)), "ks must be")
    _refused(lib, idx(row0=-1), "query_row0")
    _refused(lib, idx(q=None, row0=N - M + 1), "exceed the cloud")
    _refused(lib, at(q=None), "null query_xyz_dev")


def test_python_layer_validates_knn():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import knn, pca, quadric
    from nesti_net_amd.config import NestiConfig
    assert knn.check_ks(8) == (8,) and knn.check_ks([8, 32, 128]) == (8, 32, 128) and knn.check_ks(np.int64(256)) == (256,)
    assert knn.check_ks((5, 5)) == (5, 5)                                   # ascending, not strictly
    for bad in (0, 257, -1, [8, 4], [1, 2, 3, 4, 5], [], "a", 2.5, [8, 2.5], True, None):
        with pytest.raises(ValueError):
            knn.check_ks(bad)
    pts = np.zeros((10, 3), np.float32)
    for fn in (pca.pca_normals, quadric.quadric_fit):
        with pytest.raises(ValueError, match="ascending"):
            fn(pts, knn=[8, 4])
        with pytest.raises(ValueError, match="1 .. 256"):
            fn(pts, knn=300)
        with pytest.raises(ValueError, match="knn and cfg"):
            fn(pts, cfg=NestiConfig(), knn=8)
        with pytest.raises(ValueError, match="mutually exclusive"):
            fn(pts, knn=8, pidx=[0, 1], queries=np.zeros((2, 3), np.float32))
        with pytest.raises(ValueError, match="scale"):
            fn(pts, knn=[8, 16], scale=2)                                   # scale indexes ks
        with pytest.raises(ValueError, match="scale"):
            fn(pts, knn=8, scale=-2)
    with pytest.raises(ValueError, match="1 .. 256"):
        knn.knn(pts, 0)
    with pytest.raises(ValueError, match="mutually exclusive"):
        knn.knn(pts, 4, pidx=[0], queries=np.zeros((1, 3), np.float32))
    r = knn.default_radius(100000, 64, (2.0, 1.5, 1.0))
    assert r > 0 and np.isclose(9 * r * r * 100000 / (2 * 1.5 + 1.5 * 1 + 1 * 2), 64)          # 9 cell^2 N / A = k
    assert knn.default_radius(5000, 16, (1.0, 0.0, 0.0)) == 1e-6 and knn.default_radius(1, 1, (0.0, 0.0, 0.0)) == 1.0


@pytest.mark.parametrize("args, word", [
    (["--estimator", "net", "--knn", "8"], "--knn belongs to --estimator pca / --estimator quadric"),
    (["--knn", "8"], "--knn belongs to --estimator pca / --estimator quadric"),
    (["--estimator", "pca", "--knn", "8,4"], "ascending"),
    (["--estimator", "quadric", "--knn", "0"], "1 .. 256"),
    (["--estimator", "pca", "--knn", "1,2,3,4,5"], "1 .. 4 neighbour counts"),
    (["--estimator", "pca", "--knn", "eight"], "--knn eight"),
    (["--estimator", "pca", "--knn", "8,32", "--pca_scale", "2"], "--pca_scale"),
    (["--estimator", "pca", "--knn", "8", "--depth_images", "1"], "--estimator pca does not take --depth_images 1"),
    (["--estimator", "quadric", "--knn", "8", "--reproducible", "1"], "--estimator quadric does not take --reproducible 1"),
    (["--estimator", "pca", "--knn", "8", "--subsample", "reference"], "--estimator pca does not take --subsample reference"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code != 0 and word in (err + str(e.value.code))
    if "--pca_scale" not in word:
        assert e.value.code == 2 and not (tmp_path / "out").exists()       # refused while parsing: nothing was created
