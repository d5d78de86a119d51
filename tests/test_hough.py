"""Hough-transform normals without a GPU: every refusal of the two C entries through ctypes (each returns before any device call), the
properties of the tests' restatement (tests/_hough_fixture.py), its accuracy at the creases of a box against the plane fit, the
committed rotation table, and the ``--estimator hough`` parser errors."""
import ctypes

import numpy as np
import pytest

import _hough_fixture as hx
import _knn_fixture as kx


def _rot(R=8):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough
    return hough.rotation_table(R)


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------

def _refused(lib, rc, word):
    msg = lib.nesti_last_error() or b""
    assert rc != 0 and word.encode() in msg, (rc, msg, word)


@pytest.mark.parametrize("entry", ["nesti_hough_normals_nbr", "nesti_hough_normals_nbr_at"])
def test_refusals_need_no_device(entry):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    dummy = np.zeros(8, np.float32)                     # never dereferenced: the checks come first
    p = ctypes.c_void_p(dummy.ctypes.data)
    N, M, K = 1000, 100, 64
    good = (8, 32, 64)
    table = _rot(8)

    def call(cloud=p, n=N, q=p, m=M, row0=0, nbr=p, k=K, ks=good, s=None, T=100, B=16, R=5, rot=table, seed=7):
        ks_arr = None if ks is None else (ctypes.c_int32 * max(1, len(ks)))(*ks)
        rp = None if rot is None else np.ascontiguousarray(rot, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return getattr(lib, entry)(cloud, n, q, m, row0, nbr, k, ks_arr, len(ks) if s is None else s, T, B, R, rp, seed, p, p, p, p, p,
                                   None)

    # the errors of nesti_pca_normals_nbr
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
    _refused(lib, call(row0=-1), "query_row0")                             # both entries: the key row
    # the estimator's own
    for T in (0, -1, 4097):
        _refused(lib, call(T=T), "T (triplets) must be in 1 .. 4096")
    for B in (1, 0, 17):
        _refused(lib, call(B=B), "B (bins per axis) must be in 2 .. 16")
    for R in (0, 9):
        _refused(lib, call(R=R), "R (rotations) must be in 1 .. 8")
    _refused(lib, call(rot=None), "null rot")
    for bad in (np.nan, np.inf):
        t = table.copy()
        t[2, 4] = bad
        _refused(lib, call(rot=t), "rotation 2 is not finite")
    t = table.copy()
    t[1, 0] += 1e-5
    _refused(lib, call(rot=t), "rotation 1 is not orthonormal")
    t = table.copy()
    t[4] *= 2.0
    _refused(lib, call(rot=t), "rotation 4 is not orthonormal")
    assert lib.nesti_last_error().startswith((entry + ":").encode())       # under the entry's name
    t = table.copy()
    t[6] = np.nan
    assert call(R=5, rot=t, m=0) == 0                                      # rotations beyond R are not read; M = 0 is a no-op ...
    _refused(lib, call(m=0, T=0), "T (triplets)")                          # ... and an argument error is still one
    _refused(lib, call(m=0, rot=None), "null rot")
    if entry.endswith("_at"):
        _refused(lib, call(q=None), "null query_xyz_dev")
    else:
        _refused(lib, call(q=None, row0=N - M + 1), "exceed the cloud")


def test_python_layer_validates():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough
    from nesti_net_amd.config import NestiConfig
    pts = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="no ball variant"):
        hough.hough_normals(pts, knn=None)
    with pytest.raises(ValueError, match="knn and cfg"):
        hough.hough_normals(pts, knn=8, cfg=NestiConfig())
    for kw, word in (({"triplets": 0}, "triplets"), ({"triplets": 4097}, "triplets"), ({"bins": 1}, "bins"), ({"bins": 17}, "bins"),
                     ({"rotations": 0}, "rotations"), ({"rotations": 9}, "rotations"), ({"seed": -1}, "seed"), ({"bins": 2.5}, "bins"),
                     ({"knn": [8, 4]}, "ascending"), ({"knn": 300}, "1 .. 256"), ({"knn": [8, 16], "scale": 2}, "scale")):
        with pytest.raises(ValueError, match=word):
            hough.hough_normals(pts, **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        hough.hough_normals(pts, knn=8, pidx=[0, 1], queries=np.zeros((2, 3), np.float32))


# ---- 2. fixture properties -------------------------------------------------------------------------------------------------------------

def test_triplet_indices_are_distinct_and_in_range():
    ns = np.arange(3, 301)
    i0, i1, i2 = hx.triplet_indices(12345, np.arange(len(ns)) + 17, ns, 200)
    for i in (i0, i1, i2):
        assert (i >= 0).all() and (i < ns[:, None]).all()
    assert (i0 != i1).all() and (i0 != i2).all() and (i1 != i2).all()
    # every slot of a small neighbourhood is drawn in every position: the skips do not starve an index
    for i in (i0, i1, i2):
        assert set(np.unique(i[2])) == set(range(5))
    # the hash is the documented splitmix64 finaliser: one value worked out by hand in Python integers
    z = (99 ^ (5 << 34) ^ 7) & (2 ** 64 - 1)
    z = (z + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    assert int(hx.subsample_hash(99, 5, 0, 7)) == (z ^ (z >> 31)) >> 32


def _box(n=300, seed=3):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    return synth.make_cloud("box", n=n, seed=seed)


def test_a_scale_equals_its_single_scale_run():
    pts, _ = _box()
    nbr = kx.search(pts, pts, 40)[0]
    ks = (3, 17, 40)
    rot = _rot(3)
    every = hx.restate(pts, pts, nbr, ks, 65, 16, 3, rot, 5, row0=11)
    for s, k in enumerate(ks):
        one = hx.restate(pts, pts, nbr, (k,), 65, 16, 3, rot, 5, row0=11)
        for key in every:
            assert np.array_equal(every[key][:, s:s + 1].view(np.uint8), one[key].view(np.uint8)), (key, k)
    # ... and a row's result follows its key row, not its position in the call
    part = hx.restate(pts, pts[100:120], nbr[100:120], ks, 65, 16, 3, rot, 5, row0=111)
    for key in every:
        assert np.array_equal(every[key][100:120].view(np.uint8), part[key].view(np.uint8)), key
    assert not np.isnan(every["normals"]).any() and (every["votes"][..., 0] <= every["votes"][..., 1]).all()


def lattice(side=9):
    g = np.arange(side, dtype=np.float32) * np.float32(0.125)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(side * side, np.float32)], 1)


def test_planar_lattice_is_exact():
    pts = lattice()
    nbr = kx.search(pts, pts, 25)[0]
    res = hx.restate(pts, pts, nbr, (9, 25), 200, 16, 5, _rot(5), 0)
    assert np.array_equal(res["normals"].view(np.uint32), np.broadcast_to(np.array([0, 0, 1], np.float32), res["normals"].shape).view(np.uint32))
    assert (res["conf"] == 1.0).all() and (res["votes"][..., 0] == res["votes"][..., 1]).all()
    assert (res["votes"][..., 1] > 0).all() and (res["votes"][..., 1] < 200).all()      # collinear triplets of the lattice are not valid
    # sentinels: fewer than 3 neighbours, coincident neighbours, neighbours on a line
    line = np.stack([np.arange(10, dtype=np.float32), np.zeros(10, np.float32), np.zeros(10, np.float32)], 1)
    same = np.ones((10, 3), np.float32)
    for cloud, k in ((pts, 2), (same, 10), (line, 10)):
        r = hx.restate(cloud, cloud, kx.search(cloud, cloud, k)[0], (k,), 64, 8, 2, _rot(2), 1)
        assert not r["normals"].any() and not r["conf"].any() and not r["votes"].any() and (r["count"] == k).all()


# ---- 3. accuracy, on the fixture alone -------------------------------------------------------------------------------------------------

def test_accuracy_at_the_creases_of_a_box():
    """box, n = 2000, seed 3, the 64 nearest neighbours, T = 512, B = 16, R = 5.  NEAR rows: closer to a box edge (the second-smallest
    of 1 - |coord|) than their neighbourhood radius.  The Hough share within 10 degrees of the analytic normal must be at least twice
    the plane fit's on the same rows; every other row is exact: a signed unit axis vector (one face only: the cross products are
    exact) with conf == 1.

    Measured with this restatement: 1 453 near rows of 2 000; share within 10 degrees: Hough 0.9360, plane fit 0.2953 (ratio 3.2)."""
    pts, nrm = _box(2000, 3)
    nbr, d2, _ = kx.search(pts, pts, 64)
    res = hx.restate(pts, pts, nbr, (64,), 512, 16, 5, _rot(5), 0)
    plane = kx.plane_lists(pts, pts, nbr, (64,))
    radius = np.sqrt(d2[:, -1])
    edge = np.sort(1.0 - np.abs(pts.astype(np.float64)), axis=1)[:, 1]
    near = edge < radius
    assert np.array_equal(res["radius"][:, 0], radius.astype(np.float32))
    cos10 = np.cos(np.deg2rad(10.0))

    def share(normals):
        return float((np.abs((normals[near].astype(np.float64) * nrm[near]).sum(1)) >= cos10).mean())

    hough_share, plane_share = share(res["normals"][:, 0]), share(plane["normals"][:, 0])
    print("near rows %d of %d; within 10 degrees: hough %.4f, plane fit %.4f" % (near.sum(), len(pts), hough_share, plane_share))
    assert near.sum() > 1000 and (~near).sum() > 100
    assert hough_share >= 2.0 * plane_share
    flat = res["normals"][~near, 0]
    assert np.array_equal(flat, np.abs(nrm[~near]))                        # exactly the face's axis, signed by the library's rule
    assert (res["conf"][~near, 0] == 1.0).all() and (res["votes"][~near, 0, 1] > 0).all()


# ---- 4. the rotation table ---------------------------------------------------------------------------------------------------------------

def test_rotation_literals_are_orthonormal():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough
    R = np.array(hough.ROTATIONS, np.float64)
    assert R.shape == (8, 3, 3) and np.array_equal(R[0], np.eye(3))
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    assert hough.rotation_table(5).shape == (5, 9) and np.array_equal(hough.rotation_table(8).reshape(8, 3, 3), R)
    assert len({r.tobytes() for r in R}) == 8


# ---- 5. the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, word", [
    (["--estimator", "hough"], "--estimator hough needs --knn"),
    (["--estimator", "hough", "--knn", "8,4"], "ascending"),
    (["--estimator", "hough", "--knn", "64", "--depth_images", "1"], "--estimator hough does not take --depth_images 1"),
    (["--estimator", "hough", "--knn", "64", "--reproducible", "1"], "--estimator hough does not take --reproducible 1"),
    (["--estimator", "hough", "--knn", "64", "--subsample", "reference"], "--estimator hough does not take --subsample reference"),
    (["--estimator", "hough", "--knn", "64", "--hough_triplets", "0"], "triplets must be an integer in 1 .. 4096"),
    (["--estimator", "hough", "--knn", "64", "--hough_bins", "17"], "bins must be an integer in 2 .. 16"),
    (["--estimator", "hough", "--knn", "64", "--hough_rotations", "9"], "rotations must be an integer in 1 .. 8"),
    (["--estimator", "pca", "--hough_scale", "0"], "--hough_scale belongs to --estimator hough"),
    (["--estimator", "pca", "--knn", "8", "--hough_triplets", "10"], "--hough_triplets belongs to --estimator hough"),
    (["--estimator", "hough", "--knn", "64", "--pca_scale", "0"], "--pca_scale belongs to --estimator pca"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and not (tmp_path / "out").exists()       # refused while parsing: nothing was created
