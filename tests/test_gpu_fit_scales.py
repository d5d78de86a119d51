"""The model-free fits at every number of scales S = 1 .. 4 on the GPU.  ``pca_kernel<S>``, ``quadric_kernel<S>`` (csrc/pca.hip,
csrc/quadric.hip), ``pca_nbr_kernel<S>``, ``quadric_nbr_kernel<S>`` (csrc/knn.hip) are one program per S, chosen by ``with_scales``
(csrc/pca_dev.h), and ``hough_nbr_kernel`` (csrc/hough.hip) loops over S at run time; the other GPU tests run S = 3 and little else.
Here S = 1, 2 and 4 of each family -- radii out of order and repeated, 256 = NESTI_KNN_MAX_K neighbours, a partial last trip -- are held

  1  to the tests' numpy restatements, through the ``check`` functions of tests/test_gpu_pca.py, tests/test_gpu_quadric.py and
     tests/test_gpu_knn.py with their bounds as they are: counts integer for integer, sentinel rows and failed fits byte for byte, no
     plane fit excluded as ill-conditioned, at most 1 % of the quadric fits of a scale (tests/test_fit_scales.py pins on the CPU that the
     restatement has none); ``radius_out`` and ``plane_out`` on the bits; index queries and position queries
  2  to each other: column s of a run is byte-identical to the column of any other run ON THE SAME GRID that has the same radius,
     whatever its companions -- every scale's sums receive the same candidates in the same lane order, contraction is off and the
     butterfly is fixed.  This ties S = 1, 2, 4 to the S = 3 program the other tests trust
  3  likewise over lists: a column equals the single-scale run at its count
  4  Hough: both sets of counts on the bytes of the restatement, and column s equal to the single-scale run with ks = (ks[s],)
  5  through ``pca.pca_normals`` / ``quadric.quadric_fit`` and ``--estimator pca --patch_radius`` with one and four scales.

The inputs are those of tests/_fit_scales_fixture.py.  scripts/fit_scales_check.py records the figures these checks print."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _fit_scales_fixture as sx
import _hough_fixture as hx
from test_gpu_knn import _quadric_check as quadric_list_check
from test_gpu_pca import check as plane_check
from test_gpu_quadric import check as quadric_check

pytestmark = pytest.mark.gpu

HOUGH_KEYS = ("normals", "conf", "votes", "radius", "count")


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _col(a, s):
    return np.ascontiguousarray(a[:, s:s + 1])


_balls, _lists = {}, {}


def ball_run(key, dev):
    """{cp, pca, quadric, counts} of a ball case over index queries on ONE grid, once; pca = (normals, eig, n_ball), quadric =
    (normals, curv, plane, n_ball) as numpy."""
    if key not in _balls:
        from nesti_net_amd.provider import CloudPatches
        c = sx.scale_set(key)
        cp = CloudPatches(c["pts"], c["cfg"], device=dev, pidx=c["rows"])
        assert cp.r_abs == c["r_abs"] and cp.patch_count == len(c["rows"])
        _balls[key] = {"cp": cp, "pca": _np(cp.pca(0, cp.patch_count)), "quadric": _np(cp.quadric(0, cp.patch_count)),
                       "counts": cp.count_balls(0, cp.patch_count).cpu().numpy()}
    return _balls[key]


def list_cloud(name, dev):
    """(cloud over the rows of ``name``, their 256 nearest neighbours by nesti_knn on the device), once."""
    if name not in _lists:
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        c = sx.cloud(name)
        cp = CloudPatches(c["pts"], NestiConfig(), device=dev, pidx=c["rows"], radius_grid=False)
        idx, d2, n = cp.knn(0, cp.patch_count, 256)
        ref = sx.lists(name)
        assert np.array_equal(idx.cpu().numpy(), ref[0]) and np.array_equal(d2.cpu().numpy().view(np.uint64), ref[1].view(np.uint64))
        assert np.array_equal(n.cpu().numpy(), ref[2])
        _lists[name] = (cp, idx)
    return _lists[name]


def list_run(name, ks, dev):
    """(pca_knn, quadric_knn) outputs as numpy over the first ks[-1] columns of the device's own lists, once per (cloud, ks)."""
    if (name, ks) not in _lists:
        cp, idx = list_cloud(name, dev)
        nbr = idx[:, :ks[-1]].contiguous()
        _lists[(name, ks)] = (_np(cp.pca_knn(0, cp.patch_count, ks, nbr=nbr)), _np(cp.quadric_knn(0, cp.patch_count, ks, nbr=nbr)))
    return _lists[(name, ks)]


def _as_positions(cp, fn):
    """``fn()`` with the rows of ``cp`` given as positions of the same coordinates instead of indices: the same object, so the same grid."""
    pidx = cp.pidx
    cp.pidx, cp.queries = None, cp.cloud[pidx.long()].contiguous()
    try:
        return fn()
    finally:
        cp.pidx, cp.queries = pidx, None


# ---- 1. against the restatements -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(sx.SCALE_SETS))
def test_balls_against_the_restatement(key, gpu_device):
    """1.  ``CloudPatches.pca`` and ``.quadric`` of every scale set: S = 4 on both clouds, S = 2 with the larger radius first, S = 1,
    and S = 4 with a repeated radius out of order.  No plane fit may be excluded; ``plane_out`` is the plane fit's normals on the bits;
    the position form gives the bytes of the index form."""
    c, run = sx.scale_set(key), ball_run(key, gpu_device)
    cp, S = run["cp"], len(c["radii"])
    normals, eig, n_ball = run["pca"]
    assert normals.shape == (250, S, 3) and eig.shape == (250, S, 3) and n_ball.shape == (250, S) and n_ball.dtype == np.int32
    assert np.array_equal(n_ball, run["counts"])                                  # ... equal to nesti_patches_count's
    ref = sx.plane_balls(key)
    ill, live = plane_check(run["pca"], ref, key + " plane", allow_excluded=None)
    assert not ill.any()
    qn, qc, qp, qcount = run["quadric"]
    assert qn.shape == (250, S, 3) and qc.shape == (250, S, 2) and qp.shape == (250, S, 3) and qcount.shape == (250, S)
    assert _same_bytes(qp, normals) and _same_bytes(qcount, n_ball)               # plane_out IS nesti_pca_normals' output on this grid
    fitted = quadric_check(run["quadric"], sx.quadric_balls(key, qp), c["r_abs"], key + " quadric", ill_share_cap=0.01)
    print("%s: live plane fits per scale %s, fitted quadrics per scale %s" % (key, live.sum(0).tolist(), fitted.sum(0).tolist()))
    if c["cloud"] == "torus_clean":
        assert live.all() and fitted.all()
    if key == "ellipsoid_4":                                                      # sentinel rows, failed fits and live rows in one wave
        assert live.sum(0).tolist() == [107, 250, 250, 250] and (n_ball[:, 0] >= 6).sum() == 7
        assert fitted[:, 0].sum() >= 6 and fitted[:, 2:].all()                    # the n = 6 boundary; 7 by the restatement
    if key == "ellipsoid_4_repeated":                                             # the two equal radii: two equal columns
        for a in run["pca"] + run["quadric"]:
            assert _same_bytes(_col(a, 0), _col(a, 1))
    at = _as_positions(cp, lambda: (_np(cp.pca(0, cp.patch_count)), _np(cp.quadric(0, cp.patch_count))))
    for a, b in zip(run["pca"] + run["quadric"], at[0] + at[1]):
        assert _same_bytes(a, b)


@pytest.mark.parametrize("ks", sx.KS_SETS)
@pytest.mark.parametrize("name", sx.CLOUDS)
def test_lists_against_the_restatement(name, ks, gpu_device):
    """1.  ``pca_knn`` and ``quadric_knn`` over the device's own lists at S = 4 (256 neighbours: four full trips per lane), S = 2 (200:
    a partial last trip) and S = 1.  Every pair is live; ``radius_out`` equals the restatement's bits, ``plane_out`` and the quadric
    entry's radius and counts those of the plane entry; the position form gives the bytes of the index form."""
    cp, idx = list_cloud(name, gpu_device)
    plane, quadric = list_run(name, ks, gpu_device)
    S, M = len(ks), cp.patch_count
    normals, eig, radius, n = plane
    assert normals.shape == (M, S, 3) and eig.shape == (M, S, 3) and radius.shape == (M, S) and n.shape == (M, S)
    ref = sx.plane_lists(name, ks)
    ill, live = plane_check((normals, eig, n), ref, "%s knn %s plane" % (name, ks), allow_excluded=None)
    assert live.all() and not ill.any() and (n == np.array(ks)).all()
    assert _same_bytes(radius, ref["radius"])
    qn, qc, qp, qr, qcount = quadric
    assert qn.shape == (M, S, 3) and qc.shape == (M, S, 2)
    assert _same_bytes(qp, normals) and _same_bytes(qr, radius) and _same_bytes(qcount, n)
    fitted = quadric_list_check((qn, qc, qp, qcount), sx.quadric_lists(name, ks, qp), "%s knn %s quadric" % (name, ks),
                                cap_scales=range(S), cap=0.01)
    assert fitted.all()
    nbr = idx[:, :ks[-1]].contiguous()
    at = _as_positions(cp, lambda: (_np(cp.pca_knn(0, M, ks, nbr=nbr)), _np(cp.quadric_knn(0, M, ks, nbr=nbr))))
    for a, b in zip(plane + quadric, at[0] + at[1]):
        assert _same_bytes(a, b)
    searched = _np(cp.pca_knn(0, M, ks))                                          # the search inside the call: K = ks[-1], the same bytes
    for a, b in zip(plane, searched):
        assert _same_bytes(a, b)


# ---- 2. a scale is independent of its companions: balls --------------------------------------------------------------------------------

def lib_ball_fit(cp, cols, entry):
    """``nesti_pca_normals`` / ``nesti_quadric_fit`` (``entry``) through ctypes over the index queries and ON THE GRID WORKSPACE of the
    prepared cloud ``cp``, with the sub-configuration that holds the scales ``cols`` of ``cp``'s own: n_scales = len(cols) and the
    sub-list of r_abs.  The outputs are pre-filled, so an entry the kernel does not write shows.  -> numpy arrays."""
    from nesti_net_amd import _lib
    conf = sx.config([cp.cfg.patch_radius[i] for i in cols]).to_c()
    r = (ctypes.c_double * len(cols))(*[cp.r_abs[i] for i in cols])
    M, S, dev = cp.patch_count, len(cols), cp.device
    widths = {"nesti_pca_normals": (3, 3), "nesti_quadric_fit": (3, 2, 3)}[entry]
    out = [torch.full((M, S, w), 7.0, device=dev) for w in widths] + [torch.full((M, S), 7, dtype=torch.int32, device=dev)]
    with torch.cuda.device(dev):
        _lib.check(getattr(cp.lib, entry)(ctypes.byref(conf), _lib.ptr(cp.cloud), cp.n_points, _lib.ptr(cp.pidx), M, r, 0,
                                          *[_lib.ptr(t) for t in out], _lib.ptr(cp._ws), cp._ws.numel(),
                                          _lib.stream_ptr(torch.cuda.current_stream(dev))), entry)
    return _np(out)


@pytest.mark.parametrize("name", sx.CLOUDS)
def test_a_ball_scale_does_not_depend_on_its_companions(name, gpu_device):
    """2.  ONE grid, built for the four radii.  Every single radius (S = 1), the pairs (0, 2) and (3, 1) (S = 2, one out of order) and
    the triple (0, 1, 2) (S = 3) run on that grid as a configuration of their own: column s of every run is byte-identical to the
    column of the S = 4 run with the same radius -- normals, eigenvalues, curvatures, plane normals and counts."""
    run = ball_run(sx.FULL_SET[name], gpu_device)
    cp = run["cp"]
    for entry, whole in (("nesti_pca_normals", run["pca"]), ("nesti_quadric_fit", run["quadric"])):
        for a, b in zip(whole, lib_ball_fit(cp, (0, 1, 2, 3), entry)):           # the helper itself: the S = 4 run again
            assert _same_bytes(a, b), entry
        for cols in sx.SUB_CONFIGS:
            got = lib_ball_fit(cp, cols, entry)
            for s, full_s in enumerate(cols):
                for k, (a, b) in enumerate(zip(whole, got)):
                    assert b.shape[1] == len(cols)
                    assert _same_bytes(_col(a, full_s), _col(b, s)), "%s: output %d, column %d of the run over scales %s differs " \
                        "from column %d of the four-scale run" % (entry, k, s, cols, full_s)
    # the columns are not all alike: the comparison above could otherwise not tell them apart
    assert len({run["pca"][0][:, s].tobytes() for s in range(4)}) == 4 and len({run["quadric"][1][:, s].tobytes() for s in range(4)}) == 4


# ---- 3. ... and lists ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sx.CLOUDS)
def test_a_list_scale_does_not_depend_on_its_companions(name, gpu_device):
    """3.  The prefix property of tests/test_gpu_knn.py at every column: each column of the ks = (8, 16, 64, 256) run equals, byte for
    byte, the single-scale run at that count (which searches for itself, at K = k), for the plane fit and the quadric fit; column 0 of
    (16, 200) equals column 1 of the four-scale run and its column 1 the single-scale run at 200, and (24,) over the 256-wide list
    equals (24,) over its own search."""
    cp, idx = list_cloud(name, gpu_device)
    M = cp.patch_count
    ks4, ks2, ks1 = sx.KS_SETS
    plane4, quadric4 = list_run(name, ks4, gpu_device)
    for s, k in enumerate(ks4):
        for whole, single in ((plane4, _np(cp.pca_knn(0, M, (k,)))), (quadric4, _np(cp.quadric_knn(0, M, (k,))))):
            for a, b in zip(whole, single):
                assert b.shape[1] == 1 and _same_bytes(_col(a, s), b), (name, k)
    plane2, quadric2 = list_run(name, ks2, gpu_device)
    assert ks2[0] == ks4[1]
    for a, b in zip(plane4 + quadric4, plane2 + quadric2):
        assert _same_bytes(_col(a, 1), _col(b, 0)), name
    for whole, single in ((plane2, _np(cp.pca_knn(0, M, ks2[1:]))), (quadric2, _np(cp.quadric_knn(0, M, ks2[1:])))):
        for a, b in zip(whole, single):                                           # ... and its column 1 the single-scale run at 200
            assert _same_bytes(_col(a, 1), b), name
    plane1, quadric1 = list_run(name, ks1, gpu_device)
    wide = idx.contiguous()                                                       # K = 256 columns, ks = (24,): the row stride is K, not k
    for a, b in zip(plane1 + quadric1, _np(cp.pca_knn(0, M, ks1, nbr=wide)) + _np(cp.quadric_knn(0, M, ks1, nbr=wide))):
        assert _same_bytes(a, b), name
    assert len({plane4[0][:, s].tobytes() for s in range(4)}) == 4


# ---- 4. Hough ------------------------------------------------------------------------------------------------------------------------

_hough = {}


def _box(dev):
    if "box" not in _hough:
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        pts = sx.box()
        cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
        nbr = cp.knn(0, len(pts), sx.HOUGH_K)[0]
        _hough["box"] = (pts, cp, nbr, nbr.cpu().numpy())
    return _hough["box"]


@pytest.mark.parametrize("T", sx.HOUGH_T)
@pytest.mark.parametrize("ks", sx.HOUGH_KS_SETS)
def test_hough_scales(ks, T, gpu_device):
    """4.  Four and two scales of ``hough_nbr_kernel`` on the 300-point box: every output equals the restatement on the bytes, and column
    s equals the single-scale run with ks = (ks[s],) -- the hash is keyed with scale 0 (the header of csrc/hough.hip)."""
    from nesti_net_amd import hough
    pts, cp, nbr, nbr_h = _box(gpu_device)
    B, R, seed = sx.HOUGH_B, sx.HOUGH_R, sx.HOUGH_SEED
    M = len(pts)
    got = _np(cp.hough_knn(0, M, ks, T, B, R, seed, nbr=nbr))
    ref = hx.restate(pts, pts, nbr_h, ks, T, B, R, hough.rotation_table(R), seed)
    for key, g in zip(HOUGH_KEYS, got):
        assert _same_bytes(g, ref[key]), (ks, T, key, np.flatnonzero((g != ref[key]).reshape(M, -1).any(1))[:8])
    assert (got[4] == np.array(ks)).all() and np.isfinite(got[0]).all() and (got[2][:, -1, 0] > 0).all()
    for s, k in enumerate(ks):
        single = _np(cp.hough_knn(0, M, (k,), T, B, R, seed, nbr=nbr))
        for key, a, b in zip(HOUGH_KEYS, got, single):
            assert b.shape[1] == 1 and _same_bytes(_col(a, s), b), (ks, T, key, k)
    assert len({got[0][:, s].tobytes() for s in range(len(ks))}) == len(ks)


# ---- 5. the Python layer and the command line -------------------------------------------------------------------------------------------

def _check_scale_argument(fit, pts, rows, S, dev, keys, **kw):
    """``scale`` of a k-NN fit with S scales: -1 is the last column, 0 and S - 1 the named ones, S and -S - 1 are refused.  (A k-NN fit
    does not depend on the grid build, so two calls give the same bytes.)"""
    last = fit(pts, pidx=rows, device=dev, **kw)
    for key, width in keys:
        assert last[key + "_all"].shape == (len(rows), S, width) and last[key].shape == (len(rows), width), key
        assert _same_bytes(last[key], np.ascontiguousarray(last[key + "_all"][:, -1])), key
    assert last["n_ball"].shape == (len(rows), S)
    for scale in (0, S - 1, -S):
        res = fit(pts, pidx=rows, scale=scale, device=dev, **kw)
        for key, _ in keys:
            assert _same_bytes(res[key + "_all"], last[key + "_all"]), key
            assert _same_bytes(res[key], np.ascontiguousarray(res[key + "_all"][:, scale])), (key, scale)
    for bad in (S, -S - 1):
        with pytest.raises(ValueError, match=r"scale must be in \[-%d, %d\)" % (S, S)):
            fit(pts, pidx=rows, scale=bad, device=dev, **kw)
    return last


def test_python_layer_with_one_and_four_scales(gpu_device):
    """5.  ``pca.pca_normals`` and ``quadric.quadric_fit`` with a one-scale and a four-scale configuration and with ``knn=`` of one and
    four counts: shapes [M, S, ...], ``scale`` picks the named column, an out-of-range ``scale`` is refused with a message, ``variation``
    has the shape of ``n_ball``; the values are the restatement's to the bounds (counts and sentinels exactly)."""
    from nesti_net_amd import pca, quadric
    dev = str(gpu_device)
    c = sx.scale_set("ellipsoid_4")
    pts, rows = c["pts"], c["rows"]
    for key, S in (("ellipsoid_4", 4), ("torus_1", 1)):
        c = sx.scale_set(key)
        # res[...]_all of two calls come from two grid builds: equal to the bounds only, so each call is compared with itself
        res = pca.pca_normals(c["pts"], c["cfg"], pidx=c["rows"], device=dev)
        assert res["normals_all"].shape == (250, S, 3) and res["eig"].shape == (250, S, 3) and res["normals"].shape == (250, 3)
        assert res["variation"].shape == res["n_ball"].shape == (250, S)
        assert _same_bytes(res["normals"], np.ascontiguousarray(res["normals_all"][:, -1]))
        plane_check((res["normals_all"], res["eig"], res["n_ball"]), sx.plane_balls(key), key + " pca_normals", allow_excluded=None)
        for scale in (0, S - 1, -S):
            one = pca.pca_normals(c["pts"], c["cfg"], pidx=c["rows"], scale=scale, device=dev)
            assert _same_bytes(one["normals"], np.ascontiguousarray(one["normals_all"][:, scale])) and np.array_equal(one["n_ball"], res["n_ball"])
        q = quadric.quadric_fit(c["pts"], c["cfg"], pidx=c["rows"], scale=0, device=dev)
        assert q["normals_all"].shape == (250, S, 3) and q["curv_all"].shape == (250, S, 2) and q["plane_all"].shape == (250, S, 3)
        assert q["curv"].shape == (250, 2) and q["n_ball"].shape == (250, S)
        assert _same_bytes(q["normals"], np.ascontiguousarray(q["normals_all"][:, 0])) and _same_bytes(q["curv"], np.ascontiguousarray(q["curv_all"][:, 0]))
        quadric_check((q["normals_all"], q["curv_all"], q["plane_all"], q["n_ball"]), sx.quadric_balls(key, q["plane_all"]), c["r_abs"],
                      key + " quadric_fit", ill_share_cap=0.01)
        for fit in (pca.pca_normals, quadric.quadric_fit):
            for bad in (S, -S - 1):
                with pytest.raises(ValueError, match=r"scale must be in \[-%d, %d\)" % (S, S)):
                    fit(c["pts"], c["cfg"], pidx=c["rows"], scale=bad, device=dev)
    for ks in (sx.KS_SETS[0], sx.KS_SETS[2]):
        S = len(ks)
        plane, quad = list_run("ellipsoid", ks, gpu_device)
        res = _check_scale_argument(pca.pca_normals, pts, rows, S, dev, (("normals", 3),), knn=ks)
        assert res["eig"].shape == (250, S, 3) and res["radius"].shape == res["variation"].shape == res["n_ball"].shape == (250, S)
        for a, k in zip(plane, ("normals_all", "eig", "radius", "n_ball")):          # the k-NN fits do not depend on the grid build
            assert _same_bytes(a, res[k]), k
        res = _check_scale_argument(quadric.quadric_fit, pts, rows, S, dev, (("normals", 3), ("curv", 2)), knn=ks)
        for a, k in zip(quad, ("normals_all", "curv_all", "plane_all", "radius", "n_ball")):
            assert _same_bytes(a, res[k]), k


def test_command_line_with_four_radii_and_with_one(tmp_path, gpu_device):
    """5.  ``--estimator pca --patch_radius 0.01 0.03 0.05 0.08 --pca_scale 1`` on one small shape: .pca_eig has 3 S = 12 columns and
    .pca_count 4; ``--estimator quadric --patch_radius 0.05``: .quadric_curv has 2 columns.  The files equal what the Python call
    returns, written through the same writers.  (The command and the call build two grids, as in tests/test_gpu_pca.py.)"""
    from nesti_net_amd import pca, quadric, textio
    from nesti_net_amd.cli import main
    c = sx.scale_set("ellipsoid_4")
    pidx = c["rows"]
    d = tmp_path / "data"
    d.mkdir()
    np.savetxt(d / "ell.xyz", c["pts"].astype(np.float64))
    np.savetxt(d / "ell.pidx", pidx, fmt="%d")
    (d / "testset.txt").write_text("ell\n")
    common = ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt", "--sparse_patches", "1"]
    pts32 = np.loadtxt(d / "ell.xyz").astype("float32")
    want = str(tmp_path / "want")

    results = str(tmp_path / "res")
    assert main(["--estimator", "pca", "--patch_radius"] + [repr(r) for r in sx.A4] + ["--pca_scale", "1", "--results_path", results]
                + common) == 0
    out = os.path.join(results, "synth_results")
    exts = (".normals", ".pca_eig", ".pca_count")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["ell" + e for e in exts])
    res = pca.pca_normals(pts32, c["cfg"], pidx=pidx, scale=1, device=str(gpu_device))
    textio.write_f32(want + ".normals", res["normals"])
    textio.write_f32(want + ".pca_eig", res["eig"].reshape(len(pidx), -1))
    textio.write_i32_rows(want + ".pca_count", res["n_ball"])
    for e in exts:
        assert open(os.path.join(out, "ell" + e), "rb").read() == open(want + e, "rb").read(), e
    assert np.loadtxt(os.path.join(out, "ell.pca_eig")).shape == (len(pidx), 12)
    assert np.array_equal(np.loadtxt(os.path.join(out, "ell.pca_count"), dtype=np.int64), sx.plane_balls("ellipsoid_4")["n_ball"])
    assert np.loadtxt(os.path.join(out, "ell.normals")).shape == (len(pidx), 3)
    assert "(scale 1 of 4)" in open(os.path.join(out, "log.txt")).read()

    results = str(tmp_path / "resq")
    assert main(["--estimator", "quadric", "--patch_radius", "0.05", "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    exts = (".normals", ".curv", ".quadric_curv", ".quadric_count")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["ell" + e for e in exts])
    res = quadric.quadric_fit(pts32, sx.config([0.05]), pidx=pidx, device=str(gpu_device))
    textio.write_f32(want + ".normals", res["normals"])
    textio.write_f32(want + ".curv", res["curv"])
    textio.write_f32(want + ".quadric_curv", res["curv_all"].reshape(len(pidx), -1))
    textio.write_i32_rows(want + ".quadric_count", res["n_ball"])
    for e in exts:
        assert open(os.path.join(out, "ell" + e), "rb").read() == open(want + e, "rb").read(), e
    assert np.loadtxt(os.path.join(out, "ell.quadric_curv")).shape == (len(pidx), 2)
    assert np.array_equal(np.loadtxt(os.path.join(out, "ell.quadric_count"), dtype=np.int64).reshape(-1, 1),
                          sx.plane_balls("ellipsoid_4")["n_ball"][:, 2:3])
    assert "(scale 0 of 1)" in open(os.path.join(out, "log.txt")).read()
