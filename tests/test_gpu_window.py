"""Image-window neighbour lists on real kernels (csrc/window.hip, nesti_net_amd/depth.py: window_knn, depth_normals, --depth_window)
against the tests' own numpy restatement (tests/_window_fixture.py) -- lists, distances, counts and proof flags bit for bit --, the
exact mode against the grid search, and the model-free estimators on depth frames against the same estimators on the back-projected
cloud, bit for bit.

Bit equality is the expectation, not a hope: every step of the definition is one IEEE-rounded float64 operation in a fixed order
(contraction is off in the unit)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _depth_fixture as D
import _window_fixture as WF

pytestmark = pytest.mark.gpu

CROP = (24, 72, 32, 96)               # 48 x 64 of the fixture: the sphere's rim, the plane, the empty rows


def _np(t):
    return t.cpu().numpy()


def _camera(d):
    from nesti_net_amd.depth import Camera
    return Camera(**d)


def _same(got, want, what):
    idx, d2, n, proven = (_np(t) for t in got)
    assert np.array_equal(idx, want[0]), what
    assert np.array_equal(d2.view(np.uint64), want[1].view(np.uint64)), what
    assert np.array_equal(n, want[2]), what
    assert np.array_equal(proven, want[3]), what


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check(depth, cam, R, K, gpu_device, what, min_rows=1):
    """The window search of every row of ``depth`` through the dict ``cam`` against the restatement -> the restatement's tuple."""
    from nesti_net_amd.depth import depth_to_cloud, window_knn
    b = D.back_project(depth, cam)
    assert b["n_valid"] >= min_rows, what
    dc = depth_to_cloud(depth, _camera(cam), device=gpu_device)
    assert dc.n_valid == b["n_valid"]
    H, W = depth.shape
    want = WF.window_knn(b["xyz"], b["pix"], b["rank"], H, W, cam, R, K)
    _same(window_knn(dc, K, R, exact=False), want, what)
    return want


@pytest.mark.parametrize("kind", ("u16", "f32"))
def test_bits_on_the_fixture(gpu_device, kind):
    """The 96 x 128 fixture (u16 without a pose, f32 with rigid_pose(5)) at the five (R, K) pairs: all rows, and rows = dc.qidx at
    stride 3.  idx, d2, n and proven equal the restatement bit for bit.  The f32 frame has 11 537 rows and the strided ones are no
    multiple of 4 either, so the last workgroup is partial; R <= 7 and R > 7 take the two LDS sizes (see the small shapes for R = 15)."""
    from nesti_net_amd.depth import depth_to_cloud, window_knn
    depth, cam, b = WF.frame(kind)
    dc = depth_to_cloud(depth, _camera(cam), stride=3, device=gpu_device)
    assert dc.n_valid == b["n_valid"] and np.array_equal(_np(dc.xyz).view(np.uint32), b["xyz"].view(np.uint32))
    assert dc.n_queries % 4 != 0
    for R, K in WF.PAIRS:
        _same(window_knn(dc, K, R, exact=False), WF.restated(kind, R, K), (kind, R, K, "all rows"))
        _same(window_knn(dc, K, R, exact=False, rows=dc.qidx), WF.restated(kind, R, K, stride=3), (kind, R, K, "stride 3"))


@pytest.mark.parametrize("kind", ("u16", "f32"))
def test_exact_mode_equals_the_grid_search(gpu_device, kind):
    """exact=True at (3, 16) and (7, 100): idx and d2 equal knn.knn over the cloud on EVERY row, bit for bit; proven comes back as the
    window gave it, so the rows re-searched are the restatement's unproven rows -- some, and not all."""
    from nesti_net_amd import knn as _knn
    from nesti_net_amd.depth import depth_to_cloud, window_knn
    depth, cam, b = WF.frame(kind)
    dc = depth_to_cloud(depth, _camera(cam), stride=3, device=gpu_device)
    for R, K in ((3, 16), (7, 100)):
        ref = _knn.knn(b["xyz"], K)
        want_proven = WF.restated(kind, R, K)[3]
        idx, d2, n, proven = (_np(t) for t in window_knn(dc, K, R, exact=True))
        assert np.array_equal(proven, want_proven) and 0 < int((proven == 0).sum()) < len(proven)
        assert np.array_equal(idx, ref["idx"]) and np.array_equal(d2.view(np.uint64), ref["d2"].view(np.uint64))
        assert np.array_equal(n, ref["count"])
        q = _np(dc.qidx)
        idx, d2, n, proven = (_np(t) for t in window_knn(dc, K, R, exact=True, rows=dc.qidx))
        assert np.array_equal(proven, want_proven[q]) and (proven == 0).any()
        assert np.array_equal(idx, ref["idx"][q]) and np.array_equal(d2.view(np.uint64), ref["d2"][q].view(np.uint64))


def test_small_shapes(gpu_device):
    """The shapes at which the kernel can go wrong, each against the restatement."""
    cam1 = dict(D.camera("f32"), cx=0.0, cy=0.0)
    for K in (1, 4):
        idx, d2, n, proven = _check(np.array([[2.5]], np.float32), cam1, 1, K, gpu_device, "1 x 1")
        assert idx[0, 0] == 0 and n[0] == 1 and proven[0] == 1                         # the window covers the image
    # 5 x 7 with R = 15: the window is wider than the image -- every row proven, count < K, the padding
    depth, cam, b = WF.frame("u16", crop=(10, 15, 50, 57))
    idx, d2, n, proven = _check(depth, cam, 15, 64, gpu_device, "5 x 7, R 15", min_rows=30)
    assert proven.all() and (n == b["n_valid"]).all() and b["n_valid"] < 64 and (idx[:, -1] == -1).all() and np.isinf(d2[:, -1]).all()
    # R = 15, K = 256 on 40 x 40: 961 candidates in the middle, 16 trips per lane, the widest sort; holes and empty rows inside
    for kind in ("u16", "f32"):
        depth, cam, b = WF.frame(kind, crop=(20, 60, 40, 80))
        idx, d2, n, proven = _check(depth, cam, 15, 256, gpu_device, "40 x 40, R 15, K 256", min_rows=1000)
        assert (n == 256).mean() > 0.99 and (n < 256).any() and 0 < proven.sum() < len(proven)    # a corner behind a hole holds fewer
    # R = 1, K = 9: count equals the candidates -- 9 in the interior, fewer at holes and borders; K = 1: the row itself
    depth, cam, b = WF.frame("f32", crop=CROP)
    idx, d2, n, proven = _check(depth, cam, 1, 9, gpu_device, "R 1, K 9", min_rows=2000)
    assert (n == 9).any() and (n < 9).any() and n.min() >= 1
    idx, d2, n, proven = _check(depth, cam, 1, 1, gpu_device, "K 1")
    assert np.array_equal(idx[:, 0], np.arange(b["n_valid"])) and (d2 == 0).all() and (n == 1).all()
    # a 24 x 32 constant-depth frame whose coordinates are exact in float32: d2 ties in every row, ordered by index
    flat = np.full((24, 32), 2000, np.uint16)
    camf = {"fx": 128.0, "fy": 128.0, "cx": 15.5, "cy": 11.5, "depth_scale": 2.0 ** -10, "z_near": 0.0, "z_far": np.inf, "pose": None}
    for R, K in ((2, 9), (3, 25)):
        idx, d2, n, proven = _check(flat, camf, R, K, gpu_device, "constant depth")
        assert (d2[:, 1] == d2[:, 2]).all() and (idx[:, 1] < idx[:, 2]).all()       # the two nearest pixels tie in every row
    # a frame whose windows are mostly holes
    rs = np.random.RandomState(7)
    z = np.where(rs.uniform(size=(32, 32)) < 0.15, rs.uniform(1.0, 3.0, size=(32, 32)), 0.0).astype(np.float32)
    cams = dict(D.camera("f32", pose=D.rigid_pose(9)), cx=15.5, cy=15.5)
    idx, d2, n, proven = _check(z, cams, 4, 16, gpu_device, "mostly holes", min_rows=100)
    assert (n < 16).any() and (n == 16).any()


def test_untrusted_rank_and_pix(gpu_device):
    """rank entries set to N, N + 5, -7 and INT32_MIN, pix entries to -1 and H W, through the C entry with the outputs inside larger
    tensors: the results equal the restatement (those candidates are ignored, those rows have count 0) and the words round the outputs
    are untouched."""
    from nesti_net_amd import _lib
    lib = _lib.load()
    depth, cam, b = WF.frame("f32", crop=CROP)
    H, W = depth.shape
    N = b["n_valid"]
    rank, pix = b["rank"].copy(), b["pix"].copy()
    hit = np.flatnonzero(rank >= 0)
    for at, v in zip(hit[[100, 500, 901, 1500]], (N, N + 5, -7, -2 ** 31)):
        rank[at] = v
    pix[[10, 700]] = -1, H * W
    for R, K in ((3, 16), (9, 64)):
        want = WF.window_knn(b["xyz"], pix, rank, H, W, cam, R, K)
        assert (want[2][[10, 700]] == 0).all() and (want[3][[10, 700]] == 0).all()
        dev = gpu_device
        xyz_d, pix_d, rank_d = (torch.from_numpy(a).to(dev) for a in (b["xyz"], pix.astype(np.int32), rank.astype(np.int32)))
        G = 256                                                                     # guard words on both sides
        bufs = {"idx": torch.full((N * K + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
                "d2": torch.full((N * K + 2 * G,), -123.0, dtype=torch.float64, device=dev),
                "n": torch.full((N + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
                "proven": torch.full((N + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device=dev)}
        before = {k: v.clone() for k, v in bufs.items()}
        ccam = _camera(cam).to_c()
        views = {k: v[G:-G] for k, v in bufs.items()}
        rc = lib.nesti_depth_window_knn(_lib.ptr(xyz_d), N, _lib.ptr(pix_d), _lib.ptr(rank_d), H, W, ctypes.byref(ccam), None, N, 0, R, K,
                                        _lib.ptr(views["idx"]), _lib.ptr(views["d2"]), _lib.ptr(views["n"]), _lib.ptr(views["proven"]),
                                        _lib.stream_ptr())
        _lib.check(rc, "nesti_depth_window_knn")
        torch.cuda.synchronize()
        _same((views["idx"].reshape(N, K), views["d2"].reshape(N, K), views["n"], views["proven"]), want, (R, K))
        for k, v in bufs.items():
            assert torch.equal(v[:G], before[k][:G]) and torch.equal(v[-G:], before[k][-G:]), k


def _compare(res, ref, keys=None):
    shared = [k for k in ref if isinstance(ref[k], np.ndarray) and k in res] if keys is None else keys
    assert "normals" in shared and len(shared) >= 4
    for k in shared:
        assert _bits_equal(res[k], ref[k]), k


@pytest.mark.parametrize("kind", ("u16", "f32"))
def test_depth_normals_plane_fit(gpu_device, kind):
    """depth_normals(estimator='pca', knn=(16, 32)): exact=True equals pca.pca_normals over the back-projected cloud with the camera
    centre as the viewpoint, every array bit for bit, and the normal map is those normals scattered; a strided frame equals pidx = the
    strided rows; exact=False equals CloudPatches.pca_knn over the RESTATED window lists on every row; smooth=2 equals
    pca_normals(smooth=2)."""
    from nesti_net_amd import pca
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.depth import default_window, depth_normals
    from nesti_net_amd.provider import CloudPatches
    depth, cam, b = WF.frame(kind)
    H, W = depth.shape
    camera = _camera(cam)
    R = default_window(32)
    want_lists = WF.restated(kind, R, 32)
    res = depth_normals(depth, camera, estimator="pca", knn=(16, 32), exact=True, device=gpu_device)
    assert np.array_equal(res["xyz"].view(np.uint32), b["xyz"].view(np.uint32)) and np.array_equal(res["pix"], b["pix"])
    ref = pca.pca_normals(b["xyz"], knn=(16, 32), orient="viewpoint", viewpoint=camera.centre, device=gpu_device)
    _compare(res, ref)
    assert res["orient"] == ref["orient"] and res["window"] == R
    assert _bits_equal(res["normal_map"], D.scatter(ref["normals"], b["pix"], H, W, 0.0))
    assert np.array_equal(res["window_proven"], want_lists[3].astype(bool)) and res["window_exact_rows"] == int((want_lists[3] == 0).sum()) > 0
    # a strided frame: the rows on the stride, neighbourhoods from every valid pixel
    s3 = D.back_project(depth, cam, 3)
    res3 = depth_normals(depth, camera, estimator="pca", knn=(16, 32), stride=3, device=gpu_device)
    ref3 = pca.pca_normals(b["xyz"], pidx=s3["qidx"], knn=(16, 32), orient="viewpoint", viewpoint=camera.centre, device=gpu_device)
    _compare(res3, ref3)
    assert np.array_equal(res3["pix"], b["pix"][s3["qidx"]]) and _bits_equal(res3["normal_map"], D.scatter(ref3["normals"], res3["pix"], H, W, 0.0))
    # exact=False: the window's lists as they are
    loose = depth_normals(depth, camera, estimator="pca", knn=(16, 32), exact=False, orient=None, device=gpu_device)
    cloud = CloudPatches(b["xyz"], NestiConfig(), device=gpu_device, radius_grid=False)
    lists = torch.from_numpy(want_lists[0]).to(gpu_device)
    normals, eig, radius, n = (_np(t) for t in cloud.pca_knn(0, b["n_valid"], (16, 32), nbr=lists))
    assert loose["window_exact_rows"] == 0 and np.array_equal(loose["window_proven"], want_lists[3].astype(bool))
    assert _bits_equal(loose["normals_all"], normals) and _bits_equal(loose["eig"], eig) and _bits_equal(loose["radius"], radius)
    assert np.array_equal(loose["n_ball"], n) and _bits_equal(loose["normals"], normals[:, -1])
    assert not _bits_equal(loose["normals_all"], ref["normals_all"])                # the unproven rows do differ somewhere
    # smoothing over the same lists
    if kind == "u16":
        sm = depth_normals(depth, camera, estimator="pca", knn=(16, 32), smooth=2, device=gpu_device)
        ref_sm = pca.pca_normals(b["xyz"], knn=(16, 32), smooth=2, orient="viewpoint", viewpoint=camera.centre, device=gpu_device)
        _compare(sm, ref_sm)
        assert "smooth_support" in sm and not _bits_equal(sm["normals"], res["normals"])
        wide = depth_normals(depth, camera, estimator="pca", knn=(8,), smooth={"k": 24, "iters": 1}, device=gpu_device)
        ref_wide = pca.pca_normals(b["xyz"], knn=(8,), smooth={"k": 24, "iters": 1}, orient="viewpoint", viewpoint=camera.centre,
                                   device=gpu_device)
        _compare(wide, ref_wide)


@pytest.mark.parametrize("estimator", ("hough", "robust", "quadric", "select"))
def test_depth_normals_other_estimators(gpu_device, estimator):
    """Each estimator's own ``*_normals(knn=...)`` under exact=True on a 48 x 64 crop, every shared array bit for bit; the quadric fit's
    curvature map is its scattered curvatures."""
    from nesti_net_amd import hough, quadric, robust, select
    from nesti_net_amd.depth import depth_normals
    depth, cam, b = WF.frame("f32", crop=CROP)
    H, W = depth.shape
    camera = _camera(cam)
    view = dict(orient="viewpoint", viewpoint=camera.centre, device=gpu_device)
    if estimator == "select":
        res = depth_normals(depth, camera, estimator="select", ladder=(8, 16, 32), slack=0.1, device=gpu_device)
        ref = select.select_normals(b["xyz"], ladder=(8, 16, 32), slack=0.1, **view)
    else:
        res = depth_normals(depth, camera, estimator=estimator, knn=(12, 24), device=gpu_device)
        ref = {"hough": hough.hough_normals, "robust": robust.robust_normals, "quadric": quadric.quadric_fit}[estimator](b["xyz"], knn=(12, 24), **view)
    _compare(res, ref)
    assert res["window_exact_rows"] > 0 and (res["normals"] != 0).any()
    assert _bits_equal(res["normal_map"], D.scatter(ref["normals"], b["pix"], H, W, 0.0))
    if estimator == "quadric":
        assert _bits_equal(res["curv_map"], D.scatter(ref["curv"], b["pix"], H, W, 0.0)) and (res["curv"] != 0).any()
    else:
        assert "curv_map" not in res


def test_frame_without_a_valid_pixel(gpu_device):
    from nesti_net_amd.depth import depth_normals
    res = depth_normals(np.zeros((6, 9), np.uint16), _camera(D.camera("u16")), estimator="quadric", knn=8, device=gpu_device)
    assert res["normal_map"].shape == (6, 9, 3) and not res["normal_map"].any() and res["curv_map"].shape == (6, 9, 2)
    assert res["normals"].shape == (0, 3) and len(res["pix"]) == 0 and len(res["window_proven"]) == 0 and res["window_exact_rows"] == 0


def test_sphere_normals_are_the_analytic_ones(gpu_device):
    """The plane fit's normals on the sphere's interior lie within a few degrees of the analytic normal (p - c) / |p - c|, turned to the
    camera: the route gives geometry, not noise."""
    from nesti_net_amd.depth import depth_normals
    depth, cam, b = WF.frame("u16")
    res = depth_normals(depth, _camera(cam), estimator="pca", knn=(32,), device=gpu_device)
    p = res["xyz"].astype(np.float64)
    rel = p - np.array(D.SPHERE_C)
    dist = np.linalg.norm(rel, axis=1)
    inner = (np.abs(dist - D.SPHERE_R) < 2e-3) & (rel[:, 2] < -0.35)                # on the sphere, away from its rim
    assert inner.sum() > 500
    want = rel[inner] / dist[inner, None]
    cos = np.clip((res["normals"][inner].astype(np.float64) * want).sum(axis=1), -1.0, 1.0)
    rms = np.degrees(np.sqrt(np.mean(np.arccos(cos) ** 2)))
    print("sphere interior: %d rows, RMS angle %.3f degrees" % (inner.sum(), rms))
    assert rms < 5.0


def test_command_line_with_depth_window(tmp_path, gpu_device, capsys):
    """Two frames (uint16 with a pose, float32 without) through --depth_images 1 --depth_window auto --estimator pca --knn 16,32: the
    files exist with the right shapes and .normal_map.npy equals the Python call's; without --depth_window the command is refused with
    the old words."""
    from nesti_net_amd.cli import main
    from nesti_net_amd.depth import depth_normals
    d = tmp_path / "frames"
    d.mkdir()
    pose4 = np.concatenate([D.rigid_pose(5), [[0.0, 0.0, 0.0, 1.0]]])
    expect = {}
    for name, kind, pose in (("frameA", "u16", pose4), ("frameB", "f32", None)):
        depth = D.scene(kind)
        np.save(str(d / (name + ".depth.npy")), depth)
        cam = D.camera(kind, pose=None if pose is None else pose[:3])
        (d / (name + ".camera")).write_text("%r %r %r %r %r\n" % (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["depth_scale"]))
        if pose is not None:
            np.savetxt(str(d / (name + ".cam2world")), pose, fmt="%.17g")
        expect[name] = depth_normals(depth, _camera(cam), estimator="pca", knn=(16, 32), device=gpu_device)
    (d / "testset.txt").write_text("frameA\nframeB\n")
    results = str(tmp_path / "log") + os.sep
    argv = ["--results_path", results, "--dataset_name", "kinect", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt",
            "--depth_images", "1", "--estimator", "pca", "--knn", "16,32"]
    assert main(argv + ["--depth_window", "auto"]) == 0
    out = os.path.join(results, "kinect_results")
    log = open(os.path.join(out, "log.txt")).read()
    print(log)
    for name, res in expect.items():
        rows = len(res["pix"])
        assert rows > 11000 and ("image window of %s: R = %d" % (name, res["window"])) in log
        normals = np.loadtxt(os.path.join(out, name + ".normals")).reshape(-1, 3).astype(np.float32)
        assert normals.shape == (rows, 3) and np.allclose(normals, res["normals"], atol=1e-6)
        assert np.array_equal(np.loadtxt(os.path.join(out, name + ".pix")).astype(np.int32), res["pix"])
        assert np.array_equal(np.loadtxt(os.path.join(out, name + ".window_proven")).astype(bool), res["window_proven"])
        assert np.loadtxt(os.path.join(out, name + ".pca_eig")).shape == (rows, 6)
        assert np.loadtxt(os.path.join(out, name + ".pca_count")).shape == (rows, 2)
        assert np.loadtxt(os.path.join(out, name + ".knn_radius")).shape == (rows, 2)
        nmap = np.load(os.path.join(out, name + ".normal_map.npy"))
        assert nmap.shape == (D.H, D.W, 3) and _bits_equal(nmap, res["normal_map"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and "--estimator pca does not take --depth_images 1" in capsys.readouterr().err


@pytest.mark.parametrize("estimator", ("quadric", "hough", "robust", "ladder"))
def test_command_line_other_estimators(tmp_path, gpu_device, estimator):
    """One 48 x 64 frame through --depth_window with each other estimator, --smooth 1 and --depth_window_exact 0 among them: the row
    files have the rows of .pix and .normals holds the Python call's normals."""
    from nesti_net_amd import textio
    from nesti_net_amd.cli import main
    from nesti_net_amd.depth import depth_normals
    depth, cam, b = WF.frame("f32", crop=CROP)
    d = tmp_path / "frames"
    d.mkdir()
    np.save(str(d / "crop.depth.npy"), depth)
    (d / "crop.camera").write_text("%r %r %r %r %r\n" % (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["depth_scale"]))
    np.savetxt(str(d / "crop.cam2world"), np.concatenate([cam["pose"], [[0.0, 0.0, 0.0, 1.0]]]), fmt="%.17g")
    (d / "testset.txt").write_text("crop\n")
    results = str(tmp_path / "log") + os.sep
    argv = ["--results_path", results, "--dataset_name", "kinect", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt",
            "--depth_images", "1", "--smooth", "1"]
    if estimator == "ladder":
        argv += ["--estimator", "pca", "--knn_ladder", "8,16,32", "--depth_window", "5", "--depth_window_exact", "0"]
        want = depth_normals(depth, _camera(cam), estimator="select", ladder=(8, 16, 32), window=5, exact=False, smooth=1, device=gpu_device)
        files = {".select_k": 1, ".select_eig": 3, ".select_variation": 3, ".knn_radius": 1}
    else:
        argv += ["--estimator", estimator, "--knn", "12,24", "--depth_window", "auto"]
        want = depth_normals(depth, _camera(cam), estimator=estimator, knn=(12, 24), smooth=1, device=gpu_device)
        files = {"quadric": {".curv": 2, ".quadric_curv": 4, ".quadric_count": 2}, "hough": {".hough_conf": 2, ".hough_votes": 4, ".hough_count": 2},
                 "robust": {".robust_support": 2, ".robust_inliers": 2, ".robust_count": 2}}[estimator]
        files[".knn_radius"] = 2
    assert main(argv) == 0
    out = os.path.join(results, "kinect_results")
    log = open(os.path.join(out, "log.txt")).read()
    print(log)
    rows = b["n_valid"]
    assert "image window of crop: R = %d" % want["window"] in log and ("--depth_window_exact 0" in log) == (estimator == "ladder")
    assert np.array_equal(np.loadtxt(os.path.join(out, "crop.pix")).astype(np.int32), b["pix"])
    tmp = str(tmp_path / "want.normals")
    textio.write_f32(tmp, want["normals"])
    assert open(os.path.join(out, "crop.normals")).read() == open(tmp).read()        # the same bits through the same writer
    for ext, width in dict(files, **{".normals": 3, ".smooth_support": 2, ".window_proven": 1}).items():
        assert np.loadtxt(os.path.join(out, "crop" + ext)).reshape(rows, -1).shape == (rows, width), ext
    assert _bits_equal(np.load(os.path.join(out, "crop.normal_map.npy")), want["normal_map"])
    assert os.path.exists(os.path.join(out, "crop.curv_map.npy")) == (estimator == "quadric")
