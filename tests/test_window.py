"""Image-window neighbour lists without a GPU: the tests' own restatement (tests/_window_fixture.py) against the brute force of
tests/_knn_fixture.py -- no PROVEN row's list differs from the exact one --, the default window, the argument refusals of the Python
layer and of the C entry (before any device call), and the command line's new flags."""
import ctypes
import math

import numpy as np
import pytest

import _depth_fixture as D
import _knn_fixture as KF
import _window_fixture as WF


@pytest.mark.parametrize("kind", ("u16", "f32"))
def test_restatement_against_brute_force(kind):
    """The 96 x 128 fixture, u16 without a pose and f32 with rigid_pose(5), at the five (R, K) pairs.  HARD: no proven row's list (indices
    and d2 bits) differs from the brute force.  Against a vacuous pass: at least 90 % of the rows are proven for the first four pairs
    (93.4 - 95.4 % measured with this restatement), and fewer than all at (7, 100), so the unproven path exists in the data."""
    depth, cam, b = WF.frame(kind)
    Kmax = max(K for _, K in WF.PAIRS)
    bi, bd, bc = KF.searched(("window", kind), b["xyz"], b["xyz"], Kmax)
    assert (bc == Kmax).all()
    for R, K in WF.PAIRS:
        idx, d2, n, proven = WF.restated(kind, R, K)
        same = (idx == bi[:, :K]).all(axis=1) & (d2.view(np.uint64) == bd[:, :K].view(np.uint64)).all(axis=1)
        p = proven.astype(bool)
        share = p.mean()
        print("%s R %d K %d: proven %.1f %%, equal to the brute force %.1f %%, proven rows that differ %d"
              % (kind, R, K, 100 * share, 100 * same.mean(), int((p & ~same).sum())))
        assert not (p & ~same).any(), (kind, R, K)
        assert (n[p] == K).all()
        if (R, K) == (7, 100):
            assert 0 < share < 1.0 and (~same).any()
        else:
            assert share >= 0.90, (kind, R, K, share)


def test_restatement_edge_rules():
    """What the GPU tests lean on: a window that covers the image proves every finite row whatever its count; a bad pix entry or a
    non-finite centre gives count 0 and proven 0; rank entries outside [0, N) are no candidates; the strided rows are a subset."""
    depth, cam, b = WF.frame("u16", crop=(10, 15, 50, 57))                          # 5 x 7
    H, W = depth.shape
    idx, d2, n, proven = WF.window_knn(b["xyz"], b["pix"], b["rank"], H, W, cam, 15, 64)
    assert proven.all() and (n == b["n_valid"]).all() and (idx[:, b["n_valid"]:] == -1).all() and np.isinf(d2[:, b["n_valid"]:]).all()
    assert (idx[:, 0] == np.arange(b["n_valid"])).all() and (d2[:, 0] == 0).all()
    pix, rank, xyz = b["pix"].copy(), b["rank"].copy(), b["xyz"].copy()
    pix[3], pix[4] = -1, H * W
    xyz[6, 1] = np.nan
    rank[rank == 9] = b["n_valid"] + 5
    idx, d2, n, proven = WF.window_knn(xyz, pix, rank, H, W, cam, 15, 64)
    assert (n[[3, 4, 6]] == 0).all() and (proven[[3, 4, 6]] == 0).all() and (idx[[3, 4, 6]] == -1).all()
    assert not (idx == 9).any() and not (idx == 6).any()                             # no candidate; a NaN d2 is never a neighbour
    all_rows = WF.restated("u16", 3, 16)
    strided = WF.restated("u16", 3, 16, stride=3)
    q = D.back_project(depth=WF.frame("u16")[0], cam=WF.frame("u16")[1], stride=3)["qidx"]
    assert len(q) % 4 != 0 and all(np.array_equal(a[q], s) for a, s in zip(all_rows, strided))
    assert WF.frame("f32")[2]["n_valid"] % 4 != 0        # four rows a workgroup: the last one is partial (and with the u16 stride above)


def test_default_window_is_monotone_and_in_range():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    from nesti_net_amd.depth import check_window, default_window
    assert _lib.WINDOW_MAX_R == WF.WINDOW_MAX_R == 15
    rs = [default_window(k) for k in range(1, 257)]
    assert all(1 <= r <= 15 for r in rs) and rs == sorted(rs) and rs[0] < rs[-1]
    for k in (8, 16, 32, 64, 256):
        assert (2 * default_window(k) + 1) ** 2 >= 2 * k                           # room for K and the proof
    assert check_window("auto", 32) == default_window(32) and check_window(7, 32) == 7
    for k in (0, 257, 2.5, None):
        with pytest.raises(ValueError):
            default_window(k)


def test_python_layer_refuses_bad_arguments():
    """``check_normals_args`` / ``check_window`` are what ``depth_normals`` and ``window_knn`` run before anything touches a GPU; the two
    entry points themselves are called with arguments that fail there."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import depth as dp
    cam = dp.Camera(**D.camera("u16"))
    frame = D.scene("u16")
    for bad in ("net", "plane", None, 3):
        with pytest.raises(ValueError, match="estimator"):
            dp.depth_normals(frame, cam, estimator=bad)
    with pytest.raises(ValueError, match="stride == 1"):
        dp.depth_normals(frame, cam, smooth=2, stride=2)
    with pytest.raises(ValueError, match="stride"):
        dp.depth_normals(frame, cam, stride=0)
    for bad in (0, 16, -1, "wide", 2.0, True):
        with pytest.raises(ValueError, match="window"):
            dp.depth_normals(frame, cam, window=bad)
        with pytest.raises(ValueError, match="window"):
            dp.window_knn(None, 16, window=bad)
    for bad in (0, 257, (8, 300), (16, 8), 1.5):
        with pytest.raises(ValueError):
            dp.depth_normals(frame, cam, knn=bad)
    for bad in (0, 257, -3, 1.5, None):
        with pytest.raises(ValueError, match="k must be"):
            dp.window_knn(None, bad)
    with pytest.raises(ValueError, match="scale"):
        dp.depth_normals(frame, cam, knn=(8, 16), scale=2)
    with pytest.raises(ValueError, match="orient"):
        dp.depth_normals(frame, cam, orient="up")
    with pytest.raises(ValueError, match="ladder"):
        dp.depth_normals(frame, cam, estimator="pca", ladder=(8, 16))
    with pytest.raises(ValueError):
        dp.depth_normals(frame, cam, estimator="select", ladder=(16, 8))
    ks, kmax, sm = dp.check_normals_args("pca", (16, 32), None, -1, 1, "viewpoint", {"k": 48})
    assert ks == (16, 32) and kmax == 48 and sm.k == 48
    assert dp.check_normals_args("select", None, (8, 24), -1, 3, None, None)[:2] == ((8, 24), 24)


def test_lists_keyword_is_optional_and_needs_knn():
    import inspect

    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough, pca, quadric, robust, select
    for f in (pca.fit_cloud, pca.pca_cloud, quadric.quadric_cloud, hough.hough_cloud, robust.robust_cloud, select.select_cloud):
        assert inspect.signature(f).parameters["lists"].default is None, f.__name__
    with pytest.raises(ValueError, match="knn must be given"):
        pca.fit_cloud(None, object(), None, ("a", "b"), -1, None, None, 8, None, lists=object())


def _camera(**kw):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    c = _lib.CCamera()
    c.fx, c.fy, c.cx, c.cy, c.depth_scale, c.z_near, c.z_far = D.FX, D.FY, D.CX, D.CY, 1e-3, 0.0, math.inf
    for k, v in kw.items():
        if k == "pose":
            c.has_pose = 1
            c.pose[:] = v
        else:
            setattr(c, k, v)
    return c


def test_entry_refuses_bad_arguments_before_any_device_call():
    """Every refusal of include/nesti_hip.h, with pointers that are never dereferenced: no device is touched."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "nesti_depth_window_knn")
    p = ctypes.c_void_p(0x1000)                   # non-null, never read: the checks come first
    good = _camera()

    def call(xyz=p, n=1000, pix=p, rank=p, h=96, w=128, c=good, idx=p, m=100, row0=0, r=3, k=16, nbr=p):
        return lib.nesti_depth_window_knn(xyz, n, pix, rank, h, w, None if c is None else ctypes.byref(c), idx, m, row0, r, k, nbr, p, p, p, None)

    def refused(rc, *words):
        msg = lib.nesti_last_error().decode()
        assert rc != 0 and all(x in msg for x in ("nesti_depth_window_knn",) + words), (rc, msg)

    for kw in ({"xyz": None}, {"pix": None}, {"rank": None}, {"c": None}, {"nbr": None}):
        refused(call(**kw), "null")
    for n in (0, -1):
        refused(call(n=n), "empty cloud")
    for kw in ({"h": 0}, {"w": 0}, {"h": -2}, {"w": -2}):
        refused(call(**kw), "H and W")
    refused(call(h=1 << 13, w=(1 << 13) + 1), "2^26")
    for r in (0, -1, 16, 1000):
        refused(call(r=r), "R must be")
    for k in (0, -1, 257):
        refused(call(k=k), "K must be")
    refused(call(m=-1), "M must be")
    refused(call(idx=None, row0=-1), "query_row0")
    refused(call(idx=None, row0=901), "exceed the cloud")
    nan, inf = float("nan"), float("inf")
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    for kw, word in (({"fx": 0.0}, "fx"), ({"fy": 0.0}, "fx"), ({"fx": nan}, "fx"), ({"fy": inf}, "fx"), ({"fx": -inf}, "fx"),
                     ({"cx": nan}, "cx"), ({"cy": inf}, "cx"),
                     ({"pose": eye[:7] + [nan] + eye[8:]}, "pose"), ({"pose": eye[:3] + [inf] + eye[4:]}, "pose")):
        refused(call(c=_camera(**kw)), word)
    # M = 0 is a no-op (no device call), with an index list and without; an argument error is still one
    assert call(m=0) == 0 and call(m=0, idx=None) == 0 and call(m=0, idx=None, row0=1000) == 0
    refused(call(m=0, k=0), "K must be")
    assert call(m=0, c=_camera(depth_scale=0.0, z_near=nan)) == 0                   # the depth unit and range are not read


def test_command_line_flags_and_refusals(tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.cli import FITS, build_parser, depth_window_args
    base = ["--results_path", str(tmp_path) + "/", "--dataset_path", str(tmp_path) + "/"]
    win = base + ["--estimator", "pca", "--knn", "8", "--depth_images", "1", "--depth_window", "auto"]
    parser = build_parser()
    flags = parser.parse_args(win)
    assert flags.depth_window == "auto" and flags.depth_window_exact == 1 and flags.depth_images == 1 and flags.knn == "8"
    assert depth_window_args(flags, parser, FITS["pca"], (8,), None) == ("auto", True)
    flags = parser.parse_args(win[:-1] + ["7", "--depth_window_exact", "0"])
    assert depth_window_args(flags, parser, FITS["pca"], None, (8, 16)) == (7, False)
    flags = parser.parse_args(base)
    assert flags.depth_window == "0" and flags.depth_window_exact == 1 and depth_window_args(flags, parser, None, None, None) is None


@pytest.mark.parametrize("extra, words", [
    (["--depth_window", "auto", "--estimator", "pca", "--knn", "8"], ("--depth_window", "--depth_images 1")),
    (["--depth_images", "1", "--depth_window", "auto", "--synthetic_weights"], ("--depth_window", "--estimator net")),
    (["--depth_images", "1", "--depth_window", "auto", "--estimator", "pca"], ("--depth_window", "--knn")),
    (["--depth_images", "1", "--depth_window", "auto", "--estimator", "quadric"], ("--depth_window", "--knn")),
    (["--depth_images", "1", "--depth_window", "16", "--estimator", "pca", "--knn", "8"], ("--depth_window",)),
    (["--depth_images", "1", "--depth_window", "wide", "--estimator", "pca", "--knn", "8"], ("--depth_window",)),
    (["--depth_images", "1", "--depth_window_exact", "0", "--estimator", "pca", "--knn", "8"], ("--depth_window_exact", "--depth_window")),
    (["--depth_images", "1", "--depth_window", "auto", "--estimator", "pca", "--knn", "8", "--outliers", "statistical"],
     ("--outliers", "left for later")),
    (["--depth_images", "1", "--depth_window", "auto", "--estimator", "pca", "--knn", "8", "--denoise", "1"], ("--denoise", "left for later")),
    (["--depth_images", "1", "--depth_window", "auto", "--estimator", "pca", "--knn", "8", "--voxel_size", "0.1"],
     ("--voxel_size", "left for later")),
    (["--depth_images", "1", "--depth_window", "auto", "--estimator", "pca", "--knn", "8", "--smooth", "2", "--depth_stride", "2"],
     ("--smooth", "--depth_stride")),
    # without --depth_window every refusal keeps its words
    (["--depth_images", "1", "--estimator", "pca", "--knn", "8"], ("--estimator pca does not take --depth_images 1",)),
    (["--depth_images", "1", "--estimator", "hough", "--knn", "8"], ("--estimator hough does not take --depth_images 1",)),
    (["--depth_images", "1", "--synthetic_weights", "--smooth", "2"], ("--smooth does not go with --depth_images 1",)),
])
def test_command_line_refuses(tmp_path, capsys, extra, words):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["--results_path", str(tmp_path) + "/", "--dataset_path", str(tmp_path) + "/"] + extra)
    err = capsys.readouterr().err
    assert e.value.code == 2 and all(w in err for w in words), (extra, err)
