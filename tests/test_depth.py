"""Depth images without a GPU: the new C entries exist and refuse bad arguments before any device call, the Python layer round-trips
a camera and reads the per-frame files strictly, the command line refuses the exclusive combinations, and the tests' own restatement
(tests/_depth_fixture.py) has the properties the GPU tests rely on."""
import ctypes
import math

import numpy as np
import pytest

import _depth_fixture as F


def _lib():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    return _lib.load()


def _camera(**kw):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    c = _lib.CCamera()
    c.fx, c.fy, c.cx, c.cy, c.depth_scale, c.z_near, c.z_far = F.FX, F.FY, F.CX, F.CY, 1e-3, 0.0, math.inf
    for k, v in kw.items():
        if k == "pose":
            c.has_pose = 1
            c.pose[:] = v
        else:
            setattr(c, k, v)
    return c


def test_symbols_and_workspace_bytes():
    lib = _lib()
    for name in ("nesti_depth_workspace_bytes", "nesti_depth_to_cloud", "nesti_image_scatter", "nesti_project_to_image"):
        assert hasattr(lib, name), name
    ws = lib.nesti_depth_workspace_bytes
    for h, w in ((0, 5), (5, 0), (-1, 5), (5, -1), (1 << 13, (1 << 13) + 1), (1 << 26, 2)):
        assert ws(h, w) == 0, (h, w)
    assert ws(1, 1) > 0 and ws(1 << 13, 1 << 13) > 0
    sizes = [ws(h, w) for h, w in ((1, 1), (1, 64), (1, 65), (37, 53), (96, 128), (480, 640), (1 << 13, 1 << 13))]
    assert sizes == sorted(sizes)
    assert ws(480, 640) >= 480 * 640 * 8 and ws(128, 96) == ws(96, 128)        # at least the key image; a function of H W


def test_entries_refuse_bad_arguments_before_any_device_call():
    """Every refusal of include/nesti_hip.h, with pointers that are never dereferenced: no device is touched."""
    lib = _lib()
    H, W = 96, 128
    p = ctypes.c_void_p(0x1000)                   # non-null, never read: the checks come first
    ws = lib.nesti_depth_workspace_bytes(H, W)
    big = ctypes.c_size_t(1 << 62)
    fill = (ctypes.c_float * 8)()
    good = _camera()

    def cloud(d=p, t=0, h=H, w=W, c=good, s=1, xyz=p, pix=p, cnt=p, wsp=p, wsb=ws):
        return lib.nesti_depth_to_cloud(d, t, h, w, None if c is None else ctypes.byref(c), s, xyz, pix, None, None, cnt, wsp, wsb, None)

    def scatter(rows=p, pix=p, m=10, ch=3, h=H, w=W, f=fill, img=p):
        return lib.nesti_image_scatter(rows, pix, m, ch, h, w, f, img, None)

    def project(xyz=p, val=p, m=10, ch=3, h=H, w=W, c=good, f=fill, img=p, idx=None, wsp=p, wsb=ws):
        return lib.nesti_project_to_image(xyz, val, m, ch, h, w, None if c is None else ctypes.byref(c), f, img, idx, wsp, wsb, None)

    def refused(rc, *words):
        msg = lib.nesti_last_error().decode()
        assert rc != 0 and all(x in msg for x in words), (rc, msg)

    who = "nesti_depth_to_cloud"
    for kw in ({"d": None}, {"xyz": None}, {"pix": None}, {"cnt": None}, {"wsp": None}, {"c": None}):
        refused(cloud(**kw), who, "null")
    for t in (2, -1, 7):
        refused(cloud(t=t), who, "unknown depth type")
    for s in (0, -3):
        refused(cloud(s=s), who, "stride")
    refused(cloud(wsb=ws - 1), who, "workspace too small")
    who = "nesti_image_scatter"
    for kw in ({"rows": None}, {"pix": None}, {"f": None}, {"img": None}):
        refused(scatter(**kw), who, "null")
    who = "nesti_project_to_image"
    for kw in ({"xyz": None}, {"val": None}, {"f": None}, {"img": None}, {"wsp": None}, {"c": None}):
        refused(project(**kw), who, "null")
    refused(project(wsb=ws - 1), who, "workspace too small")
    for call, who in ((cloud, "nesti_depth_to_cloud"), (scatter, "nesti_image_scatter"), (project, "nesti_project_to_image")):
        for kw in ({"h": 0}, {"w": 0}, {"h": -2}, {"w": -2}):
            refused(call(**kw), who, "H and W")
        kw = {"h": 1 << 13, "w": (1 << 13) + 1}
        if call is not scatter:
            kw["wsb"] = big
        refused(call(**kw), who, "2^26")
    for call, who in ((scatter, "nesti_image_scatter"), (project, "nesti_project_to_image")):
        for ch in (0, 9, -1):
            refused(call(ch=ch), who, "C must")
        refused(call(m=-1), who, "M must")
    nan, inf = float("nan"), float("inf")
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    bad = [({"fx": 0.0}, "fx"), ({"fy": 0.0}, "fx"), ({"fx": nan}, "fx"), ({"fy": inf}, "fx"), ({"fx": -inf}, "fx"),
           ({"cx": nan}, "cx"), ({"cy": inf}, "cx"),
           ({"depth_scale": 0.0}, "depth_scale"), ({"depth_scale": -1.0}, "depth_scale"), ({"depth_scale": nan}, "depth_scale"),
           ({"depth_scale": inf}, "depth_scale"),
           ({"z_near": 2.0, "z_far": 1.0}, "z_near"), ({"z_near": nan}, "z_near"), ({"z_far": nan}, "z_near"),
           ({"pose": eye[:7] + [nan] + eye[8:]}, "pose"), ({"pose": eye[:3] + [inf] + eye[4:]}, "pose")]
    for call, who in ((cloud, "nesti_depth_to_cloud"), (project, "nesti_project_to_image")):
        for kw, word in bad:
            refused(call(c=_camera(**kw)), who, word)


def test_camera_round_trips_through_to_c():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.depth import Camera
    T = F.rigid_pose(3)
    for cam in (Camera(525.0, 526.5, 319.5, 239.5), Camera(120.0, 121.0, 63.5, 47.5, 1e-3, 0.4, 3.5, T),
                Camera(1.0, 2.0, 3.0, 4.0, 0.25, pose=np.concatenate([T, [[0, 0, 0, 1.0]]]))):
        c = cam.to_c()
        assert (c.fx, c.fy, c.cx, c.cy, c.depth_scale, c.z_near, c.z_far) == (cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale,
                                                                               cam.z_near, cam.z_far)
        back = Camera.from_c(c)
        assert (back.fx, back.fy, back.cx, back.cy, back.depth_scale, back.z_near, back.z_far) == \
               (cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale, cam.z_near, cam.z_far)
        if cam.pose is None:
            assert c.has_pose == 0 and back.pose is None and np.array_equal(cam.centre, np.zeros(3))
        else:
            assert c.has_pose == 1 and np.array_equal(back.pose, T) and np.array_equal(cam.centre, T[:, 3])
            assert np.array_equal(back.to_c().pose[:], c.pose[:])
    assert Camera(1.0, 1.0, 0.0, 0.0).z_far == math.inf and Camera(1.0, 1.0, 0.0, 0.0).z_near == 0.0
    inv = Camera(1.0, 1.0, 0.0, 0.0, pose=T).inverse().pose
    assert np.allclose(inv[:, :3] @ T[:, :3], np.eye(3), atol=1e-14) and np.allclose(inv[:, :3] @ T[:, 3] + inv[:, 3], 0, atol=1e-14)
    with pytest.raises(ValueError):
        Camera(1.0, 1.0, 0.0, 0.0, pose=np.eye(3)).to_c()
    with pytest.raises(ValueError):
        Camera(1.0, 1.0, 0.0, 0.0, pose=np.ones((4, 4))).to_c()


def test_command_line_refuses_the_exclusive_combinations(tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.cli import build_parser, main
    base = ["--results_path", str(tmp_path) + "/", "--dataset_path", str(tmp_path) + "/", "--synthetic_weights", "--depth_images", "1"]
    for extra in (["--sparse_patches", "1"], ["--query_positions", "1"], ["--viewpoint", "0", "0", "0"],
                  ["--orient", "mst", "--viewpoint", "0", "0", "0"], ["--depth_stride", "0"]):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        main(base[:-2] + ["--depth_stride", "2"])                   # the stride belongs to the depth mode
    assert e.value.code == 2
    flags = build_parser().parse_args(base)
    assert flags.depth_images == 1 and flags.depth_stride == 1 and flags.orient is None      # resolved to 'viewpoint' by main


def test_frame_file_readers_reject_short_or_non_finite_files(tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.depth import read_cam2world, read_camera, read_depth
    cam = tmp_path / "a.camera"
    cam.write_text("525.0 525.5 319.5 239.5 0.001\n")
    c = read_camera(str(cam))
    assert (c.fx, c.fy, c.cx, c.cy, c.depth_scale) == (525.0, 525.5, 319.5, 239.5, 0.001) and c.pose is None
    for text in ("525 525 319.5 239.5\n", "", "525 525 nan 239.5 0.001", "525 inf 319.5 239.5 0.001", "525 525 x 239.5 0.001"):
        cam.write_text(text)
        with pytest.raises(ValueError):
            read_camera(str(cam))
    T = np.concatenate([F.rigid_pose(4), [[0, 0, 0, 1.0]]])
    pose = tmp_path / "a.cam2world"
    np.savetxt(str(pose), T, fmt="%.17g")
    assert np.array_equal(read_cam2world(str(pose)), T)
    np.savetxt(str(pose), T[:3], fmt="%.17g")
    with pytest.raises(ValueError):
        read_cam2world(str(pose))
    for bad in (np.nan, np.inf):
        B = T.copy()
        B[1, 3] = bad
        np.savetxt(str(pose), B, fmt="%.17g")
        with pytest.raises(ValueError):
            read_cam2world(str(pose))
    B = T.copy()
    B[3, 3] = 2.0
    np.savetxt(str(pose), B, fmt="%.17g")
    with pytest.raises(ValueError):
        read_cam2world(str(pose))
    np.save(str(tmp_path / "a.depth.npy"), F.scene("u16"))
    assert read_depth(str(tmp_path / "a.depth.npy")).dtype == np.uint16
    np.save(str(tmp_path / "b.depth.npy"), F.scene("f32").astype(np.float64))
    with pytest.raises(ValueError):
        read_depth(str(tmp_path / "b.depth.npy"))


def test_fixture_conditions():
    """What the GPU tests rely on: both scenes have the holes they promise, whole 256-pixel blocks empty and whole waves full, both surfaces in
    view; the restatement's projection of the fixture's own cloud has no self-collision (with or without a pose), and its
    nearest-wins rule does what it says on a hand-made case."""
    for kind in ("u16", "f32"):
        d = F.scene(kind)
        assert d.shape == (F.H, F.W) and not d[F.EMPTY_ROWS].any() and not d[F.HOLE].any() and not d.reshape(-1)[::97].any()
        b = F.back_project(d, F.camera(kind))
        # 96 x 128 = 48 blocks of 256 pixels, some empty; a zero every 97 pixels leaves no block of 256 full (the all-valid 64 x 64
        # case of the GPU test has those), but whole 64-pixel waves are
        valid = b["rank"] >= 0
        assert (~valid.reshape(-1, 256)).all(axis=1).any() and valid.reshape(-1, 64).all(axis=1).any() and 0 < b["n_valid"] < F.H * F.W
        assert np.array_equal(b["pix"], np.flatnonzero(b["rank"] >= 0)) and np.array_equal(b["rank"][b["pix"]], np.arange(b["n_valid"]))
        z = b["xyz"][:, 2]
        assert z.min() < 1.7 and z.max() > 3.3                                      # the sphere's near pole and the far plane
        if kind == "f32":
            for at in (F.NAN_AT, F.INF_AT, F.NEG_AT):
                assert b["rank"][at[0] * F.W + at[1]] == -1
        for stride in (2, 3, 7):
            q = F.back_project(d, F.camera(kind), stride)
            v, u = q["pix"][q["qidx"]] // F.W, q["pix"][q["qidx"]] % F.W
            assert (v % stride == 0).all() and (u % stride == 0).all() and 0 < q["n_queries"] < b["n_valid"] / stride
        # the fixture's own cloud through its own camera: every valid pixel gets its own row back
        for pose in (None, F.rigid_pose(11)):
            c = F.back_project(d, F.camera(kind, pose=pose))
            cam_back = F.camera(kind, pose=None if pose is None else F.inverse_pose(pose))
            idx = F.project(c["xyz"], cam_back, F.H, F.W)
            assert np.array_equal(idx.reshape(-1), c["rank"])
    # nearest wins, then the smaller row; behind the camera, outside and non-finite rows do not land
    cam = F.camera("f32")
    pts = np.array([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0], [0, 0, -1.0], [50, 0, 1.0], [np.nan, 0, 1.0], [0, 0, 0.0]], np.float32)
    idx = F.project(pts, cam, F.H, F.W)
    assert (idx >= 0).sum() == 1 and idx[48, 64] == 1             # floor(63.5 + 0.5) = 64, floor(47.5 + 0.5) = 48
