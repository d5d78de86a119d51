"""Depth images on real kernels (csrc/depth.hip, nesti_net_amd/depth.py, NormalEstimator.estimate_depth, --depth_images) against
the tests' own numpy float64 restatement (tests/_depth_fixture.py): back-projection with ordered compaction, image scatter,
nearest-wins projection -- all bit for bit, integer for integer -- and the route end to end.

Bit equality is the expectation, not a hope: every step of the definition is one IEEE-rounded float64 operation in a fixed order
(contraction is off in the unit), followed by one rounding to float32."""
import os

import numpy as np
import pytest
import torch

import _depth_fixture as F

pytestmark = pytest.mark.gpu

STRIDES = (1, 2, 3, 7)
CUT = (1.8, 3.2)            # z_near / z_far that cut into the fixture scene (1.6 .. 3.6 m) and into the ramps below (0.5 .. 3.5 m)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _camera(d):
    from nesti_net_amd.depth import Camera
    return Camera(**d)


def _as_kind(z, kind):
    """Metres [H,W] float64 (0 = hole) as uint16 millimetres or float32 metres."""
    return np.round(z * 1000.0).astype(np.uint16) if kind == "u16" else z.astype(np.float32)


def _ramp(h, w):
    return 0.5 + 3.0 * np.arange(h * w, dtype=np.float64).reshape(h, w) / max(1, h * w - 1)


def _case(name, kind):
    """(depth, camera dict without pose / cut).  The sizes are the smallest at which the scan can go wrong: one pixel, one wave, one
    wave plus one, a size that is a multiple of nothing, the fixture (whole blocks empty), all-invalid and all-valid blocks, and one
    VGA frame -- 1200 first-level blocks, more than the 256 threads of the second level."""
    if name == "fixture":
        return F.scene(kind), F.camera(kind)
    if name == "1x1_valid":
        z = np.array([[2.5]])
    elif name == "1x1_invalid":
        z = np.array([[0.0]])
    elif name in ("1x64", "1x65", "37x53"):
        h, w = (int(x) for x in name.split("x"))
        z = _ramp(h, w)
        z.reshape(-1)[::5] = 0.0
    elif name == "64x64_invalid":
        z = np.zeros((64, 64))
    elif name == "64x64_valid":
        z = _ramp(64, 64)
    elif name == "480x640":
        z = _ramp(480, 640) * (np.random.RandomState(640).uniform(size=(480, 640)) < 0.5)
    else:
        raise KeyError(name)
    h, w = z.shape
    d = _as_kind(z, kind)
    if kind == "f32" and d.size >= 64:
        d.reshape(-1)[[3, 17, 33]] = [np.nan, np.inf, -2.0]
    cam = F.camera(kind)
    cam.update(cx=(w - 1) / 2.0, cy=(h - 1) / 2.0)
    return d, cam


CASES = ("1x1_valid", "1x1_invalid", "1x64", "1x65", "37x53", "fixture", "64x64_invalid", "64x64_valid", "480x640")


@pytest.mark.parametrize("name", CASES)
def test_back_projection(gpu_device, name):
    """xyz bit-equal, pix / rank / qidx / both counts integer for integer: both depth types, with and without a random rigid pose,
    with and without a z range that cuts into the scene, strides 1, 2, 3 and 7."""
    from nesti_net_amd.depth import depth_to_cloud
    pose = F.rigid_pose(21)
    for kind in ("u16", "f32"):
        depth, base = _case(name, kind)
        for T, cut in ((None, None), (pose, None), (None, CUT), (pose, CUT)):
            cam = dict(base, pose=T)
            if cut:
                cam.update(z_near=cut[0], z_far=cut[1])
            for stride in STRIDES:
                want = F.back_project(depth, cam, stride)
                got = depth_to_cloud(depth, _camera(cam), stride=stride, device=gpu_device)
                tag = (name, kind, T is not None, cut, stride)
                assert (got.n_valid, got.n_queries) == (want["n_valid"], want["n_queries"]), tag
                assert (got.H, got.W) == depth.shape and got.xyz.shape == (want["n_valid"], 3), tag
                assert np.array_equal(_np(got.pix), want["pix"]), tag
                assert np.array_equal(_np(got.rank), want["rank"]), tag
                assert np.array_equal(_np(got.qidx), want["qidx"]), tag
                assert np.array_equal(_bits(_np(got.xyz)), _bits(want["xyz"])), tag
                assert np.array_equal(got.viewpoint, np.zeros(3) if T is None else T[:, 3]), tag
        if name == "fixture":
            assert 0 < want["n_valid"] < F.back_project(depth, base)["n_valid"]          # the cut did cut
        if name == "1x1_valid":
            assert F.back_project(depth, base)["n_valid"] == 1


def test_scatter(gpu_device):
    """Normals-shaped (C = 3, f32), expert-shaped (C = 1, i32) and probabilities-shaped (C = 7) rows land at pix, everything else is
    the fill, bit for bit; M = 0 gives an all-fill image; a pix entry of -1 or H W is skipped."""
    from nesti_net_amd.depth import scatter_to_image
    h, w, M = 37, 53, 500
    rs = np.random.RandomState(8)
    pix = np.sort(rs.choice(h * w, M, replace=False)).astype(np.int32)
    shuffled = rs.permutation(pix).astype(np.int32)
    rows = {"normals": (rs.normal(size=(M, 3)).astype(np.float32), [0.0, 0.0, 0.0]),
            "expert": (rs.randint(0, 7, size=M).astype(np.int32), -1),
            "probs": (rs.uniform(size=(M, 7)).astype(np.float32), [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5]),
            "nan_fill": (rs.normal(size=(M, 2)).astype(np.float32), [np.nan, -0.0])}
    for name, (r, fill) in rows.items():
        for p in (pix, shuffled):
            got = _np(scatter_to_image(torch.from_numpy(r).to(gpu_device), torch.from_numpy(p).to(gpu_device), h, w, fill))
            want = F.scatter(r, p, h, w, fill)
            assert got.shape == want.shape and got.dtype == want.dtype, name
            assert np.array_equal(_bits(got), _bits(want)), name
        empty = _np(scatter_to_image(torch.from_numpy(r[:0]).to(gpu_device), torch.from_numpy(pix[:0]).to(gpu_device), h, w, fill))
        assert np.array_equal(_bits(empty), _bits(F.scatter(r[:0], pix[:0], h, w, fill))), name
        bad = pix.copy()
        bad[[0, 250, 499]] = [-1, h * w, h * w + 7]
        got = _np(scatter_to_image(torch.from_numpy(r).to(gpu_device), torch.from_numpy(bad).to(gpu_device), h, w, fill))
        want = F.scatter(r, bad, h, w, fill)
        assert np.array_equal(_bits(got), _bits(want)), name
        assert np.array_equal(_bits(got.reshape(h * w, -1)[pix[0]]), _bits(np.asarray(fill, r.dtype).reshape(-1))), name


def _frustum_points():
    """5 000 random points in a frustum a little wider than the image; 500 of them again pushed 1 mm and 1 um nearer / farther along
    their rays and 100 exact copies (collisions, equal-float32-z ties among them); points behind the camera, outside the image, at
    z = 0 and non-finite."""
    rs = np.random.RandomState(31)
    n = 5000
    z = rs.uniform(0.5, 4.0, n)
    u, v = rs.uniform(-10.0, F.W + 10.0, n), rs.uniform(-10.0, F.H + 10.0, n)
    p = np.stack([(u - F.CX) * z / F.FX, (v - F.CY) * z / F.FY, z], axis=1)
    dup = p[:500]
    push = np.repeat(np.array([1e-3, -1e-3, 1e-6, -1e-6]), 125)[:, None]
    pushed = dup * (1.0 + push / np.linalg.norm(dup, axis=1, keepdims=True))
    special = np.array([[0.1, 0.1, -2.0], [0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, np.nan], [0.0, 0.0, np.inf],
                        [50.0, 0.0, 1.0], [0.0, -50.0, 1.0], [-0.2, 0.3, -0.0]])
    allp = np.concatenate([p, pushed, p[500:600], special])
    return np.ascontiguousarray(allp[rs.permutation(len(allp))].astype(np.float32))


def test_projection(gpu_device):
    """index_image integer for integer and the value images bit for bit against the restatement, without and with a world -> camera
    pose; then the fixture's own cloud through its own camera: index_image == rank on every pixel (the restatement has no
    self-collision there: tests/test_depth.py::test_fixture_conditions, at the fixture's cx = 63.5, cy = 47.5)."""
    from nesti_net_amd.depth import project_to_image
    pts = _frustum_points()
    rs = np.random.RandomState(32)
    vals3 = rs.normal(size=(len(pts), 3)).astype(np.float32)
    vals1 = np.arange(len(pts), dtype=np.int32) * 3 + 1
    T = F.rigid_pose(33)
    with np.errstate(invalid="ignore"):
        world = np.stack(F.rigid(T, *(pts[:, k].astype(np.float64) for k in range(3))), axis=1).astype(np.float32)
    for xyz, pose in ((pts, None), (world, F.inverse_pose(T))):
        cam = F.camera("f32", pose=pose)
        want = F.project(xyz, cam, F.H, F.W)
        hits = want[want >= 0]
        print("rows", len(xyz), "pixels hit", len(hits), "of", F.H * F.W)
        x = torch.from_numpy(xyz).to(gpu_device)
        img3, idx = project_to_image(x, torch.from_numpy(vals3).to(gpu_device), _camera(cam), F.H, F.W, [0.0, -1.0, np.nan])
        assert np.array_equal(_np(idx), want)
        assert np.array_equal(_bits(_np(img3)), _bits(F.resolve(want, vals3, [0.0, -1.0, np.nan])))
        img1, idx1 = project_to_image(x, torch.from_numpy(vals1).to(gpu_device), _camera(cam), F.H, F.W, -1)
        assert np.array_equal(_np(idx1), want) and np.array_equal(_np(img1), F.resolve(want, vals1, -1))
        # collisions happened, and row order decided the exact copies (equal float32 z): the first of each group may win, never a later one
        if pose is None:                                           # in camera coordinates: far more rows in front of the camera than pixels hit
            assert len(hits) < (np.isfinite(xyz).all(axis=1) & (xyz[:, 2] > 0)).sum() - 1000
        groups = {}
        for r, row in enumerate(xyz):
            groups.setdefault(row.tobytes(), []).append(r)
        copies = [g for g in groups.values() if len(g) > 1]
        won = set(hits.tolist())
        assert len(copies) >= 100 and not any(r in won for g in copies for r in g[1:])
        assert sum(g[0] in won for g in copies) > 20
    # M = 0: all fill, all -1
    img0, idx0 = project_to_image(x[:0], torch.from_numpy(vals3[:0]).to(gpu_device), _camera(cam), F.H, F.W, 7.0)
    assert (_np(idx0) == -1).all() and (_np(img0) == 7.0).all()
    for kind, pose in (("u16", None), ("f32", F.rigid_pose(11))):
        b = F.back_project(F.scene(kind), F.camera(kind, pose=pose))
        back = F.camera(kind, pose=None if pose is None else F.inverse_pose(pose))
        _, idx = project_to_image(torch.from_numpy(b["xyz"]).to(gpu_device), torch.from_numpy(b["pix"]).to(gpu_device), _camera(back), F.H, F.W, -1)
        assert np.array_equal(_np(idx).reshape(-1), b["rank"])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
P = 64
TRANSLATION = np.array([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 1.0]])


@pytest.fixture(scope="module")
def e2e(gpu_device):
    """The fixture scene (uint16), its cloud by the restatement, and ONE estimator: the configuration, synthetic weights and calibrated
    gate of tests/test_gpu_query_positions.py, in f16x3 -- a dtype whose output does not depend on the calls that came before, so two
    runs can be compared bit for bit.  Computed once, shared, never changed."""
    from nesti_net_amd import weights
    from nesti_net_amd.calibrate import calibrate_gate
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.pipeline import NormalEstimator
    from nesti_net_amd.provider import CloudPatches
    cfg = NestiConfig(num_point=P)
    depth = F.scene("u16")
    cam = F.camera("u16")
    b = F.back_project(depth, cam)
    cp = CloudPatches(b["xyz"], cfg, device=gpu_device, pidx=np.arange(7, b["n_valid"], max(1, b["n_valid"] // 512))[:512])
    sp, sn = cp.build(0, cp.patch_count)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=gpu_device)
    del cp, sp, sn
    est = NormalEstimator(cfg, W, dtype="f16x3", device=gpu_device, batch=4096)
    return {"cfg": cfg, "W": W, "est": est, "depth": depth, "cam": cam, "cloud": b}


def _check_maps(res, pix, normals, expert, probs, centre):
    """The maps are the rows scattered by pix and the fill elsewhere; every estimated pixel faces the camera in float64."""
    assert np.array_equal(res["pix"], pix)
    assert np.array_equal(_bits(res["normals"]), _bits(normals)) and np.array_equal(res["expert"], expert)
    assert np.array_equal(_bits(res["probs"]), _bits(probs))
    assert np.array_equal(_bits(res["normal_map"]), _bits(F.scatter(normals, pix, F.H, F.W, 0.0)))
    assert np.array_equal(res["expert_map"], F.scatter(expert, pix, F.H, F.W, -1))
    assert np.array_equal(_bits(res["probs_map"]), _bits(F.scatter(probs, pix, F.H, F.W, 0.0)))
    off = np.ones(F.H * F.W, bool)
    off[pix] = False
    assert not _bits(res["normal_map"].reshape(-1, 3)[off]).any() and (res["expert_map"].reshape(-1)[off] == -1).all()
    assert not _bits(res["probs_map"].reshape(F.H * F.W, -1)[off]).any()
    n, p = res["normals"].astype(np.float64), res["xyz"].astype(np.float64)
    assert (np.linalg.norm(n, axis=1) > 0).all() and (res["expert"] >= 0).all()
    d = centre[None, :] - p
    facing = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    assert (facing >= 0).all()


def test_estimate_depth_equals_estimate_on_the_cloud(e2e):
    """Stride 1: estimate_depth(depth, cam) is estimate(fixture_xyz, orient='viewpoint', viewpoint=camera centre) scattered by the
    restatement's pix."""
    from nesti_net_amd.depth import Camera
    est, b = e2e["est"], e2e["cloud"]
    res = est.estimate_depth(e2e["depth"], Camera(**e2e["cam"]))
    normals, expert, probs = est.estimate(b["xyz"], orient="viewpoint", viewpoint=np.zeros(3))
    assert np.array_equal(_bits(res["xyz"]), _bits(b["xyz"]))
    _check_maps(res, b["pix"], normals, expert, probs, np.zeros(3))
    print("stride 1:", len(b["pix"]), "rows, experts", np.bincount(expert, minlength=7).tolist(), "flipped", est.last_orient["n_flipped"])
    assert len(np.unique(expert)) >= 3 and 0 < est.last_orient["n_flipped"] < len(expert)
    # orient=None leaves the signs as the experts produced them: the same rows up to sign, some of them facing away
    raw = est.estimate_depth(e2e["depth"], Camera(**e2e["cam"]), orient=None)
    assert np.array_equal(_bits(raw["normals"]) & 0x7fffffff, _bits(normals) & 0x7fffffff)
    assert not np.array_equal(_bits(raw["normals"]), _bits(normals)) and np.array_equal(raw["expert_map"], res["expert_map"])


def test_estimate_depth_with_a_stride(e2e):
    """stride = 3 is estimate(fixture_xyz, pidx=expected qidx, orient='viewpoint'): the neighbourhoods come from every valid pixel,
    the queries are the valid pixels on the stride.  It is NOT the stride-1 result sub-sampled: the hash subsample keys on the patch
    row, which differs between the two runs, so a ball capped at P points draws a different subset."""
    from nesti_net_amd.depth import Camera
    est = e2e["est"]
    b = F.back_project(e2e["depth"], e2e["cam"], 3)
    res = est.estimate_depth(e2e["depth"], Camera(**e2e["cam"]), stride=3)
    normals, expert, probs = est.estimate(b["xyz"], pidx=b["qidx"], orient="viewpoint", viewpoint=np.zeros(3))
    assert len(expert) == b["n_queries"] and np.array_equal(_bits(res["xyz"]), _bits(b["xyz"][b["qidx"]]))
    _check_maps(res, b["pix"][b["qidx"]], normals, expert, probs, np.zeros(3))
    v, u = res["pix"] // F.W, res["pix"] % F.W
    assert (v % 3 == 0).all() and (u % 3 == 0).all()


def test_no_valid_pixel(e2e):
    """All-fill maps and empty rows, without touching the network (the estimator would refuse an empty cloud)."""
    from nesti_net_amd.depth import Camera
    for stride in (1, 5):
        res = e2e["est"].estimate_depth(np.zeros((12, 20), np.uint16), Camera(**e2e["cam"]), stride=stride)
        assert res["normal_map"].shape == (12, 20, 3) and not _bits(res["normal_map"]).any()
        assert res["expert_map"].shape == (12, 20) and (res["expert_map"] == -1).all()
        assert res["probs_map"].shape == (12, 20, 7) and not _bits(res["probs_map"]).any()
        assert res["normals"].shape == (0, 3) and res["expert"].shape == (0,) and res["probs"].shape == (0, 7)
        assert res["xyz"].shape == (0, 3) and res["pix"].shape == (0,)


def test_a_rigid_pose_moves_the_cloud_and_keeps_the_experts(e2e):
    """Moving the scene by a rigid pose changes xyz and leaves expert_map unchanged wherever the fp64 oracle's top-2 gap exceeds
    parity.TIE_MARGIN; the moved cloud is a different float input, so nothing stronger holds.  The pose is a pure translation: the
    network sees patches in world axes (no PCA) and the radii come from the axis-aligned bounding box, so a rotation changes the
    function that is evaluated, not only its rounding.  Stride 16 keeps the oracle to a few dozen rows."""
    from nesti_net_amd import parity
    from nesti_net_amd.depth import Camera
    from oracle import mups_ref, net_ref, patches_ref
    est, cfg = e2e["est"], e2e["cfg"]
    b = F.back_project(e2e["depth"], e2e["cam"], 16)
    still = est.estimate_depth(e2e["depth"], Camera(**e2e["cam"]), stride=16)
    moved = est.estimate_depth(e2e["depth"], Camera(**dict(e2e["cam"], pose=TRANSLATION)), stride=16)
    assert np.array_equal(still["pix"], moved["pix"]) and len(still["pix"]) == b["n_queries"] >= 30
    shift = moved["xyz"].astype(np.float64) - still["xyz"].astype(np.float64)
    assert np.abs(shift - TRANSLATION[:, 3]).max() < 1e-6 and not np.array_equal(_bits(moved["xyz"]), _bits(still["xyz"]))
    _, r_abs = patches_ref.patch_radii(b["xyz"], cfg.patch_radius)
    o_pts, o_neff, _, _ = patches_ref.extract_patches(b["xyz"], b["qidx"], r_abs, P, est.seed)
    mups = mups_ref.mups_assemble(o_pts, o_neff, cfg.n_scales)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    outs = net_ref.over_chunks(lambda sl: net_ref.moe_forward(mups[sl], e2e["W"], expert_dict=cfg.expert_dict, dtype=torch.float64,
                                                              top1_only=True), len(mups))
    probs = np.sort(torch.cat([o["probs"] for o in outs]).numpy(), axis=1)
    gap = probs[:, -1] - probs[:, -2]
    differ = still["expert"] != moved["expert"]
    print("rows", len(gap), "expert differs on", int(differ.sum()), "of which inside the tie margin", int((differ & (gap <= parity.TIE_MARGIN)).sum()),
          "smallest gap", gap.min())
    assert not (differ & (gap > parity.TIE_MARGIN)).any()
    d = TRANSLATION[:, 3][None, :] - moved["xyz"].astype(np.float64)
    n = moved["normals"].astype(np.float64)
    assert ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] >= 0).all()


def test_command_line_with_depth_images(tmp_path, gpu_device):
    """Two frames (uint16 with a pose, float32 without) through --depth_images 1 --depth_stride 4: the files exist with the right
    shapes, .pix is the restatement's, and the images are the row files scattered by .pix."""
    from nesti_net_amd.cli import main
    d = tmp_path / "frames"
    d.mkdir()
    pose4 = np.concatenate([TRANSLATION, [[0.0, 0.0, 0.0, 1.0]]])
    expect = {}
    for name, kind, pose in (("frameA", "u16", pose4), ("frameB", "f32", None)):
        depth = F.scene(kind)
        np.save(str(d / (name + ".depth.npy")), depth)
        cam = F.camera(kind)
        (d / (name + ".camera")).write_text("%r %r %r %r %r\n" % (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["depth_scale"]))
        if pose is not None:
            np.savetxt(str(d / (name + ".cam2world")), pose, fmt="%.17g")
        b = F.back_project(depth, dict(cam, pose=None if pose is None else pose[:3]), 4)
        expect[name] = (b["pix"][b["qidx"]], b["xyz"][b["qidx"]], np.zeros(3) if pose is None else pose[:3, 3])
    (d / "testset.txt").write_text("frameA\nframeB\n")
    results = str(tmp_path / "log") + os.sep
    assert main(["--results_path", results, "--dataset_name", "kinect", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt",
                 "--synthetic_weights", "--depth_images", "1", "--depth_stride", "4"]) == 0
    out = os.path.join(results, "kinect_results")
    print(open(os.path.join(out, "log.txt")).read())
    for name, (pix, xyz, centre) in expect.items():
        normals = np.loadtxt(os.path.join(out, name + ".normals")).reshape(-1, 3).astype(np.float32)
        experts = np.loadtxt(os.path.join(out, name + ".experts")).reshape(-1).astype(np.int32)
        probs = np.loadtxt(os.path.join(out, name + ".experts_probs")).reshape(len(experts), -1).astype(np.float32)
        got_pix = np.loadtxt(os.path.join(out, name + ".pix")).reshape(-1).astype(np.int32)
        nmap, emap = np.load(os.path.join(out, name + ".normal_map.npy")), np.load(os.path.join(out, name + ".expert_map.npy"))
        assert len(normals) == len(experts) == len(probs) == len(pix) > 300 and probs.shape[1] == 7
        assert np.array_equal(got_pix, pix)
        assert nmap.shape == (F.H, F.W, 3) and nmap.dtype == np.float32 and emap.shape == (F.H, F.W) and emap.dtype == np.int32
        assert np.array_equal(_bits(nmap), _bits(F.scatter(normals, pix, F.H, F.W, 0.0)))
        assert np.array_equal(emap, F.scatter(experts, pix, F.H, F.W, -1))
        dv = centre[None, :] - xyz.astype(np.float64)
        n = normals.astype(np.float64)
        assert ((n[:, 0] * dv[:, 0] + n[:, 1] * dv[:, 1]) + n[:, 2] * dv[:, 2] >= 0).all()      # --orient defaults to viewpoint
