"""Quadric-fit normals and principal curvatures on the GPU (csrc/quadric.hip, ``CloudPatches.quadric``, ``quadric.quadric_fit``,
``--estimator quadric``) against the tests' own numpy restatement (tests/_quadric_fixture.py), which is fed the GPU's own plane normals
(``plane_out``): ball sizes integer for integer, failed fits byte for byte, and normals and curvatures to bounds that come from the
arithmetic, not from what the kernel gives.

Notation: n the ball size, r the radius, N the 6 x 6 matrix of the restatement, a its float64 coefficients, eps = 2^-53,
    B = 16 n eps kappa_2(N) (||a||_2 + 1),
the first-order bound on ||delta a|| for normal equations whose every entry is a length-n float64 sum of terms of magnitude <= 1.
A (row, scale) pair with n >= 6 is ILL-CONDITIONED iff not B <= 1e-6 (kappa ~ 1e8 at most: far from the kernel's pivot threshold at
kappa ~ 1e13, so a well-conditioned pair can never be a failed fit).  Every well-conditioned pair is live and has
  length      | |nu| - 1 | <= 2^-22
  direction   sin(angle(nu, nu_ref)) <= 2^-22 + 2 B
  curvatures  r |k - k_ref| <= 2^-23 r |k_ref| + 8 (1 + ||a||_2) B, both of them; k_max >= k_min
  side        nu . n0 > 0
An ill-conditioned pair may be a failed fit or any finite values.  Every output is finite everywhere.

Measured on the CPU when the estimator was defined, on these clouds, rows and radii: reordering a ball at random moved a by at most
1.9e-3 B and an 80-bit evaluation by 1.3e-3 B, the curvatures by 2.4e-4 of their bound -- a margin of ~500 over what a summation order
should give.  The ill-conditioned share was 0 everywhere except box at the middle scale (1 of 464 pairs).

Every cloud here has three radii: this module runs ``quadric_kernel<3>``.  S = 1, 2 and 4: tests/test_gpu_fit_scales.py."""
import os

import numpy as np
import pytest
import torch

import _orient_fixture as OF
import _pca_fixture as fx
import _quadric_fixture as qx

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CLOUDS = ("ellipsoid", "sphere_big", "torus", "box", "torus_clean")


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_gpu = {}


def _run(name, dev):
    """((normals, curv, plane, n_ball), pca normals, counts) of a fixture's rows on ONE grid (index queries), once."""
    if name not in _gpu:
        from nesti_net_amd.provider import CloudPatches
        c = qx.cloud(name)
        every = len(c["rows"]) == len(c["pts"])
        cp = CloudPatches(c["pts"], c["cfg"], device=dev, pidx=None if every else c["rows"])
        assert cp.r_abs == c["r_abs"]
        out = _np(cp.quadric(0, cp.patch_count))
        plane = cp.pca(0, cp.patch_count)[0].cpu().numpy()
        counts = cp.count_balls(0, cp.patch_count).cpu().numpy()
        _gpu[name] = (out, plane, counts)
    return _gpu[name]


def check(got, ref, r_abs, label, ill_share_cap=0.01):
    """The assertions of the module docstring on (normals, curv, plane, n_ball) against a ``restate`` dict computed FROM got's plane.
    ``ill_share_cap``: the largest share of the n >= 6 pairs of one scale that may be ill-conditioned (None: all may be).  Prints each
    figure before it asserts.  Returns the mask of live (fitted) pairs."""
    normals, curv, plane, n_ball = got
    assert np.array_equal(n_ball, ref["n_ball"]), label
    for a in (normals, curv, plane):
        assert np.isfinite(a).all(), label
    short = n_ball < 6
    assert not _bits(normals)[short].any() and not _bits(curv)[short].any(), label        # failed fits, byte for byte
    live = (normals != 0).any(axis=-1)
    assert not _bits(curv)[~live].any(), label                                            # a failed fit has k = +0 +0 too
    B = qx.bound_B(ref)
    with np.errstate(invalid="ignore"):
        well = ~short & (B <= 1e-6)
    ill = ~short & ~well
    share = [ill[:, s].sum() / max(1, (~short[:, s]).sum()) for s in range(n_ball.shape[1])]
    assert ref["ok"][well].all(), label                                                   # the restatement agrees with the rule's premise
    g = normals[well].astype(np.float64)
    rn, a = ref["nu"][well], ref["a"][well]
    b = B[well]
    na = np.linalg.norm(a, axis=1)
    length = np.linalg.norm(g, axis=1)
    sin = np.linalg.norm(np.cross(g, rn), axis=1) / np.where(length > 0, length, 1.0)
    sin_bound = 2.0 ** -22 + 2 * b
    r = np.broadcast_to(np.asarray(r_abs, np.float64)[None, :], n_ball.shape)[well]
    k, kr = curv[well].astype(np.float64), ref["k"][well]
    k_err = r[:, None] * np.abs(k - kr)
    k_bound = 2.0 ** -23 * r[:, None] * np.abs(kr) + (8 * (1 + na) * b)[:, None]
    side = (g * plane[well].astype(np.float64)).sum(1)
    print("%s: %d (row, scale) pairs, %d with n >= 6, %d ill-conditioned (share per scale %s), %d live; largest B of the others %.3g, "
          "kappa %.3g; largest | |nu| - 1 | %.3g, sin / bound %.3g, curvature error / bound %.3g"
          % (label, n_ball.size, (~short).sum(), ill.sum(), ["%.4f" % x for x in share], live.sum(), b.max() if len(b) else 0.0,
             ref["kappa"][well].max() if len(b) else 0.0, np.abs(length - 1).max() if len(b) else 0.0,
             (sin / sin_bound).max() if len(b) else 0.0, (k_err / k_bound).max() if len(b) else 0.0))
    assert live[well].all(), "%s: %d well-conditioned pairs are failed fits" % (label, (~live[well]).sum())
    assert (np.abs(length - 1) <= 2.0 ** -22).all(), label
    assert (sin <= sin_bound).all(), label
    assert (k_err <= k_bound).all(), label
    assert (curv[..., 0] >= curv[..., 1]).all(), label
    assert (side > 0).all(), label
    if ill_share_cap is not None:
        assert max(share) <= ill_share_cap, "%s: ill-conditioned share per scale %s" % (label, share)
    return live


@pytest.mark.parametrize("name", CLOUDS)
def test_surfaces_against_the_restatement(name, gpu_device):
    """Five surface clouds: the n = 6 - 7 boundary interleaved with failed fits (ellipsoid, smallest scale), balls of ~150 / 600 / 2 400
    points with many trips per lane on an umbilic surface (sphere), noise (torus), edges and corners (box) and a clean surface with
    curvatures of both signs (torus_clean).

    Printed, not asserted -- RMS unoriented angle to the analytic normals, quadric fit against plane fit.  Measured with a numpy
    prototype when the estimator was defined: 4 000-point ellipsoid at the largest default radius 0.43 against 1.34 degrees; the
    12 000-point clean torus at radius 0.06 0.70 against 1.38 degrees but at 0.1 2.47 against 1.72; on the noisy torus the plane fit
    is better at the two smaller default scales (16.9 against 11.9, 61.7 against 53.2 degrees): the quadric fit is not uniformly
    better."""
    c = qx.cloud(name)
    got, pca_normals, counts = _run(name, gpu_device)
    assert np.array_equal(got[3], counts)                                 # ... equal to nesti_patches_count's
    assert np.array_equal(_bits(got[2]), _bits(pca_normals))              # plane_out IS nesti_pca_normals' output on this grid
    ref = qx.restate(c["pts"], c["pts"][c["rows"]], c["r_abs"], got[2])
    live = check(got, ref, c["r_abs"], name)
    S = got[0].shape[1]
    if name == "ellipsoid":
        assert live[:, 0].sum() >= 10                                     # the n = 6 - 7 boundary; 12 by the restatement
    if name in ("sphere_big", "torus_clean"):
        assert all(live[:, s].mean() >= 0.95 for s in range(S))
    gt = c["gt"][c["rows"]]
    print("%s: RMS angle to the analytic normals per scale, degrees: quadric fit %s, plane fit %s; live per scale %s"
          % (name, [round(fx.angle_rms_deg(got[0][:, s], gt), 3) for s in range(S)],
             [round(fx.angle_rms_deg(got[2][:, s], gt), 3) for s in range(S)], live.sum(0).tolist()))


def test_lattice(gpu_device):
    """Ties, duplicates and exact degeneracy.  On the grid rows h is identically an exact zero, so b = 0 and a = 0: nu is exactly
    (0, 0, 1) and k exactly +0 +0 wherever n >= 6 -- every grid row at the two larger scales.  On the collinear rows one of u, v is
    identically an exact zero, so a pivot is exactly 0: failed fits, all of them.  The smallest scale is all failed fits (n <= 2 on the
    grid)."""
    c = qx.cloud("lattice")
    got, pca_normals, counts = _run("lattice", gpu_device)
    normals, curv, plane, n_ball = got
    assert np.array_equal(n_ball, counts) and np.array_equal(_bits(plane), _bits(pca_normals))
    ref = qx.restate(c["pts"], c["pts"], c["r_abs"], plane)
    assert np.array_equal(n_ball, ref["n_ball"])
    P = fx.LATTICE_PLANE_ROWS
    grid = np.zeros(n_ball.shape, bool)
    grid[:P] = n_ball[:P] >= 6
    assert grid[:, 1:].sum() == 2 * P and not grid[:, 0].any() and n_ball[:P, 0].max() <= 2
    assert np.array_equal(_bits(normals)[grid], _bits(np.broadcast_to(np.array([0, 0, 1], np.float32), normals.shape))[grid])
    assert not _bits(curv)[grid].any()
    failed = ~grid
    assert (n_ball[P:, 1:] >= 6).all()                                    # the collinear rows fail on a pivot, not on the count
    assert not _bits(normals)[failed].any() and not _bits(curv)[failed].any()
    assert not ref["ok"][P:].any() and np.array_equal(ref["ok"], grid)


def test_query_kinds(gpu_device):
    """pidx rows and positions equal to them give the bits of the all-points call on ONE grid; positions 0.5 r off the surface are held
    to the restatement (all of them may be ill-conditioned); far, NaN and infinite positions come back as zero bytes with n_ball = 0."""
    from nesti_net_amd.provider import CloudPatches
    c = fx.cloud("ellipsoid")
    pts, cfg = c["pts"], c["cfg"]
    cp = CloudPatches(pts, cfg, device=gpu_device)
    full = cp.quadric(0, cp.patch_count)
    pidx = np.arange(0, len(pts), 7)
    # one grid: the same object serves the three kinds (the grid belongs to the cloud, the queries are per call)
    cp.pidx, cp.patch_count = torch.as_tensor(pidx, dtype=torch.int32, device=gpu_device), len(pidx)
    by_index = cp.quadric(0, len(pidx))
    cp.pidx, cp.queries = None, torch.from_numpy(pts[pidx]).to(gpu_device)
    by_position = cp.quadric(0, len(pidx))
    for a, b, d in zip(full, by_index, by_position):
        assert torch.equal(a[pidx.tolist()].view(torch.int32), b.view(torch.int32))
        assert torch.equal(b.view(torch.int32), d.view(torch.int32))
    # positions 0.5 r off the surface along the analytic normal, then far outside, NaN, inf
    off = (pts[pidx].astype(np.float64) + 0.5 * c["r_abs"][-1] * c["gt"][pidx].astype(np.float64)).astype(np.float32)
    lost = np.array([[50, 50, 50], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    q = np.concatenate([off, lost])
    cq = CloudPatches(pts, cfg, device=gpu_device, queries=torch.from_numpy(q))
    got = _np(cq.quadric(0, len(q)))
    assert np.array_equal(_bits(got[2]), _bits(cq.pca(0, len(q))[0].cpu().numpy()))
    ref = qx.restate(pts, q, c["r_abs"], got[2])
    assert (ref["n_ball"][len(off):] == 0).all() and (ref["n_ball"][:len(off), 2] >= 6).mean() > 0.5
    check(got, ref, c["r_abs"], "off-surface positions", ill_share_cap=None)
    for a in got:
        assert not _bits(a)[len(off):].any()


def test_partition(gpu_device):
    """Rows [0, M) in one call against [0, 1), [1, 1000), [1000, M) on two streams into pre-filled buffers: identical bytes;
    count = 0 is a no-op; rows beyond the end raise."""
    from nesti_net_amd.provider import CloudPatches
    c = fx.cloud("ellipsoid")
    cp = CloudPatches(c["pts"], c["cfg"], device=gpu_device)
    M, S = cp.patch_count, c["cfg"].n_scales
    whole = cp.quadric(0, M)
    parts = (torch.full((M, S, 3), 7.0, device=gpu_device), torch.full((M, S, 2), 7.0, device=gpu_device),
             torch.full((M, S, 3), 7.0, device=gpu_device), torch.full((M, S), 7, dtype=torch.int32, device=gpu_device))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)]
    for i, (a, b) in enumerate(((0, 1), (1, 1000), (1000, M))):
        cp.quadric(a, b - a, out=tuple(t[a:b] for t in parts), stream=streams[i % 2])
    cp.quadric(500, 0, out=tuple(t[500:500] for t in parts), stream=streams[0])
    empty = cp.quadric(M, 0)
    assert [tuple(t.shape) for t in empty] == [(0, S, 3), (0, S, 2), (0, S, 3), (0, S)]
    torch.cuda.synchronize()
    for a, b in zip(whole, parts):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        cp.quadric(M - 1, 2)
    with pytest.raises(ValueError):
        cp.quadric(0, 1, out=parts[:3])


def _check_oriented(res, want, s):
    """normals = the orientation restatement of the call's own unoriented rows; curv follows the flip rule; failed rows stay zero."""
    unoriented, c = res["normals_all"][:, s], res["curv_all"][:, s]
    assert np.array_equal(_bits(res["normals"]), _bits(want["out"])) and res["orient"] == want["stats"]
    assert np.array_equal(np.abs(res["normals"]), np.abs(unoriented))                     # only sign bits changed
    flipped = (_bits(res["normals"]) != _bits(unoriented)).any(axis=1)
    expect = np.where(flipped[:, None], -c[:, ::-1], c)
    assert np.array_equal(_bits(res["curv"]), _bits(expect))
    zero = (unoriented == 0).all(axis=1)
    assert not _bits(res["normals"])[zero].any() and not _bits(res["curv"])[zero].any() and not flipped[zero].any()
    return flipped, zero


def test_composition_with_orientation(gpu_device):
    """``quadric_fit(orient='mst')`` at the largest scale equals the orientation restatement fed with the call's own unoriented
    normals, every bit and the stats; the curvatures of a turned row are (-k_min, -k_max) of its unoriented ones, bit for bit, and
    every other row's are unchanged.  ``orient='viewpoint'`` likewise, at the middle scale."""
    from nesti_net_amd import quadric
    c = fx.cloud("ellipsoid")
    K = 8
    plain = quadric.quadric_fit(c["pts"], c["cfg"], device=str(gpu_device))
    assert plain["orient"] is None and np.array_equal(_bits(plain["normals"]), _bits(plain["normals_all"][:, -1]))
    assert np.array_equal(_bits(plain["curv"]), _bits(plain["curv_all"][:, -1]))
    assert plain["curv"].shape == (len(c["pts"]), 2) and plain["plane_all"].shape == plain["normals_all"].shape
    res = quadric.quadric_fit(c["pts"], c["cfg"], orient="mst", orient_k=K, device=str(gpu_device))
    assert np.array_equal(plain["n_ball"], res["n_ball"])
    want = OF.orient(c["pts"], res["normals_all"][:, -1], c["r_abs"][-1], K)
    flipped, zero = _check_oriented(res, want, -1)
    assert flipped.any() and not flipped.all()                            # both branches of the flip rule are exercised
    H, Kg = quadric.mean_gauss(res["curv"])
    print("ellipsoid, quadric fit + mst at r = %.4g, K = %d: %s; %d of %d oriented normals point inward; mean curvature of the oriented "
          "rows in [%.3g, %.3g], Gauss curvature in [%.3g, %.3g]"
          % (c["r_abs"][-1], K, res["orient"], OF.inward(res["normals"], c["gt"], res["normals_all"][:, -1]), int((~zero).sum()),
             H[~zero].min(), H[~zero].max(), Kg[~zero].min(), Kg[~zero].max()))
    vp = quadric.quadric_fit(c["pts"], c["cfg"], scale=1, orient="viewpoint", viewpoint=(0.0, 0.0, 9.0), device=str(gpu_device))
    want = OF.orient_viewpoint(c["pts"], vp["normals_all"][:, 1], (0.0, 0.0, 9.0))
    _check_oriented(vp, want, 1)


def test_command_line(tmp_path, gpu_device):
    """``--estimator quadric --sparse_patches 1 --orient mst --quadric_scale 1`` on two shapes with no model file anywhere: the four
    files per shape equal what the Python call returns, written through the same writers; no .experts file appears.  (The command and the
    call build two grids, which may order the points inside a cell differently: a float64 sum may then differ in its last bits, and an
    f32 result only where its rounding boundary lies within ~1e-16 relative of the value -- about 2e-9 per value.)"""
    from nesti_net_amd import quadric, textio
    from nesti_net_amd.cli import main
    from nesti_net_amd.config import NestiConfig
    d = tmp_path / "data"
    d.mkdir()
    shapes = {"ell": (fx.cloud("ellipsoid")["pts"], np.arange(0, 4000, 5)), "box": (fx.cloud("box")["pts"], np.arange(3, 6000, 11))}
    for name, (pts, pidx) in shapes.items():
        np.savetxt(d / (name + ".xyz"), pts.astype(np.float64))
        np.savetxt(d / (name + ".pidx"), pidx, fmt="%d")
    (d / "testset.txt").write_text("ell\nbox\n")
    results = str(tmp_path / "res")
    assert main(["--estimator", "quadric", "--results_path", results, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep,
                 "--testset", "testset.txt", "--sparse_patches", "1", "--orient", "mst", "--quadric_scale", "1"]) == 0
    out = os.path.join(results, "synth_results")
    exts = (".normals", ".curv", ".quadric_curv", ".quadric_count")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + [n + e for n in shapes for e in exts])
    S = NestiConfig().n_scales
    for name, (pts, pidx) in shapes.items():
        pts32 = np.loadtxt(d / (name + ".xyz")).astype("float32")
        res = quadric.quadric_fit(pts32, NestiConfig(), pidx=pidx, scale=1, orient="mst", device=str(gpu_device))
        want = str(tmp_path / "want")
        textio.write_f32(want + ".normals", res["normals"])
        textio.write_f32(want + ".curv", res["curv"])
        textio.write_f32(want + ".quadric_curv", res["curv_all"].reshape(len(pidx), -1))
        textio.write_i32_rows(want + ".quadric_count", res["n_ball"])
        for e in exts:
            assert open(os.path.join(out, name + e), "rb").read() == open(want + e, "rb").read(), (name, e)
        assert np.array_equal(np.loadtxt(os.path.join(out, name + ".quadric_count"), dtype=np.int64), res["n_ball"])
        assert np.loadtxt(os.path.join(out, name + ".curv")).shape == (len(pidx), 2)
        assert np.loadtxt(os.path.join(out, name + ".quadric_curv")).shape == (len(pidx), 2 * S)
    log = open(os.path.join(out, "log.txt")).read()
    assert "orientation of ell (mst)" in log and "Model restored" not in log
