"""Plane-fit normals on the GPU (csrc/pca.hip, ``CloudPatches.pca``, ``pca.pca_normals``, ``--estimator pca``) against the tests' own
numpy restatement (tests/_pca_fixture.py): ball sizes integer for integer, sentinel rows byte for byte, and directions, residuals and
eigenvalues to bounds that come from the arithmetic, not from what the kernel gives.

Notation: n the ball size, w the restatement's float64 eigenvalues in r^2 units, eps = 2^-53.
  direction    per row with n >= 3: bound = 2^-22 + 16 n eps / (w1 - w0) -- the f32 rounding of a unit vector, and Davis-Kahan with
               ||E|| <= 4 n eps for each of the two summations.  A row is ill-conditioned iff bound > 1e-3; every other row has
               |sin(angle to the restatement's normal)| <= bound
  residual     every row with n >= 3: with C the restatement's matrix and nu the GPU normal, rho(nu) - w0 <= 2^-40 w2 + 16 n eps and
               | |nu| - 1 | <= 2^-22.  rho is the Rayleigh quotient nu^T C nu / nu^T nu: the bound is a statement about the direction
               (an angle delta costs at most delta^2 w2), and the length of the f32 vector, which alone would move nu^T C nu by
               2^-23 w0, is held by the second inequality
  eigenvalues  |w_k(gpu) - w_k| <= 2^-23 w_k + 8 n eps, ascending

Every cloud here has three radii: this module runs ``pca_kernel<3>``.  S = 1, 2 and 4: tests/test_gpu_fit_scales.py."""
import os

import numpy as np
import pytest
import torch

import _orient_fixture as OF
import _pca_fixture as fx

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SURFACES = ("ellipsoid", "box", "torus", "sphere_big")


def _np(ts):
    return [t.cpu().numpy() for t in ts]


_gpu = {}


def _run(name, dev):
    """(normals, eig, n_ball) of a fixture's rows on the GPU (index queries; all points where the rows are all points), once."""
    if name not in _gpu:
        from nesti_net_amd.provider import CloudPatches
        c = fx.cloud(name)
        every = len(c["rows"]) == len(c["pts"])
        cp = CloudPatches(c["pts"], c["cfg"], device=dev, pidx=None if every else c["rows"])
        assert cp.r_abs == c["r_abs"]
        out = _np(cp.pca(0, cp.patch_count))
        counts = cp.count_balls(0, cp.patch_count).cpu().numpy()
        _gpu[name] = (out, counts)
    return _gpu[name]


def check(got, ref, label, allow_excluded=None):
    """Assertions 1 - 6 of the module docstring on (normals, eig, n_ball) against a ``restate`` dict.  ``allow_excluded``: the boolean
    [M,S] mask of rows that may be ill-conditioned (None: none may be).  Prints each figure before it asserts."""
    normals, eig, n_ball = got
    assert np.array_equal(n_ball, ref["n_ball"]), label                                               # 1
    live = ref["n_ball"] >= 3
    assert not normals[~live].view(np.uint32).any() and not eig[~live].view(np.uint32).any(), label   # 2: sentinel bytes
    assert (normals[live] != 0).any(axis=-1).all(), label
    n = ref["n_ball"][live].astype(np.float64)
    w, C = ref["w"][live], ref["C"][live]
    g = normals[live].astype(np.float64)
    r = ref["normals"][live].astype(np.float64)
    with np.errstate(divide="ignore"):
        bound = 2.0 ** -22 + 16 * n * EPS / (w[:, 1] - w[:, 0])
    ill = ~(bound <= 1e-3)
    allowed = np.zeros(len(n), bool) if allow_excluded is None else allow_excluded[live]
    sin = np.linalg.norm(np.cross(g, r), axis=1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(r, axis=1))
    length = np.linalg.norm(g, axis=1)
    rho = np.einsum("ni,nij,nj->n", g, C, g) / (length * length)
    res_bound = 2.0 ** -40 * w[:, 2] + 16 * n * EPS
    ge = eig[live].astype(np.float64)
    eig_bound = 2.0 ** -23 * w + 8 * n[:, None] * EPS
    lead = np.where(g[:, 2] != 0, g[:, 2], np.where(g[:, 1] != 0, g[:, 1], g[:, 0]))
    print("%s: %d live of %d (row, scale) pairs, %d ill-conditioned; smallest gap w1 - w0 of the others %.3g; largest sin / bound %.3g, "
          "(rho - w0) / bound %.3g, | |nu| - 1 | %.3g, eigenvalue error / bound %.3g"
          % (label, live.sum(), live.size, ill.sum(), (w[~ill, 1] - w[~ill, 0]).min() if (~ill).any() else np.nan,
             (sin[~ill] / bound[~ill]).max() if (~ill).any() else 0.0, ((rho - w[:, 0]) / res_bound).max(), np.abs(length - 1).max(),
             (np.abs(ge - w) / eig_bound).max()))
    assert np.array_equal(ill, ill & allowed), "%s: %d rows ill-conditioned where none may be" % (label, (ill & ~allowed).sum())    # 3
    assert (sin[~ill] <= bound[~ill]).all(), label
    assert (rho - w[:, 0] <= res_bound).all() and (np.abs(length - 1) <= 2.0 ** -22).all(), label                                      # 4
    assert (np.abs(ge - w) <= eig_bound).all() and (np.diff(ge, axis=1) >= 0).all(), label                                             # 5
    assert (lead > 0).all(), label                                                                                                     # 6
    return ill, live


@pytest.mark.parametrize("name", SURFACES)
def test_surfaces_against_the_restatement(name, gpu_device):
    """The four surface clouds: the sentinel path interleaved with live rows (ellipsoid: 60 % of the rows at the smallest scale),
    edges and corners (box), noise (torus), balls of ~150 / 600 / 2 400 points -- above P and kListCap, many trips per lane (sphere).
    No row may be excluded as ill-conditioned."""
    c, ref = fx.cloud(name), fx.predicted(name)
    got, counts = _run(name, gpu_device)
    assert np.array_equal(got[2], counts)                       # ... and equal to nesti_patches_count's
    check(got, ref, name)
    if name == "ellipsoid":
        short = (ref["n_ball"][:, 0] < 3).mean()
        assert 0.5 < short < 0.7 and 10 < ref["n_ball"][:, 1].mean() < 16
    if name == "sphere_big":
        assert ref["n_ball"][:, 2].min() > 1024 and ref["n_ball"][:, 1].mean() > 512 and ref["n_ball"][:, 0].mean() > 100
    if c["gt"] is not None:
        print("%s: RMS angle to the analytic normals per scale, degrees: %s"
              % (name, [round(fx.angle_rms_deg(got[0][:, s], c["gt"][c["rows"]]), 3) for s in range(got[0].shape[1])]))


def test_lattice(gpu_device):
    """Ties, duplicates and exact degeneracy: on the grid rows the normal is exactly (0, 0, 1) and w0 exactly 0 (every moment with a z
    factor is an exact zero and no rotation touches it); exactly the collinear rows are ill-conditioned."""
    c, ref = fx.cloud("lattice"), fx.predicted("lattice")
    got, counts = _run("lattice", gpu_device)
    assert np.array_equal(got[2], counts)
    line = np.zeros(ref["n_ball"].shape, bool)
    line[fx.LATTICE_PLANE_ROWS:] = True
    ill, live = check(got, ref, "lattice", allow_excluded=line)
    assert np.array_equal(ill, line[live])                      # the collinear rows, all of them, and nothing else
    plane = live.copy()
    plane[fx.LATTICE_PLANE_ROWS:] = False
    assert plane.sum() > 3000
    assert (got[0][plane] == np.array([0, 0, 1], np.float32)).all() and (got[1][plane][:, 0] == 0).all()
    assert (got[1][plane][:, 1] > 0).all()


def test_query_kinds(gpu_device):
    """pidx rows and positions equal to them give the bits of the all-points call on ONE grid; positions off the surface are held to
    the restatement; far, NaN and infinite positions are sentinel rows."""
    from nesti_net_amd.provider import CloudPatches
    c = fx.cloud("ellipsoid")
    pts, cfg = c["pts"], c["cfg"]
    every, _ = _run("ellipsoid", gpu_device)
    cp = CloudPatches(pts, cfg, device=gpu_device)
    full = cp.pca(0, cp.patch_count)
    pidx = np.arange(0, len(pts), 7)
    # one grid: the same object serves the three kinds (the grid belongs to the cloud, the queries are per call)
    cp.pidx, cp.patch_count = torch.as_tensor(pidx, dtype=torch.int32, device=gpu_device), len(pidx)
    by_index = cp.pca(0, len(pidx))
    cp.pidx, cp.queries = None, torch.from_numpy(pts[pidx]).to(gpu_device)
    by_position = cp.pca(0, len(pidx))
    for a, b, d in zip(full, by_index, by_position):
        assert torch.equal(a[pidx.tolist()].view(torch.int32), b.view(torch.int32))
        assert torch.equal(b.view(torch.int32), d.view(torch.int32))
    assert np.array_equal(_np(full)[2], every[2])                # another grid build: the counts are equal (the rest: to the bounds)
    # positions 0.5 r off the surface along the analytic normal, then far outside, NaN, inf
    off = (pts[pidx].astype(np.float64) + 0.5 * c["r_abs"][-1] * c["gt"][pidx].astype(np.float64)).astype(np.float32)
    lost = np.array([[50, 50, 50], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    q = np.concatenate([off, lost])
    cq = CloudPatches(pts, cfg, device=gpu_device, queries=torch.from_numpy(q))
    got = _np(cq.pca(0, len(q)))
    ref = fx.restate(pts, q, c["r_abs"])
    assert (ref["n_ball"][len(off):] == 0).all() and (ref["n_ball"][:len(off), 2] >= 3).mean() > 0.9
    may = np.ones(ref["n_ball"].shape, bool)                    # a cap of a few points may be ill-conditioned; the rule decides
    check(got, ref, "off-surface positions", allow_excluded=may)
    assert not got[0][len(off):].view(np.uint32).any() and not got[1][len(off):].view(np.uint32).any() and not got[2][len(off):].any()


def test_partition(gpu_device):
    """Rows [0, M) in one call against [0, 1), [1, 1000), [1000, M) on two streams: identical bytes; count = 0 is a no-op."""
    from nesti_net_amd.provider import CloudPatches
    c = fx.cloud("ellipsoid")
    cp = CloudPatches(c["pts"], c["cfg"], device=gpu_device)
    M, S = cp.patch_count, c["cfg"].n_scales
    whole = cp.pca(0, M)
    parts = (torch.full((M, S, 3), 7.0, device=gpu_device), torch.full((M, S, 3), 7.0, device=gpu_device),
             torch.full((M, S), 7, dtype=torch.int32, device=gpu_device))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)]
    for i, (a, b) in enumerate(((0, 1), (1, 1000), (1000, M))):
        cp.pca(a, b - a, out=tuple(t[a:b] for t in parts), stream=streams[i % 2])
    cp.pca(500, 0, out=tuple(t[500:500] for t in parts), stream=streams[0])
    empty = cp.pca(M, 0)
    assert [tuple(t.shape) for t in empty] == [(0, S, 3), (0, S, 3), (0, S)]
    torch.cuda.synchronize()
    for a, b in zip(whole, parts):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        cp.pca(M - 1, 2)


def test_composition_with_orientation(gpu_device):
    """``pca_normals(orient='mst')`` at the largest scale equals the orientation restatement fed with the unoriented GPU normals:
    every bit and the stats.  The first time the orientation pass sees real geometry: the inward count is printed, not asserted."""
    from nesti_net_amd import pca
    c = fx.cloud("ellipsoid")
    K = 8
    plain = pca.pca_normals(c["pts"], c["cfg"], device=str(gpu_device))
    res = pca.pca_normals(c["pts"], c["cfg"], orient="mst", orient_k=K, device=str(gpu_device))
    assert plain["orient"] is None and np.array_equal(plain["normals"], plain["normals_all"][:, -1])
    assert np.array_equal(plain["n_ball"], res["n_ball"]) and np.array_equal(plain["n_ball"], fx.predicted("ellipsoid")["n_ball"])
    assert np.array_equal(res["variation"], fx.variation(res["eig"])) and res["variation"].shape == res["n_ball"].shape
    # the orientation works on res's own unoriented rows (another grid build than plain's: equal only to the documented bounds)
    unoriented = res["normals_all"][:, -1]
    want = OF.orient(c["pts"], unoriented, c["r_abs"][-1], K)
    assert np.array_equal(res["normals"].view(np.uint32), want["out"].view(np.uint32))
    assert res["orient"] == want["stats"]
    assert np.array_equal(np.abs(res["normals"]), np.abs(unoriented))                     # only sign bits changed
    zero = (unoriented == 0).all(axis=1)
    assert not res["normals"][zero].view(np.uint32).any()
    print("ellipsoid, plane fit + mst at r = %.4g, K = %d: %s; %d of %d oriented normals point inward"
          % (c["r_abs"][-1], K, res["orient"], OF.inward(res["normals"], c["gt"], unoriented), int((~zero).sum())))
    vp = pca.pca_normals(c["pts"], c["cfg"], scale=1, orient="viewpoint", viewpoint=(0.0, 0.0, 9.0), device=str(gpu_device))
    want = OF.orient_viewpoint(c["pts"], vp["normals_all"][:, 1], (0.0, 0.0, 9.0))
    assert np.array_equal(vp["normals"].view(np.uint32), want["out"].view(np.uint32)) and vp["orient"] == want["stats"]


def test_command_line(tmp_path, gpu_device):
    """``--estimator pca --sparse_patches 1 --orient mst`` on two shapes with no model file anywhere: the three files per shape equal
    what the Python call returns, written through the same writers; no .experts file appears.  (The command and the call build two grids,
    which may order the points inside a cell differently: a float64 sum may then differ in its last bits, and an f32 result only where
    its rounding boundary lies within ~1e-16 relative of the value -- about 2e-9 per value.)"""
    from nesti_net_amd import pca, textio
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
    assert main(["--estimator", "pca", "--results_path", results, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep,
                 "--testset", "testset.txt", "--sparse_patches", "1", "--orient", "mst", "--pca_scale", "1"]) == 0
    out = os.path.join(results, "synth_results")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + [n + e for n in shapes for e in (".normals", ".pca_eig", ".pca_count")])
    for name, (pts, pidx) in shapes.items():
        pts32 = np.loadtxt(d / (name + ".xyz")).astype("float32")
        res = pca.pca_normals(pts32, NestiConfig(), pidx=pidx, scale=1, orient="mst", device=str(gpu_device))
        want = tmp_path / "want"
        textio.write_i32_rows(str(want) + ".count", res["n_ball"])
        assert open(os.path.join(out, name + ".pca_count"), "rb").read() == open(str(want) + ".count", "rb").read()
        assert np.array_equal(np.loadtxt(os.path.join(out, name + ".pca_count"), dtype=np.int64), res["n_ball"])
        textio.write_f32(str(want) + ".normals", res["normals"])
        textio.write_f32(str(want) + ".eig", res["eig"].reshape(len(pidx), -1))
        assert open(os.path.join(out, name + ".normals"), "rb").read() == open(str(want) + ".normals", "rb").read()
        assert open(os.path.join(out, name + ".pca_eig"), "rb").read() == open(str(want) + ".eig", "rb").read()
        assert np.loadtxt(os.path.join(out, name + ".pca_eig")).shape == (len(pidx), 9)
    log = open(os.path.join(out, "log.txt")).read()
    assert "orientation of ell (mst)" in log and "Model restored" not in log
