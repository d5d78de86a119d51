"""k-nearest neighbourhoods on the GPU (csrc/knn.hip, ``CloudPatches.knn`` / ``pca_knn`` / ``quadric_knn``, ``knn.knn``,
``pca.pca_normals(knn=)``, ``quadric.quadric_fit(knn=)``, ``--knn``) against the tests' own numpy restatement (tests/_knn_fixture.py).

The SEARCH is exact: indices ``array_equal``, d2 equal on the uint64 bits, on every case of tests/_grid_fixture.py.  The FITS are held
to the bounds of tests/test_gpu_pca.py (its ``check``, with n = k_s and eigenvalues in units of the neighbourhood's own r2_s) and of
tests/test_gpu_quadric.py (restated in ``_quadric_check`` because the radius is per row here):
    B = 16 n eps kappa_2(N) (||a||_2 + 1);  a pair with n >= 6 is ILL-CONDITIONED iff not B <= 1e-6;  every other pair is live and has
    | |nu| - 1 | <= 2^-22,  sin(angle(nu, nu_ref)) <= 2^-22 + 2 B,  r |k - k_ref| <= 2^-23 r |k_ref| + 8 (1 + ||a||_2) B,  nu . n0 > 0.
The ill-conditioned share of a scale may not exceed 1 %, as in the radius test (computed on the CPU from the restatement: it is 0 at
every k on both clouds; the largest kappa is 1.3e6, at k = 8 on the clean torus).

The fits are held to the restatement at three counts (``pca_nbr_kernel<3>``, ``quadric_nbr_kernel<3>``); one count runs through the
prefix property (test 7), the Python layer (test 11) and the sphere (test 9), two counts only on sentinel rows (test 2) and on the
command line (test 11), four never.  S = 1, 2 and 4 of both kernels against the restatement: tests/test_gpu_fit_scales.py."""
import os

import numpy as np
import pytest
import torch

import _grid_fixture as gx
import _knn_fixture as kx
import _pca_fixture as fx
import _quadric_fixture as qx
from test_gpu_pca import check as plane_check

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
KS = (8, 32, 128)
LOST = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e6, 1e6, 1e6]], np.float32)      # counts 0, 0, K


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _b32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


_clouds = {}


def _grid_cloud(name, dev):
    """(index-query cloud over the case's rows, position-query cloud over its positions + LOST) of a grid case, prepared once."""
    if name not in _clouds:
        from nesti_net_amd.provider import CloudPatches
        c = gx.case(name)
        pos = np.concatenate([c["positions"], LOST]) if "positions" in c else LOST
        _clouds[name] = (CloudPatches(c["pts"], c["cfg"], device=dev, pidx=c["rows"]),
                         CloudPatches(c["pts"], c["cfg"], device=dev, queries=torch.from_numpy(pos)), pos)
    return _clouds[name]


@pytest.mark.parametrize("K", [1, 17, 128])
@pytest.mark.parametrize("name", gx.CASES)
def test_search_is_exact_on_every_grid_case(name, K, gpu_device):
    """1.  Rows and positions of every grid case over the case's OWN radius grid: ties at the K-th distance (lattices, duplicates), a cell
    above any buffer (duplicates), answers many cells away across empty cells (plate, needle_diag), a 127 x 1 x 1 grid, coordinates near
    2 000, positions outside the bounding box; a NaN, a +inf and a position 10^6 away have counts 0, 0, K."""
    c = gx.case(name)
    by_index, by_position, pos = _grid_cloud(name, gpu_device)
    for label, cp, centres in (("rows", by_index, c["pts"][c["rows"]]), ("positions", by_position, pos)):
        ref = kx.searched((name, label), c["pts"], centres, 128)
        idx, d2, n = _np(cp.knn(0, cp.patch_count, K, grid="radius"))
        assert idx.shape == (len(centres), K) and idx.dtype == np.int32 and d2.dtype == np.float64
        assert np.array_equal(idx, ref[0][:, :K]), (name, label)
        assert np.array_equal(d2.view(np.uint64), ref[1][:, :K].view(np.uint64)), (name, label)
        assert np.array_equal(n, np.minimum(ref[2], K)), (name, label)
    assert n[-3:].tolist() == [0, 0, K] and (idx[-3:-1] == -1).all() and np.isinf(d2[-3:-1]).all()
    if K == 128:                                                             # the properties that make the cases bite, from K = 129
        d2 = kx.searched((name, "rows", 129), c["pts"], c["pts"][c["rows"]], 129)[1]
        tie, zero = int((d2[:, 127] == d2[:, 128]).sum()), int((d2[:, 127] == 0).sum())
        print("%s: %d rows, %d tie at the K-th distance, %d have r_K = 0" % (name, len(d2), tie, zero))
        if name.startswith("lattice"):
            assert tie == len(c["rows"]) == 303                              # all of them tie at the K-th distance
        if name == "duplicates":
            assert tie == 68 and zero == 62                                  # the 1 500-fold point: one cell above any buffer


def _grid_dims(ws):
    """dims[3] of the GridHeader at the start of a grid workspace (csrc/patches_dev.h: three doubles, a double, three ints)."""
    return ws[32:44].cpu().numpy().view(np.int32).tolist()


def test_small_clouds(gpu_device):
    """2.  N = 1 and N = 5 with K = 8: -1 / +inf padding, count = N; the cloud point is its own first neighbour."""
    from nesti_net_amd import knn
    rs = np.random.RandomState(3)
    for N in (1, 5):
        pts = rs.uniform(size=(N, 3)).astype(np.float32)
        q = rs.uniform(-1, 2, size=(4, 3)).astype(np.float32)
        for kw, centres in (({}, pts), ({"queries": q}, q)):
            got = knn.knn(pts, 8, device=str(gpu_device), **kw)
            ref = kx.search(pts, centres, 8)
            assert sorted(got) == ["count", "d2", "idx"]
            assert np.array_equal(got["idx"], ref[0]) and np.array_equal(got["d2"].view(np.uint64), ref[1].view(np.uint64))
            assert (got["count"] == N).all() and (got["idx"][:, N:] == -1).all() and np.isinf(got["d2"][:, N:]).all()
        assert np.array_equal(knn.knn(pts, 8, device=str(gpu_device))["idx"][:, 0], np.arange(N))
    # a cloud without extent is served by the fits too: one point, fewer than 3 neighbours, the sentinel
    from nesti_net_amd import pca, quadric
    one = np.array([[0.25, -1.0, 3.0]], np.float32)
    res = pca.pca_normals(one, knn=(2, 8), device=str(gpu_device))
    assert not res["normals_all"].view(np.uint32).any() and not res["radius"].view(np.uint32).any() and res["n_ball"].tolist() == [[1, 1]]
    res = quadric.quadric_fit(one, knn=8, device=str(gpu_device))
    assert not res["normals"].view(np.uint32).any() and not res["curv"].view(np.uint32).any() and res["n_ball"].tolist() == [[1]]


_ell = {}


def _ellipsoid(dev):
    """The ellipsoid (4 000 points, all rows) prepared once: (cloud, (idx, d2, n) at K = 128, plane fit and quadric fit at KS)."""
    if not _ell:
        from nesti_net_amd.provider import CloudPatches
        c = fx.cloud("ellipsoid")
        cp = CloudPatches(c["pts"], c["cfg"], device=dev)
        _ell["cp"] = cp
        _ell["search"] = _np(cp.knn(0, cp.patch_count, 128))
        _ell["plane"] = _np(cp.pca_knn(0, cp.patch_count, KS))
        _ell["quadric"] = _np(cp.quadric_knn(0, cp.patch_count, KS))
    return _ell


def test_grid_independence(gpu_device):
    """3.  The default k-NN grid, the cloud's radius grid and a 1 x 1 x 1 grid (pseudo-radius above the bounding-box diagonal: the whole
    cloud in one cell): identical bytes for idx, d2, and the fitted normals, eigenvalues, radii and curvatures."""
    e = _ellipsoid(gpu_device)
    cp = e["cp"]
    ref = kx.searched(("ellipsoid", "all"), cp.host_pts, cp.host_pts, 128)
    assert np.array_equal(e["search"][0], ref[0]) and np.array_equal(e["search"][1].view(np.uint64), ref[1].view(np.uint64))
    st = torch.cuda.current_stream(gpu_device)
    assert _grid_dims(cp.knn_grid(2.0 * cp.bbdiag, 128, st)) == [1, 1, 1]               # the whole cloud in one cell
    assert min(_grid_dims(cp.knn_grid(None, 128, st))) > 1 and min(_grid_dims(cp.knn_grid("radius", 128, st))) > 1
    for grid in ("radius", 2.0 * cp.bbdiag):
        for a, b in zip(e["search"], _np(cp.knn(0, cp.patch_count, 128, grid=grid))):
            assert _same_bytes(a, b), grid
        for a, b in zip(e["plane"], _np(cp.pca_knn(0, cp.patch_count, KS, grid=grid))):
            assert _same_bytes(a, b), grid
        for a, b in zip(e["quadric"], _np(cp.quadric_knn(0, cp.patch_count, KS, grid=grid))):
            assert _same_bytes(a, b), grid
    # ... and of the grid BUILD: another cloud object, another build of the default grid
    from nesti_net_amd.provider import CloudPatches
    again = CloudPatches(cp.host_pts, cp.cfg, device=gpu_device)
    for a, b in zip(e["plane"], _np(again.pca_knn(0, again.patch_count, KS))):
        assert _same_bytes(a, b)


@pytest.mark.parametrize("batch", [7, 64, 1000])
def test_batching(batch, gpu_device):
    """4.  One call against batches of 7, 64 and 1 000 rows: identical bytes of the search and of both fits."""
    e = _ellipsoid(gpu_device)
    cp = e["cp"]
    M = cp.patch_count
    parts = {"search": [], "plane": [], "quadric": []}
    for first in range(0, M, batch):
        n = min(batch, M - first)
        parts["search"].append(cp.knn(first, n, 128))
        parts["plane"].append(cp.pca_knn(first, n, KS))
        parts["quadric"].append(cp.quadric_knn(first, n, KS))
    for key, chunks in parts.items():
        for a, b in zip(e[key], zip(*chunks)):
            assert _same_bytes(a, torch.cat(b).cpu().numpy()), (key, batch)
    assert [tuple(t.shape) for t in cp.pca_knn(M, 0, KS)] == [(0, 3, 3), (0, 3, 3), (0, 3), (0, 3)]      # count = 0 is a no-op
    with pytest.raises(ValueError):
        cp.knn(M - 1, 2, 8)


def _plane_case(name, dev):
    from nesti_net_amd.provider import CloudPatches
    c = fx.cloud(name)
    if name == "ellipsoid":
        got = _ellipsoid(dev)["plane"]
    else:
        every = len(c["rows"]) == len(c["pts"])
        cp = CloudPatches(c["pts"], c["cfg"], device=dev, pidx=None if every else c["rows"])
        got = _np(cp.pca_knn(0, cp.patch_count, KS))
    centres = c["pts"][c["rows"]]
    nbr = kx.searched((name, "plane"), c["pts"], centres, 128)[0]
    return c, got, nbr, kx.plane_lists(c["pts"], centres, nbr, KS)


@pytest.mark.parametrize("name", ["ellipsoid", "torus", "box"])
def test_plane_fit_over_lists(name, gpu_device):
    """5.  ks = (8, 32, 128) against the restatement with the bounds of tests/test_gpu_pca.py and n = k_s.  No row may be excluded as
    ill-conditioned (computed on the CPU from the restatement: the smallest gap w1 - w0 is 3.7e-3)."""
    c, got, nbr, ref = _plane_case(name, gpu_device)
    normals, eig, radius, n = got
    plane_check((normals, eig, n), ref, name + " knn")
    assert (n == np.array(KS)).all() and np.array_equal(_b32(radius), _b32(ref["radius"]))
    assert (ref["w"][..., 1] - ref["w"][..., 0]).min() > 1e-3
    print("%s: RMS angle to the analytic normals per k, degrees: %s"
          % (name, [round(fx.angle_rms_deg(normals[:, s], c["gt"][c["rows"]]), 3) for s in range(len(KS))]))


def test_plane_fit_on_the_lattice(gpu_device):
    """5.  ``_pca_fixture.lattice()``: the excluded rows are exactly those whose prefix lies on the collinear line -- 200 / 200 / 113
    rows at the three scales; the other 87 line rows reach the plane 21 units away at k = 128.  At k = 8 and k = 32 1 800+ rows tie at
    the k-th neighbour (1 662 at k = 128); the result still matches."""
    c, got, nbr, ref = _plane_case("lattice", gpu_device)
    normals, eig, radius, n = got
    P = fx.LATTICE_PLANE_ROWS
    on_line = np.stack([(nbr[:, :k] >= P).all(axis=1) for k in KS], 1)
    assert on_line.sum(0).tolist() == [200, 200, 113] and not on_line[:P].any()
    d2 = kx.search(c["pts"], c["pts"], 129)[1]
    ties = [int((d2[:, k - 1] == d2[:, k]).sum()) for k in KS]               # the k-th distance is also the (k + 1)-th: 1800, 1841, 1662
    print("lattice: rows whose k-th and (k + 1)-th neighbours are equally far, per k: %s of %d" % (ties, len(d2)))
    assert ties[0] >= 1800 and ties[1] >= 1800 and ties[2] >= 1600
    ill, live = plane_check((normals, eig, n), ref, "lattice knn", allow_excluded=on_line)
    assert live.all() and np.array_equal(ill, on_line[live])
    assert np.array_equal(_b32(radius), _b32(ref["radius"]))
    plane = ~on_line
    plane[P:] &= False                                                        # line rows that reach the plane are tilted, not (0, 0, 1)
    assert (normals[plane] == np.array([0, 0, 1], np.float32)).all() and (eig[plane][:, 0] == 0).all()


def test_sentinels(gpu_device):
    """6.  The heavy rows of ``duplicates`` (one point 1 500 times) with ks = (4, 128, 256): every neighbour coincides with the centre,
    r2_s = 0: normal and eigenvalues all-zero bytes, radius 0, count = k_s; the quadric fit fails."""
    from nesti_net_amd.provider import CloudPatches
    c = gx.case("duplicates")
    heavy = c["heavy"][:16]
    cp = CloudPatches(c["pts"], c["cfg"], device=gpu_device, pidx=heavy)
    ks = (4, 128, 256)
    normals, eig, radius, n = _np(cp.pca_knn(0, len(heavy), ks))
    assert not _b32(normals).any() and not _b32(eig).any() and not _b32(radius).any() and (n == np.array(ks)).all()
    qn, qc, qp, qr, qcount = _np(cp.quadric_knn(0, len(heavy), ks))
    assert not _b32(qn).any() and not _b32(qc).any() and not _b32(qp).any() and not _b32(qr).any() and (qcount == np.array(ks)).all()
    idx, d2, _ = _np(cp.knn(0, len(heavy), 256))
    assert not d2.view(np.uint64).any() and (np.diff(idx, axis=1) > 0).all()            # 256 copies, ordered by index
    assert np.array_equal(idx[0], np.sort(c["heavy"])[:256])


def test_prefix_property(gpu_device):
    """7.  Scale 1 of ks = (8, 32, 128) equals, byte for byte, the single scale of a separate run with knn = 32."""
    e = _ellipsoid(gpu_device)
    cp = e["cp"]
    for key, single in (("plane", cp.pca_knn(0, cp.patch_count, 32)), ("quadric", cp.quadric_knn(0, cp.patch_count, (32,)))):
        for a, b in zip(e[key], _np(single)):
            assert b.shape[1] == 1 and _same_bytes(np.ascontiguousarray(a[:, 1:2]), b), key


def test_user_lists(gpu_device):
    """8.  Lists that do not come from the search: shuffled (r2 is the maximum, not the last), an out-of-range entry in the middle (the
    prefix ends there), an all -1 row, a non-finite position.  Against the restatement; any of these small or arbitrary subsets may be
    ill-conditioned, the rule decides."""
    from nesti_net_amd.provider import CloudPatches
    c = fx.cloud("ellipsoid")
    pts = c["pts"]
    rows = np.arange(0, len(pts), 50)
    ks = (8, 20, 32)
    nbr = kx.searched(("ellipsoid", "all"), pts, pts, 128)[0][rows, :32].copy()
    rs = np.random.RandomState(5)
    for i in range(len(nbr)):
        nbr[i] = nbr[i][rs.permutation(32)]
    nbr[3, 13] = len(pts)                 # the prefix ends at 13
    nbr[4, 5] = -7                        # ... at 5
    nbr[5, 0] = 2 ** 31 - 1               # ... at 0
    nbr[6, :] = -1
    nbr[7, 2] = -1                        # fewer than 3
    t = torch.from_numpy(nbr).to(gpu_device)
    cp = CloudPatches(pts, c["cfg"], device=gpu_device, pidx=rows)
    normals, eig, radius, n = _np(cp.pca_knn(0, len(rows), ks, nbr=t))
    ref = kx.plane_lists(pts, pts[rows], nbr, ks)
    assert n[3].tolist() == [8, 13, 13] and n[4].tolist() == [5, 5, 5] and n[5].tolist() == [0, 0, 0] and n[6].tolist() == [0, 0, 0]
    assert n[7].tolist() == [2, 2, 2] and (n[8:] == np.array(ks)).all()
    sentinel = (ref["n_ball"] < 3)
    assert sentinel[5:8].all() and not sentinel[8:].any()
    plane_check((normals, eig, n), ref, "user lists", allow_excluded=np.ones(n.shape, bool))
    assert np.array_equal(_b32(radius), _b32(ref["radius"]))
    last = np.sqrt(kx.d2_all(pts[nbr[8:, 31]].astype(np.float64) - pts[rows[8:]].astype(np.float64), 0.0)).astype(np.float32)
    assert (radius[8:, 2] >= last).all() and (radius[8:, 2] > last).any()       # the maximum, not the last entry
    qn, qc, qp, qr, qcount = _np(cp.quadric_knn(0, len(rows), ks, nbr=t))
    assert _same_bytes(qp, normals) and _same_bytes(qr, radius) and np.array_equal(qcount, n)
    _quadric_check((qn, qc, qp, qcount), kx.quadric_lists(pts, pts[rows], nbr, ks, qp), "user lists", cap_scales=())
    # positions as centres, one of them lost: an empty prefix whatever the list holds
    q = pts[rows].copy()
    q[9] = [np.nan, 0, 0]
    cq = CloudPatches(pts, c["cfg"], device=gpu_device, queries=torch.from_numpy(q))
    at = _np(cq.pca_knn(0, len(rows), ks, nbr=t))
    keep = np.arange(len(rows)) != 9
    for a, b in zip((normals, eig, radius, n), at):
        assert _same_bytes(a[keep], b[keep]) and not np.ascontiguousarray(b[9]).view(np.uint32).any()


def _quadric_check(got, ref, label, cap_scales, cap=0.01):
    """The assertions of tests/test_gpu_quadric.py's ``check`` on (normals, curv, plane, count) against ``quadric_lists`` computed FROM
    got's plane, with the per-row radius ref["r"].  ``cap_scales``: the scales whose ill-conditioned share may not exceed ``cap``."""
    normals, curv, plane, n = got
    assert np.array_equal(n, ref["n_ball"]), label
    for a in (normals, curv, plane):
        assert np.isfinite(a).all(), label
    short = n < 6
    assert not _b32(normals)[short].any() and not _b32(curv)[short].any(), label
    live = (normals != 0).any(axis=-1)
    assert not _b32(curv)[~live].any(), label
    B = qx.bound_B(ref)
    with np.errstate(invalid="ignore"):
        well = ~short & (B <= 1e-6)
    ill = ~short & ~well
    share = [ill[:, s].sum() / max(1, (~short[:, s]).sum()) for s in range(n.shape[1])]
    assert ref["ok"][well].all(), label
    g = normals[well].astype(np.float64)
    rn, a, b, r = ref["nu"][well], ref["a"][well], B[well], ref["r"][well]
    na = np.linalg.norm(a, axis=1)
    length = np.linalg.norm(g, axis=1)
    sin = np.linalg.norm(np.cross(g, rn), axis=1) / np.where(length > 0, length, 1.0)
    sin_bound = 2.0 ** -22 + 2 * b
    k, kr = curv[well].astype(np.float64), ref["k"][well]
    k_err = r[:, None] * np.abs(k - kr)
    k_bound = 2.0 ** -23 * r[:, None] * np.abs(kr) + (8 * (1 + na) * b)[:, None]
    side = (g * plane[well].astype(np.float64)).sum(1)
    print("%s: %d (row, scale) pairs, %d with n >= 6, ill-conditioned share per scale %s, %d live; largest B of the others %.3g; largest "
          "| |nu| - 1 | %.3g, sin / bound %.3g, curvature error / bound %.3g"
          % (label, n.size, (~short).sum(), ["%.4f" % x for x in share], live.sum(), b.max() if len(b) else 0.0,
             np.abs(length - 1).max() if len(b) else 0.0, (sin / sin_bound).max() if len(b) else 0.0,
             (k_err / k_bound).max() if len(b) else 0.0))
    assert live[well].all(), "%s: %d well-conditioned pairs are failed fits" % (label, (~live[well]).sum())
    assert (np.abs(length - 1) <= 2.0 ** -22).all(), label
    assert (sin <= sin_bound).all(), label
    assert (k_err <= k_bound).all(), label
    assert (curv[..., 0] >= curv[..., 1]).all(), label
    assert (side > 0).all(), label
    for s in cap_scales:
        assert share[s] <= cap, "%s: ill-conditioned share per scale %s" % (label, share)
    return live


@pytest.mark.parametrize("name", ["ellipsoid", "torus_clean"])
def test_quadric_over_lists(name, gpu_device):
    """9.  The bounds of tests/test_gpu_quadric.py against the list restatement on the ellipsoid and the clean torus; ``plane_out`` is
    byte-equal to the plane fit over the same lists."""
    from nesti_net_amd.provider import CloudPatches
    c = qx.cloud(name)
    pts, rows = c["pts"], c["rows"]
    cp = CloudPatches(pts, c["cfg"], device=gpu_device, pidx=rows)
    normals, curv, plane, radius, n = _np(cp.quadric_knn(0, len(rows), KS))
    pn, _, pr, pc = _np(cp.pca_knn(0, len(rows), KS))
    assert _same_bytes(plane, pn) and _same_bytes(radius, pr) and np.array_equal(n, pc)
    nbr = kx.searched((name, "quadric"), pts, pts[rows], 128)[0]
    ref = kx.quadric_lists(pts, pts[rows], nbr, KS, plane)
    live = _quadric_check((normals, curv, plane, n), ref, name + " knn", cap_scales=(0, 1, 2))
    assert all(live[:, s].mean() >= 0.95 for s in range(3))
    gt = c["gt"][rows]
    print("%s: RMS angle to the analytic normals per k, degrees: quadric fit %s, plane fit %s; live per scale %s"
          % (name, [round(fx.angle_rms_deg(normals[:, s], gt), 3) for s in range(3)],
             [round(fx.angle_rms_deg(plane[:, s], gt), 3) for s in range(3)], live.sum(0).tolist()))


def test_sphere_curvatures(gpu_device):
    """9.  The 20 000-point unit sphere at k = 128 (a cap of radius ~0.16), normals turned outward with the flip rule: both curvatures
    within 2 x 0.033 of -1 / R = -1, the bound tests/test_quadric.py holds the restatement to at r = 0.35 -- the bias of a degree-2 fit
    grows with the neighbourhood's radius, and this one is smaller."""
    from nesti_net_amd import quadric
    c = qx.cloud("sphere_big")
    rows = c["rows"]
    res = quadric.quadric_fit(c["pts"], pidx=rows, knn=128, device=str(gpu_device))
    assert (res["normals"] != 0).any(axis=1).all() and res["radius"].max() < 0.35
    out = (res["normals"].astype(np.float64) * c["gt"][rows]).sum(1) > 0
    k = np.where(out[:, None], res["curv"], -res["curv"][:, ::-1]).astype(np.float64)
    spread = np.abs(k + 1.0).max(axis=0)
    print("unit sphere, k = 128, mean radius %.4g: largest |k + 1| %.4f (k_max), %.4f (k_min)" % (res["radius"].mean(), spread[0], spread[1]))
    assert (k < 0).all() and spread.max() <= 2 * 0.033


def test_the_point_of_it(gpu_device):
    """10.  On the ellipsoid at knn = (8, 32, 128) there is no sentinel row, where the radius path's smallest scale has more than half
    (the figure tests/test_gpu_pca.py asserts).  Both RMS angles to the analytic normals are printed, not gated."""
    e = _ellipsoid(gpu_device)
    cp, c = e["cp"], fx.cloud("ellipsoid")
    normals = e["plane"][0]
    assert (normals != 0).any(axis=-1).all() and (e["plane"][3] == np.array(KS)).all()
    ball_normals, _, n_ball = _np(cp.pca(0, cp.patch_count))
    sentinel = (ball_normals[:, 0] == 0).all(axis=1)
    assert sentinel.mean() > 0.5 and np.array_equal(sentinel, n_ball[:, 0] < 3)
    print("ellipsoid, RMS angle to the analytic normals, degrees: k-NN %s at k = %s; radius %s at r = %s (sentinel rows left out: %s)"
          % ([round(fx.angle_rms_deg(normals[:, s], c["gt"]), 3) for s in range(3)], list(KS),
             [round(fx.angle_rms_deg(ball_normals[:, s], c["gt"]), 3) for s in range(3)], [round(r, 4) for r in c["r_abs"]],
             (n_ball < 3).sum(0).tolist()))


def test_python_layer(gpu_device):
    """11.  Dict keys and shapes for all points, pidx and queries; ``queries = pts[pidx]`` reproduces ``pidx`` byte for byte;
    ``orient='viewpoint'`` changes only sign bits (and flips the curvatures of the turned rows); ``orient='mst'`` runs."""
    from nesti_net_amd import pca, quadric
    c = fx.cloud("ellipsoid")
    pts, dev = c["pts"], str(gpu_device)
    pidx = np.arange(0, len(pts), 9)
    every = pca.pca_normals(pts, knn=KS, device=dev)
    by_index = pca.pca_normals(pts, knn=KS, pidx=pidx, device=dev)
    by_position = pca.pca_normals(pts, knn=KS, queries=pts[pidx], device=dev)
    keys = ["eig", "n_ball", "normals", "normals_all", "orient", "radius", "variation"]
    for res, M in ((every, len(pts)), (by_index, len(pidx)), (by_position, len(pidx))):
        assert sorted(res) == keys and res["orient"] is None
        assert [res[k].shape for k in keys if k != "orient"] == [(M, 3, 3), (M, 3), (M, 3), (M, 3, 3), (M, 3), (M, 3)]
        assert np.array_equal(res["normals"], res["normals_all"][:, -1]) and res["radius"].dtype == np.float32
    for k in keys:
        if k != "orient":
            assert _same_bytes(by_index[k], by_position[k]) and _same_bytes(np.ascontiguousarray(every[k][pidx]), by_index[k]), k
    assert _same_bytes(every["normals_all"], _ellipsoid(gpu_device)["plane"][0])
    one = pca.pca_normals(pts, knn=32, scale=0, device=dev)
    assert one["normals_all"].shape == (len(pts), 1, 3) and _same_bytes(one["normals"], np.ascontiguousarray(every["normals_all"][:, 1]))
    vp = pca.pca_normals(pts, knn=KS, scale=1, orient="viewpoint", viewpoint=(9.0, 0.0, 0.0), device=dev)
    assert _same_bytes(vp["normals_all"], every["normals_all"]) and np.array_equal(np.abs(vp["normals"]), np.abs(every["normals_all"][:, 1]))
    assert (_b32(vp["normals"]) != _b32(every["normals_all"][:, 1])).any() and vp["orient"]["n_flipped"] > 0
    mst = pca.pca_normals(pts, knn=KS, orient="mst", device=dev)
    assert np.array_equal(np.abs(mst["normals"]), np.abs(every["normals"])) and mst["orient"]["n_eligible"] == len(pts)
    q = quadric.quadric_fit(pts, knn=KS, pidx=pidx, device=dev)
    qkeys = ["curv", "curv_all", "n_ball", "normals", "normals_all", "orient", "plane_all", "radius"]
    assert sorted(q) == qkeys and q["curv"].shape == (len(pidx), 2) and q["curv_all"].shape == (len(pidx), 3, 2)
    assert _same_bytes(q["plane_all"], by_index["normals_all"]) and _same_bytes(q["radius"], by_index["radius"])
    qv = quadric.quadric_fit(pts, knn=KS, pidx=pidx, orient="viewpoint", viewpoint=(9.0, 0.0, 0.0), device=dev)
    flipped = (_b32(qv["normals"]) != _b32(q["normals"])).any(axis=1)
    assert flipped.any() and not flipped.all() and np.array_equal(np.abs(qv["normals"]), np.abs(q["normals"]))
    assert _same_bytes(qv["curv"], np.where(flipped[:, None], -q["curv"][:, ::-1], q["curv"]))


def test_command_line(tmp_path, gpu_device, capsys):
    """11.  ``--estimator pca --knn 8,32`` writes .normals, .pca_eig, .pca_count and .knn_radius with the right rows, equal to what the
    Python call returns through the same writers (the k-NN fits do not depend on the grid build: byte for byte);
    ``--estimator quadric --knn 16`` likewise; ``--estimator net --knn 8`` exits with the parser error."""
    from nesti_net_amd import pca, quadric, textio
    from nesti_net_amd.cli import main
    d = tmp_path / "data"
    d.mkdir()
    pts, pidx = fx.cloud("ellipsoid")["pts"], np.arange(0, 4000, 5)
    np.savetxt(d / "ell.xyz", pts.astype(np.float64))
    np.savetxt(d / "ell.pidx", pidx, fmt="%d")
    (d / "testset.txt").write_text("ell\n")
    common = ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt", "--sparse_patches", "1"]
    pts32 = np.loadtxt(d / "ell.xyz").astype("float32")
    want = str(tmp_path / "want")

    results = str(tmp_path / "res")
    assert main(["--estimator", "pca", "--knn", "8,32", "--pca_scale", "0", "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    exts = (".normals", ".pca_eig", ".pca_count", ".knn_radius")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["ell" + e for e in exts])
    res = pca.pca_normals(pts32, pidx=pidx, knn=(8, 32), scale=0, device=str(gpu_device))
    textio.write_f32(want + ".normals", res["normals"])
    textio.write_f32(want + ".pca_eig", res["eig"].reshape(len(pidx), -1))
    textio.write_i32_rows(want + ".pca_count", res["n_ball"])
    textio.write_f32(want + ".knn_radius", res["radius"])
    for e in exts:
        assert open(os.path.join(out, "ell" + e), "rb").read() == open(want + e, "rb").read(), e
    assert np.loadtxt(os.path.join(out, "ell.normals")).shape == (len(pidx), 3)
    assert np.loadtxt(os.path.join(out, "ell.pca_eig")).shape == (len(pidx), 6)
    assert np.array_equal(np.loadtxt(os.path.join(out, "ell.pca_count"), dtype=np.int64), np.tile([8, 32], (len(pidx), 1)))
    assert np.loadtxt(os.path.join(out, "ell.knn_radius")).shape == (len(pidx), 2)
    assert "8 nearest neighbours" in open(os.path.join(out, "log.txt")).read()

    results = str(tmp_path / "resq")
    assert main(["--estimator", "quadric", "--knn", "16", "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    exts = (".normals", ".curv", ".quadric_curv", ".quadric_count", ".knn_radius")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["ell" + e for e in exts])
    res = quadric.quadric_fit(pts32, pidx=pidx, knn=16, device=str(gpu_device))
    textio.write_f32(want + ".normals", res["normals"])
    textio.write_f32(want + ".curv", res["curv"])
    textio.write_f32(want + ".quadric_curv", res["curv_all"].reshape(len(pidx), -1))
    textio.write_i32_rows(want + ".quadric_count", res["n_ball"])
    textio.write_f32(want + ".knn_radius", res["radius"])
    for e in exts:
        assert open(os.path.join(out, "ell" + e), "rb").read() == open(want + e, "rb").read(), e

    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(["--estimator", "net", "--knn", "8", "--results_path", str(tmp_path / "resn")] + common)
    assert e.value.code == 2 and "--knn belongs to --estimator pca / --estimator quadric" in capsys.readouterr().err
    assert not (tmp_path / "resn").exists()
