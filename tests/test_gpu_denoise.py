"""Point denoising on the GPU (csrc/denoise.hip, ``CloudPatches.denoise_knn``, ``denoise.denoise_points``, ``denoise=`` of the estimators,
``--denoise``) against the tests' own numpy restatement (tests/_denoise_fixture.py): every output -- points, delta, support, count --
equal ON THE BYTES.  The lists come from ``nesti_knn`` or are written by hand; the restatement takes the list it is given."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _denoise_fixture as dx
import _knn_fixture as kx

pytestmark = pytest.mark.gpu

KEYS = ("points", "delta", "support", "count")
COS45 = math.cos(math.radians(45.0))
K = 80
# (cos_t, falloff, sigma, step): the cross of {0, cos 45, 0.999} x {0, 0.75, 1} x {0.05, 0.5, 1e6} x {1, 0.3} thinned to six rows in
# which every value of every parameter appears (twice; a step three times)
COMBOS = ((0.0, 0.0, 0.05, 1.0), (COS45, 0.75, 0.5, 0.3), (0.999, 1.0, 1e6, 1.0), (0.0, 0.75, 1e6, 0.3), (COS45, 1.0, 0.05, 1.0),
          (0.999, 0.0, 0.5, 0.3))

_state = {}


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check(got, ref, label):
    for key, g in zip(KEYS, got):
        assert _same_bytes(g, ref[key]), (label, key, np.flatnonzero((g.view(np.uint32) != ref[key].view(np.uint32)).reshape(len(g), -1).any(1))[:8])


def _normals(nrm, seed=21):
    """The analytic normals perturbed (seeded), under random signs, with lengths in 0.5 .. 2; a few rows 0 0 0, a few NaN / inf, a few
    components -0: the planted rows of test_gpu_smooth.py."""
    rs = np.random.RandomState(seed)
    n = nrm.astype(np.float64) + rs.normal(0.0, 0.15, nrm.shape)
    n *= np.where(rs.rand(len(n)) < 0.5, -1.0, 1.0)[:, None] * rs.uniform(0.5, 2.0, len(n))[:, None]
    n = n.astype(np.float32)
    n[[3, 50, 120]] = 0.0
    n[7] = [np.nan, 0.5, 0.5]
    n[90] = [0.0, np.inf, 0.0]
    n[200, 2] = -np.inf
    n[11] = [-0.0, 0.0, 1.5]                                                 # eligible: -0 and +0 are both zero
    n[12] = [0.0, -0.0, -0.0]                                                # not eligible: no non-zero component
    n[13, 0] = -0.0
    n[240] = np.array([0.0, -1.0, -0.0], np.float32)
    return n


def _box(dev):
    """box, n = 300, seed 3 (the cloud of test_gpu_smooth.py; the perturbed normals see heights on the flat faces too): a CloudPatches
    over all rows, the 80-NN lists of nesti_knn (device and host) and the input normals (host and device), prepared once."""
    if "box" not in _state:
        from nesti_net_amd import synth
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        pts, nrm = synth.make_cloud("box", n=300, seed=3)
        cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
        nbr = cp.knn(0, len(pts), K)[0]
        given = _normals(nrm)
        _state["box"] = (pts, cp, nbr, nbr.cpu().numpy(), given, torch.from_numpy(given).to(cp.device))
    return _state["box"]


class _lanes:
    """``with _lanes(64):`` -- at least that lane group for the calls inside (nesti_debug_denoise_lanes), the default again after."""

    def __init__(self, lanes):
        from nesti_net_amd import _lib
        self.lib, self.lanes = _lib.load(), lanes

    def __enter__(self):
        assert self.lib.nesti_debug_denoise_lanes(self.lanes) == 0

    def __exit__(self, *exc):
        assert self.lib.nesti_debug_denoise_lanes(0) == 0


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 32, 33, 64, 65, 80])
def test_every_output_equals_the_restatement(k, gpu_device):
    """1.  box, all 300 rows, the lists of nesti_knn at K = 80; k at the lane-group and wave boundaries, with every value of cos_t,
    falloff, sigma and step (``COMBOS``).  Where k fits a lane group (k <= 32) the wider groups and the one-wave-per-row form give the
    same bytes."""
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    rows = np.arange(len(pts))
    took = moved = 0
    for cos_t, falloff, sigma, step in COMBOS:
        ref = dx.restate(pts, given, rows, nbr_h, k, cos_t, falloff, sigma, step)
        _check(_np(cp.denoise_knn(given_d, 0, len(pts), k, cos_t, falloff, sigma, step, nbr=nbr)), ref, (k, cos_t, falloff, sigma, step))
        for lanes in (32, 64):
            if k <= lanes // 2:
                with _lanes(lanes):
                    _check(_np(cp.denoise_knn(given_d, 0, len(pts), k, cos_t, falloff, sigma, step, nbr=nbr)), ref,
                           (k, cos_t, falloff, sigma, step, lanes))
        took += int(ref["count"].sum())
        moved += int((ref["points"].view(np.uint32) != pts.view(np.uint32)).any(1).sum())
        assert (ref["count"] <= k).all() and np.isfinite(ref["support"]).all() and np.isfinite(ref["points"]).all()
        for row in (3, 7, 12, 50, 90, 120, 200):                              # ineligible centres: the bits of the input, alone
            assert _same_bytes(ref["points"][row], pts[row]) and ref["count"][row] == 0 and ref["support"][row] == 0 and ref["delta"][row] == 0
        assert ref["count"][11] >= 1 and ref["count"][240] >= 1
    assert took > 300 * min(k, 3)
    assert moved > 0 if k > 1 else moved == 0                                 # k = 1: the row itself, whose height is 0


def test_lane_selector_refuses_other_values(gpu_device):
    from nesti_net_amd import _lib
    lib = _lib.load()
    for bad in (-1, 1, 8, 48, 128):
        assert lib.nesti_debug_denoise_lanes(bad) != 0 and b"nesti_debug_denoise_lanes" in lib.nesti_last_error()
    assert lib.nesti_debug_denoise_lanes(0) == 0


def test_rows_and_batching(gpu_device):
    """2.  The same rows as all points, as ``pidx = arange``, and split into calls of 1 / 7 / rest with the matching first row: identical
    bytes; a search inside the call (no list given) gives them too; a reversed, strided ``pidx`` subset equals the corresponding rows."""
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    M = len(pts)
    par = (COS45, 0.75, 0.5, 1.0)
    w16 = None
    for k in (40, 16):
        whole = w16 = _np(cp.denoise_knn(given_d, 0, M, k, *par, nbr=nbr))
        _check(whole, dx.restate(pts, given, np.arange(M), nbr_h, k, *par), "whole")
        by_index = CloudPatches(pts, NestiConfig(), device=gpu_device, pidx=np.arange(M), radius_grid=False)
        for label, other in (("searched", _np(cp.denoise_knn(given_d, 0, M, k, *par))),
                             ("index", _np(by_index.denoise_knn(given_d, 0, M, k, *par, nbr=nbr))),
                             ("index, searched", _np(by_index.denoise_knn(given_d, 0, M, k, *par)))):
            for key, a, b in zip(KEYS, whole, other):
                assert _same_bytes(a, b), (label, key, k)
        for c in (cp, by_index):
            parts = [_np(c.denoise_knn(given_d, first, count, k, *par, nbr=nbr[first:first + count].contiguous()))
                     for first, count in ((0, 1), (1, 7), (8, M - 8))]
            for i, key in enumerate(KEYS):
                assert _same_bytes(np.concatenate([p[i] for p in parts]), whole[i]), (key, k)
    # a subset in another order reads the positions and the normals of the whole cloud
    pidx = np.arange(M - 1, -1, -3)
    sub = CloudPatches(pts, NestiConfig(), device=gpu_device, pidx=pidx, radius_grid=False)
    got = _np(sub.denoise_knn(given_d, 0, len(pidx), 16, *par, nbr=nbr[torch.from_numpy(pidx.copy()).to(nbr.device)].contiguous()))
    for i in range(4):
        assert _same_bytes(got[i], np.ascontiguousarray(w16[i][pidx]))
    with pytest.raises(ValueError, match="position queries"):
        CloudPatches(pts, NestiConfig(), device=gpu_device, queries=torch.from_numpy(pts), radius_grid=False).denoise_knn(given_d, 0, M, 16, *par)
    for bad in (given_d[:-1], given_d.double(), given_d.t().contiguous().t(), given):
        with pytest.raises(ValueError, match="normals: a contiguous float32"):
            cp.denoise_knn(bad, 0, M, 16, *par, nbr=nbr)
    with pytest.raises(ValueError, match="nbr: a contiguous int32"):
        cp.denoise_knn(given_d, 0, M, 16, *par, nbr=nbr[:, :15].contiguous())


def _raw(lib, cloud, normals, pidx, first, nbr, k, cos_t, falloff, sigma, step, out=None, stream=None):
    """The C entry itself over device tensors: (rc, (points, delta, support, count))."""
    from nesti_net_amd import _lib
    M = len(nbr)
    dev = cloud.device
    outs = (torch.full((M, 3), 7.0, dtype=torch.float32, device=dev) if out is None else out,
            torch.full((M,), 7.0, dtype=torch.float32, device=dev), torch.full((M,), 7.0, dtype=torch.float32, device=dev),
            torch.full((M,), 7, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        rc = lib.nesti_denoise_points_nbr(_lib.ptr(cloud), len(cloud), _lib.ptr(normals), _lib.ptr(pidx), M, first, _lib.ptr(nbr),
                                          int(nbr.shape[1]), k, cos_t, falloff, sigma, step, *[_lib.ptr(t) for t in outs],
                                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
    return rc, outs


@pytest.mark.parametrize("k", [12, 16, 40])
def test_hostile_lists(k, gpu_device):
    """3.  -1 padding, a bad index mid-row (the prefix ends there), a prefix of 0, unsorted rows, a list without its own centre, a
    duplicate of the centre, all neighbours coincident (r2 = 0: u = 1 and x = 0), every neighbour ineligible (the row is copied, count
    0), a centre with an ineligible normal and a centre whose POSITION is not finite (an empty prefix; the bits of the input, NaN
    payload included) -- through the C entry itself, since ``CloudPatches`` refuses such a cloud.  The output that is the cloud is
    refused and writes nothing."""
    from nesti_net_amd import _lib
    lib = _lib.load()
    box, _, _, nbr_h, given, _ = _box(gpu_device)
    same = np.full((12, 3), 0.25, np.float32)                                # rows 300 .. 311
    lost = np.array([[np.nan, 0, 0], [0, -np.inf, 0]], np.float32)           # rows 312, 313
    lost[0] = np.array([0x7fc12345, 0x3f800000, 0x80000000], np.uint32).view(np.float32)
    pts = np.concatenate([box, same, lost])
    rs = np.random.RandomState(4)
    extra = (np.array([0.1, 0.2, 1.0]) + rs.normal(0.0, 0.05, (14, 3))).astype(np.float32)     # the coincident points agree
    normals = np.concatenate([given, extra])
    dead = np.arange(260, 300)                                               # 40 points without a usable normal
    normals[dead[0::3]] = 0.0
    normals[dead[1::3]] = np.nan
    normals[dead[2::3], 1] = np.inf
    normals[9] = np.array([0x7fc12345, 0x3f800000, 0xffc00001], np.uint32).view(np.float32)    # a centre's NaN normal
    N, KK = len(pts), 40
    centres = np.array([0, 1, 2, 4, 5, 6, 300, 8, 9, 312, 313, 10, 3, 14, 15], np.int64)
    nbr = nbr_h[centres.clip(0, 299), :KK].copy()
    nbr[0] = nbr[0][rs.permutation(KK)]                                      # unsorted
    nbr[1, 10:] = -1                                                         # padding: prefix 10
    nbr[2, 5] = N                                                            # a bad index: prefix 5
    nbr[3, 0] = 2 ** 31 - 1                                                  # prefix 0
    nbr[4, :] = -1
    nbr[5] = nbr_h[6, 1:KK + 1]                                              # without its own centre
    nbr[6] = np.arange(300, 300 + KK) % 12 + 300                             # coincident: r2 = 0
    nbr[7] = dead                                                            # every neighbour ineligible
    nbr[11, 3] = -2 ** 31                                                    # prefix 3
    nbr[13, 1::2] = dead[:KK // 2]                                           # every other neighbour ineligible
    nbr[14, 1:6] = 15                                                        # the centre, six times
    dev = torch.device(gpu_device)
    cloud_d, normals_d = torch.from_numpy(pts).to(dev), torch.from_numpy(normals).to(dev)
    nbr_d, centres_d = torch.from_numpy(nbr).to(dev), torch.from_numpy(centres.astype(np.int32)).to(dev)
    for par in ((COS45, 0.75, 0.5, 1.0), (0.0, 1.0, 1e6, 0.3)):
        rc, got = _raw(lib, cloud_d, normals_d, centres_d, 0, nbr_d, k, *par)
        assert rc == 0, lib.nesti_last_error()
        got = _np(got)
        ref = dx.restate(pts, normals, centres, nbr, k, *par)
        _check(got, ref, ("hostile", par))
        out, delta, support, count = got
        for row in (3, 4, 7, 8, 9, 10, 12):                                  # copied bit for bit, alone
            assert _same_bytes(out[row], pts[centres[row]]) and count[row] == 0 and support[row] == 0 and delta[row] == 0, row
        assert count[1] <= min(k, 10) and count[2] <= 5 and count[11] <= 3 and count[13] <= (k + 1) // 2 and count[6] == k and count[5] >= 1
        assert _same_bytes(out[6], pts[300]) and delta[6] == 0 and support[6] > 0                    # r2 = 0: u = g = 1, every h = 0
        assert np.isfinite(out[[0, 1, 2, 5, 6, 11, 13, 14]]).all()
    alias = cloud_d.clone()
    rc, outs = _raw(lib, alias, normals_d, None, 0, nbr_d, k, COS45, 0.75, 0.5, 1.0, out=alias)
    assert rc != 0 and b"nesti_denoise_points_nbr: points_out_dev must not lie inside the cloud" in lib.nesti_last_error()
    assert _same_bytes(alias.cpu().numpy(), pts) and (outs[1] == 7.0).all() and (outs[3] == 7).all()


def _fit(pts, nbr, normal_k):
    return np.ascontiguousarray(kx.plane_lists(pts, pts, nbr, (normal_k,))["normals"][:, 0])


def test_denoise_points_iterates_over_the_current_positions(gpu_device):
    """4.  ``denoise.denoise_points``: ``iters = T`` equals T chained calls of ``iters = 1`` on the bytes, and the restatement iterated
    over brute-force lists of the current positions -- with plane-fit normals fitted again in every pass (``normals=None``), and with
    a given field held fixed.  ``delta`` and ``moved`` are measured from the input row to the final row."""
    from nesti_net_amd import denoise
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    M, dev = len(pts), str(gpu_device)
    rows = np.arange(M)
    for kw, field in ((dict(k=16, sigma=0.5), None), (dict(k=12, sigma=0.25, normal_k=20, step=0.5), None), (dict(k=16), given)):
        T = 3
        res = denoise.denoise_points(pts, iters=T, normals=field, device=dev, **kw)
        cur, chained = pts, None
        for _ in range(T):
            chained = denoise.denoise_points(cur, iters=1, normals=field, device=dev, **kw)
            cur = chained["points"]
        for key in ("points", "support", "count"):
            assert _same_bytes(res[key], chained[key]), (key, kw)
        p = denoise.check_params(iters=T, **kw)
        cur, ref = pts, None
        for _ in range(T):
            lists = kx.search(cur, cur, max(p.k, p.normal_k))[0]
            nrm = field if field is not None else _fit(cur, lists, p.normal_k)
            ref = dx.restate(cur, nrm, rows, lists, p.k, p.cos_t, p.falloff, p.sigma, p.step)
            cur = ref["points"]
        for key in ("points", "support", "count"):
            assert _same_bytes(res[key], ref[key]), (key, kw)
        changed = (res["points"].view(np.uint32) != pts.view(np.uint32)).any(1)
        assert res["moved"] == int(changed.sum()) and res["moved"] > 0
        want = np.sqrt(((res["points"].astype(np.float64) - pts.astype(np.float64)) ** 2).sum(1))
        assert res["delta"].dtype == np.float32 and np.allclose(res["delta"], want, rtol=1e-6, atol=0.0)
        assert np.array_equal(res["delta"] > 0, changed)
    one = denoise.denoise_points(pts, iters=1, device=dev)
    assert not _same_bytes(one["points"], denoise.denoise_points(pts, iters=2, device=dev)["points"])


def test_estimators_denoise_before_they_fit(gpu_device):
    """5.  ``pca_normals(..., denoise=...)`` equals ``denoise_points`` followed by ``pca_normals`` on its ``points``, on the bytes, and
    adds ``points`` and ``denoise_delta``; with ``queries`` the cloud is denoised and the queries are left alone.  The other four
    estimators take the same route."""
    from nesti_net_amd import denoise, hough, pca, quadric, robust, select
    pts = _box(gpu_device)[0]
    dev = str(gpu_device)
    for dn in (True, {"k": 12, "iters": 1, "sigma": 0.25}):
        d = denoise.denoise_points(pts, device=dev, **({} if dn is True else dn))
        for fit, kw in ((pca.pca_normals, {"knn": 30}), (pca.pca_normals, {"knn": 30, "smooth": 1, "orient": "mst"}),
                        (pca.pca_normals, {"knn": 30, "queries": pts[:17] + np.float32(0.01)}), (quadric.quadric_fit, {"knn": 30}),
                        (hough.hough_normals, {"knn": 30}), (select.select_normals, {}), (robust.robust_normals, {"knn": 30})):
            if dn is not True and fit is not pca.pca_normals:
                continue
            got = fit(pts, device=dev, denoise=dn, **kw)
            want = fit(d["points"], device=dev, **kw)
            assert set(got) == set(want) | {"points", "denoise_delta"}
            for key, v in want.items():
                if isinstance(v, np.ndarray):
                    assert _same_bytes(got[key], v), (fit.__name__, key)
                else:
                    assert got[key] == v, (fit.__name__, key)
            assert _same_bytes(got["points"], d["points"]) and _same_bytes(got["denoise_delta"], d["delta"])
    plain = pca.pca_normals(pts, device=dev, knn=30)
    assert "points" not in plain and not _same_bytes(plain["normals"], pca.pca_normals(pts, device=dev, knn=30, denoise=True)["normals"])
    # after the outlier filter: the kept points are denoised, a removed row holds 0
    both = pca.pca_normals(pts, device=dev, knn=30, outliers={"std_ratio": 0.5}, denoise=True)
    kept = np.flatnonzero(both["inlier"])
    assert 0 < len(kept) < len(pts)
    d = denoise.denoise_points(pts[kept], device=dev)
    assert _same_bytes(both["points"][kept], d["points"]) and (both["points"][~both["inlier"]] == 0).all()
    assert _same_bytes(both["normals"][kept], pca.pca_normals(d["points"], device=dev, knn=30)["normals"])


def _dataset(tmp_path, pts):
    d = tmp_path / "data"
    d.mkdir()
    np.savetxt(d / "box.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("box\n")
    return d, ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]


def test_command_line(tmp_path, gpu_device):
    """6.  ``--estimator pca --knn 30``: without ``--denoise`` the files are those of the Python call without it, through the same
    writers; with ``--denoise 2`` the same file names plus ``.denoised.xyz`` and ``.denoise_delta``, which hold ``denoise_points``' rows
    as the text writer prints them, and ``.normals`` is the fit over the denoised positions."""
    from nesti_net_amd import denoise, pca, textio
    from nesti_net_amd.cli import main
    d, common = _dataset(tmp_path, _box(gpu_device)[0])
    pts = np.loadtxt(d / "box.xyz").astype("float32")
    dev = str(gpu_device)
    outs = {}
    for label, extra in (("plain", []), ("denoise", ["--denoise", "2", "--denoise_k", "12", "--denoise_sigma", "0.25"])):
        results = str(tmp_path / label)
        assert main(["--estimator", "pca", "--knn", "30", "--results_path", results] + common + extra) == 0
        outs[label] = os.path.join(results, "synth_results")
    names = ["box" + e for e in (".normals", ".pca_eig", ".pca_count", ".knn_radius")]
    assert sorted(os.listdir(outs["plain"])) == sorted(["log.txt"] + names)
    assert sorted(os.listdir(outs["denoise"])) == sorted(["log.txt", "box.denoised.xyz", "box.denoise_delta"] + names)
    dn = denoise.denoise_points(pts, k=12, iters=2, sigma=0.25, device=dev)
    for label, cloud in (("plain", pts), ("denoise", dn["points"])):
        res = pca.pca_normals(cloud, knn=30, device=dev)
        want = str(tmp_path / ("want_" + label))
        textio.write_f32(want + ".normals", res["normals"])
        textio.write_f32(want + ".pca_eig", res["eig"].reshape(len(cloud), -1))
        textio.write_i32_rows(want + ".pca_count", res["n_ball"])
        textio.write_f32(want + ".knn_radius", res["radius"])
        for e in (".normals", ".pca_eig", ".pca_count", ".knn_radius"):
            assert open(os.path.join(outs[label], "box" + e), "rb").read() == open(want + e, "rb").read(), (label, e)
    want = str(tmp_path / "want")
    textio.write_f32(want + ".denoised.xyz", dn["points"])
    textio.write_f32(want + ".denoise_delta", dn["delta"])
    for e in (".denoised.xyz", ".denoise_delta"):
        assert open(os.path.join(outs["denoise"], "box" + e), "rb").read() == open(want + e, "rb").read(), e
    log = open(os.path.join(outs["denoise"], "log.txt")).read()
    assert "denoising of box: %d rows, 2 passes over 12 nearest neighbours" % len(pts) in log and "%d rows moved" % dn["moved"] in log
    assert "denoising of" not in open(os.path.join(outs["plain"], "log.txt")).read()


def test_the_default_call_brings_a_noisy_torus_closer_to_its_surface(gpu_device):
    """7.  torus, n = 4000, noise 0.006, seed 5: the RMS distance to the analytic torus after the default call is below the input's.
    (The restatement alone, over brute-force lists and the plane-fit restatement: 0.02346 -> 0.01305 after one pass, 0.00936 after the
    default two.)"""
    from nesti_net_amd import denoise, synth
    pts, _ = synth.make_cloud("torus", n=4000, seed=5, noise=0.006)

    def rms(p):
        p = p.astype(np.float64)
        return float(np.sqrt((np.abs(np.hypot(np.hypot(p[:, 0], p[:, 1]) - 1.0, p[:, 2]) - 0.35) ** 2).mean()))

    res = denoise.denoise_points(pts, device=str(gpu_device))
    before, after = rms(pts), rms(res["points"])
    print("RMS distance to the torus: %.5f -> %.5f" % (before, after))
    assert after < before and res["moved"] > 0
