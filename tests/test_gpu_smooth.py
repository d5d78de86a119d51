"""Normal smoothing on the GPU (csrc/smooth.hip, ``CloudPatches.smooth_knn``, ``smooth.smooth_normals``, ``smooth=`` of the estimators,
``--smooth``) against the tests' own numpy restatement (tests/_smooth_fixture.py): every output -- normals, support, count -- equal ON
THE BYTES.  The lists come from ``nesti_knn`` or are written by hand; the restatement takes the list it is given."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _smooth_fixture as sx

pytestmark = pytest.mark.gpu

KEYS = ("normals", "support", "count")
COS45 = math.cos(math.radians(45.0))
K = 80

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
    components -0."""
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
    """box, n = 300 (the cloud of test_gpu_hough.py): a CloudPatches over all rows, the 80-NN lists of nesti_knn (device and host) and
    the input normals (host and device), prepared once."""
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
    """``with _lanes(64):`` -- at least that lane group for the calls inside (nesti_debug_smooth_lanes), the default again after."""

    def __init__(self, lanes):
        from nesti_net_amd import _lib
        self.lib, self.lanes = _lib.load(), lanes

    def __enter__(self):
        assert self.lib.nesti_debug_smooth_lanes(self.lanes) == 0

    def __exit__(self, *exc):
        assert self.lib.nesti_debug_smooth_lanes(0) == 0


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 32, 33, 64, 65, 80])
def test_every_output_equals_the_restatement(k, gpu_device):
    """1.  box, all 300 rows, the lists of nesti_knn at K = 80; k at the lane-group and wave boundaries, crossed with the ends and the
    middle of cos_t and falloff.  Where k fits a lane group (k <= 32) the wider groups and the one-wave-per-row form give the same
    bytes."""
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    rows = np.arange(len(pts))
    took = 0
    for cos_t in (0.0, COS45, 0.999):
        for falloff in (0.0, 0.75, 1.0):
            ref = sx.restate(pts, given, rows, nbr_h, k, cos_t, falloff)
            _check(_np(cp.smooth_knn(given_d, 0, len(pts), k, cos_t, falloff, nbr=nbr)), ref, (k, cos_t, falloff))
            for lanes in (32, 64):
                if k <= lanes // 2:
                    with _lanes(lanes):
                        _check(_np(cp.smooth_knn(given_d, 0, len(pts), k, cos_t, falloff, nbr=nbr)), ref, (k, cos_t, falloff, lanes))
            took += int(ref["count"].sum())
            assert (ref["count"] <= k).all() and np.isfinite(ref["support"]).all()
            for row in (3, 7, 12, 50, 90, 120, 200):                          # ineligible centres: the bits of the input, alone
                assert _same_bytes(ref["normals"][row], given[row]) and ref["count"][row] == 0 and ref["support"][row] == 0
            assert ref["count"][11] >= 1 and ref["count"][240] >= 1
    assert took > 300 * min(k, 3)
    assert not _same_bytes(ref["normals"], given)


def test_lane_selector_refuses_other_values(gpu_device):
    from nesti_net_amd import _lib
    lib = _lib.load()
    for bad in (-1, 1, 8, 48, 128):
        assert lib.nesti_debug_smooth_lanes(bad) != 0 and b"nesti_debug_smooth_lanes" in lib.nesti_last_error()
    assert lib.nesti_debug_smooth_lanes(0) == 0


def test_rows_and_batching(gpu_device):
    """2.  The same rows as all points, as ``pidx = arange``, and split into calls of 1 / 7 / rest with the matching first row: identical
    bytes; a search inside the call (no list given) gives them too."""
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    M = len(pts)
    w16 = None
    for k in (40, 16):
        whole = w16 = _np(cp.smooth_knn(given_d, 0, M, k, COS45, 0.75, nbr=nbr))
        _check(whole, sx.restate(pts, given, np.arange(M), nbr_h, k, COS45, 0.75), "whole")
        by_index = CloudPatches(pts, NestiConfig(), device=gpu_device, pidx=np.arange(M), radius_grid=False)
        for label, other in (("searched", _np(cp.smooth_knn(given_d, 0, M, k, COS45, 0.75))),
                             ("index", _np(by_index.smooth_knn(given_d, 0, M, k, COS45, 0.75, nbr=nbr))),
                             ("index, searched", _np(by_index.smooth_knn(given_d, 0, M, k, COS45, 0.75)))):
            for key, a, b in zip(KEYS, whole, other):
                assert _same_bytes(a, b), (label, key, k)
        for c in (cp, by_index):
            parts = [_np(c.smooth_knn(given_d, first, count, k, COS45, 0.75, nbr=nbr[first:first + count].contiguous()))
                     for first, count in ((0, 1), (1, 7), (8, M - 8))]
            for i, key in enumerate(KEYS):
                assert _same_bytes(np.concatenate([p[i] for p in parts]), whole[i]), (key, k)
    # a subset in another order reads the normals of the whole cloud
    pidx = np.arange(M - 1, -1, -3)
    sub = CloudPatches(pts, NestiConfig(), device=gpu_device, pidx=pidx, radius_grid=False)
    got = _np(sub.smooth_knn(given_d, 0, len(pidx), 16, COS45, 0.75, nbr=nbr[torch.from_numpy(pidx.copy()).to(nbr.device)].contiguous()))
    for i in range(3):
        assert _same_bytes(got[i], np.ascontiguousarray(w16[i][pidx]))
    with pytest.raises(ValueError, match="position queries"):
        CloudPatches(pts, NestiConfig(), device=gpu_device, queries=torch.from_numpy(pts), radius_grid=False).smooth_knn(
            given_d, 0, M, 16, COS45, 0.75)
    for bad in (given_d[:-1], given_d.double(), given_d.t().contiguous().t(), given):
        with pytest.raises(ValueError, match="normals: a contiguous float32"):
            cp.smooth_knn(bad, 0, M, 16, COS45, 0.75, nbr=nbr)
    with pytest.raises(ValueError, match="nbr: a contiguous int32"):
        cp.smooth_knn(given_d, 0, M, 16, COS45, 0.75, nbr=nbr[:, :15].contiguous())


def _raw(lib, cloud, normals, pidx, first, nbr, k, cos_t, falloff, out=None, stream=None):
    """The C entry itself over device tensors: (rc, (normals, support, count))."""
    from nesti_net_amd import _lib
    M = len(nbr)
    dev = cloud.device
    outs = (torch.full((M, 3), 7.0, dtype=torch.float32, device=dev) if out is None else out,
            torch.full((M,), 7.0, dtype=torch.float32, device=dev), torch.full((M,), 7, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        rc = lib.nesti_smooth_normals_nbr(_lib.ptr(cloud), len(cloud), _lib.ptr(normals), _lib.ptr(pidx), M, first, _lib.ptr(nbr),
                                          int(nbr.shape[1]), k, cos_t, falloff, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]),
                                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
    return rc, outs


@pytest.mark.parametrize("k", [12, 16, 40])
def test_hostile_lists(k, gpu_device):
    """3.  -1 padding, a bad index mid-row (the prefix is cut), a prefix of 0, unsorted rows, a list without its own centre, all
    neighbours coincident (r2 = 0), every neighbour ineligible (the row is copied, count 0), a centre with an ineligible normal (copied
    bit for bit, NaN payload included) and a centre whose POSITION is not finite (an empty prefix) -- through the C entry itself, since
    ``CloudPatches`` refuses such a cloud."""
    from nesti_net_amd import _lib
    lib = _lib.load()
    box, _, _, nbr_h, given, _ = _box(gpu_device)
    same = np.full((12, 3), 0.25, np.float32)                                # rows 300 .. 311
    lost = np.array([[np.nan, 0, 0], [0, -np.inf, 0]], np.float32)           # rows 312, 313
    pts = np.concatenate([box, same, lost])
    rs = np.random.RandomState(4)
    extra = (np.array([0.1, 0.2, 1.0]) + rs.normal(0.0, 0.05, (14, 3))).astype(np.float32)     # the coincident points agree
    normals = np.concatenate([given, extra])
    dead = np.arange(260, 300)                                               # 40 points without a usable normal
    normals[dead[0::3]] = 0.0
    normals[dead[1::3]] = np.nan
    normals[dead[2::3], 1] = np.inf
    normals[9] = np.array([0x7fc12345, 0x3f800000, 0xffc00001], np.uint32).view(np.float32)    # a centre's NaN, with payloads
    N, KK = len(pts), 40
    centres = np.array([0, 1, 2, 4, 5, 6, 300, 8, 9, 312, 313, 10, 3, 14], np.int64)
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
    dev = torch.device(gpu_device)
    cloud_d, normals_d = torch.from_numpy(pts).to(dev), torch.from_numpy(normals).to(dev)
    rc, got = _raw(lib, cloud_d, normals_d, torch.from_numpy(centres.astype(np.int32)).to(dev), 0, torch.from_numpy(nbr).to(dev), k, COS45, 0.75)
    assert rc == 0, lib.nesti_last_error()
    got = _np(got)
    ref = sx.restate(pts, normals, centres, nbr, k, COS45, 0.75)
    _check(got, ref, "hostile")
    out, support, count = got
    for row in (3, 4, 7, 8, 9, 10, 12):                                      # copied bit for bit, alone
        assert _same_bytes(out[row], normals[centres[row]]) and count[row] == 0 and support[row] == 0, row
    assert count[1] <= min(k, 10) and count[2] <= 5 and count[11] <= 3 and count[13] <= (k + 1) // 2 and count[6] == k and count[5] >= 1
    assert support[6] > 0 and np.isfinite(out[[0, 1, 2, 5, 6, 11, 13]]).all()


def test_iterations_and_the_refused_alias(gpu_device):
    """4.  ``smooth.smooth_normals`` with ``iters = 3`` equals three passes of the restatement; a call whose output is its input is
    refused and writes nothing."""
    from nesti_net_amd import _lib, smooth
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    M = len(pts)
    for k, lists in ((16, None), (24, nbr_h)):
        res = smooth.smooth_normals(pts, given, k=k, iters=3, angle=45.0, falloff=0.75, nbr=lists, device=str(gpu_device))
        ref = sx.iterate(pts, given, np.arange(M), nbr_h, k, COS45, 0.75, 3)
        assert sorted(res) == sorted(KEYS)
        _check([res[key] for key in KEYS], ref, ("iterate", k))
    one = sx.restate(pts, given, np.arange(M), nbr_h, 16, COS45, 0.75)
    assert not _same_bytes(one["normals"], sx.iterate(pts, given, np.arange(M), nbr_h, 16, COS45, 0.75, 3)["normals"])
    lib = _lib.load()
    alias = given_d.clone()
    rc, outs = _raw(lib, cp.cloud, alias, None, 0, nbr, 16, COS45, 0.75, out=alias)
    assert rc != 0 and b"nesti_smooth_normals_nbr: normals_out_dev must not be normals_in_dev" in lib.nesti_last_error()
    assert _same_bytes(alias.cpu().numpy(), given) and (outs[1] == 7.0).all() and (outs[2] == 7).all()


def test_graph_capture(gpu_device):
    """One kernel per call, nothing read back: two passes captured into a graph (default queue settings) replay to the same bytes."""
    pts, cp, nbr, nbr_h, given, given_d = _box(gpu_device)
    M = len(pts)
    want = sx.iterate(pts, given, np.arange(M), nbr_h, 16, COS45, 0.75, 2)
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.device(gpu_device):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            first = cp.smooth_knn(given_d, 0, M, 16, COS45, 0.75, nbr=nbr)
            out = cp.smooth_knn(first[0], 0, M, 16, COS45, 0.75, nbr=nbr)
        for t in out + first:
            t.zero_()
        g.replay()
        torch.cuda.synchronize(gpu_device)
    _check(_np(out), want, "graph")


def test_estimators_smooth_before_they_orient(gpu_device, monkeypatch):
    """5.  ``hough_normals(..., smooth=2)``: ``normals`` is the restatement applied to the unsmoothed ``normals_all`` over the lists of the
    estimator's ONE search; with ``orient='mst'`` only sign bits differ from the unoriented smoothed rows.  The plane fit and the
    quadric fit go the same way (a ball fit searches once for the passes); the quadric fit's curvatures are untouched by the
    smoothing and still flip with the orientation."""
    from nesti_net_amd import hough, pca, quadric
    from nesti_net_amd.provider import CloudPatches
    pts, cp, nbr, nbr_h, _, _ = _box(gpu_device)
    M, dev = len(pts), str(gpu_device)
    rows = np.arange(M)
    searches = []
    knn = CloudPatches.knn
    monkeypatch.setattr(CloudPatches, "knn", lambda self, first, count, k, **kw: (searches.append(k), knn(self, first, count, k, **kw))[1])
    kw = dict(knn=(17, 40), triplets=130, bins=8, rotations=3, seed=4, device=dev)
    plain = hough.hough_normals(pts, **kw)
    assert searches == [40] and "smooth_support" not in plain
    del searches[:]
    res = hough.hough_normals(pts, smooth=2, **kw)
    assert searches == [40]                                                  # the lists of the estimator's search, reused
    assert _same_bytes(res["normals_all"], plain["normals_all"]) and _same_bytes(res["conf"], plain["conf"])
    ref = sx.iterate(pts, np.ascontiguousarray(plain["normals_all"][:, -1]), rows, nbr_h[:, :40], 16, COS45, 0.75, 2)
    _check([res["normals"], res["smooth_support"], res["smooth_count"]], ref, "hough")
    assert not _same_bytes(res["normals"], plain["normals"]) and res["orient"] is None
    del searches[:]
    small = hough.hough_normals(pts, smooth={"iters": 1, "k": 24, "angle": 30.0, "falloff": 0.5}, scale=0, **dict(kw, knn=(17,)))
    assert searches == [17, 24]                                              # lists shorter than k: one more search
    ref = sx.restate(pts, np.ascontiguousarray(small["normals_all"][:, 0]), rows, nbr_h, 24, math.cos(math.radians(30.0)), 0.5)
    _check([small["normals"], small["smooth_support"], small["smooth_count"]], ref, "hough, own search")
    mst = hough.hough_normals(pts, smooth=2, orient="mst", **kw)
    assert np.array_equal(mst["normals"].view(np.uint32) & 0x7fffffff, res["normals"].view(np.uint32) & 0x7fffffff)
    assert (mst["normals"].view(np.uint32) != res["normals"].view(np.uint32)).any() and mst["orient"]["n_flipped"] > 0
    assert _same_bytes(mst["smooth_support"], res["smooth_support"]) and _same_bytes(mst["smooth_count"], res["smooth_count"])
    # the plane fit over balls and over lists, the quadric fit with its curvatures
    for fit, fkw in ((pca.pca_normals, {}), (pca.pca_normals, {"knn": 30}), (quadric.quadric_fit, {"knn": 30})):
        base = fit(pts, device=dev, **fkw)
        sm = fit(pts, device=dev, smooth=1, **fkw)
        ref = sx.restate(pts, base["normals"], rows, nbr_h, 16, COS45, 0.75)
        _check([sm["normals"], sm["smooth_support"], sm["smooth_count"]], ref, (fit.__name__, fkw))
        assert _same_bytes(sm["normals_all"], base["normals_all"])
    vp = quadric.quadric_fit(pts, device=dev, knn=30, smooth=1, orient="viewpoint", viewpoint=(9.0, 0.0, 0.0))
    flipped = (vp["normals"].view(np.uint32) != sm["normals"].view(np.uint32)).any(1)
    assert flipped.any() and not flipped.all()
    assert np.array_equal(vp["normals"].view(np.uint32) & 0x7fffffff, sm["normals"].view(np.uint32) & 0x7fffffff)
    assert _same_bytes(sm["curv"], base["curv"])                             # untouched by the smoothing ...
    assert _same_bytes(vp["curv"], np.where(flipped[:, None], -base["curv"][:, ::-1], base["curv"]))   # ... and flipped with the normal


def _dataset(tmp_path, pts):
    d = tmp_path / "data"
    d.mkdir()
    np.savetxt(d / "box.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("box\n")
    return d, ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]


def test_command_line_network(tmp_path, gpu_device):
    """6.  ``--smooth 2`` with ``--estimator net`` on the synthetic weights writes ``.normals`` and ``.smooth_support`` and leaves
    ``.experts`` and ``.experts_probs`` byte-identical to the run without it (two runs of the command line, a model each)."""
    from nesti_net_amd.cli import main
    pts = _box(gpu_device)[0]
    M = len(pts)
    d, common = _dataset(tmp_path, pts)
    outs = {}
    for label, extra in (("plain", []), ("smooth", ["--smooth", "2", "--smooth_k", "12"])):
        results = str(tmp_path / label)
        assert main(["--synthetic_weights", "--results_path", results] + common + extra) == 0
        outs[label] = os.path.join(results, "synth_results")
    plain_files, smooth_files = set(os.listdir(outs["plain"])), set(os.listdir(outs["smooth"]))
    assert {"box.experts", "box.experts_probs", "box.normals", "log.txt"} <= plain_files
    assert smooth_files - plain_files == {"box.smooth_support"} and plain_files <= smooth_files
    for name in ("box.experts", "box.experts_probs"):
        assert open(os.path.join(outs["plain"], name), "rb").read() == open(os.path.join(outs["smooth"], name), "rb").read(), name
    before = np.loadtxt(os.path.join(outs["plain"], "box.normals"), dtype=np.float32)
    after = np.loadtxt(os.path.join(outs["smooth"], "box.normals"), dtype=np.float32)
    support = np.loadtxt(os.path.join(outs["smooth"], "box.smooth_support"))
    assert after.shape == (M, 3) and support.shape == (M, 2) and not np.array_equal(before, after)
    assert (support[:, 1] >= 1).all() and (support[:, 1] <= 12).all() and (support[:, 1] == np.round(support[:, 1])).all()
    assert np.abs(np.linalg.norm(after.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    log = open(os.path.join(outs["smooth"], "log.txt")).read()
    assert "smoothing of box: %d rows, 2 passes over 12 nearest neighbours" % M in log and "rows with count 1" in log
    assert "smoothing of" not in open(os.path.join(outs["plain"], "log.txt")).read()


def test_command_line_model_free(tmp_path, gpu_device):
    """6.  ``--estimator pca --knn 30 --smooth 1``: the files of the Python call, through the same writers."""
    from nesti_net_amd import pca, textio
    from nesti_net_amd.cli import main, write_smooth_support
    d, common = _dataset(tmp_path, _box(gpu_device)[0])
    results = str(tmp_path / "fit")
    assert main(["--estimator", "pca", "--knn", "30", "--smooth", "1", "--smooth_angle", "30", "--smooth_falloff", "0.5",
                 "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    res = pca.pca_normals(np.loadtxt(d / "box.xyz").astype("float32"), knn=30, smooth={"iters": 1, "angle": 30.0, "falloff": 0.5},
                          device=str(gpu_device))
    want = str(tmp_path / "want")
    textio.write_f32(want + ".normals", res["normals"])
    write_smooth_support(want + ".smooth_support", res["smooth_support"], res["smooth_count"])
    for e in (".normals", ".smooth_support"):
        assert open(os.path.join(out, "box" + e), "rb").read() == open(want + e, "rb").read(), e
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["box" + e for e in (".normals", ".pca_eig", ".pca_count", ".knn_radius", ".smooth_support")])
