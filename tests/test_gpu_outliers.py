"""The outlier filter on the GPU (csrc/outlier.hip, ``CloudPatches.outlier_scores`` / ``outlier_threshold`` / ``outlier_compact``,
``outliers.remove_outliers``, ``outliers=`` of the estimators, ``--outliers``) against the tests' own numpy restatement
(tests/_outliers_fixture.py, brute-force search): every output equal ON THE BYTES."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _outliers_fixture as ox

pytestmark = pytest.mark.gpu

K = 256
SIZES = (1, 2, 255, 256, 257, 65535, 65536, 65537, 65536 + 257)
# the compaction's: a trip of the kept scan covers 256 x 16 block counts of 256 rows -- the smallest sizes that take one full trip and two
COMPACT_SIZES = SIZES + (1048576, 1048577)
_state = {}


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _lib():
    from nesti_net_amd import _lib as L
    return L, L.load()


def _crafted(dev):
    """box, n = 300 (seed 3), plus two duplicate pairs (300 = 10, 301 = 20), a triple (302 = 303 = 30), five far points, and -- last --
    a point with a NaN and a point with an inf coordinate.  The lists are ``nesti_knn`` at K = 256 over the finite rows (whose indices
    are the same in the whole cloud; a non-finite point is no one's neighbour); the two non-finite rows borrow the lists of rows 0 and
    1: their centres are lost whatever the list holds."""
    if "crafted" not in _state:
        from nesti_net_amd import synth
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        box, _ = synth.make_cloud("box", n=300, seed=3)
        far = np.array([[3, 0, 0], [0, -4, 0.5], [2, 2, 2], [-5, 1, 0], [0.2, 0.1, 6]], np.float32)
        finite = np.concatenate([box, box[[10, 20, 30, 30]], far]).astype(np.float32)
        lost = np.array([[0.1, np.nan, 0.2], [np.inf, 0.0, 0.0]], np.float32)
        pts = np.ascontiguousarray(np.concatenate([finite, lost]))
        cp = CloudPatches(finite, NestiConfig(), device=dev, radius_grid=False)
        nbr_f = cp.knn(0, len(finite), K)[0].cpu().numpy()
        nbr = np.ascontiguousarray(np.concatenate([nbr_f, nbr_f[:2]]))
        _state["crafted"] = (pts, nbr, torch.from_numpy(pts).to(dev), torch.from_numpy(nbr).to(dev), cp, len(finite))
    return _state["crafted"]


def _scores(cloud_t, row0, nbr_t, k, stream=None):
    """The C entry itself over device tensors -> the three outputs as numpy (``CloudPatches`` refuses a cloud with a non-finite row)."""
    L, lib = _lib()
    M, dev = len(nbr_t), cloud_t.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        out = (torch.full((M,), 7.0, dtype=torch.float64, device=dev), torch.full((M,), 7.0, dtype=torch.float64, device=dev),
               torch.full((M,), 7, dtype=torch.int32, device=dev))
        rc = lib.nesti_outlier_scores_nbr(L.ptr(cloud_t), len(cloud_t), row0, M, L.ptr(nbr_t), int(nbr_t.shape[1]), k,
                                          L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), ctypes.c_void_p(st.cuda_stream))
        assert rc == 0, lib.nesti_last_error()
        st.synchronize()
    return dict(zip(("mean", "kth_d2", "n_other"), (t.cpu().numpy() for t in out)))


def _check(got, ref, label):
    for key in ("mean", "kth_d2", "n_other"):
        assert _same_bytes(got[key], ref[key]), (label, key, np.flatnonzero(got[key].view(np.uint8).reshape(len(ref[key]), -1)
                                                                           != ref[key].view(np.uint8).reshape(len(ref[key]), -1))[:8])


class _lanes:
    """``with _lanes(64):`` -- at least that lane group for the calls inside (nesti_debug_outlier_lanes), the default again after."""

    def __init__(self, lanes):
        self.lib, self.lanes = _lib()[1], lanes

    def __enter__(self):
        assert self.lib.nesti_debug_outlier_lanes(self.lanes) == 0

    def __exit__(self, *exc):
        assert self.lib.nesti_debug_outlier_lanes(0) == 0


# ---- 1. scores ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 14, 15, 16, 31, 32, 63, 64, 65, 127, 128, 255])
def test_scores_equal_the_restatement(k, gpu_device):
    """1.  The crafted cloud, prefixes of the lists of nesti_knn at K = 256; all three outputs; the same bytes in two batches split at
    row 137, on a second stream, with the list cut to K = k + 1, and at every lane-group width that holds k + 1."""
    pts, nbr, cloud_t, nbr_t, _, n_finite = _crafted(gpu_device)
    ref = ox.scores(pts, 0, nbr, k)
    _check(_scores(cloud_t, 0, nbr_t, k), ref, "whole")
    a, b = _scores(cloud_t, 0, nbr_t[:137].contiguous(), k), _scores(cloud_t, 137, nbr_t[137:].contiguous(), k)
    _check({key: np.concatenate([a[key], b[key]]) for key in a}, ref, "two batches")
    _check(_scores(cloud_t, 0, nbr_t, k, stream=torch.cuda.Stream(gpu_device)), ref, "second stream")
    _check(_scores(cloud_t, 0, nbr_t[:, :k + 1].contiguous(), k), ref, "K = k + 1")
    for lanes in (16, 32, 64):
        if k + 1 <= lanes:
            with _lanes(lanes):
                _check(_scores(cloud_t, 0, nbr_t, k), ref, ("lanes", lanes))
    # what the crafted rows are there for
    assert (ref["n_other"][:n_finite] == k).all() and np.isfinite(ref["mean"][:n_finite]).all()
    assert np.isnan(ref["mean"][n_finite:]).all() and np.isnan(ref["kth_d2"][n_finite:]).all() and (ref["n_other"][n_finite:] == 0).all()
    assert _same_bytes(ref["mean"][n_finite:], np.array([0x7ff8000000000000] * 2, np.uint64).view(np.float64))
    if k <= 2:
        for row in (30, 302, 303):                                           # the triple: two other copies at distance 0
            assert ref["mean"][row] == 0.0 and ref["kth_d2"][row] == 0.0
    if k == 1:
        for row in (10, 300, 20, 301):
            assert ref["mean"][row] == 0.0
    if k <= 16:                                                              # the far points stand out
        assert (ref["mean"][n_finite - 5:n_finite] > 4 * np.median(ref["mean"][:300])).all()


# ---- 2. hand-written lists ---------------------------------------------------------------------------------------------------------------

def test_hand_written_lists(gpu_device):
    """2.  Unsorted rows, -1 in slot 0 and in mid-row, an index >= N, the own index absent, the own index in slot k, a neighbour with a
    NaN coordinate, a duplicate ahead of the row itself -- and a 5-point cloud at k = 16."""
    pts, nbr, cloud_t, _, _, n_finite = _crafted(gpu_device)
    N, k, KK = len(pts), 16, 40
    rs = np.random.RandomState(5)
    rows = nbr[:14, :KK].copy()                                              # rows 0 .. 13 of the cloud
    rows[0] = rows[0][rs.permutation(KK)]                                    # unsorted (the own index somewhere, perhaps beyond k)
    rows[1, 0] = -1                                                          # prefix 0
    rows[2, 9] = -1                                                          # prefix 9, the own index inside it
    rows[3, 5] = N                                                           # an index >= N: prefix 5
    rows[4, 3] = 2 ** 31 - 1
    rows[5] = nbr[5, 1:KK + 1]                                               # the own index absent: the first k slots
    rows[6, :k + 1] = np.concatenate([nbr[6, 1:k + 1], [6]])                 # the own index in slot k
    rows[7, 4] = n_finite                                                    # a neighbour with a NaN coordinate: NaN, n_other stays
    rows[8, 2] = n_finite + 1                                                # a neighbour with an inf coordinate: +inf
    rows[9, :3] = [9, 9, 9]                                                  # the own index three times: only the first is skipped
    rows[10, 0], rows[10, 1] = rows[10, 1], rows[10, 0]                      # the own index in slot 1
    rows[11, :] = -1
    rows[12, k:] = -1                                                        # prefix k: the own index inside, k - 1 others
    rows[13, 0] = -(2 ** 31)
    ref = ox.scores(pts, 0, rows, k)
    got = _scores(cloud_t, 0, torch.from_numpy(rows).to(gpu_device), k)
    _check(got, ref, "hand-written")
    for lanes in (32, 64):
        with _lanes(lanes):
            _check(_scores(cloud_t, 0, torch.from_numpy(rows).to(gpu_device), k), ref, ("hand-written", lanes))
    assert ref["n_other"].tolist()[:14] == [k, 0, 8, 4, 2, k, k, k, k, k, k, 0, k - 1, 0]
    assert np.isinf(ref["mean"][[1, 11, 13]]).all() and np.isinf(ref["kth_d2"][[1, 2, 3, 4, 11, 12, 13]]).all()
    assert np.isnan(ref["mean"][7]) and np.isnan(ref["kth_d2"][7]) and ref["mean"][8] == np.inf and ref["kth_d2"][8] == np.inf
    assert ref["mean"][9] > 0 and np.isfinite(ref["kth_d2"][[5, 6, 9, 10]]).all()
    # a 5-point cloud at k = 16: the search pads with -1, four others exist
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    five = pts[[0, 40, 80, 120, 120]].copy()
    cp = CloudPatches(five, NestiConfig(), device=gpu_device, radius_grid=False)
    mean, kth, n_other = (t.cpu().numpy() for t in cp.outlier_scores(0, 5, k))
    r5 = ox.scores(five, 0, ox.knn_brute(five, k + 1), k)
    _check({"mean": mean, "kth_d2": kth, "n_other": n_other}, r5, "five points")
    assert (n_other == 4).all() and np.isinf(kth).all() and np.isfinite(mean).all()
    with pytest.raises(ValueError, match="nbr: a contiguous int32"):
        cp.outlier_scores(0, 5, k, nbr=torch.zeros((5, k), dtype=torch.int32, device=gpu_device))
    with pytest.raises(ValueError, match="pidx or queries"):
        CloudPatches(five, NestiConfig(), device=gpu_device, pidx=[0, 1], radius_grid=False).outlier_scores(0, 2, 1)


# ---- 3. threshold ------------------------------------------------------------------------------------------------------------------------

def _synthetic_scores(M, seed):
    """Magnitudes from 1e-8 to 1e8 -- a sum in another order differs in its last bits -- with NaN and +inf sprinkled in."""
    rs = np.random.RandomState(seed)
    sc = 10.0 ** rs.uniform(-8.0, 8.0, M)
    if M > 2:
        hole = rs.rand(M) < 0.05
        sc[hole] = np.where(rs.rand(int(hole.sum())) < 0.5, np.nan, np.inf)
    return sc


@pytest.mark.parametrize("M", SIZES)
def test_threshold_equals_the_restatement(M, gpu_device):
    """3.  Synthetic scores at the block borders of both stages; std_ratio 0, 1, 2.5; an all-absent array and one finite score."""
    cp = _crafted(gpu_device)[4]
    cases = [("synthetic", _synthetic_scores(M, M))]
    absent = np.full(M, np.nan)
    absent[::2] = np.inf
    one = absent.copy()
    one[M // 2] = 0.375
    cases += [("all absent", absent), ("one finite", one)]
    for label, sc in cases:
        sc_t = torch.from_numpy(sc).to(gpu_device)
        for ratio in (0.0, 1.0, 2.5):
            got = cp.outlier_threshold(sc_t, ratio).cpu().numpy()
            ref = ox.threshold(sc, ratio)
            assert _same_bytes(got, ref), (label, M, ratio, got.tolist(), ref.tolist())
    assert ox.threshold(absent, 1.0).tolist() == [0.0, 0.0, 0.0, np.inf] and ox.threshold(one, 2.5).tolist() == [1.0, 0.375, 0.0, 0.375]


def test_threshold_in_a_graph_and_with_no_rows(gpu_device):
    """Nothing is read back: the four launches are captured into a graph and replayed on new scores; 0 rows give (0, 0, 0, +inf)."""
    L, lib = _lib()
    cp = _crafted(gpu_device)[4]
    M = 1000
    sc = _synthetic_scores(M, 1)
    sc_t = torch.from_numpy(sc).to(gpu_device)
    stats = torch.zeros(4, dtype=torch.float64, device=gpu_device)
    ws = torch.empty(lib.nesti_outlier_workspace_bytes(M), dtype=torch.uint8, device=gpu_device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream(gpu_device)
        assert lib.nesti_outlier_threshold(L.ptr(sc_t), M, 1.0, L.ptr(stats), L.ptr(ws), ws.numel(), ctypes.c_void_p(st.cuda_stream)) == 0
    other = _synthetic_scores(M, 2)
    sc_t.copy_(torch.from_numpy(other))
    g.replay()
    torch.cuda.synchronize(gpu_device)
    assert _same_bytes(stats.cpu().numpy(), ox.threshold(other, 1.0))
    assert cp.outlier_threshold(torch.zeros(0, dtype=torch.float64, device=gpu_device), 1.0).cpu().tolist() == [0.0, 0.0, 0.0, np.inf]
    with pytest.raises(ValueError, match="scores: a contiguous float64"):
        cp.outlier_threshold(sc_t.float(), 1.0)
    with pytest.raises(ValueError, match="std_ratio"):
        cp.outlier_threshold(sc_t, -1.0)


# ---- 4. compaction -----------------------------------------------------------------------------------------------------------------------

def _compact(cloud_t, sc_t, thr, on_device):
    L, lib = _lib()
    N, dev = len(sc_t), sc_t.device
    out = (torch.full((N, 3), 7.0, dtype=torch.float32, device=dev), torch.full((N,), -7, dtype=torch.int32, device=dev),
           torch.full((N,), -7, dtype=torch.int32, device=dev), torch.full((N,), 7, dtype=torch.uint8, device=dev),
           torch.full((1,), -7, dtype=torch.int32, device=dev))
    ws = torch.empty(lib.nesti_outlier_workspace_bytes(N), dtype=torch.uint8, device=dev)
    thr_t = torch.tensor([thr], dtype=torch.float64).to(dev) if on_device else None
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        rc = lib.nesti_outlier_compact(L.ptr(cloud_t), N, L.ptr(sc_t), L.ptr(thr_t), float("nan") if on_device else thr,
                                       *[L.ptr(t) for t in out], L.ptr(ws), ws.numel(), ctypes.c_void_p(st.cuda_stream))
        assert rc == 0, lib.nesti_last_error()
        torch.cuda.synchronize(dev)
    xyz, kept_idx, new_of_old, keep, n_kept = (t.cpu().numpy() for t in out)
    n = int(n_kept[0])
    return {"xyz": xyz[:n], "kept_idx": kept_idx[:n], "new_of_old": new_of_old, "keep": keep, "n_kept": n,
            "untouched": (xyz[n:] == 7.0).all() and (kept_idx[n:] == -7).all()}


@pytest.mark.parametrize("M", COMPACT_SIZES)
def test_compaction_equals_the_restatement(M, gpu_device):
    """4.  Patterns all / none / alternating / only the first / only the last / random; a tie on the threshold is kept, NaN and +inf are
    removed; the threshold on the device and on the host; every output, a -0.0 coordinate among them; nothing beyond n_kept is written."""
    rs = np.random.RandomState(M)
    pts = rs.uniform(-1, 1, (M, 3)).astype(np.float32)
    pts[0, 1] = -0.0
    pts[M - 1, 2] = -0.0
    cloud_t = torch.from_numpy(pts).to(gpu_device)
    thr = 0.5
    lo, hi = np.full(M, 0.25), np.full(M, 0.75)
    rnd = rs.uniform(0.0, 1.0, M)
    rnd[rs.rand(M) < 0.1] = thr                                              # ties: kept
    rnd[rs.rand(M) < 0.05] = np.nan
    rnd[rs.rand(M) < 0.05] = np.inf
    rnd[rs.rand(M) < 0.02] = -np.inf
    first, last = hi.copy(), hi.copy()
    first[0], last[M - 1] = thr, 0.0
    patterns = {"all": lo, "none": hi, "alternating": np.where(np.arange(M) % 2 == 0, lo, hi), "first": first, "last": last, "random": rnd}
    for label, sc in patterns.items():
        ref = ox.compact(pts, sc, thr)
        sc_t = torch.from_numpy(sc).to(gpu_device)
        for on_device in (True, False):
            got = _compact(cloud_t, sc_t, thr, on_device)
            assert got["n_kept"] == ref["n_kept"] and got["untouched"], (label, M, on_device)
            for key in ("xyz", "kept_idx", "new_of_old", "keep"):
                assert _same_bytes(got[key], ref[key]), (label, key, M, on_device)
    assert ox.compact(pts, first, thr)["kept_idx"].tolist() == [0] and ox.compact(pts, last, thr)["kept_idx"].tolist() == [M - 1]
    r = ox.compact(pts, rnd, thr)
    assert not r["keep"][~np.isfinite(rnd)].any() and r["keep"][rnd == thr].all()
    assert np.signbit(ox.compact(pts, lo, thr)["xyz"][0, 1])
    # the outputs may be NULL, all but the count
    L, lib = _lib()
    n_kept = torch.full((1,), -1, dtype=torch.int32, device=gpu_device)
    ws = torch.empty(lib.nesti_outlier_workspace_bytes(M), dtype=torch.uint8, device=gpu_device)
    sc_t = torch.from_numpy(rnd).to(gpu_device)
    with torch.cuda.device(gpu_device):
        assert lib.nesti_outlier_compact(None, M, L.ptr(sc_t), None, thr, None, None, None, None, L.ptr(n_kept), L.ptr(ws), ws.numel(),
                                         ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)) == 0
    assert int(n_kept.cpu()[0]) == r["n_kept"]


# ---- 5. remove_outliers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape, seed", ox.FILTER_CLOUDS)
def test_remove_outliers_equals_the_restatement(shape, seed, gpu_device):
    """5.  2000 surface points + 100 uniform in the bounding box, shuffled: kept set, points, scores and the statistics of every pass,
    both modes, one and two passes.  The property of tests/test_outliers.py (far points leave, the surface stays) is inherited."""
    from nesti_net_amd import outliers
    pts = ox.noisy_cloud(shape, seed)[0]
    for kw in ({"mode": "statistical", "k": 16, "std_ratio": 1.0}, {"mode": "radius", "radius": 0.12, "min_neighbours": 6},
               {"mode": "statistical", "k": 40, "std_ratio": 2.0}):
        for passes in (1, 2):
            got = outliers.remove_outliers(pts, passes=passes, device=str(gpu_device), **kw)
            ref = ox.remove(pts, passes=passes, **kw)
            label = (shape, kw, passes)
            assert got["kept"].dtype == np.int64 and np.array_equal(got["kept"], ref["kept"]), label
            assert np.array_equal(got["inlier"], ref["inlier"]) and got["inlier"].dtype == np.bool_, label
            assert _same_bytes(got["points"], ref["points"]) and _same_bytes(got["score"], ref["score"]), label
            assert got["passes"] == ref["passes"] and len(got["passes"]) == passes, (label, got["passes"], ref["passes"])
            assert 0 < got["passes"][0]["removed"] < len(pts) and (np.diff(got["kept"]) > 0).all()


# ---- 6. estimators -----------------------------------------------------------------------------------------------------------------------

def _small(dev):
    """box, n = 300, plus 20 points uniform in the bounding box, shuffled; the filter's result for it."""
    if "small" not in _state:
        from nesti_net_amd import outliers
        pts, injected, _ = ox.noisy_cloud("box", 3, n=300, n_out=20)
        f = outliers.remove_outliers(pts, k=8, device=str(dev))
        ref = ox.remove(pts, k=8)
        assert np.array_equal(f["kept"], ref["kept"]) and 0 < len(f["kept"]) < len(pts)
        _state["small"] = (pts, f)
    return _state["small"]


def _scattered_equal(got, plain, kept, n):
    for key, v in plain.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == len(kept):
            want = ox.scatter(v, kept, n, -1 if key == "expert" else 0)
            assert _same_bytes(got[key], want), key
        else:
            assert got[key] == v, key
    return True


def test_model_free_estimators_run_on_the_filtered_cloud(gpu_device):
    """6.  For each of the five model-free estimators f(pts, outliers=...) is f(pts[kept]) scattered to the rows of pts, on the bytes,
    with smooth= and orient= set once; inlier and the scores are added; with queries nothing is scattered."""
    from nesti_net_amd import hough, pca, quadric, robust, select
    pts, f = _small(gpu_device)
    o = {"k": 8}
    kept, n, dev = f["kept"], len(pts), str(gpu_device)
    removed = np.flatnonzero(~f["inlier"])
    for fit, kw in ((pca.pca_normals, {"knn": (12, 24), "smooth": 1, "orient": "mst"}), (pca.pca_normals, {}),
                    (quadric.quadric_fit, {"knn": 24}), (hough.hough_normals, {"knn": 30}), (robust.robust_normals, {"knn": 30, "iters": 3}),
                    (select.select_normals, {"ladder": (8, 16, 32)})):
        got = fit(pts, outliers=o, device=dev, **kw)
        plain = fit(pts[kept], device=dev, **kw)
        extra = {key: got.pop(key) for key in ("inlier", "outlier_score", "outlier_passes")}
        assert set(got) == set(plain) and _scattered_equal(got, plain, kept, n), fit.__name__
        assert np.array_equal(extra["inlier"], f["inlier"]) and _same_bytes(extra["outlier_score"], f["score"]) and extra["outlier_passes"] == f["passes"]
        assert got["normals"].shape == (n, 3) and not got["normals"][removed].any() and got["normals"][kept].any()
    # an init per point is cut to the kept points
    init = pca.pca_normals(pts, knn=30, device=dev)["normals"]
    a = robust.robust_normals(pts, knn=30, init=init, outliers=o, device=dev)
    b = robust.robust_normals(pts[kept], knn=30, init=init[kept], device=dev)
    assert _same_bytes(a["normals"], ox.scatter(b["normals"], kept, n))
    # positions: the rows are the queries', nothing is scattered
    q = pts[:7] + np.float32(0.01)
    a, b = pca.pca_normals(pts, knn=12, queries=q, outliers=o, device=dev), pca.pca_normals(pts[kept], knn=12, queries=q, device=dev)
    assert _same_bytes(a["normals"], b["normals"]) and a["normals"].shape == (7, 3) and a["inlier"].shape == (n,)
    with pytest.raises(ValueError, match="outliers with pidx is not served yet"):
        pca.pca_normals(pts, pidx=[1, 2], outliers=o, device=dev)


@pytest.fixture(scope="module")
def estimator(gpu_device):
    """ONE network estimator in the reproducible mode, where a row's bytes do not depend on the calls that came before."""
    from nesti_net_amd import weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.pipeline import NormalEstimator
    cfg = NestiConfig(num_point=64)
    return NormalEstimator(cfg, weights.synthetic_weights(cfg), dtype="f16x3c", device=gpu_device, batch=1024, gate_margin=0.02, reproducible=True)


def test_network_estimate_runs_on_the_filtered_cloud(estimator, gpu_device):
    """6.  NormalEstimator.estimate(outliers=...) is estimate(pts[kept]) scattered: 0 0 0 / -1 / 0 in the removed rows."""
    pts, f = _small(gpu_device)
    kept, n = f["kept"], len(pts)
    got = estimator.estimate(pts, orient="mst", outliers={"k": 8})
    assert np.array_equal(estimator.last_outliers["inlier"], f["inlier"]) and estimator.last_outliers["passes"] == f["passes"]
    plain = estimator.estimate(pts[kept], orient="mst")
    for g, p, fill in zip(got, plain, (0, -1, 0)):
        assert _same_bytes(g, ox.scatter(p, kept, n, fill))
    removed = ~f["inlier"]
    assert not got[0][removed].any() and (got[1][removed] == -1).all() and not got[2][removed].any() and (got[1][kept] >= 0).all()
    with pytest.raises(ValueError, match="outliers with pidx is not served yet"):
        estimator.estimate(pts, pidx=[0, 1], outliers="statistical")


def test_depth_frames_lose_their_flying_pixels(estimator, gpu_device):
    """6.  A 48 x 64 tilted plane with 12 flying pixels half way to the camera: estimate_depth(outliers=...) equals the route done by
    hand -- back-project, filter, estimate the kept points, scatter -- and the flying pixels hold the fill in rows and maps."""
    from nesti_net_amd import outliers
    from nesti_net_amd.depth import Camera, depth_to_cloud
    H, W = 48, 64
    v, u = np.mgrid[0:H, 0:W]
    depth = (1000.0 + 2.0 * u + 1.5 * v).astype(np.uint16)                   # millimetres
    flying = np.array([(5, 7), (5, 40), (11, 22), (17, 58), (20, 3), (24, 31), (29, 47), (33, 12), (38, 25), (41, 60), (44, 5), (45, 38)])
    depth[flying[:, 0], flying[:, 1]] = 500
    cam = Camera(fx=60.0, fy=60.0, cx=31.5, cy=23.5, depth_scale=0.001)
    o = {"k": 8, "std_ratio": 1.0}
    res = estimator.estimate_depth(depth, cam, outliers=o)
    dc = depth_to_cloud(depth, cam, device=gpu_device)
    xyz, pix = dc.xyz.cpu().numpy(), dc.pix.cpu().numpy()
    f = outliers.remove_outliers(xyz, device=str(gpu_device), **o)
    ref = ox.remove(xyz, **o)
    assert np.array_equal(f["kept"], ref["kept"])
    fly_rows = np.flatnonzero(np.isin(pix, flying[:, 0] * W + flying[:, 1]))
    assert len(fly_rows) == 12 and not f["inlier"][fly_rows].any() and f["inlier"].mean() > 0.9
    kept, n = f["kept"], len(xyz)
    cloud = estimator.prepare(xyz[kept])                                      # the route by hand: a reproducible estimator verifies its run
    triple = estimator.run_verified(cloud)
    estimator.orient(cloud, triple[0], "viewpoint", np.zeros(3), 8)
    torch.cuda.synchronize(gpu_device)
    plain = [t.cpu().numpy() for t in triple]
    assert n == H * W and _same_bytes(res["xyz"], xyz) and np.array_equal(res["pix"], pix) and np.array_equal(res["inlier"], f["inlier"])
    for key, p, fill in zip(("normals", "expert", "probs"), plain, (0, -1, 0)):
        rows = ox.scatter(p, kept, n, fill)
        assert _same_bytes(res[key], rows), key
        img = ox.scatter(rows, pix, H * W, fill).reshape((H, W) + rows.shape[1:])
        assert _same_bytes(res[{"normals": "normal_map", "expert": "expert_map", "probs": "probs_map"}[key]], img), key
    assert not res["normal_map"][flying[:, 0], flying[:, 1]].any() and (res["expert_map"][flying[:, 0], flying[:, 1]] == -1).all()
    assert res["normal_map"][f["inlier"].reshape(H, W)].any(axis=-1).all()
    with pytest.raises(ValueError, match="outliers needs stride == 1"):
        estimator.estimate_depth(depth, cam, stride=2, outliers=o)


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------------

def _dataset(tmp_path, pts):
    d = tmp_path / "data"
    d.mkdir()
    np.savetxt(d / "box.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("box\n")
    return d, ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]


def _rows(path):
    return sum(1 for _ in open(path))


def test_command_line_statistical_model_free(tmp_path, gpu_device):
    """7.  ``--estimator pca --knn 12,24 --outliers statistical``: every file has the rows of the .xyz, .inliers and the normals are
    the Python call's."""
    from nesti_net_amd import pca, textio
    from nesti_net_amd.cli import main
    pts, _ = _small(gpu_device)
    d, common = _dataset(tmp_path, pts)
    results = str(tmp_path / "fit")
    assert main(["--estimator", "pca", "--knn", "12,24", "--outliers", "statistical", "--outlier_k", "8", "--outlier_passes", "2",
                 "--smooth", "1", "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    loaded = np.loadtxt(d / "box.xyz").astype("float32")
    res = pca.pca_normals(loaded, knn=(12, 24), smooth=1, outliers={"k": 8, "passes": 2}, device=str(gpu_device))
    files = sorted(os.listdir(out))
    assert files == sorted(["log.txt"] + ["box" + e for e in (".normals", ".pca_eig", ".pca_count", ".knn_radius", ".smooth_support",
                                                              ".inliers", ".outlier_score")])
    for name in files:
        if name != "log.txt":
            assert _rows(os.path.join(out, name)) == len(pts), name
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.inliers")).astype(bool), res["inlier"]) and 0 < (~res["inlier"]).sum() < len(pts)
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.outlier_score")), res["outlier_score"])
    want = str(tmp_path / "want.normals")
    textio.write_f32(want, res["normals"])
    assert open(os.path.join(out, "box.normals"), "rb").read() == open(want, "rb").read()
    log = open(os.path.join(out, "log.txt")).read()
    assert "outlier filter of box (statistical" in log and "%d of %d rows removed in 2 passes; threshold " % ((~res["inlier"]).sum(), len(pts)) in log


def test_command_line_radius_network(tmp_path, gpu_device):
    """7.  ``--outliers radius`` with the network on synthetic weights: every file has the rows of the .xyz, a removed row is
    0 0 0 / -1 / 0, .inliers is the Python result."""
    from nesti_net_amd import outliers
    from nesti_net_amd.cli import main
    pts, _ = _small(gpu_device)
    d, common = _dataset(tmp_path, pts)
    results = str(tmp_path / "net")
    assert main(["--synthetic_weights", "--outliers", "radius", "--outlier_radius", "0.25", "--outlier_k", "5", "--results_path", results]
                + common) == 0
    out = os.path.join(results, "synth_results")
    f = outliers.remove_outliers(np.loadtxt(d / "box.xyz").astype("float32"), mode="radius", radius=0.25, min_neighbours=5, device=str(gpu_device))
    assert {"box.normals", "box.experts", "box.experts_probs", "box.inliers", "box.outlier_score", "log.txt"} <= set(os.listdir(out))
    for e in (".normals", ".experts", ".experts_probs", ".inliers", ".outlier_score"):
        assert _rows(os.path.join(out, "box" + e)) == len(pts), e
    inl = np.loadtxt(os.path.join(out, "box.inliers")).astype(bool)
    assert np.array_equal(inl, f["inlier"]) and 0 < (~inl).sum() < len(pts)
    normals, experts = np.loadtxt(os.path.join(out, "box.normals")), np.loadtxt(os.path.join(out, "box.experts"))
    probs = np.loadtxt(os.path.join(out, "box.experts_probs"))
    assert not normals[~inl].any() and (experts[~inl] == -1).all() and not probs[~inl].any()
    assert normals[inl].any(axis=1).all() and (experts[inl] >= 0).all()
    assert "outlier filter of box (radius: at least 5 other points within 0.25): %d of %d rows removed in 1 pass; threshold 0.0625" \
        % ((~inl).sum(), len(pts)) in open(os.path.join(out, "log.txt")).read()
