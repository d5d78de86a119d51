"""The preprocessing chain (``stages.py``; DESIGN.md 2 "The preprocessing chain") without a GPU: the three primitives are replaced by the
tests' own restatements -- the voxel grid and the outlier filter -- and a deterministic stand-in for the denoising, and the chain's
points, its composed row map, the taken ``init`` and the mapped-back result are compared, for all eight on/off combinations, with the
stage-by-stage route written out here over ``downsample.gather_host`` and ``outliers.scatter_host``."""
import itertools

import numpy as np
import pytest

import _outliers_fixture as of
import _voxel_fixture as vx

DOWNSAMPLE = {"voxel": 0.25, "origin": (0.0, 0.0, 0.0)}
OUTLIERS = {"k": 4, "std_ratio": 1.0}
DENOISE = {"k": 5, "iters": 1}
FAR, OUTSIDE, DUPLICATES = (55, 56, 57), 58, (3, 20, 40)


def _cloud():
    """60 points: the unit cube, three rows on one spot (one voxel), three far points inside the grid that the filter removes, one
    point below the grid's origin (``voxel_of`` -1) and one spare row."""
    pts = np.random.RandomState(7).uniform(0.05, 0.95, (60, 3)).astype(np.float32)
    pts[list(DUPLICATES)] = pts[3]
    pts[list(FAR)] = [[6, 6, 6], [7, 1, 5], [1, 8, 2]]
    pts[OUTSIDE] = [-0.5, 0.5, 0.5]
    return pts


def _denoise(pts, k, iters, angle, falloff, sigma, step, normals, normal_k, device="cuda:0"):
    """A stand-in with the keys of ``denoise.denoise_points``: every row moves along z by a function of its own bits."""
    assert normals is None
    pts = np.ascontiguousarray(pts, np.float32)
    delta = (np.float32(0.01) * (1 + np.abs(pts).sum(1))).astype(np.float32)
    out = pts.copy()
    out[:, 2] += delta
    return {"points": out, "delta": delta, "support": np.ones(len(pts), np.float32), "count": np.full(len(pts), k, np.int32), "moved": len(pts)}


def _estimator(points):
    """A fake estimator: per-row arrays that name their row, a dict, a scalar and an array that is not per row."""
    rows = len(points)
    return {"normals": np.arange(rows, dtype=np.float32)[:, None] * np.float32(0.5) + points, "expert": np.arange(rows, dtype=np.int32) % 7,
            "orient": {"n_flipped": 1}, "scalar": 3, "other": np.ones(rows + 1)}


@pytest.fixture
def lib(monkeypatch):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import denoise, downsample, outliers, stages
    calls = []

    def voxel_downsample(pts, voxel, mode="centroid", origin=None, device="cuda:0"):
        calls.append("downsample")
        return vx.downsample(pts, voxel, mode, origin)

    def remove_outliers(pts, mode, k, std_ratio, radius, min_neighbours, passes, device="cuda:0"):
        calls.append("outliers")
        return of.remove(pts, mode, k, std_ratio, radius, min_neighbours, passes)

    def denoise_points(*args, **kw):
        calls.append("denoise")
        return _denoise(*args, **kw)

    monkeypatch.setattr(downsample, "voxel_downsample", voxel_downsample)
    monkeypatch.setattr(outliers, "remove_outliers", remove_outliers)
    monkeypatch.setattr(denoise, "denoise_points", denoise_points)
    return stages, downsample, outliers, calls


def _manual(ds, ol, pts, init, on):
    """The route stage by stage: (points, src, init, result, the stage outputs)."""
    D, O, Dn = on
    cur, start = pts, init
    vd = f = d = None
    if D:
        vd = vx.downsample(pts, (0.25, 0.25, 0.25), "centroid", DOWNSAMPLE["origin"])
        cur, start = vd["points"], start[vd["rep"]]
    if O:
        f = of.remove(cur, "statistical", OUTLIERS["k"], OUTLIERS["std_ratio"], None, None, 1)
        full, cur, start = len(cur), f["points"], start[f["kept"]]
    if Dn:
        d = _denoise(cur, 5, 1, 45.0, 0.75, 0.5, 1.0, None, 10)
        cur = d["points"]
    res = _estimator(cur)
    src = np.arange(len(cur), dtype=np.int64)
    per_row, fills = ("normals", "expert", "points", "denoise_delta", "inlier", "outlier_score"), {"expert": -1}
    if Dn:
        res.update(points=d["points"], denoise_delta=d["delta"])
    if O:
        src = ol.scatter_host(src, f["kept"], full, -1)
        res = {k: ol.scatter_host(v, f["kept"], full, fills.get(k, 0)) if k in per_row else v for k, v in res.items()}
        res.update(inlier=f["inlier"], outlier_score=f["score"], outlier_passes=f["passes"])
    if D:
        src = ds.gather_host(src, vd["voxel_of"], -1)
        res = {k: ds.gather_host(v, vd["voxel_of"], fills.get(k, 0)) if k in per_row else v for k, v in res.items()}
        res.update(voxel_of=vd["voxel_of"], voxel_points=vd["points"], voxel_count=vd["count"])
    return cur, src, start, res, (vd, f, d)


@pytest.mark.parametrize("on", list(itertools.product((False, True), repeat=3)), ids=lambda on: "".join("DOd"[i] if b else "-" for i, b in enumerate(on)))
def test_chain_against_the_route_stage_by_stage(lib, on):
    stages, ds, ol, calls = lib
    pts = _cloud()
    init = np.random.RandomState(8).normal(size=(60, 3)).astype(np.float32)
    params = stages.check(DOWNSAMPLE if on[0] else None, OUTLIERS if on[1] else None, DENOISE if on[2] else None, None)
    chain = stages.run(pts, params)
    want_pts, want_src, want_init, want, (vd, f, d) = _manual(ds, ol, pts, init, on)
    assert calls == [name for name, b in zip(("downsample", "outliers", "denoise"), on) if b]
    if not any(on):
        assert params is None and chain.points is pts and chain.keys == {} and chain.kept is None and chain.take(init) is init
        res = _estimator(pts)
        assert chain.back(res) is res
    else:
        assert chain.points.dtype == np.float32 and chain.points.tobytes() == want_pts.tobytes()
    assert chain.n == 60 and chain.src.dtype == np.int64 and chain.src.tolist() == want_src.tolist()
    assert chain.take(init).tobytes() == want_init.tobytes() and chain.take(None) is None
    if on[0]:                                                  # the cloud is what the stages are meant to meet
        assert vd["voxel_of"][OUTSIDE] == -1 and len(set(vd["voxel_of"][list(DUPLICATES)])) == 1 and 20 <= len(vd["rep"]) < 59
        assert chain.src[OUTSIDE] == -1
    if on[1]:
        gone = np.flatnonzero(~f["inlier"])
        assert 3 <= len(gone) <= 6 and chain.kept is not None and chain.kept.tolist() == f["kept"].tolist()
        assert (chain.src[list(FAR)] == -1).all()
    est = _estimator(chain.points)
    back = chain.back(dict(est))
    assert list(back) == list(want)
    for key, v in want.items():
        if isinstance(v, np.ndarray):
            assert back[key].dtype == v.dtype and back[key].shape == v.shape and back[key].tobytes() == v.tobytes(), key
        else:
            assert back[key] == v, key
    assert back["orient"] is est["orient"] and back["other"] is est["other"] and back["scalar"] == 3
    lost = chain.src == -1
    assert (back["expert"][lost] == -1).all() and (back["normals"][lost] == 0).all() and lost.any() == (on[0] or on[1])
    live = ~lost
    assert back["expert"][live].tolist() == est["expert"][chain.src[live]].tolist()
    shapes = {"inlier": (60,), "outlier_score": (60,), "points": (60, 3), "denoise_delta": (60,), "voxel_of": (60,)}
    for key, shape in shapes.items():
        assert key not in back or back[key].shape == shape, key
    if on[0]:
        V = len(vd["rep"])
        assert back["voxel_points"].shape == (V, 3) and back["voxel_count"].shape == (V,) and back["voxel_count"].dtype == np.int32
    if on[1]:
        assert back["inlier"].dtype == bool and back["outlier_score"].dtype == np.float64 and back["outlier_passes"] == f["passes"]


def test_queries_map_nothing(lib):
    """With ``queries`` the estimator's rows are positions: nothing is mapped, ``init`` is left alone and the keys of a stage keep the
    rows of the cloud that stage ran on."""
    stages, ds, ol, calls = lib
    pts = _cloud()
    queries = pts[::7] + np.float32(0.01)
    init = np.ones((len(queries), 3), np.float32)
    chain = stages.run(pts, stages.check(DOWNSAMPLE, OUTLIERS, DENOISE, None), queries)
    want_pts, _, _, _, (vd, f, d) = _manual(ds, ol, pts, np.zeros((60, 3), np.float32), (True, True, True))
    assert chain.points.tobytes() == want_pts.tobytes() and chain.take(init) is init
    res = {"normals": np.ones((len(chain.points), 3), np.float32), "expert": np.zeros(len(queries), np.int32)}
    back = chain.back(dict(res))
    assert back["normals"] is res["normals"] and back["expert"] is res["expert"]
    V, K = len(vd["rep"]), len(f["kept"])
    assert V > K and back["inlier"].tobytes() == f["inlier"].tobytes() and back["inlier"].shape == (V,) and back["outlier_score"].shape == (V,)
    assert back["points"].shape == (K, 3) and back["denoise_delta"].shape == (K,) and back["voxel_of"].shape == (60,)
    assert back["voxel_points"].shape == (V, 3) and back["voxel_count"].shape == (V,)


def test_check_precedence_and_refusals(lib):
    """Every ``ValueError`` of the three stages comes from ``check`` before any primitive runs: denoise, then downsample, then
    outliers; ``run`` refuses an empty cloud, a grid that catches no point and a filter that keeps no point."""
    stages, ds, ol, calls = lib
    with pytest.raises(ValueError, match="denoise: unknown key"):
        stages.check(0, {"k": 0}, {"bad": 1}, [0])
    with pytest.raises(ValueError, match="denoise with pidx is not served"):
        stages.check(0, {"k": 0}, True, [0])
    with pytest.raises(ValueError, match="voxel must be"):
        stages.check(0, {"k": 0}, None, [0])
    with pytest.raises(ValueError, match="downsample with pidx is not served yet"):
        stages.check(0.1, {"k": 0}, False, [0])
    with pytest.raises(ValueError, match="k must be"):
        stages.check(0.1, {"k": 0}, None, None)
    with pytest.raises(ValueError, match="outliers with pidx is not served yet"):
        stages.check(None, "statistical", None, [0])
    assert stages.check(None, None, False, [0]) is None and stages.check(None, None, None, None) is None
    p = stages.check(0.1, "statistical", True, None)
    assert p.downsample.voxel == (0.1, 0.1, 0.1) and p.outliers.k == 16 and p.denoise.iters == 2
    with pytest.raises(ValueError, match="pts must be \\[N, 3\\]"):
        stages.run(np.zeros((4, 2), np.float32), p)
    with pytest.raises(ValueError, match="downsample: an empty cloud"):
        stages.run(np.zeros((0, 3), np.float32), p)
    assert calls == []
    with pytest.raises(ValueError, match="downsample: none of the 60 points lies in the grid of origin"):
        stages.run(_cloud(), stages.check({"voxel": 0.25, "origin": 50.0}, "statistical", None, None))
    assert calls == ["downsample"]
    with pytest.raises(ValueError, match="outliers: the filter kept none of the 0 points"):
        stages.run(np.zeros((0, 3), np.float32), stages.check(None, "statistical", True, None))
    # the four kept names are thin functions over the one gather
    rows = np.array([[1, 1], [2, 2], [3, 3]], np.float32)
    assert ol.scatter_host(rows, [4, 0, 2], 5, 9).tolist() == [[2, 2], [9, 9], [3, 3], [9, 9], [1, 1]]
    assert ds.gather_host(rows, [2, -1, 0, 2]).tolist() == [[3, 3], [0, 0], [1, 1], [3, 3]]
    assert ol.FILLS is stages.FILLS and stages.inverse([4, 0, 2], 5).tolist() == [1, -1, 2, -1, 0]
