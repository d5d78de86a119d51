"""Voxel downsampling without a GPU: every refusal of ``nesti_voxel_keys``, ``nesti_sort_pairs`` and ``nesti_voxel_reduce`` through
ctypes (each returns before any device call), the workspace size and the sort's tile, the range checks of the Python layer, the grid
(dims, the 2^62 refusal, ``key_bits``), the ``--voxel_*`` parser errors, and the tests' restatement (tests/_voxel_fixture.py) held to
independent statements: its centroid against ``np.mean``, a lane group against the 64-lane statement, its voxel sets against a
dictionary of cells."""
import ctypes

import numpy as np
import pytest

import _voxel_fixture as vx


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------

def _refused(lib, entry, rc, word):
    msg = lib.nesti_last_error() or b""
    assert rc != 0 and word.encode() in msg and msg.startswith((entry + ":").encode()), (entry, rc, msg, word)


def _d3(*v):
    return (ctypes.c_double * 3)(*v)


def _i3(*v):
    return (ctypes.c_int64 * 3)(*v)


def test_refusals_need_no_device():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    dummy, other = np.zeros(8, np.float64), np.zeros(8, np.float64)          # never dereferenced: the checks come first
    p, q = ctypes.c_void_p(dummy.ctypes.data), ctypes.c_void_p(other.ctypes.data)
    N = 1000
    ws = lib.nesti_voxel_workspace_bytes(N)
    assert lib.nesti_voxel_workspace_bytes(0) == 0 and lib.nesti_voxel_workspace_bytes(-1) == 0
    sizes = [lib.nesti_voxel_workspace_bytes(n) for n in (1, 2, 1000, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 24)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[2] > 0
    assert sizes[-1] >= (1 << 24) * 12                                        # a second (key, index) buffer at the least
    T = lib.nesti_sort_tile_items()
    assert T > 0 and T == lib.nesti_sort_tile_items()
    o, v, d = _d3(0.0, -1.0, 2.0), _d3(0.1, 0.2, 0.3), _i3(10, 20, 30)

    def keys(cloud=p, n=N, org=o, vox=v, dims=d, out=p):
        return lib.nesti_voxel_keys(cloud, n, org, vox, dims, out, None)

    e = "nesti_voxel_keys"
    for kw in ({"cloud": None}, {"org": None}, {"vox": None}, {"dims": None}, {"out": None}):
        _refused(lib, e, keys(**kw), "null")
    _refused(lib, e, keys(n=0), "empty cloud")
    _refused(lib, e, keys(n=-3), "empty cloud")
    for bad in (0.0, -0.1, np.nan, np.inf, -np.inf):
        for a in range(3):
            vv = [0.1, 0.2, 0.3]
            vv[a] = bad
            _refused(lib, e, keys(vox=_d3(*vv)), "voxel sizes must be finite and > 0")
    for bad in (np.nan, np.inf, -np.inf):
        _refused(lib, e, keys(org=_d3(0.0, bad, 0.0)), "origin must be finite")
    for dd in ((0, 20, 30), (10, -1, 30), (10, 20, 0)):
        _refused(lib, e, keys(dims=_i3(*dd)), "dims must be >= 1")
    for dd in ((1 << 31, 1 << 31, 1), (1 << 62, 1, 1), (1 << 40, 1 << 40, 1 << 40), ((1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 1),
               (1 << 21, 1 << 21, 1 << 20)):
        _refused(lib, e, keys(dims=_i3(*dd)), "the number of cells must be below 2^62")

    def sort(kin=p, n=N, bits=32, kout=q, iout=p, w=p, nbytes=ws):
        return lib.nesti_sort_pairs(kin, n, bits, kout, iout, w, nbytes, None)

    e = "nesti_sort_pairs"
    for kw in ({"kin": None}, {"kout": None}, {"iout": None}, {"w": None}):
        _refused(lib, e, sort(**kw), "null")
    _refused(lib, e, sort(n=0), "N must be > 0")
    _refused(lib, e, sort(n=-1), "N must be > 0")
    for bits in (0, -1, 65, 128):
        _refused(lib, e, sort(bits=bits), "key_bits must be in 1 .. 64")
    _refused(lib, e, sort(nbytes=ws - 1), "workspace too small")
    _refused(lib, e, sort(n=1, bits=1, nbytes=0), "workspace too small")
    _refused(lib, e, sort(kout=p), "keys_out must not be keys_in")

    def reduce(cloud=p, n=N, sk=p, si=p, org=o, nv=p, w=p, nbytes=ws, outs=(p, p, p, p, p)):
        return lib.nesti_voxel_reduce(cloud, n, sk, si, 6000, org, *outs, nv, w, nbytes, None)

    e = "nesti_voxel_reduce"
    for kw in ({"cloud": None}, {"sk": None}, {"si": None}, {"org": None}, {"nv": None}, {"w": None}):
        _refused(lib, e, reduce(**kw), "null")
    _refused(lib, e, reduce(n=0), "empty cloud")
    _refused(lib, e, reduce(n=-1), "empty cloud")
    for bad in (np.nan, np.inf, -np.inf):
        _refused(lib, e, reduce(org=_d3(bad, 0.0, 0.0)), "origin must be finite")
    _refused(lib, e, reduce(nbytes=ws - 1), "workspace too small")
    _refused(lib, e, reduce(nbytes=ws - 1, outs=(None,) * 5), "workspace too small")      # the NULL-able outputs are no error


# ---- 2. the Python layer ---------------------------------------------------------------------------------------------------------------

def test_python_layer_validates():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import downsample as ds, hough, pca, quadric, robust, select
    p = ds.check_params(0.1)
    assert p == ((0.1, 0.1, 0.1), "centroid", None) and ds.as_params(None) is None and ds.as_params(0.1) == p and ds.as_params(p) == p
    assert ds.as_params(np.float32(0.5)).voxel == (0.5, 0.5, 0.5) and ds.as_params(2).voxel == (2.0, 2.0, 2.0)
    assert ds.as_params([0.1, 0.2, 0.3]).voxel == (0.1, 0.2, 0.3) and ds.as_params((1, 2, 3)).voxel == (1.0, 2.0, 3.0)
    q = ds.as_params({"voxel": 0.2, "mode": "nearest", "origin": [0, -1, 2]})
    assert q == ((0.2, 0.2, 0.2), "nearest", (0.0, -1.0, 2.0)) and ds.as_params({"voxel": (1, 2, 3)}).mode == "centroid"
    for kw, word in (({"voxel": 0}, "voxel must be"), ({"voxel": -1.0}, "voxel must be"), ({"voxel": float("nan")}, "voxel must be"),
                     ({"voxel": float("inf")}, "voxel must be"), ({"voxel": [0.1, 0.2]}, "voxel must be"), ({"voxel": [0.1, 0.0, 0.1]}, "voxel must be"),
                     ({"voxel": "fine"}, "voxel must be"), ({"voxel": True}, "voxel must be"), ({"voxel": None}, "voxel must be"),
                     ({"voxel": 0.1, "mode": "median"}, "mode must be"), ({"voxel": 0.1, "origin": [0, 1]}, "origin must be"),
                     ({"voxel": 0.1, "origin": [0, float("nan"), 0]}, "origin must be"), ({"voxel": 0.1, "origin": [0, float("inf"), 0]}, "origin must be")):
        with pytest.raises(ValueError, match=word):
            ds.check_params(**kw)
        with pytest.raises(ValueError, match=word):
            ds.as_params(kw)
        with pytest.raises(ValueError, match=word):
            ds.voxel_downsample(np.zeros((10, 3), np.float32), **kw)
    for bad, word in (("centroid", "downsample must be"), (True, "downsample must be"), ({"size": 2}, "unknown key"), ({"mode": "nearest"}, "needs 'voxel'")):
        with pytest.raises(ValueError, match=word):
            ds.as_params(bad)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        ds.voxel_downsample(np.zeros((10, 2), np.float32), 0.1)
    for bits in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="key_bits must be"):
            ds.check_key_bits(bits)
    assert ds.check_key_bits(1) == 1 and ds.check_key_bits(64) == 64
    for dims, word in (((0, 1, 1), "dims must be"), ((1, 2), "dims must be"), ((1 << 31, 1 << 31, 1), "below 2\\^62")):
        with pytest.raises(ValueError, match=word):
            ds.check_grid((0, 0, 0), 0.1, dims)
    # an empty cloud gives empty arrays, without a device
    e = ds.voxel_downsample(np.zeros((0, 3), np.float32), 0.1, mode="nearest")
    assert e["points"].shape == (0, 3) and e["centroid"].shape == (0, 3) and e["cell"].shape == (0, 3) and e["key"].dtype == np.uint64
    assert all(len(e[k]) == 0 for k in ("rep", "count", "key", "voxel_of")) and e["rep"].dtype == np.int64 and e["count"].dtype == np.int32
    # downsample= of the estimators: the ranges and the pidx refusal come before anything is prepared
    pts = np.zeros((10, 3), np.float32)
    for fit, kw in ((pca.pca_normals, {}), (pca.pca_normals, {"knn": 8}), (quadric.quadric_fit, {}), (hough.hough_normals, {"knn": 8}),
                    (robust.robust_normals, {"knn": 8}), (select.select_normals, {})):
        with pytest.raises(ValueError, match="downsample with pidx is not served yet"):
            fit(pts, pidx=[0, 1], downsample=0.1, **kw)
        with pytest.raises(ValueError, match="voxel must be"):
            fit(pts, downsample=0, **kw)
        with pytest.raises(ValueError, match="k must"):                       # the filter's ranges too, before any work
            fit(pts, downsample=0.1, outliers={"k": 0}, **kw)
        with pytest.raises(ValueError, match="an empty cloud"):
            fit(np.zeros((0, 3), np.float32), downsample=0.1, **kw)
    # the host gather: the voxels' rows to the rows of the input
    res = {"normals": np.array([[1, 1], [2, 2], [3, 3]], np.float32), "expert": np.array([4, 5, 6], np.int32), "orient": {"n_flipped": 1},
           "scalar": 3, "other": np.ones(4)}
    back = ds.gather_result(res, np.array([2, 0, -1, 2, 1]), 3)
    assert back["normals"].dtype == np.float32 and back["normals"].tolist() == [[3, 3], [1, 1], [0, 0], [3, 3], [2, 2]]
    assert back["expert"].tolist() == [6, 4, -1, 6, 5] and back["orient"] == {"n_flipped": 1} and back["scalar"] == 3 and back["other"] is res["other"]


def test_the_grid_of_a_cloud():
    """dims as the kernel computes a cell, at least 1; ``key_bits`` the bit length of the lost key; the 2^62 refusal names the voxel size."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import downsample as ds
    lo, hi = np.array([-1.0, 0.0, 2.0], np.float32), np.array([1.0, 0.0, 2.75], np.float32)
    origin, voxel, dims, lost, bits = ds.grid_of(lo, hi, ds.check_params(0.25))
    assert origin == (-1.0, 0.0, 2.0) and dims == (9, 1, 4) and lost == 36 and bits == 6          # the maximum corner opens a cell of its own
    assert ds.grid_of(lo, hi, ds.check_params((0.3, 5.0, 0.75)))[2] == (7, 1, 2)
    assert ds.grid_of(lo, lo, ds.check_params(1e-3))[2:] == ((1, 1, 1), 1, 1)
    assert ds.grid_of(lo, hi, ds.check_params(0.25, origin=(5.0, 5.0, 5.0)))[2] == (1, 1, 1)       # an origin above the cloud: every row is lost
    o, _, d, lost, bits = ds.grid_of(lo, hi, ds.check_params(1.0, origin=(-3.0, -3.0, -3.0)))
    assert o == (-3.0, -3.0, -3.0) and d == (5, 4, 6) and lost == 120 and bits == 7
    for v, want in ((2.0 ** -20, 41), (2.0 ** -10, 21)):                                           # (2 / v + 1) x 1 x (0.75 / v + 1) cells
        d, lost, bits = ds.grid_of(lo, hi, ds.check_params(v))[2:]
        assert d == (int(2 / v) + 1, 1, int(0.75 / v) + 1) and lost == d[0] * d[2] and bits == lost.bit_length() == want
    wide = np.array([1.0, 1.0, 3.0], np.float32)
    for v in (1e-7, 1e-30, 5e-324):
        with pytest.raises(ValueError, match="voxel size .* is too small for this cloud"):
            ds.grid_of(lo, wide, ds.check_params(v))
    with pytest.raises(ValueError, match="voxel size .*1e-07.* is too small for this cloud"):
        ds.voxel_downsample(np.stack([lo, wide]), 1e-7)
    # a cloud whose grid has exactly 2^62 cells is refused, one cell fewer along an axis is served
    lo0 = np.zeros(3, np.float32)
    hi62 = np.array([2.0 ** 21 - 1, 2.0 ** 21 - 1, 2.0 ** 20 - 1], np.float32)
    with pytest.raises(ValueError, match="too small"):
        ds.grid_of(lo0, hi62, ds.check_params(1.0))
    hi61 = np.array([2.0 ** 21 - 1, 2.0 ** 21 - 1, 2.0 ** 20 - 2], np.float32)
    assert ds.grid_of(lo0, hi61, ds.check_params(1.0))[3:] == ((1 << 62) - (1 << 42), 62)
    # the restatement's grid is the library's
    rs = np.random.RandomState(5)
    pts = rs.uniform(-1, 1, (500, 3)).astype(np.float32)
    for v in (0.3, (0.1, 0.25, 0.7), 1e-4):
        o, vox, dims, lost, bits = vx.grid_of(pts, v)
        assert ds.grid_of(pts.min(0), pts.max(0), ds.check_params(v)) == (tuple(o), tuple(vox), tuple(dims), lost, bits)
    assert ds.cells_of(np.array([0, 35, 17], np.uint64), (9, 1, 4)).tolist() == [[0, 0, 0], [8, 0, 3], [8, 0, 1]]


# ---- 3. the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, word", [
    (["--voxel_size", "0.1"], "--voxel_size does not go with --estimator net: left for later"),
    (["--voxel_size", "0.1", "--depth_images", "1"], "--voxel_size does not go with --depth_images 1: left for later"),
    (["--estimator", "pca", "--voxel_size", "0.1", "--sparse_patches", "1"], "--voxel_size does not go with --sparse_patches 1: left for later"),
    (["--estimator", "quadric", "--voxel_size", "0.1", "--query_positions", "1"], "--voxel_size does not go with --query_positions 1: left for later"),
    (["--estimator", "pca", "--voxel_size", "0.1", "--subsample", "reference"], "--voxel_size does not go with --subsample reference: left for later"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--voxel_size", "0.1", "--sparse_patches", "1"], "--voxel_size does not go with --sparse_patches 1"),
    (["--estimator", "robust", "--knn", "16", "--voxel_size", "0.1", "--query_positions", "1"], "--voxel_size does not go with --query_positions 1"),
    (["--estimator", "pca", "--voxel_mode", "nearest"], "--voxel_mode belongs to --voxel_size V"),
    (["--voxel_mode", "centroid"], "--voxel_mode belongs to --voxel_size V"),
    (["--estimator", "pca", "--voxel_size", "0.1", "--voxel_mode", "median"], "invalid choice"),
    (["--estimator", "pca", "--voxel_size", "-1"], "voxel must be a finite positive number"),
    (["--estimator", "hough", "--knn", "16", "--voxel_size", "inf"], "voxel must be a finite positive number"),
    (["--estimator", "pca", "--voxel_size", "nan"], "voxel must be a finite positive number"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and not (tmp_path / "out").exists()       # refused while parsing: nothing was created


# ---- 4. the restatement ------------------------------------------------------------------------------------------------------------------

def _cloud(n, seed, dup=True):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-1, 1, (n, 3)).astype(np.float32)
    if dup and n > 20:
        pts[n // 2] = pts[3]
        pts[n - 1] = pts[3]
    return pts


def test_lane_group_gives_the_bytes_of_the_wave():
    """A group of 16 lanes with four accumulators, met as (a0 + a2) + (a1 + a3), and a group of 32 with two give the bytes of the
    64-lane statement for counts 1 .. 200 -- every term is >= +0 --, and the batched sums of ``reduce`` are ``lane_sum``'s."""
    rs = np.random.RandomState(11)
    for count in range(1, 201):
        d = rs.uniform(0, 3, (count, 3)) * 10.0 ** rs.randint(-6, 3, (count, 3))
        if count % 7 == 0:
            d[rs.randint(count)] = 0.0
        want = vx.lane_sum(d, 64)
        assert want.tobytes() == vx.lane_sum(d, 16).tobytes() == vx.lane_sum(d, 32).tobytes(), count
        got = vx._lane_sums(d, np.array([0]), np.array([count]))[0]
        assert got.tobytes() == want.tobytes(), count
        assert np.all(np.abs(want - d.sum(0)) <= 1e-13 * d.sum(0))
    # -0.0 terms (a point at -0.0 over an origin of +0.0) leave +0.0, in every form
    z = np.full((5, 3), -0.0)
    for g in (16, 32, 64):
        assert vx.lane_sum(z, g).tobytes() == np.zeros(3).tobytes()


@pytest.mark.parametrize("n, voxel, seed", [(1, 0.5, 0), (2, 0.5, 1), (300, 0.5, 2), (3000, 0.11, 3), (3000, (0.05, 0.3, 1.1), 4), (2000, 3.0, 5)])
def test_restatement_against_a_dictionary_of_cells(n, voxel, seed):
    """The voxel sets equal a dictionary-of-cells brute force; voxels come in ascending key order; the centroid is within 1 ulp (f32) of
    ``np.mean`` in fp64; ``rep`` is a row of the voxel at the least distance, the lowest index among such rows."""
    pts = _cloud(n, seed)
    r = vx.downsample(pts, voxel)
    origin, vox, dims = r["origin"], r["voxel"], r["dims"]
    cells = {}
    for i, p in enumerate(pts):
        c = tuple(int(np.floor((np.float64(p[a]) - origin[a]) / vox[a])) for a in range(3))
        assert all(0 <= c[a] < dims[a] for a in range(3))
        cells.setdefault(c, []).append(i)
    order = sorted(cells, key=lambda c: (c[2], c[1], c[0]))
    assert len(order) == len(r["rep"]) and [list(c) for c in order] == r["cell"].tolist()
    assert (np.diff(r["key"].astype(np.int64)) > 0).all() and r["count"].sum() == n
    for v, c in enumerate(order):
        rows = np.array(cells[c])
        assert r["count"][v] == len(rows) and (r["voxel_of"][rows] == v).all()
        mean = pts[rows].astype(np.float64).mean(0)
        got = r["centroid"][v]
        ulp = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - mean) <= ulp), (v, got, mean)
        d2 = ((pts[rows].astype(np.float64) - mean) ** 2).sum(1)
        assert r["rep"][v] in rows and d2[list(rows).index(r["rep"][v])] <= d2.min() * (1 + 1e-9) + 1e-30
    near = vx.downsample(pts, voxel, mode="nearest")
    assert near["points"].tobytes() == pts[r["rep"]].tobytes() and near["rep"].tolist() == r["rep"].tolist()


def test_restatement_ties_duplicates_and_lost_rows():
    """Identical points in one voxel: ``rep`` the lowest index; an equidistant pair: the lower index; a caller's origin loses the rows
    below it and at or above the dims; non-finite rows are lost."""
    pts = np.array([[0.25, 0.25, 0.25]] * 4 + [[1.25, 0.25, 0.25], [1.75, 0.25, 0.25]], np.float32)
    r = vx.downsample(pts, 1.0, origin=(0.0, 0.0, 0.0))
    assert r["rep"].tolist() == [0, 4] and r["count"].tolist() == [4, 2] and r["voxel_of"].tolist() == [0, 0, 0, 0, 1, 1]
    assert r["centroid"].tolist() == [[0.25, 0.25, 0.25], [1.5, 0.25, 0.25]]
    origin, voxel, dims = np.zeros(3), np.ones(3), [2, 2, 2]
    pts = np.array([[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, 2.0, 0.5], [1.5, 1.5, 1.5], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
                    [-0.0, 0.0, 1.0], [1e30, 0, 0]], np.float32)
    k = vx.keys(pts, origin, voxel, dims)
    assert k.tolist() == [0, 8, 8, 7, 8, 8, 8, 4, 8]
    sk, si = vx.sort_pairs(k, 4)
    assert sk.tolist() == [0, 4, 7, 8, 8, 8, 8, 8, 8] and si.tolist() == [0, 7, 3, 1, 2, 4, 5, 6, 8]
    red = vx.reduce(pts, sk, si, 8, origin)
    assert red["V"] == 3 and red["voxel_of"].tolist() == [0, -1, -1, 2, -1, -1, -1, 1, -1] and red["count"].tolist() == [1, 1, 1]
    # bits above key_bits are carried and ignored: the order is that of the low bits, stable
    key = np.array([0x10, 0x01, 0x11, 0x00, 0x21], np.uint64)
    sk, si = vx.sort_pairs(key, 4)
    assert si.tolist() == [0, 3, 1, 2, 4] and sk.tolist() == [0x10, 0x00, 0x01, 0x11, 0x21]


def test_downsample_none_leaves_an_estimator_untouched(monkeypatch):
    """With no stage given no primitive of the preprocessing chain is entered and the estimator's arguments reach its preparation as
    they were given."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import denoise, downsample as ds, outliers, pca
    seen = {}

    def prepare(*args):
        seen["args"] = args
        raise RuntimeError("stop here")

    def never(*a, **kw):
        raise AssertionError("a stage was entered")

    monkeypatch.setattr(pca, "prepare_cloud", prepare)
    monkeypatch.setattr(ds, "voxel_downsample", never)
    monkeypatch.setattr(outliers, "remove_outliers", never)
    monkeypatch.setattr(denoise, "denoise_points", never)
    pts = np.zeros((10, 3), np.float32)
    with pytest.raises(RuntimeError, match="stop here"):
        pca.pca_normals(pts, knn=8, scale=0, orient_k=4)
    assert seen["args"][0] is pts and seen["args"][1:] == (None, None, None, 0, None, None, 4, "cuda:0", 8, None)
    with pytest.raises(RuntimeError, match="stop here"):
        pca.pca_normals(pts, knn=8, scale=0, orient_k=4, downsample=None)
    assert seen["args"][0] is pts and seen["args"][1:] == (None, None, None, 0, None, None, 4, "cuda:0", 8, None)
    # as_params / gather pass None and foreign values through
    assert ds.as_params(None) is None
    res = {"a": 1, "b": np.arange(3)}
    back = ds.gather_result(res, np.array([0, 0]), 5)
    assert back["a"] == 1 and back["b"] is res["b"]
