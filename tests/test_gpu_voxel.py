"""Voxel downsampling on the GPU (csrc/voxel.hip, ``CloudPatches.voxel_keys`` / ``sort_pairs`` / ``voxel_reduce``,
``downsample.voxel_downsample``, ``downsample=`` of the estimators, ``--voxel_size``) against the tests' own numpy restatement
(tests/_voxel_fixture.py): every output equal ON THE BYTES."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _voxel_fixture as vx

pytestmark = pytest.mark.gpu

OUTPUTS = ("centroid", "rep", "count", "key", "voxel_of")
_state = {}


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _lib():
    from nesti_net_amd import _lib as L
    return L, L.load()


def _tile():
    return _lib()[1].nesti_sort_tile_items()


def _random_keys(rs, n):
    return np.frombuffer(rs.bytes(8 * n), np.uint64).copy()


# ---- the C entries over device tensors (``CloudPatches`` refuses a cloud with a non-finite row, and a sort needs no cloud) -------------------

def _sort(keys, bits, dev, stream=None):
    L, lib = _lib()
    n = len(keys)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        kin = torch.from_numpy(keys.view(np.int64)).to(dev)
        kout = torch.full((n,), -7, dtype=torch.int64, device=dev)
        iout = torch.full((n,), -7, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.nesti_voxel_workspace_bytes(n), dtype=torch.uint8, device=dev)
        rc = lib.nesti_sort_pairs(L.ptr(kin), n, bits, L.ptr(kout), L.ptr(iout), L.ptr(ws), ws.numel(), ctypes.c_void_p(st.cuda_stream))
        assert rc == 0, lib.nesti_last_error()
        st.synchronize()
        assert np.array_equal(kin.cpu().numpy().view(np.uint64), keys)        # the input is left as it was
    return kout.cpu().numpy().view(np.uint64), iout.cpu().numpy()


def _keys(pts, origin, voxel, dims, dev):
    L, lib = _lib()
    with torch.cuda.device(dev):
        cloud = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
        out = torch.full((len(pts),), -7, dtype=torch.int64, device=dev)
        rc = lib.nesti_voxel_keys(L.ptr(cloud), len(pts), (ctypes.c_double * 3)(*[float(x) for x in origin]),
                                  (ctypes.c_double * 3)(*[float(x) for x in voxel]), (ctypes.c_int64 * 3)(*[int(x) for x in dims]),
                                  L.ptr(out), None)
        assert rc == 0, lib.nesti_last_error()
        torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint64)


def _reduce(pts, skeys, sidx, lost, origin, dev, outputs=OUTPUTS, stream=None):
    L, lib = _lib()
    N = len(pts)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    specs = {"centroid": ((N, 3), torch.float32), "rep": ((N,), torch.int32), "count": ((N,), torch.int32), "key": ((N,), torch.int64),
             "voxel_of": ((N,), torch.int32)}
    with torch.cuda.device(dev), torch.cuda.stream(st):
        cloud = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
        sk, si = torch.from_numpy(skeys.view(np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(sidx, np.int32)).to(dev)
        out = {k: torch.full(specs[k][0], -7, dtype=specs[k][1], device=dev) for k in outputs}
        nv = torch.full((1,), -7, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.nesti_voxel_workspace_bytes(N), dtype=torch.uint8, device=dev)
        rc = lib.nesti_voxel_reduce(L.ptr(cloud), N, L.ptr(sk), L.ptr(si), ctypes.c_uint64(int(lost)),
                                    (ctypes.c_double * 3)(*[float(x) for x in origin]), *[L.ptr(out.get(k)) for k in OUTPUTS], L.ptr(nv),
                                    L.ptr(ws), ws.numel(), ctypes.c_void_p(st.cuda_stream))
        assert rc == 0, lib.nesti_last_error()
        st.synchronize()
    V = int(nv.cpu()[0])
    res = {"V": V}
    for k, t in out.items():
        a = t.cpu().numpy()
        if k != "voxel_of":
            assert (a[V:] == -7).all(), (k, "rows beyond V are written")
            a = a[:V]
        res[k] = a.view(np.uint64) if k == "key" else a
    return res


def _check_reduce(got, ref, label, outputs=OUTPUTS):
    assert got["V"] == ref["V"], (label, got["V"], ref["V"])
    for k in outputs:
        assert _same_bytes(got[k], ref[k]), (label, k, np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(1))[:8])


def _pipeline(pts, origin, voxel, dims, dev, label, halves=True):
    """keys -> sort -> reduce on the device against the restatement, every stage on the bytes; the reduce again in two halves of the
    NULL-able outputs and on a second stream."""
    lost = int(dims[0]) * int(dims[1]) * int(dims[2])
    bits = lost.bit_length()
    key = _keys(pts, origin, voxel, dims, dev)
    ref_key = vx.keys(pts, origin, voxel, dims)
    assert _same_bytes(key, ref_key), (label, "keys", np.flatnonzero(key != ref_key)[:8])
    sk, si = _sort(key, bits, dev)
    rk, ri = vx.sort_pairs(ref_key, bits)
    assert _same_bytes(sk, rk) and _same_bytes(si, ri), (label, "sort")
    ref = vx.reduce(pts, rk, ri, lost, origin)
    _check_reduce(_reduce(pts, sk, si, lost, origin, dev), ref, label)
    if halves:
        for part in (("centroid", "count", "voxel_of"), ("rep", "key"), ()):
            _check_reduce(_reduce(pts, sk, si, lost, origin, dev, outputs=part, stream=torch.cuda.Stream(dev)), ref, (label, part), part)
    return ref_key, ref


# ---- 1. the sort: sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [1, 7, 8, 9, 16, 17, 33, 63, 64])
def test_sort_sizes(bits, gpu_device):
    """1.  Random 64-bit keys at sizes around the wave, the workgroup and the tile, every pass count: keys and indices are the stable
    argsort of the masked keys; the same bytes on a second stream."""
    T = _tile()
    rs = np.random.RandomState(100 + bits)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5, 65537):
        keys = _random_keys(rs, n)
        rk, ri = vx.sort_pairs(keys, bits)
        sk, si = _sort(keys, bits, gpu_device)
        assert _same_bytes(sk, rk) and _same_bytes(si, ri), (n, bits, np.flatnonzero(si != ri)[:8])
        sk, si = _sort(keys, bits, gpu_device, stream=torch.cuda.Stream(gpu_device))
        assert _same_bytes(sk, rk) and _same_bytes(si, ri), (n, bits, "second stream")


# ---- 2. the sort: stability and degenerate digits -----------------------------------------------------------------------------------------

def test_sort_stability_and_degenerate_digits(gpu_device):
    """2.  At N = 3T + 5: all keys equal (the identity); four distinct keys (indices ascend within a key); two keys that differ only in
    bit key_bits - 1; sorted and reverse sorted; every digit constant in all passes but one; bits above key_bits carried, not ordered."""
    T = _tile()
    n = 3 * T + 5
    rs = np.random.RandomState(7)
    cases = []
    for bits in (1, 8, 32, 64):
        cases.append(("all equal", np.full(n, (0xdeadbeefcafef00d & ((1 << bits) - 1)) | (1 << (bits - 1)), np.uint64), bits))
    for bits in (2, 8, 32):
        cases.append(("four keys", rs.randint(0, 4, n).astype(np.uint64), bits))
    for bits in (1, 8, 9, 33, 64):
        base = np.uint64(0x0123456789abcdef & ((1 << (bits - 1)) - 1))
        cases.append(("top bit", base | (rs.randint(0, 2, n).astype(np.uint64) << np.uint64(bits - 1)), bits))
    cases.append(("sorted", np.arange(n, dtype=np.uint64), 16))
    cases.append(("reverse sorted", np.arange(n, dtype=np.uint64)[::-1].copy(), 16))
    cases.append(("reverse sorted, 64 bits", (np.arange(n, dtype=np.uint64)[::-1] * np.uint64(0x9e3779b97f4a7c15 >> 14)).copy(), 64))
    for p in range(4):
        const = np.uint64(0x5a3c96e1 & ~(0xff << (8 * p)))
        cases.append(("one live digit %d" % p, const | (rs.randint(0, 256, n).astype(np.uint64) << np.uint64(8 * p)), 32))
    cases.append(("bits above", (_random_keys(rs, n) & ~np.uint64(0xf)) | rs.randint(0, 16, n).astype(np.uint64), 4))
    cases.append(("bits above, 12", _random_keys(rs, n), 12))
    for label, keys, bits in cases:
        rk, ri = vx.sort_pairs(keys, bits)
        sk, si = _sort(keys, bits, gpu_device)
        assert _same_bytes(sk, rk) and _same_bytes(si, ri), (label, bits, np.flatnonzero(si != ri)[:8])
        if label == "all equal":
            assert np.array_equal(si, np.arange(n))
        if label in ("four keys", "top bit", "bits above"):
            m = np.uint64((1 << bits) - 1)
            for k in np.unique(keys & m):
                assert (np.diff(si[(sk & m) == k]) > 0).all(), (label, bits, k)
        if label == "bits above":
            assert len(np.unique(sk >> np.uint64(4))) > n // 2 and _same_bytes(sk, keys[si])       # carried whole


# ---- 3. keys (and, on them, the sort and the reduce) ----------------------------------------------------------------------------------------

def test_keys_on_cell_faces_and_lost_rows(gpu_device):
    """3.  Points exactly on cell faces (a power-of-two voxel and one that is none), the maximum corner, an anisotropic voxel, a caller's
    origin and dims that lose rows on both sides, NaN and +-inf rows, dims of (1, 1, 1), dims whose product needs more than 32 bits."""
    rs = np.random.RandomState(21)
    origin = np.array([-1.0, 0.5, 2.0])
    for voxel in ((0.25, 0.25, 0.25), (0.3, 0.3, 0.3), (0.25, 0.3, 0.7)):
        m = rs.randint(0, 12, (600, 3))
        pts = (origin + m * np.asarray(voxel)).astype(np.float32)                          # on the faces, or one ulp to either side
        pts = np.concatenate([pts, (origin + 12 * np.asarray(voxel)).astype(np.float32)[None], origin.astype(np.float32)[None]])
        _, vox, dims, lost, _ = vx.grid_of(pts, voxel, origin)
        key, ref = _pipeline(pts, origin, vox, dims, gpu_device, ("faces", voxel))
        assert (key < lost).all() and key.max() == lost - 1                                 # the maximum corner has the last cell
        if voxel == (0.25, 0.25, 0.25):                                                    # exact in binary: cell m of every point
            assert np.array_equal(key[:600], ((m[:, 2] * dims[1] + m[:, 1]) * dims[0] + m[:, 0]).astype(np.uint64))
        # a caller's grid inside the cloud: rows below its origin and at or above its dims are lost
        inner = origin + 3 * np.asarray(voxel)
        key, ref = _pipeline(pts, inner, vox, (5, 4, 6), gpu_device, ("inner grid", voxel))
        assert 0 < (key == 120).sum() < len(pts) and (ref["voxel_of"] == -1).sum() == (key == 120).sum()
    # non-finite rows, through the C entry
    pts = rs.uniform(-1, 1, (300, 3)).astype(np.float32)
    pts[5, 1], pts[17, 0], pts[40, 2], pts[41] = np.nan, np.inf, -np.inf, (np.nan, np.inf, -np.inf)
    pts[299, 0] = np.nan                                                                   # the last row
    key, ref = _pipeline(pts, (-1.0, -1.0, -1.0), (0.25,) * 3, (8, 8, 8), gpu_device, "non-finite rows")
    assert np.flatnonzero(key == 512).tolist() == [5, 17, 40, 41, 299] and ref["V"] > 50
    # one cell
    key, ref = _pipeline(pts, (-1.0, -1.0, -1.0), (2.0,) * 3, (1, 1, 1), gpu_device, "dims 1 1 1")
    assert ref["V"] == 1 and ref["count"].tolist() == [295] and set(key.tolist()) == {0, 1}
    # more than 32 bits
    pts = rs.uniform(0, 1, (2000, 3)).astype(np.float32)
    dims = (1 << 20, 1 << 20, 1 << 10)
    key, ref = _pipeline(pts, (0.0,) * 3, (2.0 ** -20, 2.0 ** -20, 2.0 ** -10), dims, gpu_device, "50-bit keys")
    assert key.max() > 1 << 45 and (key < 1 << 50).all() and ref["V"] == 2000


# ---- 4. the reduce ---------------------------------------------------------------------------------------------------------------------------

def _stack(rs, cell, count, voxel):
    """``count`` jittered points strictly inside cell ``cell`` of a grid of origin 0."""
    return ((np.asarray(cell) + rs.uniform(0.05, 0.95, (count, 3))) * voxel).astype(np.float32)


def test_reduce_counts_ties_and_lost_rows(gpu_device):
    """4.  Voxels of 1 .. 5000 points on both sides of every lane-group border, duplicates, an equidistant pair, lost rows; the rows
    shuffled, so that a voxel's rows meet through the sort alone."""
    rs = np.random.RandomState(33)
    voxel = 0.5
    counts = (1, 2, 15, 16, 17, 63, 64, 65, 200, 255, 256, 257, 300, 5000)
    parts = [_stack(rs, (i % 5, i // 5, i % 3), c, voxel) for i, c in enumerate(counts)]
    parts.append(np.repeat(np.array([[2.7, 2.2, 0.1]], np.float32), 7, axis=0))            # duplicates in cell (5, 4, 0)
    parts.append(np.array([[3.125, 2.25, 0.25], [3.375, 2.25, 0.25]], np.float32))          # an equidistant pair in cell (6, 4, 0)
    parts.append(np.array([[-0.1, 0.2, 0.2], [0.2, 9.0, 0.2], [0.2, 0.2, -3.0], [50.0, 0.0, 0.0]], np.float32))   # outside the grid
    pts = np.concatenate(parts)
    perm = rs.permutation(len(pts))
    pts = np.ascontiguousarray(pts[perm])
    dims = (8, 6, 3)
    key, ref = _pipeline(pts, (0.0, 0.0, 0.0), (voxel,) * 3, dims, gpu_device, "crafted counts")
    assert sorted(ref["count"].tolist()) == sorted(counts + (7, 2)) and ref["V"] == len(counts) + 2
    assert (ref["voxel_of"] == -1).sum() == 4 and ref["count"].sum() == len(pts) - 4
    inv = np.empty(len(pts), np.int64)
    inv[perm] = np.arange(len(pts))
    n0 = sum(counts)
    dup_rows, pair_rows = inv[n0:n0 + 7], inv[n0 + 7:n0 + 9]
    v = ref["voxel_of"][dup_rows[0]]
    assert ref["rep"][v] == dup_rows.min() and ref["count"][v] == 7 and ref["centroid"][v].tolist() == pts[dup_rows[0]].tolist()
    v = ref["voxel_of"][pair_rows[0]]
    assert ref["rep"][v] == pair_rows.min() and ref["centroid"][v].tolist() == [3.25, 2.25, 0.25]
    # all points in one voxel: a handful (a lane group) and more than a tile (the wave)
    T = _tile()
    for n in (100, 3 * T + 5):
        one = _stack(rs, (0, 0, 0), n, 1.0)
        _, ref = _pipeline(one, (0.0,) * 3, (1.0,) * 3, (1, 1, 1), gpu_device, ("one voxel", n), halves=False)
        assert ref["V"] == 1 and ref["count"].tolist() == [n]
    # every point in its own voxel
    g = np.stack(np.meshgrid(np.arange(17), np.arange(13), np.arange(11), indexing="ij"), -1).reshape(-1, 3)
    own = ((g[rs.permutation(len(g))] + 0.5) * 0.25).astype(np.float32)
    _, ref = _pipeline(own, (0.0,) * 3, (0.25,) * 3, (17, 13, 11), gpu_device, "own voxels", halves=False)
    assert ref["V"] == len(own) and (ref["count"] == 1).all() and sorted(ref["rep"].tolist()) == list(range(len(own)))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------

def _clouds():
    if "clouds" not in _state:
        from nesti_net_amd import synth
        _state["clouds"] = {"box": synth.make_cloud("box", n=20000)[0], "ellipsoid": synth.make_cloud("ellipsoid", n=4000)[0]}
    return _state["clouds"]


ARRAYS = ("points", "centroid", "rep", "count", "key", "cell", "voxel_of", "origin", "voxel", "dims")


@pytest.mark.parametrize("name", ["box", "ellipsoid"])
@pytest.mark.parametrize("cells, passes", [(1 << 20, 8), (5000, 5), (64, 3)])
def test_voxel_downsample_end_to_end(name, cells, passes, gpu_device):
    """5.  ``voxel_downsample`` at three voxel sizes (8, 5 and 3 sort passes), both modes: every array is the restatement's; 'nearest'
    points are ``pts[rep]``; the counts add up; ``voxel_of`` agrees with ``cell``; twice and on two streams the same bytes."""
    from nesti_net_amd import downsample as ds
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts = _clouds()[name]
    voxel = float((pts.max(0).astype(np.float64) - pts.min(0)).max() / cells)
    assert (vx.grid_of(pts, voxel)[4] + 7) // 8 == passes
    ref = vx.downsample(pts, voxel)
    got = ds.voxel_downsample(pts, voxel, device=str(gpu_device))
    near = ds.voxel_downsample(pts, voxel, mode="nearest", device=str(gpu_device))
    assert set(got) == set(ARRAYS) == set(near)
    for k in ARRAYS:
        assert _same_bytes(got[k], ref[k]), (k, got[k].dtype, ref[k].dtype)
        if k != "points":
            assert _same_bytes(near[k], ref[k]), ("nearest", k)
    assert _same_bytes(near["points"], pts[got["rep"]]) and _same_bytes(got["points"], got["centroid"])
    N, V = len(pts), len(got["rep"])
    assert got["count"].sum() == N and got["voxel_of"].min() == 0 and got["voxel_of"].max() == V - 1
    cell = np.floor((pts.astype(np.float64) - got["origin"]) / got["voxel"]).astype(np.int64)
    assert np.array_equal(got["cell"][got["voxel_of"]], cell) and (got["cell"] < got["dims"]).all()
    assert np.array_equal(np.bincount(got["voxel_of"], minlength=V), got["count"])
    again = ds.voxel_downsample(pts, voxel, device=str(gpu_device))
    assert all(_same_bytes(again[k], got[k]) for k in ARRAYS)
    cloud = CloudPatches(pts, NestiConfig(), device=gpu_device, radius_grid=False)
    for st in (torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)):
        dev = ds.voxel_cloud(cloud, voxel, stream=st)
        st.synchronize()
        assert dev["n_voxels"] == V and dev["key_bits"] == vx.grid_of(pts, voxel)[4]
        for k in ("points", "centroid", "rep", "count", "voxel_of"):
            assert _same_bytes(dev[k].cpu().numpy(), got[k]), ("stream", k)
        assert _same_bytes(dev["key"].cpu().numpy().view(np.uint64), got["key"])


# ---- 6. composition ----------------------------------------------------------------------------------------------------------------------------

def _small():
    if "small" not in _state:
        from nesti_net_amd import synth
        pts, _ = synth.make_cloud("box", n=6000, seed=5)
        far = np.array([[3, 0, 0], [0, -4, 0.5], [2, 2, 2]], np.float32)
        _state["small"] = np.ascontiguousarray(np.concatenate([pts, far]).astype(np.float32))
    return _state["small"]


def _gathered(direct, voxel_of, V):
    from nesti_net_amd import downsample as ds
    return ds.gather_result(direct, voxel_of, V)


def _same_result(got, want, label):
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert _same_bytes(got[k], v), (label, k)
        else:
            assert got[k] == v, (label, k)


def test_downsample_composes_with_the_estimators(gpu_device):
    """6.  ``downsample=`` is the estimator on the voxels' points gathered through ``voxel_of``, on the bytes -- with the outlier filter
    (which runs second, on the downsampled cloud), with ``init=`` of the robust fit taken at ``rep``, and with ``queries=`` ungathered."""
    from nesti_net_amd import downsample as ds, pca, robust
    pts, dev = _small(), str(gpu_device)
    voxel = 0.06
    vd = ds.voxel_downsample(pts, voxel, device=dev)
    V, N = len(vd["rep"]), len(pts)
    assert 0.2 * N < V < 0.8 * N and vd["count"].max() > 3
    extra = {"voxel_of": vd["voxel_of"], "voxel_points": vd["points"], "voxel_count": vd["count"]}

    got = pca.pca_normals(pts, knn=16, downsample=voxel, device=dev)
    direct = pca.pca_normals(vd["points"], knn=16, device=dev)
    assert set(got) == set(direct) | set(extra) and got["normals"].shape == (N, 3)
    _same_result(got, dict(_gathered(direct, vd["voxel_of"], V), **extra), "pca")
    assert _same_bytes(got["normals"], direct["normals"][vd["voxel_of"]])

    # a dict, mode 'nearest', with smoothing and orientation: still the estimator of the voxels' points
    near = ds.voxel_downsample(pts, voxel, mode="nearest", device=dev)
    got = pca.pca_normals(pts, knn=(8, 16), smooth=1, orient="mst", downsample={"voxel": voxel, "mode": "nearest"}, device=dev)
    direct = pca.pca_normals(near["points"], knn=(8, 16), smooth=1, orient="mst", device=dev)
    _same_result(got, _gathered(direct, vd["voxel_of"], V), "pca nearest")
    assert _same_bytes(got["voxel_points"], pts[vd["rep"]])

    # with the outlier filter: it sees the downsampled cloud; the maps compose; a removed voxel's rows hold the fill
    got = pca.pca_normals(pts, knn=16, downsample=voxel, outliers="statistical", device=dev)
    direct = pca.pca_normals(vd["points"], knn=16, outliers="statistical", device=dev)
    _same_result(got, dict(_gathered(direct, vd["voxel_of"], V), **extra), "pca + outliers")
    removed = ~direct["inlier"]
    assert 0 < removed.sum() < V and got["inlier"].shape == (N,) and not got["inlier"][-3:].any()
    assert (got["normals"][removed[vd["voxel_of"]]] == 0).all() and np.array_equal(got["inlier"], direct["inlier"][vd["voxel_of"]])

    # the robust fit: init is taken at rep
    init = pca.pca_normals(pts, knn=16, device=dev)["normals"]
    got = robust.robust_normals(pts, knn=16, init=init, downsample=voxel, device=dev)
    direct = robust.robust_normals(vd["points"], knn=16, init=init[vd["rep"]], device=dev)
    _same_result(got, dict(_gathered(direct, vd["voxel_of"], V), **extra), "robust")
    init[vd["rep"][5]] = 0.0                                                               # a start of 0 0 0 comes back 0 0 0: seen at rep alone
    got = robust.robust_normals(pts, knn=16, init=init, downsample=voxel, device=dev)
    assert (got["normals"][vd["voxel_of"] == 5] == 0).all() and (got["normals"][vd["voxel_of"] == 6] != 0).any()

    # queries: the rows are the positions, the downsampled cloud is the surface they search
    q = pts[::7]
    got = pca.pca_normals(pts, knn=16, queries=q, downsample=voxel, device=dev)
    direct = pca.pca_normals(vd["points"], knn=16, queries=q, device=dev)
    _same_result(got, dict(direct, **extra), "queries")
    assert got["normals"].shape == (len(q), 3)


def _dataset(tmp_path, pts):
    d = tmp_path / "data"
    d.mkdir()
    np.savetxt(d / "box.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("box\n")
    return d, ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]


def _rows(path):
    return sum(1 for _ in open(path))


def test_command_line_writes_the_voxel_files(tmp_path, gpu_device):
    """6.  ``--estimator pca --knn 16 --voxel_size V --outliers statistical``: the three voxel files, every file with the rows of the
    .xyz, the normals those of the Python call; the ladder route too."""
    from nesti_net_amd import downsample as ds, pca, textio
    from nesti_net_amd.cli import main
    pts = _small()
    d, common = _dataset(tmp_path, pts)
    results = str(tmp_path / "fit")
    assert main(["--estimator", "pca", "--knn", "16", "--voxel_size", "0.06", "--voxel_mode", "nearest", "--outliers", "statistical",
                 "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    loaded = np.loadtxt(d / "box.xyz").astype("float32")
    res = pca.pca_normals(loaded, knn=16, downsample={"voxel": 0.06, "mode": "nearest"}, outliers="statistical", device=str(gpu_device))
    files = sorted(os.listdir(out))
    assert files == sorted(["log.txt"] + ["box" + e for e in (".normals", ".pca_eig", ".pca_count", ".knn_radius", ".inliers", ".outlier_score",
                                                              ".voxel_xyz", ".voxel_of", ".voxel_count")])
    for name in files:
        if name != "log.txt":
            assert _rows(os.path.join(out, name)) == len(pts), name
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.voxel_of")).astype(np.int64), res["voxel_of"])
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.voxel_count")).astype(np.int32), res["voxel_count"][res["voxel_of"]])
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.voxel_xyz")).astype(np.float32), res["voxel_points"][res["voxel_of"]])
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.inliers")).astype(bool), res["inlier"])
    want = str(tmp_path / "want.normals")
    textio.write_f32(want, res["normals"])
    assert open(os.path.join(out, "box.normals"), "rb").read() == open(want, "rb").read()
    log = open(os.path.join(out, "log.txt")).read()
    assert "voxel grid of box (cell 0.06 0.06 0.06, nearest): %d voxels from %d rows; largest count %d" % (
        len(res["voxel_count"]), len(pts), res["voxel_count"].max()) in log
    results = str(tmp_path / "ladder")
    assert main(["--estimator", "pca", "--knn_ladder", "auto", "--voxel_size", "0.06", "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    vd = ds.voxel_downsample(loaded, 0.06, device=str(gpu_device))
    for ext in (".normals", ".select_k", ".voxel_xyz", ".voxel_of", ".voxel_count"):
        assert _rows(os.path.join(out, "box" + ext)) == len(pts), ext
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.voxel_of")).astype(np.int64), vd["voxel_of"])


@pytest.mark.parametrize("args, word", [
    (["--voxel_size", "0.1"], "--voxel_size does not go with --estimator net"),
    (["--voxel_size", "0.1", "--depth_images", "1"], "--voxel_size does not go with --depth_images 1"),
    (["--estimator", "pca", "--voxel_size", "0.1", "--sparse_patches", "1"], "--voxel_size does not go with --sparse_patches 1"),
    (["--estimator", "pca", "--voxel_size", "0.1", "--query_positions", "1"], "--voxel_size does not go with --query_positions 1"),
    (["--estimator", "pca", "--voxel_size", "0.1", "--subsample", "reference"], "--voxel_size does not go with --subsample reference"),
])
def test_command_line_refusals_say_left_for_later(args, word, capsys, tmp_path, gpu_device):
    """6.  Each refused combination exits with its message, before anything is created."""
    from nesti_net_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and "left for later" in err and not (tmp_path / "out").exists()
