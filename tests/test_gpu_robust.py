"""The robust plane fit on the GPU (``nesti_robust_normals_nbr`` / ``_at``; csrc/robust.hip).

  1. one iteration from a given start against the tests' restatement (tests/_robust_fixture.py): the ten moments, support, inliers,
     iterations, radius and count bit for bit, for neighbour counts on both sides of every multiple of the wave; the normal bit for bit
     against the host solver ``nesti_sym3_eig`` applied to the kernel's own moments
  2. ``plane_out`` is ``nesti_pca_normals_nbr`` bit for bit, and no init is the init ``plane_out``
  3. ``iters = T`` equals T chained calls of ``iters = 1``, bit for bit
  4. edges: a lattice (the floor carries the weights), collinear points, duplicates, a prefix shorter than 3, ``falloff = 1``, ``iters``
     0 and 64, one row, rows by ``query_row0``, positions outside the box and with a NaN, a cloud point with a NaN, init rows that are 0
     or of opposite sign
  5. untrusted lists: a -1 in mid-row, an index beyond the cloud, a shuffled row
  6. rows fitted in two calls on two streams equal one call; any subset of NULL outputs leaves the others unchanged; the launch is
     booked in the profiler's patches category and replays from a captured graph
  7. ``robust.robust_normals``, its smoothing and orientation, and the command line"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _knn_fixture as kx
import _robust_fixture as rx

pytestmark = pytest.mark.gpu

# both sides of every multiple of 64 (a lane's second, third and fourth slot begin there) and the smallest counts that can be fitted
GROUPS = ((3, 4, 5, 63), (64, 65, 127, 128), (129, 191, 192, 193), (255, 256))
NAMES = ("normals", "plane", "support", "inliers", "iters_done", "moments", "radius", "count")
EXACT = ("moments", "support", "inliers", "iters_done", "radius", "count")
DEFAULTS = {"iters": 8, "sigma": 2.0, "falloff": 0.5, "floor": 0.01}
_cache = {}


def _b32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_bytes_or_nan(a, b):
    """``_same_bytes`` wherever either side is not a NaN, and NaN on both sides elsewhere: the payload of a NaN that two kernels form by
    the same operations is the hardware's business, not the entry's."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0, _b32(a)), np.where(nan, 0, _b32(b)))


def _outs(M, S, dev, fill=-7):
    f32, i32 = torch.float32, torch.int32
    specs = (((M, S, 3), f32), ((M, S, 3), f32), ((M, S), f32), ((M, S), i32), ((M, S), i32), ((M, S, 10), torch.float64), ((M, S), f32),
             ((M, S), i32))
    return [torch.full(shape, fill, dtype=dt, device=dev) for shape, dt in specs]


def _raw(lib, cloud_d, q_d, M, row0, nbr_d, ks, init=None, at=False, null=(), outs=None, stream=None, **params):
    """One call of the entry with outputs pre-filled with -7 (NULL for the names in ``null``) -> (rc, dict of the output tensors).
    ``init``: None, or a numpy / torch array [M,S,3]."""
    from nesti_net_amd import _lib
    p = dict(DEFAULTS, **params)
    S, dev = len(ks), cloud_d.device
    outs = outs if outs is not None else _outs(M, S, dev)
    ptrs = [None if name in null else _lib.ptr(t) for name, t in zip(NAMES, outs)]
    if init is not None and not isinstance(init, torch.Tensor):
        init = torch.from_numpy(np.ascontiguousarray(init, np.float32)).to(dev)
    assert init is None or (tuple(init.shape) == (M, S, 3) and init.is_contiguous())
    head = (_lib.ptr(cloud_d), cloud_d.shape[0], None if q_d is None else _lib.ptr(q_d), M) + (() if at else (row0,))
    fn = lib.nesti_robust_normals_nbr_at if at else lib.nesti_robust_normals_nbr
    with torch.cuda.device(dev):
        rc = fn(*head, _lib.ptr(nbr_d), int(nbr_d.shape[1]), (ctypes.c_int32 * S)(*ks), S, p["iters"], ctypes.c_double(p["sigma"]),
                ctypes.c_double(p["falloff"]), ctypes.c_double(p["floor"]), None if init is None else _lib.ptr(init), *ptrs,
                _lib.stream_ptr(stream))
    return rc, dict(zip(NAMES, outs))


def _np(d):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in d.items()}


def _run(lib, *args, **kw):
    rc, outs = _raw(lib, *args, **kw)
    assert rc == 0, lib.nesti_last_error()
    return _np(outs)


def _pca_nbr_raw(lib, cloud_d, q_d, M, row0, nbr_d, ks, at=False):
    """``nesti_pca_normals_nbr`` / ``_at`` over the same lists -> (normals, eig, radius, count) as numpy [M,S,..]."""
    from nesti_net_amd import _lib
    S, dev = len(ks), cloud_d.device
    outs = [torch.full((M, S, 3), -7, dtype=torch.float32, device=dev), torch.full((M, S, 3), -7, dtype=torch.float32, device=dev),
            torch.full((M, S), -7, dtype=torch.float32, device=dev), torch.full((M, S), -7, dtype=torch.int32, device=dev)]
    head = (_lib.ptr(cloud_d), cloud_d.shape[0], None if q_d is None else _lib.ptr(q_d), M) + (() if at else (row0,))
    fn = lib.nesti_pca_normals_nbr_at if at else lib.nesti_pca_normals_nbr
    with torch.cuda.device(dev):
        rc = fn(*head, _lib.ptr(nbr_d), int(nbr_d.shape[1]), (ctypes.c_int32 * S)(*ks), S, *[_lib.ptr(t) for t in outs], _lib.stream_ptr())
    assert rc == 0, lib.nesti_last_error()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def _one_iteration_is_the_restatement(got, pts, centres, nbr, ks, init, label="", **params):
    """The outputs of an ``iters = 1`` call against the fixture, scale by scale: EXACT bit for bit, the plane against the fixture's own,
    and the normal against the host solver over the kernel's own moments (a row whose iteration failed keeps its start normal)."""
    p = dict(DEFAULTS, **params)
    for s, k in enumerate(ks):
        start = got["plane"][:, s] if init is None else init[:, s]               # no init: the kernel's own plane fit, checked on its own
        ref = rx.restate(pts, centres, nbr, k, 1, p["sigma"], p["falloff"], p["floor"], start)
        for key in EXACT:
            assert _same_bytes(got[key][:, s], ref[key]), (label, key, k, np.flatnonzero((got[key][:, s] != ref[key]).reshape(len(ref[key]), -1).any(1))[:8])
        ok = ref["iters_done"] == 1
        mom = got["moments"][:, s]
        solved = rx.solve(mom[:, 1:], mom[:, 0], ref["geo"]["r2"], ok)
        differ = np.flatnonzero((_b32(got["normals"][:, s]) != _b32(np.where(ok[:, None], solved, ref["normals"]))).any(1))
        print("%s k = %d: %d rows, %d iterated, %d differ from the host solver over the kernel's moments" % (label, k, len(ok), ok.sum(), len(differ)))
        assert len(differ) == 0, (label, k, differ[:8])
        assert _same_bytes(got["plane"][:, s], ref["plane"]), (label, "plane", k)


def _random_cloud(dev):
    """N = 300 random points, M = 301 rows through pidx with repeats, their sorted lists at K = 256 and random start normals."""
    if "random" not in _cache:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd import _lib
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        rs = np.random.RandomState(20)
        pts = rs.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
        pidx = np.concatenate([rs.randint(0, 300, 299), [5, 5]]).astype(np.int32)
        cp = CloudPatches(pts, NestiConfig(), device=dev, pidx=pidx, radius_grid=False)
        nbr = cp.knn(0, len(pidx), 256)[0]
        torch.cuda.synchronize()
        init = (rs.normal(size=(len(pidx), 4, 3)) * 10.0 ** rs.uniform(-2, 2, (len(pidx), 4, 1))).astype(np.float32)
        init[-1] = -init[-2]                                                    # the repeated row starts from the opposite sign
        _cache["random"] = {"lib": _lib.load(), "pts": pts, "pidx": pidx, "cp": cp, "nbr": nbr, "nbr_np": nbr.cpu().numpy(), "init": init}
    return _cache["random"]


def _roof(dev):
    """600 points on two planes meeting in a ridge along y (z = -0.6 |x|) with a little noise, all rows, lists at K = 64."""
    if "roof" not in _cache:
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        rs = np.random.RandomState(21)
        xy = rs.uniform(-1.0, 1.0, (600, 2))
        pts = np.stack([xy[:, 0], xy[:, 1], -0.6 * np.abs(xy[:, 0]) + rs.normal(scale=0.003, size=600)], 1).astype(np.float32)
        cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
        nbr = cp.knn(0, 600, 64)[0]
        torch.cuda.synchronize()
        _cache["roof"] = {"pts": pts, "cp": cp, "nbr": nbr}
    return _cache["roof"]


# ---- 1, 2 -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ks", GROUPS)
def test_one_iteration_is_the_restatement_bit_for_bit(ks, gpu_device):
    r = _random_cloud(gpu_device)
    M, S = len(r["pidx"]), len(ks)
    assert M == 301 and M % 4
    init = np.ascontiguousarray(r["init"][:, :S])
    got = _run(r["lib"], r["cp"].cloud, r["cp"].pidx, M, 0, r["nbr"], ks, init=init, iters=1)
    _one_iteration_is_the_restatement(got, r["pts"], r["pts"][r["pidx"]], r["nbr_np"], ks, init, "random")
    assert (got["iters_done"] == 1).all() and np.array_equal(got["count"], np.tile(np.array(ks, np.int32), (M, 1)))
    assert (got["support"] > 0).all() and (got["inliers"] >= 1).all() and (got["inliers"] <= got["count"]).all()
    for key in NAMES:
        assert _same_bytes(got[key][-1], got[key][-2]), key                     # the repeated row, started from the opposite sign


@pytest.mark.parametrize("ks", GROUPS)
def test_plane_out_is_the_list_fit_and_the_default_start(ks, gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, M = r["lib"], r["cp"], len(r["pidx"])
    got = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, iters=1)
    normals, _, radius, count = _pca_nbr_raw(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks)
    assert _same_bytes(got["plane"], normals) and _same_bytes(got["radius"], radius) and _same_bytes(got["count"], count)
    again = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, init=got["plane"], iters=1)
    for key in NAMES:
        assert _same_bytes(got[key], again[key]), key
    _one_iteration_is_the_restatement(got, r["pts"], r["pts"][r["pidx"]], r["nbr_np"], ks, None, "no init")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [2, 5, 8])
def test_iterations_chain_through_the_f32_normal(T, gpu_device):
    r, roof = _random_cloud(gpu_device), _roof(gpu_device)
    for label, cloud, q, M, nbr, ks in (("random", r["cp"].cloud, r["cp"].pidx, len(r["pidx"]), r["nbr"], (5, 64, 100, 256)),
                                        ("roof", roof["cp"].cloud, None, 600, roof["nbr"], (16, 50))):
        whole = _run(r["lib"], cloud, q, M, 0, nbr, ks, iters=T)
        cur = None
        for _ in range(T):
            step = _run(r["lib"], cloud, q, M, 0, nbr, ks, init=cur, iters=1)
            cur = step["normals"]
        for key in NAMES:
            if key != "iters_done":
                assert _same_bytes(whole[key], step[key]), (label, T, key)
        assert (whole["iters_done"] == T).all() and (step["iters_done"] == 1).all(), label
        assert not _same_bytes(whole["normals"], whole["plane"])


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------

def _cloud(pts, dev, **kw):
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    return CloudPatches(np.ascontiguousarray(pts, np.float32), NestiConfig(), device=dev, radius_grid=False, **kw)


def test_degenerate_neighbourhoods(gpu_device):
    from nesti_net_amd import _lib
    lib = _lib.load()
    # a 9 x 9 lattice on z = 0: every height is 0, so med = 0 and the floor carries the weights; the normal is 0 0 1 exactly
    g = np.arange(9, dtype=np.float32)
    lat = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    lat = np.concatenate([lat, np.zeros((81, 1), np.float32)], 1)
    cp = _cloud(lat, gpu_device)
    nbr = cp.knn(0, 81, 81)[0]
    ks = (9, 25, 81)
    got = _run(lib, cp.cloud, None, 81, 0, nbr, ks)
    assert _same_bytes(got["normals"], np.tile(np.array([0, 0, 1], np.float32), (81, 3, 1))) and _same_bytes(got["plane"], got["normals"])
    assert np.array_equal(got["inliers"], got["count"]) and np.array_equal(got["count"], np.tile(np.array(ks, np.int32), (81, 1)))
    assert (got["iters_done"] == 8).all() and (got["support"] > 0).all() and not got["moments"][..., [3, 6, 8, 9]].any()
    one = _run(lib, cp.cloud, None, 81, 0, nbr, ks, iters=1)
    _one_iteration_is_the_restatement(one, lat, lat, nbr.cpu().numpy(), ks, None, "lattice")
    # 40 collinear points: the plane fit has no unique normal; whatever it gives, the iteration is the restatement's
    line = np.stack([0.25 * np.arange(40), np.full(40, 3.0), np.zeros(40)], 1).astype(np.float32)
    cl = _cloud(line, gpu_device)
    nbr = cl.knn(0, 40, 32)[0]
    one = _run(lib, cl.cloud, None, 40, 0, nbr, (8, 32), iters=1)
    _one_iteration_is_the_restatement(one, line, line, nbr.cpu().numpy(), (8, 32), None, "line")
    full = _run(lib, cl.cloud, None, 40, 0, nbr, (8, 32))
    assert np.isfinite(full["normals"]).all() and np.isfinite(full["moments"]).all()
    # ten copies of one point: r2 = 0, nothing can be fitted; radius and count are still written
    dup = np.tile(np.array([[0.5, -0.25, 2.0]], np.float32), (10, 1))
    cd = _cloud(dup, gpu_device)
    nbr = cd.knn(0, 10, 8)[0]
    got = _run(lib, cd.cloud, None, 10, 0, nbr, (4, 8))
    for key in ("normals", "plane", "support", "inliers", "iters_done", "radius"):
        assert not got[key].view(np.uint32).any(), key
    assert not got["moments"].any() and np.array_equal(got["count"], np.tile(np.array([4, 8], np.int32), (10, 1)))
    # a cloud of two points: a prefix shorter than 3
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    ct = _cloud(two, gpu_device)
    nbr = ct.knn(0, 2, 8)[0]
    got = _run(lib, ct.cloud, None, 2, 0, nbr, (2, 8), init=np.ones((2, 2, 3), np.float32))
    assert not got["normals"].view(np.uint32).any() and not got["iters_done"].any() and not got["support"].view(np.uint32).any()
    assert (got["count"] == 2).all() and (got["radius"] == 1).all()


def test_falloff_1_and_the_iteration_counts(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, M, pts = r["lib"], r["cp"], len(r["pidx"]), r["pts"]
    # falloff = 1: the farthest slot weighs 0.  Over 3 neighbours fewer than 3 slots are left: the iteration fails, the start stays
    ks = (3, 4, 100, 256)
    init = np.ascontiguousarray(r["init"])
    got = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, init=init, iters=1, falloff=1.0)
    _one_iteration_is_the_restatement(got, pts, pts[r["pidx"]], r["nbr_np"], ks, init, "falloff 1", falloff=1.0)
    assert not got["iters_done"][:, 0].any() and (got["iters_done"][:, 1:] == 1).all()
    assert not got["support"][:, 0].any() and not got["moments"][:, 0].any() and not got["inliers"][:, 0].any()
    from _pca_fixture import sign_rule
    assert _same_bytes(got["normals"][:, 0], sign_rule(init[:, 0]))              # as given, under the sign rule: not renormalised
    eight = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, falloff=1.0)
    assert _same_bytes(eight["normals"][:, 0], eight["plane"][:, 0]) and not eight["iters_done"][:, 0].any()
    assert (eight["iters_done"][:, 1:] == 8).all()
    # iters = 0: the start normal under the sign rule, renormalised; nothing else happens
    zero = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, init=init, iters=0)
    for s, k in enumerate(ks):
        want = rx.restate(pts, pts[r["pidx"]], r["nbr_np"], k, 0, init=init[:, s])
        for key in ("normals", "plane", "support", "inliers", "iters_done", "moments", "radius", "count"):
            assert _same_bytes(zero[key][:, s], want[key]), (key, k)
    assert not zero["iters_done"].any() and np.abs(np.linalg.norm(zero["normals"].astype(np.float64), axis=2) - 1).max() <= 2.0 ** -22
    # iters = 64 equals 32 and 32 more
    ks = (64, 100)
    most = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, iters=64)
    half = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, iters=32)
    rest = _run(lib, cp.cloud, cp.pidx, M, 0, r["nbr"], ks, init=half["normals"], iters=32)
    assert (most["iters_done"] == 64).all() and (rest["iters_done"] == 32).all()
    for key in NAMES:
        if key != "iters_done":
            assert _same_bytes(most[key], rest[key]), key


def test_rows_positions_and_start_normals(gpu_device):
    r = _random_cloud(gpu_device)
    lib, pts = r["lib"], r["pts"]
    ks = (5, 64, 100, 256)
    # M = 1, and rows by query_row0 with a NULL index: rows 40 .. 59 of the cloud itself
    call = _cloud(pts, gpu_device)
    lists = call.knn(40, 20, 256)[0]
    rows = torch.arange(40, 60, dtype=torch.int32, device=gpu_device)
    init = np.ascontiguousarray(r["init"][:20])
    by_index = _run(lib, call.cloud, rows, 20, 0, lists, ks, init=init)
    by_row0 = _run(lib, call.cloud, None, 20, 40, lists, ks, init=init)
    single = _run(lib, call.cloud, None, 1, 47, lists[7:8].contiguous(), ks, init=init[7:8])
    for key in NAMES:
        assert _same_bytes(by_index[key], by_row0[key]) and _same_bytes(single[key], by_index[key][7:8]), key
    assert (by_row0["iters_done"] == 8).all()
    # an init of opposite sign gives equal bytes; an init row of 0 0 0 or with a NaN comes back 0 0 0, its plane still written
    start = init.copy()
    start[3] = 0.0
    start[4, :, 1] = np.nan
    start[5, 2] = np.inf
    plus = _run(lib, call.cloud, None, 20, 40, lists, ks, init=start)
    minus = _run(lib, call.cloud, None, 20, 40, lists, ks, init=-start)
    for key in NAMES:
        assert _same_bytes(plus[key], minus[key]), key
    dead = np.zeros((20, 4), bool)
    dead[[3, 4]] = True
    dead[5, 2] = True
    for key in ("normals", "support", "inliers", "iters_done"):
        assert not plus[key][dead].view(np.uint32).any() and _same_bytes(plus[key][~dead], by_row0[key][~dead]), key
    assert not plus["moments"][dead].any() and _same_bytes(plus["plane"], by_row0["plane"]) and _same_bytes(plus["radius"], by_row0["radius"])
    # positions: a cloud point's own position, one far outside the box, one with a NaN (an empty prefix whatever its list holds)
    q = np.stack([pts[3], np.array([40.0, -3.0, 2.5], np.float32), np.array([0.1, np.nan, 0.2], np.float32), pts[8] + np.float32(0.01)])
    cq = _cloud(pts, gpu_device, queries=torch.from_numpy(np.where(np.isfinite(q), q, 0.0).astype(np.float32)))
    nbr = cq.knn(0, 4, 256)[0]
    q_d = torch.from_numpy(q).to(gpu_device)
    one = _run(lib, cq.cloud, q_d, 4, 0, nbr, ks, at=True, iters=1)
    _one_iteration_is_the_restatement(one, pts, q, nbr.cpu().numpy(), ks, None, "positions")
    got = _run(lib, cq.cloud, q_d, 4, 0, nbr, ks, at=True)
    normals, _, radius, count = _pca_nbr_raw(lib, cq.cloud, q_d, 4, 0, nbr, ks, at=True)
    assert _same_bytes(got["plane"], normals) and _same_bytes(got["radius"], radius) and _same_bytes(got["count"], count)
    assert not got["count"][2].any() and not got["normals"][2].view(np.uint32).any() and not got["radius"][2].view(np.uint32).any()
    assert (got["iters_done"][[0, 1, 3]] == 8).all() and got["radius"][1, 0] > 30.0
    idx = torch.tensor([3], dtype=torch.int32, device=gpu_device)
    own = _run(lib, cq.cloud, idx, 1, 0, nbr[:1].contiguous(), ks)
    for key in NAMES:
        assert _same_bytes(own[key], got[key][:1]), key                          # a position equal to a cloud point is that point
    # a cloud point with a NaN coordinate inside the prefix: the robust row is 0 0 0, plane_out is as the plane fit writes it
    bad = pts.copy()
    bad[77, 2] = np.nan
    cloud_d = torch.from_numpy(bad).to(gpu_device)
    rows = torch.tensor([1, 2, 77], dtype=torch.int32, device=gpu_device)
    lists = r["cp"].knn(0, 3, 256)[0].clone()                                   # any valid lists will do: those of three other rows
    lists[lists == 77] = 0
    lists[0, 40] = 77                                                           # the scales above 40 of row 0 reach the NaN point
    lists[1, 200] = 77
    got = _run(lib, cloud_d, rows, 3, 0, lists, ks)
    normals, _, radius, count = _pca_nbr_raw(lib, cloud_d, rows, 3, 0, lists, ks)
    assert _same_bytes_or_nan(got["plane"], normals) and _same_bytes(got["radius"], radius) and _same_bytes(got["count"], count)
    reached = np.array([[False, True, True, True], [False, False, False, True], [True, True, True, True]])
    assert not got["normals"][reached].view(np.uint32).any() and not got["iters_done"][reached].any() and not got["moments"][reached].any()
    assert (got["iters_done"][~reached] == 8).all() and np.isfinite(got["normals"]).all() and not got["count"][2].any()
    assert _same_bytes(got["count"][:2], np.tile(np.array(ks, np.int32), (2, 1)))


# ---- 5. untrusted lists -----------------------------------------------------------------------------------------------------------------

def test_untrusted_lists(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, pts, pidx = r["lib"], r["cp"], r["pts"], r["pidx"]
    M, ks = 12, (5, 64, 100, 256)
    nbr = r["nbr_np"][:M].copy()
    nbr[0, 100] = -1                                                            # the prefix ends at 100
    nbr[1, 64] = len(pts)                                                       # ... at 64: an index beyond the cloud
    nbr[2, 2] = 2 ** 31 - 1                                                     # ... at 2: nothing can be fitted
    nbr[3, 0] = -5                                                              # ... at 0
    nbr[4] = nbr[4][np.random.RandomState(3).permutation(256)]                  # shuffled: r2_s is a prefix maximum
    nbr[5, 255] = -1
    nbr_d = torch.from_numpy(nbr).to(gpu_device)
    q_d = cp.pidx[:M].contiguous()
    one = _run(lib, cp.cloud, q_d, M, 0, nbr_d, ks, iters=1)
    _one_iteration_is_the_restatement(one, pts, pts[pidx[:M]], nbr, ks, None, "untrusted")
    got = _run(lib, cp.cloud, q_d, M, 0, nbr_d, ks)
    k = np.array(ks)
    for row, prefix in ((0, 100), (1, 64), (2, 2), (3, 0), (4, 256), (5, 255), (6, 256)):
        assert np.array_equal(got["count"][row], np.minimum(k, prefix)), row
    ref = kx.plane_lists(pts, pts[pidx[:M]], nbr, ks)
    assert _same_bytes(got["radius"], ref["radius"]) and _same_bytes(got["count"], ref["n_ball"])
    normals, _, radius, count = _pca_nbr_raw(lib, cp.cloud, q_d, M, 0, nbr_d, ks)
    assert _same_bytes(got["plane"], normals) and _same_bytes(got["radius"], radius) and _same_bytes(got["count"], count)
    assert not got["normals"][2:4].view(np.uint32).any() and not got["iters_done"][2:4].any() and (got["iters_done"][4:] == 8).all()
    assert _same_bytes(got["normals"][0, 2], got["normals"][0, 3])              # the prefix of 100 serves both scales


# ---- 6. batching, NULL outputs, the profiler and graphs ---------------------------------------------------------------------------------

def test_two_calls_on_two_streams_equal_one(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    ks, cut = (5, 64, 100, 256), 133
    # the start normals and the pre-filled outputs are made on the default stream and outlive the calls: settled before the streams start
    init = torch.from_numpy(np.ascontiguousarray(r["init"])).to(gpu_device)
    i1, i2 = init[:cut].contiguous(), init[cut:].contiguous()
    o1, o2, o = _outs(cut, 4, gpu_device), _outs(M - cut, 4, gpu_device), _outs(M, 4, gpu_device)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)
    rc1, a = _raw(lib, cp.cloud, cp.pidx[:cut].contiguous(), cut, 0, nbr[:cut].contiguous(), ks, init=i1, outs=o1, stream=s1)
    rc2, b = _raw(lib, cp.cloud, cp.pidx[cut:].contiguous(), M - cut, 0, nbr[cut:].contiguous(), ks, init=i2, outs=o2, stream=s2)
    rc, whole = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, ks, init=init, outs=o)
    assert rc1 == 0 and rc2 == 0 and rc == 0
    a, b, whole = _np(a), _np(b), _np(whole)
    for key in NAMES:
        assert _same_bytes(np.concatenate([a[key], b[key]]), whole[key]), key


def test_null_outputs_leave_the_others_unchanged(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    ks = (5, 64, 100, 256)
    full = _run(lib, cp.cloud, cp.pidx, M, 0, nbr, ks, iters=2)
    subsets = [(name,) for name in NAMES] + [tuple(n for n in NAMES if n != "normals"), NAMES[4:], NAMES[:4], ("plane", "moments", "count"), NAMES]
    for null in subsets:
        got = _run(lib, cp.cloud, cp.pidx, M, 0, nbr, ks, iters=2, null=null)
        for key in NAMES:
            if key in null:
                assert (got[key] == -7).all(), (null, key)                      # never touched
            else:
                assert _same_bytes(got[key], full[key]), (null, key)


def test_profiler_category_and_graph_capture(gpu_device):
    from nesti_net_amd import _lib
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    ks = (5, 64, 100, 256)
    torch.cuda.synchronize()
    assert lib.nesti_profile_enable(1) == 0
    try:
        rc, _ = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, ks)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(lib)
    finally:
        lib.nesti_profile_enable(0)
    assert rc == 0 and sum(ph["patches"] for ph in launches.values()) == 1
    assert sum(n for ph in launches.values() for c, n in ph.items() if c != "patches") == 0 and sum(ph["patches"] for ph in ms.values()) > 0
    start = torch.from_numpy(np.ascontiguousarray(r["init"])).to(gpu_device)
    with torch.cuda.device(gpu_device):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = cp.robust_knn(0, M, ks, 8, 2.0, 0.5, 0.01, init=start, nbr=nbr)
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
    want = _run(lib, cp.cloud, cp.pidx, M, 0, nbr, ks, init=start)
    for name, t in zip(NAMES, out):
        assert _same_bytes(t.cpu().numpy(), want[name]), name


# ---- 7. the Python layer and the command line -------------------------------------------------------------------------------------------

KEYS = ["inliers", "iters_done", "n_ball", "normals", "normals_all", "orient", "plane_all", "radius", "support"]


def test_python_layer(gpu_device, monkeypatch):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough, pca, robust, smooth, synth
    from nesti_net_amd.provider import CloudPatches
    pts, gt = synth.make_cloud("box", n=2000, seed=3, noise=0.002)
    dev, M = str(gpu_device), 2000
    searches = []
    knn = CloudPatches.knn
    monkeypatch.setattr(CloudPatches, "knn", lambda self, first, count, k, **kw: (searches.append(k), knn(self, first, count, k, **kw))[1])
    res = robust.robust_normals(pts, knn=(16, 32), device=dev)
    assert searches == [32]                                                     # one search, at the largest count
    assert sorted(res) == KEYS and res["orient"] is None
    shapes = {"inliers": (M, 2), "iters_done": (M, 2), "n_ball": (M, 2), "normals": (M, 3), "normals_all": (M, 2, 3), "plane_all": (M, 2, 3),
              "radius": (M, 2), "support": (M, 2)}
    assert {k: res[k].shape for k in shapes} == shapes
    assert all(res[k].dtype == np.int32 for k in ("inliers", "iters_done", "n_ball")) and all(
        res[k].dtype == np.float32 for k in ("normals", "normals_all", "plane_all", "radius", "support"))
    assert _same_bytes(res["normals"], res["normals_all"][:, 1]) and (res["iters_done"] == 8).all()
    # ... plane_all is pca_normals(knn=...), and the near-edge rows gain what the restatement promised (tests/test_robust.py)
    fixed = pca.pca_normals(pts, knn=(16, 32), device=dev)
    assert _same_bytes(fixed["normals_all"], res["plane_all"]) and _same_bytes(fixed["radius"], res["radius"])
    near = rx.near_edge(pts, res["radius"][:, 1])
    share, plane = rx.within_deg(res["normals"][near], gt[near]), rx.within_deg(res["plane_all"][near, 1], gt[near])
    print("box 2000, noise 0.002, k = 32, %d near-edge rows: robust %.1f %%, plane %.1f %%" % (near.sum(), share, plane))
    assert share >= plane + 20.0
    # subsets: pidx and positions give the rows of the whole cloud
    pidx = np.arange(0, M, 9)
    by_index = robust.robust_normals(pts, knn=(16, 32), pidx=pidx, device=dev)
    by_position = robust.robust_normals(pts, knn=(16, 32), queries=pts[pidx], device=dev)
    for k in KEYS:
        if k != "orient":
            assert _same_bytes(by_index[k], by_position[k]) and _same_bytes(np.ascontiguousarray(res[k][pidx]), by_index[k]), k
    # init = the Hough normals, two iterations: a refinement; [M,3] is used at every scale
    del searches[:]
    h = hough.hough_normals(pts, knn=32, device=dev)
    refined = robust.robust_normals(pts, knn=(16, 32), init=h["normals"], iters=2, device=dev)
    both = robust.robust_normals(pts, knn=(16, 32), init=np.repeat(h["normals"][:, None], 2, 1), iters=2, device=dev)
    flipped = robust.robust_normals(pts, knn=(16, 32), pidx=pidx, init=-h["normals"][pidx], iters=2, device=dev)
    for k in KEYS:
        if k != "orient":
            assert _same_bytes(refined[k], both[k]) and _same_bytes(np.ascontiguousarray(refined[k][pidx]), flipped[k]), k
    assert (refined["iters_done"] == 2).all() and not _same_bytes(refined["normals"], res["normals"])
    print("... from the Hough normals, 2 iterations: %.1f %% (Hough itself %.1f %%)"
          % (rx.within_deg(refined["normals"][near], gt[near]), rx.within_deg(h["normals"][near], gt[near])))
    # smooth=1: the pass over the searched lists (32 reaches the smoothing's k: no second search), everything else as fitted
    del searches[:]
    sm = robust.robust_normals(pts, knn=(16, 32), smooth=1, device=dev)
    assert searches == [32] and sorted(sm) == sorted(KEYS + ["smooth_support", "smooth_count"])
    for k in KEYS:
        if k not in ("orient", "normals"):
            assert _same_bytes(sm[k], res[k]), k
    p = smooth.check_params(iters=1)
    cp = _cloud(pts, gpu_device)
    lists = cp.knn(0, M, 32)[0]
    want = cp.smooth_knn(torch.from_numpy(res["normals"]).to(gpu_device), 0, M, p.k, p.cos_t, p.falloff, nbr=lists)
    assert _same_bytes(sm["normals"], want[0].cpu().numpy()) and not _same_bytes(sm["normals"], res["normals"])
    # orient='viewpoint': only sign bits differ from the unoriented run
    vp = robust.robust_normals(pts, knn=(16, 32), orient="viewpoint", viewpoint=(9.0, 0.5, 0.25), device=dev)
    assert np.array_equal(np.abs(vp["normals"]), np.abs(res["normals"])) and (_b32(vp["normals"]) != _b32(res["normals"])).any()
    assert vp["orient"]["n_flipped"] > 0 and vp["orient"]["n_eligible"] == M
    for k in KEYS:
        if k not in ("orient", "normals"):
            assert _same_bytes(vp[k], res[k]), k


def test_command_line(tmp_path, gpu_device):
    from nesti_net_amd import robust, synth, textio
    from nesti_net_amd.cli import main
    d = tmp_path / "data"
    d.mkdir()
    pts, _ = synth.make_cloud("box", n=500, seed=3, noise=0.002)
    np.savetxt(d / "cube.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("cube\n")
    common = ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]
    pts32 = np.loadtxt(d / "cube.xyz").astype("float32")
    exts = (".normals", ".robust_support", ".robust_inliers", ".robust_count", ".knn_radius")
    for tag, flags, kw in (("defaults", ["--knn", "24"], {"knn": 24}),
                           ("flags", ["--knn", "12,24,48", "--robust_scale", "1", "--robust_iters", "3", "--robust_sigma", "1.5", "--robust_falloff",
                                      "0.25", "--robust_floor", "0.02"],
                            {"knn": (12, 24, 48), "scale": 1, "iters": 3, "sigma": 1.5, "falloff": 0.25, "floor": 0.02})):
        results = str(tmp_path / tag)
        assert main(["--estimator", "robust", "--results_path", results] + flags + common) == 0
        out = os.path.join(results, "synth_results")
        assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["cube" + e for e in exts])
        res = robust.robust_normals(pts32, device=str(gpu_device), **kw)
        want = str(tmp_path / ("want_" + tag))
        textio.write_f32(want + ".normals", res["normals"])
        textio.write_f32(want + ".robust_support", res["support"])
        textio.write_i32_rows(want + ".robust_inliers", res["inliers"])
        textio.write_i32_rows(want + ".robust_count", res["n_ball"])
        textio.write_f32(want + ".knn_radius", res["radius"])
        for e in exts:
            assert open(os.path.join(out, "cube" + e), "rb").read() == open(want + e, "rb").read(), (tag, e)
        ks = kw["knn"] if isinstance(kw["knn"], tuple) else (kw["knn"],)
        s = kw.get("scale", -1) % len(ks)
        assert np.loadtxt(os.path.join(out, "cube.robust_support")).reshape(500, -1).shape == (500, len(ks))
        log = open(os.path.join(out, "log.txt")).read()
        assert "robust plane fit of cube: 500 rows, %d nearest neighbours (scale %d of %d); 0 rows without a fit" % (ks[s], s, len(ks)) in log
        assert ("re-weighting of cube: %d iterations (sigma %g, falloff %g, floor %g); 0 rows stopped early; %.1f %% of the neighbours are inliers"
                % (kw.get("iters", 8), kw.get("sigma", 2.0), kw.get("falloff", 0.5), kw.get("floor", 0.01),
                   100.0 * res["inliers"][:, s].sum() / res["n_ball"][:, s].sum())) in log
    # with --smooth and --orient the written normals are the Python call's
    results = str(tmp_path / "both")
    assert main(["--estimator", "robust", "--knn", "24", "--smooth", "1", "--orient", "viewpoint", "--viewpoint", "9", "0.5", "0.25",
                 "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    assert sorted(os.listdir(out)) == sorted(["log.txt", "cube.smooth_support"] + ["cube" + e for e in exts])
    res = robust.robust_normals(pts32, knn=24, smooth=1, orient="viewpoint", viewpoint=(9.0, 0.5, 0.25), device=str(gpu_device))
    textio.write_f32(str(tmp_path / "want_both.normals"), res["normals"])
    assert open(os.path.join(out, "cube.normals"), "rb").read() == open(str(tmp_path / "want_both.normals"), "rb").read()
    # refusals that need no device
    for argv in (["--estimator", "robust"], ["--estimator", "robust", "--knn", "24", "--robust_iters", "65"],
                 ["--estimator", "robust", "--knn", "24", "--depth_images", "1"]):
        with pytest.raises(SystemExit) as e:
            main(argv + ["--results_path", str(tmp_path / "no")] + common)
        assert e.value.code == 2 and not (tmp_path / "no").exists()
