"""The scale-selected plane fit on the GPU (``nesti_pca_select_nbr`` / ``_at``; csrc/select.hip).

  1. every candidate of the four ``*_all`` outputs is ``nesti_pca_normals_nbr`` on the same lists, bit for bit, for a ladder of 32 counts
     on both sides of every multiple of the wave
  2. the selected outputs and ``variation_all`` are the tests' restatement of the selection (tests/_select_fixture.py) applied to the
     kernel's own per-candidate outputs, bit for bit, for slack 0, 0.5 and 1e300
  3. edges: L = 1, a ladder that can fit nothing, a prefix shorter than every count, one row, rows by ``query_row0``, positions outside
     the box and with a NaN, a cloud point with a NaN coordinate
  4. untrusted lists: a -1 in mid-row, an index beyond the cloud, a shuffled row
  5. rows fitted in two calls on two streams equal one call; any subset of NULL outputs leaves the others unchanged; the launch is
     booked in the profiler's patches category and replays from a captured graph
  6. ``select.select_normals``, its smoothing and orientation, and the command line"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _knn_fixture as kx
import _select_fixture as sx

pytestmark = pytest.mark.gpu

# both sides of every multiple of 64 (a lane's second, third and fourth slot begin there), the smallest counts that can be fitted, and 19 more
LADDER32 = (1, 2, 3, 4, 5, 8, 12, 16, 24, 31, 32, 33, 48, 62, 63, 64, 65, 66, 96, 100, 126, 127, 128, 129, 130, 190, 191, 192, 193, 254, 255,
            256)
NAMES = ("normals", "eig", "sel", "k", "radius", "variation_all", "normals_all", "eig_all", "radius_all", "count_all")
SELECTED = ("sel", "k", "radius", "eig", "normals", "variation_all")
_cache = {}


def _b32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _outs(M, L, dev, fill=-7):
    f32, i32 = torch.float32, torch.int32
    specs = (((M, 3), f32), ((M, 3), f32), ((M,), i32), ((M,), i32), ((M,), f32), ((M, L), f32), ((M, L, 3), f32), ((M, L, 3), f32),
             ((M, L), f32), ((M, L), i32))
    return [torch.full(shape, fill, dtype=dt, device=dev) for shape, dt in specs]


def _raw(lib, cloud_d, q_d, M, row0, nbr_d, ladder, slack, at=False, null=(), outs=None, stream=None, N=None):
    """One call of the entry with outputs pre-filled with -7 (NULL for the names in ``null``) -> (rc, dict of the output tensors)."""
    from nesti_net_amd import _lib
    L, dev = len(ladder), cloud_d.device
    outs = outs if outs is not None else _outs(M, L, dev)
    ptrs = [None if name in null else _lib.ptr(t) for name, t in zip(NAMES, outs)]
    head = (_lib.ptr(cloud_d), cloud_d.shape[0] if N is None else N, _lib.ptr(q_d), M) + (() if at else (row0,))
    fn = lib.nesti_pca_select_nbr_at if at else lib.nesti_pca_select_nbr
    with torch.cuda.device(dev):
        rc = fn(*head, _lib.ptr(nbr_d), int(nbr_d.shape[1]), (ctypes.c_int32 * L)(*ladder), L, ctypes.c_double(slack), *ptrs,
                _lib.stream_ptr(stream))
    return rc, dict(zip(NAMES, outs))


def _np(d):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in d.items()}


def _pca_nbr_raw(lib, cloud_d, q_d, M, row0, nbr_d, ks, at=False):
    """``nesti_pca_normals_nbr`` / ``_at`` over the same lists -> (normals, eig, radius, count) as numpy [M,S,..]."""
    from nesti_net_amd import _lib
    S, dev = len(ks), cloud_d.device
    outs = [torch.full((M, S, 3), -7, dtype=torch.float32, device=dev), torch.full((M, S, 3), -7, dtype=torch.float32, device=dev),
            torch.full((M, S), -7, dtype=torch.float32, device=dev), torch.full((M, S), -7, dtype=torch.int32, device=dev)]
    head = (_lib.ptr(cloud_d), cloud_d.shape[0], _lib.ptr(q_d), M) + (() if at else (row0,))
    fn = lib.nesti_pca_normals_nbr_at if at else lib.nesti_pca_normals_nbr
    with torch.cuda.device(dev):
        rc = fn(*head, _lib.ptr(nbr_d), int(nbr_d.shape[1]), (ctypes.c_int32 * S)(*ks), S, *[_lib.ptr(t) for t in outs], _lib.stream_ptr())
    assert rc == 0, lib.nesti_last_error()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def _same_bytes_or_nan(a, b):
    """``_same_bytes`` wherever either side is not a NaN, and NaN on both sides elsewhere: the payload of a NaN that two kernels form by
    the same operations is the hardware's business, not the entry's."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0, _b32(a)), np.where(nan, 0, _b32(b)))


def _candidates_equal_the_list_fit(lib, got, cloud_d, q_d, M, row0, nbr_d, ladder, at=False, label="", same=_same_bytes):
    """Every candidate of the four ``*_all`` outputs against ``nesti_pca_normals_nbr`` called with the ladder in groups of at most 4."""
    for g in range(0, len(ladder), 4):
        ks = ladder[g:g + 4]
        normals, eig, radius, count = _pca_nbr_raw(lib, cloud_d, q_d, M, row0, nbr_d, ks, at)
        sl = slice(g, g + len(ks))
        assert same(got["normals_all"][:, sl], normals), (label, "normals_all", ks)
        assert same(got["eig_all"][:, sl], eig), (label, "eig_all", ks)
        assert _same_bytes(got["radius_all"][:, sl], radius), (label, "radius_all", ks)
        assert _same_bytes(got["count_all"][:, sl], count), (label, "count_all", ks)


def _selection_is_the_restatement(got, slack, label=""):
    """The selected outputs and ``variation_all`` against the fixture's selection over the kernel's own per-candidate outputs."""
    ref = sx.select(got["eig_all"], got["count_all"], got["radius_all"], slack, got["normals_all"])
    for key in SELECTED:
        assert _same_bytes(got[key], ref[key]), (label, key, slack)
    return ref


def _random_cloud(dev):
    """N = 300 random points, M = 301 rows through pidx with repeats, their sorted lists at K = 256, and the fit at LADDER32 and slack 0."""
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
        lib = _lib.load()
        rc, outs = _raw(lib, cp.cloud, cp.pidx, len(pidx), 0, nbr, LADDER32, 0.0)
        assert rc == 0, lib.nesti_last_error()
        _cache["random"] = {"lib": lib, "pts": pts, "pidx": pidx, "cp": cp, "nbr": nbr, "got": _np(outs)}
    return _cache["random"]


# ---- 1, 2 -------------------------------------------------------------------------------------------------------------------------------

def test_every_candidate_is_the_list_fit_bit_for_bit(gpu_device):
    r = _random_cloud(gpu_device)
    M = len(r["pidx"])
    assert len(LADDER32) == 32 and M == 301 and M % 4 and {3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256} <= set(LADDER32)
    got = r["got"]
    _candidates_equal_the_list_fit(r["lib"], got, r["cp"].cloud, r["cp"].pidx, M, 0, r["nbr"], LADDER32, label="random")
    assert np.array_equal(got["count_all"], np.tile(np.array(LADDER32, np.int32), (M, 1)))
    live = got["count_all"] >= 3
    assert (got["normals_all"][live] != 0).any(-1).all() and not got["normals_all"][~live].any() and (got["eig_all"][live].sum(-1) > 0).all()
    assert _same_bytes(got["normals_all"][-1], got["normals_all"][-2])          # the repeated row


@pytest.mark.parametrize("slack", [0.0, 0.5, 1e300])
def test_the_selection_is_the_restatement_bit_for_bit(slack, gpu_device):
    """On the full ladder, where three neighbours are always coplanar (a score of 0 or of rounding size: thr stays there whatever the
    slack), and on its counts from 12 on, where the scores are those of real neighbourhoods."""
    r = _random_cloud(gpu_device)
    M = len(r["pidx"])
    for ladder in (LADDER32, LADDER32[6:]):
        rc, outs = _raw(r["lib"], r["cp"].cloud, r["cp"].pidx, M, 0, r["nbr"], ladder, slack)
        assert rc == 0, r["lib"].nesti_last_error()
        got = _np(outs)
        first = 32 - len(ladder)
        for key in ("normals_all", "eig_all", "radius_all", "count_all", "variation_all"):  # the candidates do not depend on the slack
            assert _same_bytes(got[key], r["got"][key][:, first:]), key
        _selection_is_the_restatement(got, slack, "random")
        v, ok = sx.scores(got["eig_all"], got["count_all"], got["radius_all"])
        assert np.array_equal(ok, got["count_all"] >= 3) and not got["variation_all"][~ok].any()
        assert (got["sel"] >= 0).all() and ok[np.arange(M), got["sel"]].all() and np.array_equal(got["k"], np.array(ladder, np.int32)[got["sel"]])
        if slack == 0.0:
            assert np.array_equal(np.where(ok, v, np.inf).min(1), v[np.arange(M), got["sel"]])
    # the counts from 12 on (the last ladder of the loop): scores above 0, so a huge slack reaches the largest candidate
    assert (got["variation_all"] > 0).all()
    if slack == 1e300:
        assert (got["sel"] == len(ladder) - 1).all()


@pytest.mark.parametrize("L", [7, 8, 9, 15, 16, 17])
def test_ladder_lengths_round_the_fold_widths(L, gpu_device):
    """The kernel folds 8, 16 or 32 candidates at a time, the narrowest that holds L: the lengths on both sides of 8 and 16 give the
    candidates of the 32-count run bit for bit, and the restatement's selection."""
    r = _random_cloud(gpu_device)
    M = len(r["pidx"])
    pool = LADDER32[6:]                                                         # 12 or more neighbours
    ladder = tuple(pool[i] for i in np.linspace(0, len(pool) - 1, L).round().astype(int))      # spread from 12 to 256
    assert len(set(ladder)) == L and ladder[0] == 12 and ladder[-1] == 256
    rc, outs = _raw(r["lib"], r["cp"].cloud, r["cp"].pidx, M, 0, r["nbr"], ladder, 0.5)
    assert rc == 0, r["lib"].nesti_last_error()
    got = _np(outs)
    at = [LADDER32.index(k) for k in ladder]
    for key in ("normals_all", "eig_all", "radius_all", "count_all", "variation_all"):
        assert _same_bytes(got[key], np.ascontiguousarray(r["got"][key][:, at])), (L, key)
    _selection_is_the_restatement(got, 0.5, L)
    assert (got["sel"] >= 0).all() and np.array_equal(got["k"], np.array(ladder, np.int32)[got["sel"]])


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------

def test_edges(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    # L = 1: the one candidate is the selection wherever it can be fitted
    rc, outs = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, (100,), 0.0)
    assert rc == 0
    one = _np(outs)
    _candidates_equal_the_list_fit(lib, one, cp.cloud, cp.pidx, M, 0, nbr, (100,), label="L = 1")
    _selection_is_the_restatement(one, 0.0, "L = 1")
    assert not one["sel"].any() and (one["k"] == 100).all() and _same_bytes(one["normals"], one["normals_all"][:, 0])
    assert _same_bytes(one["normals_all"][:, 0], r["got"]["normals_all"][:, LADDER32.index(100)])
    # the ladder (1, 2) can fit nothing: every row -1 and zeros, the radii and counts of the candidates still written
    rc, outs = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, (1, 2), 0.5)
    assert rc == 0
    none = _np(outs)
    assert (none["sel"] == -1).all() and not none["k"].any()
    for key in ("normals", "eig", "radius", "variation_all", "normals_all", "eig_all"):
        assert not _b32(none[key]).any(), key
    assert np.array_equal(none["count_all"], np.tile(np.array([1, 2], np.int32), (M, 1))) and (none["radius_all"][:, 1] > 0).all()
    # M = 1, and rows by query_row0 with a NULL index: rows 40 .. 59 of the cloud itself
    rows = torch.arange(40, 60, dtype=torch.int32, device=gpu_device)
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    call = CloudPatches(r["pts"], NestiConfig(), device=gpu_device, radius_grid=False)
    lists = call.knn(40, 20, 256)[0]
    rc, by_index = _raw(lib, call.cloud, rows, 20, 0, lists, LADDER32, 0.0)
    assert rc == 0
    rc, by_row0 = _raw(lib, call.cloud, None, 20, 40, lists, LADDER32, 0.0)
    assert rc == 0
    rc, single = _raw(lib, call.cloud, None, 1, 47, lists[7:8].contiguous(), LADDER32, 0.0)
    assert rc == 0
    by_index, by_row0, single = _np(by_index), _np(by_row0), _np(single)
    for key in NAMES:
        assert _same_bytes(by_index[key], by_row0[key]) and _same_bytes(single[key], by_index[key][7:8]), key
    _selection_is_the_restatement(by_row0, 0.0, "row0")
    assert (by_row0["sel"] >= 0).all()


def test_a_prefix_shorter_than_every_count(gpu_device):
    from nesti_net_amd import _lib
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    lib = _lib.load()
    pts = np.random.RandomState(4).uniform(-1, 1, (5, 3)).astype(np.float32)
    cp = CloudPatches(pts, NestiConfig(), device=gpu_device, radius_grid=False)
    nbr = cp.knn(0, 5, 8)[0]                                                    # 5 entries, then -1
    ladder = (6, 7, 8)
    rc, outs = _raw(lib, cp.cloud, None, 5, 0, nbr, ladder, 0.0)
    assert rc == 0
    got = _np(outs)
    assert (got["count_all"] == 5).all() and (got["sel"] == 2).all() and (got["k"] == 5).all()      # duplicates: ties to the larger index
    _candidates_equal_the_list_fit(lib, got, cp.cloud, None, 5, 0, nbr, ladder, label="N = 5")
    _selection_is_the_restatement(got, 0.0, "N = 5")
    assert _same_bytes(got["normals_all"][:, 0], got["normals_all"][:, 2]) and (got["normals"] != 0).any(1).all()
    via = cp.pca_select(0, 5, ladder)                                          # the method searches at ladder[-1] itself
    torch.cuda.synchronize()
    for name, t in zip(NAMES, via):
        assert _same_bytes(t.cpu().numpy(), got[name]), name


def test_positions_and_a_cloud_point_with_a_nan(gpu_device):
    r = _random_cloud(gpu_device)
    lib, pts = r["lib"], r["pts"]
    # positions: a cloud point's own position, one far outside the box, one with a NaN (an empty prefix whatever its list holds)
    q = np.stack([pts[3], np.array([40.0, -3.0, 2.5], np.float32), np.array([0.1, np.nan, 0.2], np.float32), pts[8] + np.float32(0.01)])
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    cq = CloudPatches(pts, NestiConfig(), device=gpu_device, queries=torch.from_numpy(np.where(np.isfinite(q), q, 0.0).astype(np.float32)),
                      radius_grid=False)
    nbr = cq.knn(0, 4, 256)[0]
    q_d = torch.from_numpy(q).to(gpu_device)
    rc, outs = _raw(lib, cq.cloud, q_d, 4, 0, nbr, LADDER32, 0.5, at=True)
    assert rc == 0, lib.nesti_last_error()
    got = _np(outs)
    _candidates_equal_the_list_fit(lib, got, cq.cloud, q_d, 4, 0, nbr, LADDER32, at=True, label="positions")
    _selection_is_the_restatement(got, 0.5, "positions")
    assert got["sel"][2] == -1 and not got["count_all"][2].any() and not _b32(got["normals_all"][2]).any() and not _b32(got["normals"][2]).any()
    assert (got["sel"][[0, 1, 3]] >= 0).all() and got["radius"][1] > 30.0
    idx = torch.tensor([3], dtype=torch.int32, device=gpu_device)
    rc, own = _raw(lib, cq.cloud, idx, 1, 0, nbr[:1].contiguous(), LADDER32, 0.5)
    own = _np(own)
    for key in NAMES:
        assert _same_bytes(own[key], got[key][:1]), key                          # a position equal to a cloud point is that point
    # a cloud point with a NaN coordinate: its terms poison the sums of the candidates that reach it, exactly as in the list fit
    bad = pts.copy()
    bad[77, 2] = np.nan
    cloud_d = torch.from_numpy(bad).to(gpu_device)
    rows = torch.tensor([1, 2, 77], dtype=torch.int32, device=gpu_device)
    lists = r["cp"].knn(0, 3, 256)[0].clone()                                   # any valid lists will do: those of three other rows
    lists[lists == 77] = 0
    lists[0, 40] = 77                                                           # the candidates above 40 of row 0 reach the NaN point
    lists[1, 200] = 77
    rc, outs = _raw(lib, cloud_d, rows, 3, 0, lists, LADDER32, 0.0)
    assert rc == 0
    got = _np(outs)
    _candidates_equal_the_list_fit(lib, got, cloud_d, rows, 3, 0, lists, LADDER32, label="NaN point", same=_same_bytes_or_nan)
    _selection_is_the_restatement(got, 0.0, "NaN point")
    assert got["sel"][2] == -1 and not got["count_all"][2].any()                # the NaN point as a centre: an empty prefix
    assert (got["sel"][:2] >= 0).all() and np.isfinite(got["eig_all"]).all() and np.isfinite(got["variation_all"]).all()
    clean = np.array(LADDER32) <= 40
    assert np.isfinite(got["normals_all"][0, clean]).all() and _same_bytes(got["count_all"][:2], np.tile(np.array(LADDER32, np.int32), (2, 1)))


# ---- 4. untrusted lists -----------------------------------------------------------------------------------------------------------------

def test_untrusted_lists(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, pts, pidx = r["lib"], r["cp"], r["pts"], r["pidx"]
    M = 12
    nbr = r["nbr"][:M].clone().cpu().numpy()
    nbr[0, 100] = -1                                                            # the prefix ends at 100
    nbr[1, 64] = len(pts)                                                       # ... at 64: an index beyond the cloud
    nbr[2, 2] = 2 ** 31 - 1                                                     # ... at 2: nothing can be fitted
    nbr[3, 0] = -5                                                              # ... at 0
    nbr[4] = nbr[4][np.random.RandomState(3).permutation(256)]                  # shuffled: r2_c is a prefix maximum
    nbr[5, 255] = -1
    nbr_d = torch.from_numpy(nbr).to(gpu_device)
    q_d = cp.pidx[:M].contiguous()
    rc, outs = _raw(lib, cp.cloud, q_d, M, 0, nbr_d, LADDER32, 0.0)
    assert rc == 0
    got = _np(outs)
    lad = np.array(LADDER32)
    for row, prefix in ((0, 100), (1, 64), (2, 2), (3, 0), (4, 256), (5, 255), (6, 256)):
        assert np.array_equal(got["count_all"][row], np.minimum(lad, prefix)), row
    _candidates_equal_the_list_fit(lib, got, cp.cloud, q_d, M, 0, nbr_d, LADDER32, label="untrusted")
    _selection_is_the_restatement(got, 0.0, "untrusted")
    assert got["sel"][2] == -1 and got["sel"][3] == -1 and got["k"][0] <= 100 and got["k"][1] <= 64
    # duplicate n_c where the prefix is short: the candidates from 126 on of row 0 are one fit, and a tie goes to the largest index
    assert _same_bytes(got["normals_all"][0, LADDER32.index(100)], got["normals_all"][0, 31])
    if got["k"][0] == 100:
        assert got["sel"][0] == 31
    ref = kx.plane_lists(pts, pts[pidx[:M]], nbr, LADDER32)
    assert _same_bytes(got["radius_all"], ref["radius"])
    last = np.sqrt(kx.d2_all(pts[nbr[4, lad - 1]].astype(np.float64) - pts[pidx[4]].astype(np.float64), 0.0)).astype(np.float32)
    assert (got["radius_all"][4] >= last).all() and (got["radius_all"][4] > last).any()      # the maximum, not the last slot
    assert (np.diff(got["radius_all"][4]) >= 0).all()


# ---- 5. batching, NULL outputs, the profiler and graphs ---------------------------------------------------------------------------------

def test_two_calls_on_two_streams_equal_one(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    cut = 133
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)
    rc1, a = _raw(lib, cp.cloud, cp.pidx[:cut].contiguous(), cut, 0, nbr[:cut].contiguous(), LADDER32, 0.5, stream=s1)
    rc2, b = _raw(lib, cp.cloud, cp.pidx[cut:].contiguous(), M - cut, 0, nbr[cut:].contiguous(), LADDER32, 0.5, stream=s2)
    rc, whole = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, LADDER32, 0.5)
    assert rc1 == 0 and rc2 == 0 and rc == 0
    a, b, whole = _np(a), _np(b), _np(whole)
    for key in NAMES:
        assert _same_bytes(np.concatenate([a[key], b[key]]), whole[key]), key


def test_null_outputs_leave_the_others_unchanged(gpu_device):
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    full = r["got"]
    subsets = [(name,) for name in NAMES] + [tuple(n for n in NAMES if n != "sel"), NAMES[5:], NAMES[:5], ("normals", "eig_all", "count_all"),
                                              NAMES]
    for null in subsets:
        rc, outs = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, LADDER32, 0.0, null=null)
        assert rc == 0, (null, lib.nesti_last_error())
        got = _np(outs)
        for key in NAMES:
            if key in null:
                assert (got[key] == -7).all(), (null, key)                      # never touched
            else:
                assert _same_bytes(got[key], full[key]), (null, key)


def test_profiler_category_and_graph_capture(gpu_device):
    from nesti_net_amd import _lib
    r = _random_cloud(gpu_device)
    lib, cp, nbr, M = r["lib"], r["cp"], r["nbr"], len(r["pidx"])
    torch.cuda.synchronize()
    assert lib.nesti_profile_enable(1) == 0
    try:
        rc, _ = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, LADDER32, 0.0)
        torch.cuda.synchronize()
        ms, launches = _lib.profile_read(lib)
    finally:
        lib.nesti_profile_enable(0)
    assert rc == 0 and sum(ph["patches"] for ph in launches.values()) == 1
    assert sum(n for ph in launches.values() for c, n in ph.items() if c != "patches") == 0 and sum(ph["patches"] for ph in ms.values()) > 0
    with torch.cuda.device(gpu_device):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = cp.pca_select(0, M, LADDER32, 0.5, nbr=nbr)
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
    rc, want = _raw(lib, cp.cloud, cp.pidx, M, 0, nbr, LADDER32, 0.5)
    want = _np(want)
    for name, t in zip(NAMES, out):
        assert _same_bytes(t.cpu().numpy(), want[name]), name


# ---- 6. the Python layer and the command line -------------------------------------------------------------------------------------------

KEYS = ["eig", "eig_all", "k", "n_ball", "normals", "normals_all", "orient", "radius", "radius_all", "sel", "variation", "variation_all"]


def test_python_layer(gpu_device, monkeypatch):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import pca, select, smooth, synth
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts, gt = synth.make_cloud("box", n=2000, seed=3, noise=0.002)
    dev, M, L = str(gpu_device), 2000, len(select.DEFAULT_LADDER)
    searches = []
    knn = CloudPatches.knn
    monkeypatch.setattr(CloudPatches, "knn", lambda self, first, count, k, **kw: (searches.append(k), knn(self, first, count, k, **kw))[1])
    res = select.select_normals(pts, device=dev)
    assert searches == [256]                                                    # one search, at the top of the ladder
    assert sorted(res) == KEYS and res["orient"] is None
    shapes = {"eig": (M, 3), "eig_all": (M, L, 3), "k": (M,), "n_ball": (M, L), "normals": (M, 3), "normals_all": (M, L, 3), "radius": (M,),
              "radius_all": (M, L), "sel": (M,), "variation": (M,), "variation_all": (M, L)}
    assert {k: res[k].shape for k in shapes} == shapes and res["k"].dtype == np.int32 and res["variation"].dtype == np.float32
    # ... agrees with CloudPatches.pca_select, with the fixture's selection, and candidate c with pca_normals(knn=ladder[c])
    cp = CloudPatches(pts, NestiConfig(), device=gpu_device, radius_grid=False)
    direct = [t.cpu().numpy() for t in cp.pca_select(0, M, select.DEFAULT_LADDER, 0.0)]
    for name, a in zip(NAMES, direct):
        assert _same_bytes(res["n_ball" if name == "count_all" else name], a), name
    ref = sx.select(res["eig_all"], res["n_ball"], res["radius_all"], 0.0, res["normals_all"])
    for key in SELECTED:
        assert _same_bytes(res[key], ref[key]), key
    assert _same_bytes(res["variation"], res["variation_all"][np.arange(M), res["sel"]]) and (res["sel"] >= 0).all()
    fixed = pca.pca_normals(pts, knn=select.DEFAULT_LADDER[2:6], device=dev)
    assert _same_bytes(fixed["normals_all"], res["normals_all"][:, 2:6]) and _same_bytes(fixed["radius"], res["radius_all"][:, 2:6])
    assert len(np.unique(res["sel"])) >= 2                                     # rows do choose differently
    share, shares = sx.within_deg(res["normals"], gt), [sx.within_deg(res["normals_all"][:, c], gt) for c in range(L)]
    print("box 2000, noise 0.002: selected %.1f %%, fixed counts %s" % (share, " ".join("%.1f" % s for s in shares)))
    # subsets: pidx and positions give the rows of the whole cloud
    pidx = np.arange(0, M, 9)
    by_index = select.select_normals(pts, pidx=pidx, slack=0.5, device=dev)
    by_position = select.select_normals(pts, queries=pts[pidx], slack=0.5, device=dev)
    loose = select.select_normals(pts, slack=0.5, device=dev)
    for k in KEYS:
        if k != "orient":
            assert _same_bytes(by_index[k], by_position[k]) and _same_bytes(np.ascontiguousarray(loose[k][pidx]), by_index[k]), k
    assert (loose["sel"] >= res["sel"]).all() and (loose["sel"] > res["sel"]).any()
    # smooth=1: the pass over the searched lists (256 reaches the smoothing's k: no second search), everything else as fitted
    del searches[:]
    sm = select.select_normals(pts, smooth=1, device=dev)
    assert searches == [256] and sorted(sm) == sorted(KEYS + ["smooth_support", "smooth_count"])
    for k in KEYS:
        if k not in ("orient", "normals"):
            assert _same_bytes(sm[k], res[k]), k
    p = smooth.check_params(iters=1)
    lists = cp.knn(0, M, 256)[0]
    want = cp.smooth_knn(torch.from_numpy(res["normals"]).to(gpu_device), 0, M, p.k, p.cos_t, p.falloff, nbr=lists)
    assert _same_bytes(sm["normals"], want[0].cpu().numpy()) and _same_bytes(sm["smooth_count"], want[2].cpu().numpy())
    assert not _same_bytes(sm["normals"], res["normals"])
    # a ladder that does not reach the smoothing's k: the passes search for themselves
    del searches[:]
    short = select.select_normals(pts, ladder=(8, 12), smooth=1, device=dev)
    assert searches == [12, 16] and short["normals"].shape == (M, 3)
    # orient='viewpoint': only sign bits differ from the unoriented run
    vp = select.select_normals(pts, orient="viewpoint", viewpoint=(9.0, 0.5, 0.25), device=dev)
    assert np.array_equal(np.abs(vp["normals"]), np.abs(res["normals"])) and (_b32(vp["normals"]) != _b32(res["normals"])).any()
    assert vp["orient"]["n_flipped"] > 0 and vp["orient"]["n_eligible"] == M
    for k in KEYS:
        if k not in ("orient", "normals"):
            assert _same_bytes(vp[k], res[k]), k
    both = select.select_normals(pts, smooth=1, orient="mst", device=dev)
    assert np.array_equal(np.abs(both["normals"]), np.abs(sm["normals"])) and both["orient"]["n_eligible"] == M


def test_command_line(tmp_path, gpu_device):
    from nesti_net_amd import select, synth, textio
    from nesti_net_amd.cli import main
    d = tmp_path / "data"
    d.mkdir()
    pts, _ = synth.make_cloud("box", n=500, seed=3, noise=0.002)
    np.savetxt(d / "cube.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("cube\n")
    common = ["--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]
    pts32 = np.loadtxt(d / "cube.xyz").astype("float32")
    exts = (".normals", ".select_k", ".select_eig", ".select_variation", ".knn_radius")
    for tag, flags, kw in (("auto", ["--knn_ladder", "auto"], {}),
                           ("slack", ["--knn_ladder", "8,20,50,120", "--select_slack", "0.5"], {"ladder": (8, 20, 50, 120), "slack": 0.5})):
        results = str(tmp_path / tag)
        assert main(["--estimator", "pca", "--results_path", results] + flags + common) == 0
        out = os.path.join(results, "synth_results")
        assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["cube" + e for e in exts])
        res = select.select_normals(pts32, device=str(gpu_device), **kw)
        want = str(tmp_path / ("want_" + tag))
        textio.write_f32(want + ".normals", res["normals"])
        textio.write_i32(want + ".select_k", res["k"])
        textio.write_f32(want + ".select_eig", res["eig"])
        textio.write_f32(want + ".select_variation", res["variation_all"])
        textio.write_f32(want + ".knn_radius", res["radius"])
        for e in exts:
            assert open(os.path.join(out, "cube" + e), "rb").read() == open(want + e, "rb").read(), (tag, e)
        L = len(kw.get("ladder", select.DEFAULT_LADDER))
        assert np.loadtxt(os.path.join(out, "cube.select_variation")).shape == (500, L)
        assert np.array_equal(np.loadtxt(os.path.join(out, "cube.select_k"), dtype=np.int64), res["k"])
        log = open(os.path.join(out, "log.txt")).read()
        ladder = kw.get("ladder", select.DEFAULT_LADDER)
        hist = np.bincount(res["sel"], minlength=L)
        assert "scale-selected plane fit of cube: 500 rows, slack %g; chosen neighbour counts: %s; 0 rows without a fit" % (
            kw.get("slack", 0.0), ", ".join("%d: %d" % (k, n) for k, n in zip(ladder, hist))) in log
    # with --smooth and --orient the written normals are the Python call's
    results = str(tmp_path / "both")
    assert main(["--estimator", "pca", "--knn_ladder", "auto", "--smooth", "1", "--orient", "viewpoint", "--viewpoint", "9", "0.5", "0.25",
                 "--results_path", results] + common) == 0
    out = os.path.join(results, "synth_results")
    assert sorted(os.listdir(out)) == sorted(["log.txt", "cube.smooth_support"] + ["cube" + e for e in exts])
    res = select.select_normals(pts32, smooth=1, orient="viewpoint", viewpoint=(9.0, 0.5, 0.25), device=str(gpu_device))
    textio.write_f32(str(tmp_path / "want_both.normals"), res["normals"])
    assert open(os.path.join(out, "cube.normals"), "rb").read() == open(str(tmp_path / "want_both.normals"), "rb").read()
