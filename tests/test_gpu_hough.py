"""Hough-transform normals on the GPU (csrc/hough.hip, ``CloudPatches.hough_knn``, ``hough.hough_normals``, ``--estimator hough``)
against the tests' own numpy restatement (tests/_hough_fixture.py): every output -- normals, conf, votes, radius, count -- equal ON THE
BYTES.  The lists come from ``nesti_knn`` or are written by hand; the restatement takes the list it is given."""
import os

import numpy as np
import pytest
import torch

import _hough_fixture as hx
from test_hough import lattice

pytestmark = pytest.mark.gpu

KEYS = ("normals", "conf", "votes", "radius", "count")
KS = (3, 17, 40)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check(got, ref, label):
    for key, g in zip(KEYS, got):
        assert _same_bytes(g, ref[key]), (label, key, np.flatnonzero((g != ref[key]).reshape(len(g), -1).any(1))[:8])


def _rot(R):
    from nesti_net_amd import hough
    return hough.rotation_table(R)


_state = {}


def _box(dev):
    """box, n = 300: the cloud, a CloudPatches over all rows and the 40-NN lists of nesti_knn (device and host), prepared once."""
    if "box" not in _state:
        from nesti_net_amd import synth
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        pts, _ = synth.make_cloud("box", n=300, seed=3)
        cp = CloudPatches(pts, NestiConfig(), device=dev, radius_grid=False)
        nbr = cp.knn(0, len(pts), 40)[0]
        _state["box"] = (pts, cp, nbr, nbr.cpu().numpy())
    return _state["box"]


@pytest.mark.parametrize("B, R", [(2, 1), (16, 3), (16, 8)])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 200])
def test_every_output_equals_the_restatement(T, B, R, gpu_device):
    """1.  box, all 300 rows, the lists of nesti_knn at K = 40, ks = (3, 17, 40); T at the wave boundaries and tiny (ties between bins)."""
    pts, cp, nbr, nbr_h = _box(gpu_device)
    got = _np(cp.hough_knn(0, len(pts), KS, T, B, R, 9, nbr=nbr))
    _check(got, hx.restate(pts, pts, nbr_h, KS, T, B, R, _rot(R), 9), (T, B, R))
    assert (got[4] == np.array(KS)).all() and np.isfinite(got[0]).all()
    if T >= 63:
        assert (got[2][:, 2, 0] > 0).all()                                  # 40 neighbours on a box: some triplet is valid


def test_queries_and_batching(gpu_device):
    """2.  The same rows as index queries, as position queries of the same coordinates, and split into calls of 1 / 7 / rest with the
    matching first row: identical bytes, and a search inside the call (no list given) gives them too."""
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts, cp, nbr, nbr_h = _box(gpu_device)
    M = len(pts)
    T, B, R, seed = 130, 16, 5, 2 ** 40 + 5
    whole = _np(cp.hough_knn(0, M, KS, T, B, R, seed, nbr=nbr))
    _check(whole, hx.restate(pts, pts, nbr_h, KS, T, B, R, _rot(R), seed), "whole")
    searched = _np(cp.hough_knn(0, M, KS, T, B, R, seed))
    by_index = CloudPatches(pts, NestiConfig(), device=gpu_device, pidx=np.arange(M), radius_grid=False)
    by_position = CloudPatches(pts, NestiConfig(), device=gpu_device, queries=torch.from_numpy(pts), radius_grid=False)
    for label, other in (("searched", searched), ("index", _np(by_index.hough_knn(0, M, KS, T, B, R, seed, nbr=nbr))),
                         ("position", _np(by_position.hough_knn(0, M, KS, T, B, R, seed, nbr=nbr)))):
        for key, a, b in zip(KEYS, whole, other):
            assert _same_bytes(a, b), (label, key)
    for c in (cp, by_index, by_position):
        parts = [_np(c.hough_knn(first, count, KS, T, B, R, seed, nbr=nbr[first:first + count].contiguous()))
                 for first, count in ((0, 1), (1, 7), (8, M - 8))]
        for k, key in enumerate(KEYS):
            assert _same_bytes(np.concatenate([p[k] for p in parts]), whole[k]), key
    other_seed = _np(cp.hough_knn(0, M, KS, T, B, R, seed + 1, nbr=nbr))
    assert not _same_bytes(other_seed[2], whole[2])                          # the seed reaches the kernel, all 64 bits of it
    assert not _same_bytes(_np(cp.hough_knn(0, M, KS, T, B, R, 5, nbr=nbr))[2], whole[2])


def test_hostile_lists(gpu_device):
    """3.  -1 padding, a bad index mid-row (the prefix is cut; a prefix of 2 gives the sentinel), unsorted lists, a non-finite centre,
    all neighbours coincident (valid = 0, votes (0, 0)), neighbours on one line."""
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    box, _, _, nbr_h = _box(gpu_device)
    same = np.full((12, 3), 0.25, np.float32)                                # rows 300 .. 311
    line = np.stack([np.arange(12, dtype=np.float32) * np.float32(0.1), np.zeros(12, np.float32), np.ones(12, np.float32)], 1)   # 312 .. 323
    pts = np.concatenate([box, same, line])
    N, K, ks = len(pts), 16, (3, 9, 16)
    rs = np.random.RandomState(4)
    nbr = nbr_h[:12, :K].copy()
    for i in range(len(nbr)):
        nbr[i] = nbr[i][rs.permutation(K)]                                   # unsorted
    nbr[1, 10:] = -1                                                         # padding: prefix 10
    nbr[2, 5] = N                                                            # a bad index: prefix 5
    nbr[3, 2] = -9                                                           # prefix 2: sentinel
    nbr[4, 0] = 2 ** 31 - 1                                                  # prefix 0
    nbr[5, :] = -1
    nbr[6, :] = np.arange(300, 300 + K) % 12 + 300                           # coincident
    nbr[7, :] = np.arange(312, 312 + K) % 12 + 312                           # on one line
    nbr[7, :12] = rs.permutation(12) + 312
    centres = pts[[0, 1, 2, 3, 4, 5, 300, 312, 8, 9, 10, 11]].copy()
    centres[9] = [np.nan, 0, 0]                                              # lost centres: empty prefixes
    centres[10] = [0, -np.inf, 0]
    cq = CloudPatches(pts, NestiConfig(), device=gpu_device, queries=torch.from_numpy(centres), radius_grid=False)
    got = _np(cq.hough_knn(0, len(centres), ks, 200, 16, 5, 3, nbr=torch.from_numpy(nbr).to(gpu_device)))
    ref = hx.restate(pts, centres, nbr, ks, 200, 16, 5, _rot(5), 3)
    _check(got, ref, "hostile")
    normals, conf, votes, radius, count = got
    assert count[1].tolist() == [3, 9, 10] and count[2].tolist() == [3, 5, 5] and count[3].tolist() == [2, 2, 2]
    for row in (4, 5, 9, 10):
        assert not count[row].any() and not radius[row].any()
    for row in (3, 4, 5, 6, 7, 9, 10):                                       # sentinels: 0 0 0, confidence 0, votes (0, 0)
        assert not normals[row].any() and not conf[row].any() and not votes[row].any(), row
    assert count[6].tolist() == list(ks) and count[7].tolist() == list(ks) and not radius[6].any() and (radius[7] > 0).all()
    assert (votes[[0, 8, 11], 2, 0] > 0).all() and np.isfinite(normals).all() and np.isfinite(conf).all()


def test_lds_capacity_corner(gpu_device):
    """4.  K = 256, ks = (256,), T = 4096, B = 16, R = 8 on 32 rows: every staged slot and every counter in use."""
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts = _box(gpu_device)[0]
    rows = np.arange(0, 288, 9)
    cp = CloudPatches(pts, NestiConfig(), device=gpu_device, pidx=rows, radius_grid=False)
    nbr = cp.knn(0, len(rows), 256)[0]
    got = _np(cp.hough_knn(0, len(rows), (256,), 4096, 16, 8, 1, nbr=nbr))
    _check(got, hx.restate(pts, pts[rows], nbr.cpu().numpy(), (256,), 4096, 16, 8, _rot(8), 1), "corner")
    assert (got[4] == 256).all() and (got[2][:, 0, 1] > 3000).all()


def test_planar_lattice(gpu_device):
    """5.  Every neighbourhood lies in z = 0: the bytes of (0, 0, 1) and of 1.0f."""
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.provider import CloudPatches
    pts = lattice()
    cp = CloudPatches(pts, NestiConfig(), device=gpu_device, radius_grid=False)
    normals, conf, votes, radius, count = _np(cp.hough_knn(0, len(pts), (9, 25), 200, 16, 5, 0))
    assert _same_bytes(normals, np.broadcast_to(np.array([0, 0, 1], np.float32), normals.shape).copy())
    assert _same_bytes(conf, np.ones(conf.shape, np.float32)) and (votes[..., 0] == votes[..., 1]).all() and (votes[..., 1] > 0).all()


def test_graph_capture(gpu_device):
    """6.  The call enqueues one kernel and reads nothing back: captured into a graph (default queue settings), the replay writes the
    same bytes."""
    pts, cp, nbr, _ = _box(gpu_device)
    args = (0, len(pts), KS, 200, 16, 5, 9)
    want = _np(cp.hough_knn(*args, nbr=nbr))
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.device(gpu_device):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = cp.hough_knn(*args, nbr=nbr)
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize(gpu_device)
    for key, a, b in zip(KEYS, want, _np(out)):
        assert _same_bytes(a, b), key
    assert want[2][..., 0].any()


def test_python_layer_and_command_line(tmp_path, gpu_device):
    """7.  ``hough_normals``: keys and shapes; ``orient='viewpoint'`` changes sign bits only.  ``--estimator hough`` writes the arrays
    the Python call returns, through the same writers."""
    from nesti_net_amd import hough, textio
    from nesti_net_amd.cli import main
    pts, cp, nbr, nbr_h = _box(gpu_device)
    dev = str(gpu_device)
    kw = dict(knn=KS, triplets=130, bins=8, rotations=3, seed=4, device=dev)
    plain = hough.hough_normals(pts, **kw)
    keys = ["conf", "n_ball", "normals", "normals_all", "orient", "radius", "votes"]
    M = len(pts)
    assert sorted(plain) == keys and plain["orient"] is None
    assert [plain[k].shape for k in keys if k != "orient"] == [(M, 3), (M, 3), (M, 3), (M, 3, 3), (M, 3), (M, 3, 2)]
    ref = hx.restate(pts, pts, nbr_h, KS, 130, 8, 3, _rot(3), 4)
    for key, mine in (("normals_all", "normals"), ("conf", "conf"), ("votes", "votes"), ("radius", "radius"), ("n_ball", "count")):
        assert _same_bytes(plain[key], ref[mine]), key
    assert _same_bytes(plain["normals"], np.ascontiguousarray(plain["normals_all"][:, -1]))
    vp = hough.hough_normals(pts, scale=1, orient="viewpoint", viewpoint=(9.0, 0.0, 0.0), **kw)
    before = np.ascontiguousarray(plain["normals_all"][:, 1])
    assert _same_bytes(vp["normals_all"], plain["normals_all"]) and _same_bytes(vp["conf"], plain["conf"])
    assert np.array_equal(vp["normals"].view(np.uint32) & 0x7fffffff, before.view(np.uint32) & 0x7fffffff)
    assert (vp["normals"].view(np.uint32) != before.view(np.uint32)).any() and vp["orient"]["n_flipped"] > 0
    pidx = np.arange(0, M, 3)
    sub = hough.hough_normals(pts, pidx=pidx, **kw)                           # the key row is the patch row: not the rows of `plain`
    assert sub["normals_all"].shape == (len(pidx), 3, 3) and _same_bytes(sub["radius"], np.ascontiguousarray(plain["radius"][pidx]))

    d = tmp_path / "data"
    d.mkdir()
    np.savetxt(d / "box.xyz", pts.astype(np.float64))
    (d / "testset.txt").write_text("box\n")
    results = str(tmp_path / "res")
    assert main(["--estimator", "hough", "--knn", "17,40", "--hough_scale", "0", "--hough_triplets", "130", "--hough_bins", "8",
                 "--hough_rotations", "3", "--hough_seed", "4", "--orient", "viewpoint", "--viewpoint", "9", "0", "0",
                 "--results_path", results, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt"]) == 0
    out = os.path.join(results, "synth_results")
    exts = (".normals", ".hough_conf", ".hough_votes", ".hough_count", ".knn_radius")
    assert sorted(os.listdir(out)) == sorted(["log.txt"] + ["box" + e for e in exts])
    pts32 = np.loadtxt(d / "box.xyz").astype("float32")
    res = hough.hough_normals(pts32, knn=(17, 40), scale=0, triplets=130, bins=8, rotations=3, seed=4, orient="viewpoint",
                              viewpoint=(9.0, 0.0, 0.0), device=dev)
    want = str(tmp_path / "want")
    textio.write_f32(want + ".normals", res["normals"])
    textio.write_f32(want + ".hough_conf", res["conf"])
    textio.write_i32_rows(want + ".hough_votes", res["votes"].reshape(M, -1))
    textio.write_i32_rows(want + ".hough_count", res["n_ball"])
    textio.write_f32(want + ".knn_radius", res["radius"])
    for e in exts:
        assert open(os.path.join(out, "box" + e), "rb").read() == open(want + e, "rb").read(), e
    assert np.loadtxt(os.path.join(out, "box.normals"), dtype=np.float32).shape == (M, 3)
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.hough_votes"), dtype=np.int64).reshape(M, 2, 2), res["votes"])
    assert np.array_equal(np.loadtxt(os.path.join(out, "box.hough_conf"), dtype=np.float32), res["conf"])
    log = open(os.path.join(out, "log.txt")).read()
    assert "Hough transform of box" in log and "17 nearest neighbours" in log
