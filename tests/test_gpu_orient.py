"""Orientation of estimated normals on real kernels (csrc/orient.hip) against the tests' own numpy restatement
(tests/_orient_fixture.py): the neighbour lists and edges integer for integer, the weights to f32 rounding, and -- with the
restatement's Kruskal ordering the edges by the LIBRARY's weight bits -- every sign bit, the spanning forest and the stats exactly."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _orient_fixture as F

pytestmark = pytest.mark.gpu

_graphs, _runs = {}, {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def lib_graph(xyz, normals, R, K, device):
    """``nesti_orient_graph`` -> {nbr [M,K], u, v, wbits, flip [M K]} as numpy."""
    from nesti_net_amd import _lib
    lib = _lib.load()
    M = len(xyz)
    x, n = _dev(xyz, device), _dev(normals, device)
    gws = torch.empty(max(1, lib.nesti_patches_workspace_bytes(M)), dtype=torch.uint8, device=device)
    ws = torch.empty(max(1, lib.nesti_orient_workspace_bytes(M, K)), dtype=torch.uint8, device=device)
    nbr = torch.full((M, K), -7, dtype=torch.int32, device=device)
    u, v = (torch.full((M * K,), -7, dtype=torch.int32, device=device) for _ in range(2))
    wb = torch.zeros(M * K, dtype=torch.int32, device=device)
    fl = torch.full((M * K,), 9, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.nesti_orient_graph(_lib.ptr(x), M, _lib.ptr(n), ctypes.c_double(R), K, _lib.ptr(gws), gws.numel(), _lib.ptr(ws),
                                          ws.numel(), _lib.ptr(nbr), _lib.ptr(u), _lib.ptr(v), _lib.ptr(wb), _lib.ptr(fl),
                                          _lib.stream_ptr(torch.cuda.current_stream(device))), "nesti_orient_graph")
    torch.cuda.synchronize(device)
    return {"nbr": nbr.cpu().numpy(), "u": u.cpu().numpy(), "v": v.cpu().numpy(), "wbits": wb.cpu().numpy().view(np.uint32),
            "flip": fl.cpu().numpy()}


def lib_orient(xyz, normals, R, K, device, viewpoint=None, mode=0, extras=True, stream=None, in_place_on=None):
    """``nesti_orient_normals`` -> (normals, tree [M K] or None, stats dict or None) as numpy."""
    from nesti_net_amd import _lib
    lib = _lib.load()
    M = len(xyz)
    st = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.device(device), torch.cuda.stream(st):
        x = _dev(xyz, device)
        n = in_place_on if in_place_on is not None else _dev(normals, device)
        gws = torch.empty(max(1, lib.nesti_patches_workspace_bytes(M)), dtype=torch.uint8, device=device)
        ws = torch.empty(max(1, lib.nesti_orient_workspace_bytes(M, K)), dtype=torch.uint8, device=device)
        tree = torch.full((max(1, M * K),), 7, dtype=torch.uint8, device=device) if extras else None
        stats = torch.full((4,), -7, dtype=torch.int32, device=device) if extras else None
        vp = (ctypes.c_double * 3)(*viewpoint) if viewpoint is not None else None
        _lib.check(lib.nesti_orient_normals(_lib.ptr(x), M, _lib.ptr(n), mode, ctypes.c_double(R), K, vp, _lib.ptr(gws), gws.numel(),
                                            _lib.ptr(ws), ws.numel(), _lib.ptr(tree), _lib.ptr(stats), ctypes.c_void_p(st.cuda_stream)),
                   "nesti_orient_normals")
        st.synchronize()
    names = ("n_eligible", "n_components", "n_flipped", "n_edges")
    return (n.cpu().numpy(), tree.cpu().numpy()[:M * K] if extras else None,
            dict(zip(names, stats.cpu().tolist())) if extras else None)


def _extra_case(name):
    """The cases beyond the table: (xyz, normals, R, K, viewpoint, mode)."""
    c = F.case("ellipsoid3001")
    if name == "one_point":
        return c["xyz"][:1], c["normals"][:1], c["R"], 8, None, 0
    if name == "tiny_radius":                      # every row is its own component
        return c["xyz"], c["normals"], 1e-7, 8, None, 0
    if name == "view_outside":
        return c["xyz"], c["normals"], c["R"], 8, (0.3, -0.2, 5.0), 0
    if name == "view_inside":
        return c["xyz"], c["normals"], c["R"], 8, (0.05, 0.02, -0.01), 0
    if name == "viewpoint_mode":
        return c["xyz"], c["normals"], c["R"], 8, (2.0, 3.0, 1.0), 1
    if name == "non_finite_normals":               # NaN / inf / -0 rows on top of the 10 % zero rows: all ineligible, all untouched
        z = F.case("ellipsoid3001_zero10")
        n = z["normals"].copy()
        n[5] = (np.nan, 1.0, 0.0)
        n[6] = (np.inf, 0.0, 0.0)
        n[7] = (0.0, -0.0, 0.0)
        n[8] = (-np.inf, np.nan, 2.0)
        n[3000] = (1.0, 2.0, np.nan)
        return z["xyz"], n, z["R"], 8, None, 0
    raise KeyError(name)


EXTRAS = ("one_point", "tiny_radius", "view_outside", "view_inside", "viewpoint_mode", "non_finite_normals")


def _inputs(name):
    if name in F.TABLE:
        c = F.case(name)
        return c["xyz"], c["normals"], c["R"], c["K"], c["viewpoint"], 0
    return _extra_case(name)


def _graph_pair(name, device):
    """(the restatement's graph, the library's) of a case, each computed once."""
    if name not in _graphs:
        xyz, normals, R, K, _, _ = _inputs(name)
        ref = F.predicted(name)["g"] if name in F.TABLE else F.graph(xyz, normals, R, K)
        _graphs[name] = (ref, lib_graph(xyz, normals, R, K, device))
    return _graphs[name]


def _run(name, device):
    """(library output, tree, stats) of a case, computed once."""
    if name not in _runs:
        xyz, normals, R, K, vp, mode = _inputs(name)
        _runs[name] = lib_orient(xyz, normals, R, K, device, vp, mode)
    return _runs[name]


@pytest.mark.parametrize("name", ("ellipsoid3001", "ellipsoid3001_k1", "ellipsoid3001_k16", "lattice", "ellipsoid3001_zero10"))
def test_graph_parity(name, gpu_device):
    """Neighbour lists (order included), edge slots, ends and flip bits exact; weights within 1e-6 (f32 rounding of a value in
    [0, 1] is 6e-8; the margin is for the fp64 division) -- the expectation is that no weight differs in a single bit."""
    ref, got = _graph_pair(name, gpu_device)
    assert np.array_equal(got["nbr"], ref["nbr"])
    assert np.array_equal(got["u"], ref["u"]) and np.array_equal(got["v"], ref["v"])
    edges = ref["u"] >= 0
    assert edges.sum() > 1000
    assert np.array_equal(got["flip"][edges], ref["flip"][edges])
    w = got["wbits"].view(np.float32)
    diff = np.abs(w[edges].astype(np.float64) - ref["w"][edges].astype(np.float64))
    print("%s: %d edges, %d weights differ in their bits, largest |dw| %.3g"
          % (name, int(edges.sum()), int((got["wbits"][edges] != ref["wbits"][edges]).sum()), float(diff.max())))
    assert (diff <= 1e-6).all()
    assert not got["wbits"][~edges].any() and not got["flip"][~edges].any()      # empty slots carry nothing


@pytest.mark.parametrize("name", F.TABLE + EXTRAS)
def test_orientation_bit_for_bit(name, gpu_device):
    """Every output row has the bits of +input or -input as predicted, the forest is Kruskal's, the stats are equal, ineligible rows
    are bit-identical to the input.  The restatement orders the edges by the library's weight bits (checked above, to tolerance), so
    everything here is integer-exact."""
    xyz, normals, R, K, vp, mode = _inputs(name)
    out, tree, stats = _run(name, gpu_device)
    if mode == 1:
        want = F.orient_viewpoint(xyz, normals, vp)
        assert not tree.any()
    else:
        ref, got = _graph_pair(name, gpu_device)
        assert np.array_equal(got["u"], ref["u"]) and np.array_equal(got["v"], ref["v"]) and np.array_equal(got["nbr"], ref["nbr"])
        want = F.orient(xyz, normals, R, K, vp, g=ref, wbits=got["wbits"])
        assert np.array_equal(tree, want["tree"])
        if name == "helix2000":
            assert want["depth"] >= 1000           # pointer jumping over a path as long as the cloud
        if name == "tiny_radius":
            assert want["stats"]["n_components"] == len(xyz) and want["stats"]["n_edges"] == 0
    assert np.array_equal(out.view(np.uint32), want["out"].view(np.uint32))
    assert stats == want["stats"]
    el = F.eligible(normals)
    assert np.array_equal(out[~el].view(np.uint32), np.asarray(normals)[~el].view(np.uint32))
    if name == "non_finite_normals":
        assert (~el).sum() > 300 and not el[[5, 6, 7, 8, 3000]].any()
    if name == "view_outside":
        assert F.inward(out, F.case("ellipsoid3001")["gt"], normals) == 0
    if name == "view_inside":
        assert F.inward(out, F.case("ellipsoid3001")["gt"], normals) == len(xyz)


def test_empty_input_is_a_no_op(gpu_device):
    out, tree, stats = lib_orient(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.1, 8, gpu_device)
    assert out.shape == (0, 3) and stats == dict.fromkeys(("n_eligible", "n_components", "n_flipped", "n_edges"), -7)   # nothing written
    from nesti_net_amd.orient import orient_normals
    n, st = orient_normals(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.1, device=gpu_device)
    assert n.shape == (0, 3) and st == dict.fromkeys(("n_eligible", "n_components", "n_flipped", "n_edges"), 0)


@pytest.mark.parametrize("name", F.SANITY)
def test_semantics_on_the_device(name, gpu_device):
    """No oriented row points against the analytic normal, one tree per surface, oriented RMS == unoriented RMS."""
    from nesti_net_amd.evaluate import shape_metrics
    c = F.case(name)
    out, _, stats = _run(name, gpu_device)
    el = F.eligible(c["normals"])
    assert F.inward(out, c["gt"], c["normals"]) == 0 and stats["n_components"] == c["surfaces"]
    m = shape_metrics(out[el], c["gt"][el])
    assert m["rms_o"] == m["rms"]


def test_purity(gpu_device):
    """The same call twice, on two other streams, in place on a tensor of the caller's, and without the optional outputs: identical
    bits every time."""
    c = F.case("ellipsoid3001_zero10")
    base = _run("ellipsoid3001_zero10", gpu_device)[0].view(np.uint32)
    args = (c["xyz"], c["normals"], c["R"], c["K"], gpu_device)
    assert np.array_equal(lib_orient(*args)[0].view(np.uint32), base)
    for _ in range(2):
        s = torch.cuda.Stream(device=gpu_device)
        assert np.array_equal(lib_orient(*args, stream=s)[0].view(np.uint32), base)
    mine = _dev(c["normals"], gpu_device)
    torch.cuda.synchronize(gpu_device)
    got = lib_orient(*args, in_place_on=mine)[0]
    assert np.array_equal(got.view(np.uint32), base) and np.array_equal(mine.cpu().numpy().view(np.uint32), base)
    assert np.array_equal(lib_orient(*args, extras=False)[0].view(np.uint32), base)
    # orienting an oriented field changes nothing but (at most) nothing: the root rule already holds and no edge asks for a flip
    again, _, st = lib_orient(c["xyz"], got, c["R"], c["K"], gpu_device)
    assert st["n_flipped"] == 0 and np.array_equal(again.view(np.uint32), base)


@pytest.fixture(scope="module")
def stack(gpu_device):
    """A small estimator (synthetic weights, plain f16) and ~600 sparse rows of a 6 000-point ellipsoid."""
    from nesti_net_amd import synth, weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.pipeline import NormalEstimator
    cfg = NestiConfig(num_point=64)
    pts = synth.make_cloud("ellipsoid", n=6000, seed=21)[0]
    pidx = np.arange(3, 6000, 10)[:600].astype(np.int32)
    est = NormalEstimator(cfg, weights.synthetic_weights(cfg), dtype="f16", device=gpu_device, batch=256)
    return {"est": est, "pts": pts, "pidx": pidx, "plain": est.estimate(pts, pidx=pidx)}


def _signed_rows(a, b):
    """Every row of a equals the row of b or its negation, bit for bit."""
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    same = (ua == ub).all(axis=1)
    neg = (ua == (ub ^ np.uint32(0x80000000))).all(axis=1)
    return bool((same | neg).all())


def test_estimate_with_orientation(stack, gpu_device):
    from nesti_net_amd.orient import orient_normals
    est, pts, pidx = stack["est"], stack["pts"], stack["pidx"]
    n0, e0, p0 = stack["plain"]
    n1, e1, p1 = est.estimate(pts, pidx=pidx, orient="mst")
    r = float(est.prepare(pts, pidx=pidx).r_abs[-1])
    want, st = orient_normals(pts[pidx], n0, r, device=gpu_device)
    assert np.array_equal(n1.view(np.uint32), want.view(np.uint32)) and est.last_orient == st
    assert st["n_eligible"] == 600 and 0 < st["n_flipped"] < 600
    assert _signed_rows(n1, n0) and np.array_equal(e1, e0) and np.array_equal(p1.view(np.uint32), p0.view(np.uint32))
    # torch in, torch out; the viewpoint mode through the same door
    nv, _, _ = est.estimate(pts, pidx=pidx, orient="viewpoint", viewpoint=(0.0, 0.0, 9.0))
    wv, sv = orient_normals(torch.from_numpy(pts[pidx]), torch.from_numpy(n0), r, viewpoint=(0.0, 0.0, 9.0), mode="viewpoint", device=gpu_device)
    assert isinstance(wv, torch.Tensor) and np.array_equal(nv.view(np.uint32), wv.numpy().view(np.uint32)) and sv["n_components"] == 0
    with pytest.raises(ValueError):
        est.estimate(pts, pidx=pidx, orient="viewpoint")


def test_sentinel_rows_stay_with_queries(stack, gpu_device):
    """Position queries that include far-away and non-finite positions: their rows stay (0, 0, 0) / -1, the others are oriented."""
    est, pts = stack["est"], stack["pts"]
    q = pts[5::12][:400].copy()
    q[::50] += 40.0
    q[7] = (np.nan, 0.0, 0.0)
    q = torch.from_numpy(q)                        # a host array with a non-finite row is refused as a caller's mistake; a tensor is served
    n0, e0, _ = est.estimate(pts, queries=q)
    n1, e1, _ = est.estimate(pts, queries=q, orient="mst")
    alone = e0 == -1
    assert alone[::50].all() and alone[7] and not alone.all()
    assert np.array_equal(e1, e0) and not n1[alone].any() and not np.signbit(n1[alone]).any()
    assert _signed_rows(n1, n0) and est.last_orient["n_eligible"] == int((~alone).sum())


def test_command_line(stack, tmp_path, gpu_device, capsys):
    """--orient mst against --orient 0: .experts and .experts_probs byte-identical, every .normals row equal or negated;
    --orient viewpoint without --viewpoint is refused with a message."""
    from nesti_net_amd.cli import main
    d = tmp_path / "pcp"
    d.mkdir()
    np.savetxt(str(d / "shapeA.xyz"), stack["pts"], fmt="%.9g")
    np.savetxt(str(d / "shapeA.pidx"), stack["pidx"], fmt="%d")
    (d / "testset.txt").write_text("shapeA\n")
    files = {}
    for mode in ("0", "mst"):
        results = str(tmp_path / ("log_" + mode)) + os.sep
        assert main(["--results_path", results, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt",
                     "--synthetic_weights", "--sparse_patches", "1", "--dtype", "f16", "--lib_batch", "512", "--orient", mode]) == 0
        out = os.path.join(results, "synth_results")
        files[mode] = {ext: open(os.path.join(out, "shapeA" + ext), "rb").read() for ext in (".normals", ".experts", ".experts_probs")}
        log = open(os.path.join(out, "log.txt")).read()
        assert ("orientation of shapeA (mst): 600 of 600 rows oriented" in log) == (mode == "mst")
    assert files["0"][".experts"] == files["mst"][".experts"] and files["0"][".experts_probs"] == files["mst"][".experts_probs"]
    a = np.array([l.split() for l in files["0"][".normals"].decode().splitlines()])
    b = np.array([l.split() for l in files["mst"][".normals"].decode().splitlines()])
    assert a.shape == b.shape == (600, 3)
    af, bf = a.astype(np.float64), b.astype(np.float64)
    same, neg = (af == bf).all(axis=1), (af == -bf).all(axis=1)
    assert (same | neg).all() and neg.any() and files["0"][".normals"] != files["mst"][".normals"]
    with pytest.raises(SystemExit):
        main(["--results_path", str(tmp_path / "log_v") + os.sep, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep,
              "--testset", "testset.txt", "--synthetic_weights", "--orient", "viewpoint"])
    assert "--orient viewpoint needs --viewpoint" in capsys.readouterr().err
