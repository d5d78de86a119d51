"""The uniform search grid (csrc/patches.hip, the walk in csrc/patches_dev.h) and the six kernels on it, on clouds that leave the regime
of the surface clouds (tests/_grid_fixture.py): the kMaxDim clamp (cell edge = ext / 127, not tied to the radius), 128 x 1 x 1 and
~127^3 grids, an integer lattice with thousands of pairs at d2 == r^2 exactly, a cloud far from the origin, duplicates above kListCap,
positions outside the bounding box and inside empty cells.  Every comparison is exact unless it names an existing bound:

  grid header      dims / ncells / minv equal to the host restatement of header_kernel, inv_cell to 1 ulp
  patches          n_ball, n_eff, nbr and the patch bits equal to oracle/patches_ref.py (scipy); on the lattice n_ball also equal to an
                   int64 brute force; nesti_patches_count equal; a second grid build gives the same bits
  reference order  patches_ref_kernel equal to refsample.ReferencePatchSampler bit for bit
  plane fit        pca_kernel's counts equal to the same n_ball, sentinel rows zero; tests/test_gpu_pca.py's ``check`` with its bounds
  orientation      orient_knn_kernel's lists, edges and flips equal to tests/_orient_fixture.py's, weights within test_graph_parity's 1e-6
  positions        patches_kernel / pca_kernel at positions equal to tests/_query_positions_fixture.py's scipy restatement
  fused path       patches_mups_kernel -> gate -> experts byte-identical to build -> NestiNet in f32"""
import numpy as np
import pytest
import torch

import _grid_fixture as G
import _orient_fixture as OF
import _pca_fixture as PF
import _query_positions_fixture as QF

pytestmark = pytest.mark.gpu

SEED = 3627473
_host, _gpu = {}, {}


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cloud(name, dev):
    """The case's ``CloudPatches`` over its rows, built once."""
    if ("cp", name) not in _gpu:
        from nesti_net_amd.provider import CloudPatches
        c = G.case(name)
        cp = CloudPatches(c["pts"], c["cfg"], device=dev, seed=SEED, pidx=c["rows"])
        assert cp.r_abs == c["r_abs"] and cp.bbdiag == c["bbdiag"]
        _gpu[("cp", name)] = cp
    return _gpu[("cp", name)]


def _built(name, dev):
    """(points, n_eff, nbr, n_ball) of the case's rows on the GPU, once."""
    if ("built", name) not in _gpu:
        cp = _cloud(name, dev)
        _gpu[("built", name)] = _np(cp.build(0, cp.patch_count, want_idx=True))
    return _gpu[("built", name)]


def _oracle(name):
    """oracle/patches_ref.py on the case's rows, once."""
    if name not in _host:
        from oracle import patches_ref
        c = G.case(name)
        _host[name] = patches_ref.extract_patches(c["pts"], c["rows"], c["r_abs"], c["cfg"].num_point, SEED)
    return _host[name]


def _device_header(cp):
    """``GridHeader`` (csrc/patches_dev.h: double minv[3], double inv_cell, int dims[3], int ncells) from the head of the workspace."""
    torch.cuda.synchronize()
    raw = cp._ws[:48].cpu().numpy()
    f, i = raw[:32].view(np.float64), raw[32:48].view(np.int32)
    return {"minv": f[:3].tolist(), "inv_cell": float(f[3]), "dims": i[:3].tolist(), "ncells": int(i[3])}


@pytest.mark.parametrize("name", G.CASES)
def test_grid_header(name, gpu_device):
    c, want = G.case(name), G.case(name)["header"]
    got = _device_header(_cloud(name, gpu_device))
    print("%s: device dims %s ncells %d cell %.9g (1.0001 r_max = %.9g); host dims %s ncells %d cell %.9g"
          % (name, got["dims"], got["ncells"], 1.0 / got["inv_cell"], 1.0001 * max(c["r_abs"]), want["dims"], want["ncells"], want["cell"]))
    assert got["dims"] == want["dims"] and got["ncells"] == want["ncells"]
    assert got["minv"] == want["minv"]
    assert abs(got["inv_cell"] - want["inv_cell"]) <= np.spacing(want["inv_cell"])
    if name in G.CLAMPED:
        assert 1.0 / got["inv_cell"] > 1.0001 * max(c["r_abs"]) and max(got["dims"]) >= 127      # the device reached the clamp
    else:
        assert 1.0 / got["inv_cell"] == pytest.approx(1.0001 * max(c["r_abs"]), rel=1e-15)


@pytest.mark.parametrize("name", G.CASES)
def test_patches(name, gpu_device):
    c = G.case(name)
    cp = _cloud(name, gpu_device)
    points, n_eff, nbr, n_ball = _built(name, gpu_device)
    o_points, o_n_eff, o_nbr, o_n_ball = _oracle(name)
    P = c["cfg"].num_point
    print("%s: balls per scale min %s mean %s max %s; %d of %d (row, scale) balls above P = %d, %d above kListCap"
          % (name, n_ball.min(0).tolist(), n_ball.mean(0).round(1).tolist(), n_ball.max(0).tolist(), int((n_ball > P).sum()), n_ball.size,
             P, int((n_ball > G.K_LIST_CAP).sum())))
    assert np.array_equal(n_ball, G.ball_sizes(name))          # the lattices: the int64 brute force; elsewhere scipy's count
    assert np.array_equal(n_ball, o_n_ball)
    assert np.array_equal(n_eff, o_n_eff) and np.array_equal(nbr, o_nbr)
    assert np.array_equal(_bits(points), _bits(o_points))
    assert (n_ball > P).any() and (n_ball <= P).any()
    assert np.array_equal(cp.count_balls(0, cp.patch_count).cpu().numpy(), n_ball)
    # another grid build may order the points inside a cell differently: the selection is by key, so the bits stay
    cp.build_grid()
    again = _np(cp.build(0, cp.patch_count, want_idx=True))
    for a, b in zip(again, (points, n_eff, nbr, n_ball)):
        assert np.array_equal(_bits(a), _bits(b))
    if name == "lattice_exact":
        row = int(np.flatnonzero(c["rows"] == G.lattice_index(*G.LATTICE_CENTRE))[0])
        assert n_ball[row].tolist() == [123, 515, 1417]        # 93 / 485 / 1365 with d2 < r^2


@pytest.mark.parametrize("name", ("lattice_exact", "needle_x", "duplicates"))
def test_reference_order(name, gpu_device):
    """As test_reference_order_gpu_equals_the_host_sampler_on_a_dense_cloud, on the boundary, collinear and tied balls."""
    from nesti_net_amd import _lib
    from nesti_net_amd.refsample import ReferencePatchSampler, RefStream
    c = G.case(name)
    cp = _cloud(name, gpu_device)
    P, M = c["cfg"].num_point, cp.patch_count
    sizes = cp.count_balls(0, M).cpu().numpy()
    assert np.array_equal(sizes, G.ball_sizes(name))
    assert sizes.max() <= _lib.load().nesti_patches_ref_max_ball()
    assert (sizes > P).any() and (sizes <= P).any()
    picks, offs = RefStream(SEED).picks(sizes.ravel(), P)
    p, n, nbr = cp.build_reference_order(0, M, torch.from_numpy(picks.view(np.int16).copy()).to(gpu_device),
                                         torch.from_numpy(offs.copy()).to(gpu_device), want_idx=True)
    host = ReferencePatchSampler(SEED)
    hp, hn = host.patches(c["pts"], host.build_tree(c["pts"]), c["rows"].astype(np.int64), c["r_abs"], P)
    assert np.array_equal(n.cpu().numpy(), hn)
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(hp))
    nbr, S = nbr.cpu().numpy(), len(c["r_abs"])
    for q in range(0, M, 7):                                    # members without repetition, -1 beyond n_eff
        for s in range(S):
            sel = nbr[q, s * P:s * P + hn[q, s]]
            assert len(np.unique(sel)) == len(sel) and (sel >= 0).all() and (nbr[q, s * P + hn[q, s]:(s + 1) * P] == -1).all()


def _pca(name, dev):
    if ("pca", name) not in _gpu:
        cp = _cloud(name, dev)
        _gpu[("pca", name)] = _np(cp.pca(0, cp.patch_count))
    return _gpu[("pca", name)]


@pytest.mark.parametrize("name", G.CASES)
def test_plane_fit_counts_and_sentinels(name, gpu_device):
    normals, eig, n_ball = _pca(name, gpu_device)
    want = G.ball_sizes(name)
    assert np.array_equal(n_ball, want) and np.array_equal(n_ball, _built(name, gpu_device)[3])
    live = want >= 3
    assert not _bits(normals[~live]).any() and not _bits(eig[~live]).any()
    assert (normals[live] != 0).any(axis=-1).all() and np.isfinite(normals).all() and np.isfinite(eig).all()
    if name == "plate":
        assert (~live).sum() > 100                              # the sentinel path is taken, interleaved with live rows


@pytest.mark.parametrize("name", ("plate", "offset", "needle_x", "duplicates"))
def test_plane_fit_against_the_restatement(name, gpu_device):
    """tests/test_gpu_pca.py's assertions with its bounds.  On the collinear and the duplicate cloud any row may be ill-conditioned (the
    rule of ``check`` decides); on the plate and the shifted slab none may."""
    from test_gpu_pca import check
    c = G.case(name)
    ref = PF.restate(c["pts"], c["pts"][c["rows"]], c["r_abs"])
    may = np.ones(ref["n_ball"].shape, bool) if name in ("needle_x", "duplicates") else None
    check(_pca(name, gpu_device), ref, name, allow_excluded=may)


@pytest.mark.parametrize("name", ("needle_diag", "plate", "lattice_exact", "duplicates"))
def test_orientation_graph(name, gpu_device):
    """orient_knn_kernel walks a grid of its own over the cloud with cell edge from R = max(r_abs): the same regime as the case's."""
    from test_gpu_orient import lib_graph
    xyz, normals, R, K = G.orient_input(name)
    h = G.header(xyz, [R])
    assert h["clamped"] == (name in G.CLAMPED)
    ref = OF.graph(xyz, normals, R, K)
    got = lib_graph(xyz, normals, R, K, gpu_device)
    assert np.array_equal(got["nbr"], ref["nbr"])
    assert np.array_equal(got["u"], ref["u"]) and np.array_equal(got["v"], ref["v"])
    edges = ref["u"] >= 0
    assert edges.sum() > 1000
    assert np.array_equal(got["flip"][edges], ref["flip"][edges])
    w = got["wbits"].view(np.float32)
    diff = np.abs(w[edges].astype(np.float64) - ref["w"][edges].astype(np.float64))
    print("%s: %d points, grid dims %s, %d edges, %d rows with fewer than K neighbours, %d weights differ in their bits, largest |dw| %.3g"
          % (name, len(xyz), h["dims"], int(edges.sum()), int((ref["nbr"][:, -1] < 0).sum()),
             int((got["wbits"][edges] != ref["wbits"][edges]).sum()), float(diff.max())))
    assert (diff <= 1e-6).all()
    assert not got["wbits"][~edges].any() and not got["flip"][~edges].any()


@pytest.mark.parametrize("name", G.WITH_POSITIONS)
def test_positions_outside_the_box_and_inside_empty_cells(name, gpu_device):
    """In the clamp regime the cell edge is larger than 1.0001 r_max, not equal to it: the argument above cell_axis (a centre one cell
    outside has its ball inside the border cell's block) is used with slack.  The scipy restatement of test_patches_against_scipy."""
    from nesti_net_amd.provider import CloudPatches
    c = G.case(name)
    pos, n_out, P = c["positions"], c["n_outside"], c["cfg"].num_point
    o_pts, o_neff, o_nbr, o_ball = QF.extract_at(c["pts"], pos, c["r_abs"], P, SEED)
    cp = CloudPatches(c["pts"], c["cfg"], device=gpu_device, seed=SEED, queries=pos)
    assert cp.r_abs == c["r_abs"]
    p, n_eff, nbr, n_ball = _np(cp.build(0, len(pos), want_idx=True))
    print("%s: %d positions outside the box, %d of them with a non-empty ball; %d inside empty cells, %d of them with a non-empty ball; "
          "largest ball %d" % (name, n_out, int((o_ball[:n_out].sum(1) > 0).sum()), len(pos) - n_out,
                               int((o_ball[n_out:].sum(1) > 0).sum()), int(o_ball.max())))
    assert np.array_equal(n_ball, o_ball) and np.array_equal(n_eff, o_neff) and np.array_equal(nbr, o_nbr)
    assert np.array_equal(_bits(p), _bits(o_pts))
    assert (o_ball[:n_out, -1] > 0).sum() >= 50 and (o_ball[:n_out, -1] == 0).sum() >= 50      # tests/test_grid_fixture.py
    normals, eig, counts = _np(cp.pca(0, len(pos)))
    assert np.array_equal(counts, o_ball)
    assert not _bits(normals[o_ball < 3]).any() and not _bits(eig[o_ball < 3]).any()


@pytest.fixture(scope="module")
def synthetic():
    from nesti_net_amd import weights
    from nesti_net_amd.config import NestiConfig
    return weights.synthetic_weights(NestiConfig())             # the variables do not depend on the radii or on num_point


@pytest.mark.parametrize("name", ("needle_diag", "lattice_exact"))
def test_fused_path(name, synthetic, gpu_device):
    """patches_mups_kernel (its own copy of the walk) -> gate -> experts equals CloudPatches.build -> NestiNet byte for byte in f32, as in
    test_fused_entry_matches_the_two_call_path; 200 rows in ragged batches of 64."""
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.pipeline import NormalEstimator
    from nesti_net_amd.provider import CloudPatches
    c = G.case(name)
    q = c["rows"][:200]
    if name == "lattice_exact":
        assert G.lattice_index(*G.LATTICE_CENTRE) in q
    cp = CloudPatches(c["pts"], c["cfg"], device=gpu_device, seed=SEED, pidx=q)
    p_all, n_all = cp.build(0, len(q))
    assert np.array_equal(n_all.cpu().numpy(), np.minimum(G.ball_sizes(name)[:200], c["cfg"].num_point))
    net = NestiNet(c["cfg"], synthetic, dtype="f32", device=gpu_device, max_batch=len(q))
    ref = _np(net(p_all, n_all))
    del net
    est = NormalEstimator(c["cfg"], synthetic, dtype="f32", device=gpu_device, batch=64, seed=SEED)      # 64 + 64 + 64 + 8
    assert est._fused
    got = est.estimate(c["pts"], pidx=q)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
    for x, y in zip(got, ref):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))
    del est
    torch.cuda.empty_cache()
