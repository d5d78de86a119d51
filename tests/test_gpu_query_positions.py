"""Position queries on real kernels: normals at arbitrary positions (``CloudPatches(..., queries=)``, the ``nesti_*_at`` entries),
against the tests' own scipy restatement (tests/_query_positions_fixture.py), against the unfused path, across partitions in the
reproducible mode, against the fp64 oracle, on the 3^3 grid, on two ranks and through the command line.

Conventions under test: a scale whose ball is empty has n_eff = 0 and contributes zero MuPS channels; a query
whose balls are empty at every scale comes back as normal (0, 0, 0), expert -1, probabilities 0; the subsample key is the patch
row, not the position."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _query_positions_fixture as F
from conftest import REPO

pytestmark = pytest.mark.gpu

SEED = 3627473
TAU = 0.02          # as tests/test_gpu_reproducible.py: far below the f16 filter's error on a logit difference
WORKER = os.path.join(REPO, "tests", "_dist_positions_worker.py")


def _np(ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits_equal(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def fx(gpu_device):
    """Cloud, the two query sets and their scipy patches -- computed once, shared, never changed -- plus weights whose gate is
    calibrated on index queries of the cloud to route to every expert."""
    from nesti_net_amd import weights
    from nesti_net_amd.calibrate import calibrate_gate
    from nesti_net_amd.provider import CloudPatches
    f = F.make()
    for name in ("jittered", "faces"):
        f["ref_" + name] = F.extract_at(f["pts"], f[name], f["r_abs"], F.P, SEED)
        f["cls_" + name] = F.classes(f["ref_" + name][3])
    cp = CloudPatches(f["pts"], f["cfg"], device=gpu_device, pidx=np.arange(7, 20000, 39)[:512])
    sp, sn = cp.build(0, 512)
    f["W"] = calibrate_gate(f["cfg"], weights.synthetic_weights(f["cfg"]), sp, sn, device=gpu_device)
    return f


def _estimate_at(est, cloud, want_n_ball=True):
    """``nesti_estimate_normals_at`` itself, on the estimator's arena: (normals, expert, probs, n_ball)."""
    from nesti_net_amd import _lib
    M, E, S = cloud.patch_count, max(1, est.cfg.n_gate_out), est.cfg.n_scales
    dev = est.device
    normals = torch.empty((M, 3), dtype=torch.float32, device=dev)
    expert = torch.empty((M,), dtype=torch.int32, device=dev)
    probs = torch.empty((M, E), dtype=torch.float32, device=dev)
    n_ball = torch.full((M, S), -7, dtype=torch.int32, device=dev) if want_n_ball else None
    _lib.check(est.net.lib.nesti_estimate_normals_at(
        est.net._handle, _lib.ptr(cloud.cloud), cloud.n_points, _lib.ptr(cloud.queries), M, cloud._r, ctypes.c_uint64(cloud.seed), 0,
        est.batch, 0, _lib.ptr(cloud._ws), cloud._ws.numel(), _lib.ptr(est._arena), est._arena.numel(), _lib.ptr(normals),
        _lib.ptr(expert), _lib.ptr(probs), _lib.ptr(n_ball), _lib.stream_ptr(torch.cuda.current_stream(dev))), "nesti_estimate_normals_at")
    return normals, expert, probs, n_ball


def _unfused(net, cloud, with_gate=True):
    """build -> forward -> nesti_mask_empty_queries: (normals, expert, probs, n_eff)."""
    from nesti_net_amd import _lib
    M = cloud.patch_count
    p, n = cloud.build(0, M)
    normals, expert, probs = net.forward(p, n)
    _lib.check(net.lib.nesti_mask_empty_queries(_lib.ptr(n), M, net.cfg.n_scales, _lib.ptr(normals), _lib.ptr(expert) if with_gate else None,
                                                _lib.ptr(probs) if with_gate else None, probs.shape[1] if with_gate else 0,
                                                _lib.stream_ptr(torch.cuda.current_stream(net.device))), "nesti_mask_empty_queries")
    return normals, expert, probs, n


@pytest.fixture(scope="module")
def frozen(fx, gpu_device):
    """Three reproducible f16x8c estimators that batch differently (one call; two streams of 192-row batches; a captured graph of 256
    rows), thresholds set as tests/test_gpu_reproducible.py sets them: tau = 0.02, thr = the 9th smallest non-sentinel |n| of the
    jittered set measured with the guard off."""
    from nesti_net_amd.pipeline import NormalEstimator
    kws = ({"batch": 512}, {"batch": 192, "n_streams": 2}, {"batch": 256, "use_graph": True})
    ests = [NormalEstimator(fx["cfg"], fx["W"], dtype="f16x8c", device=gpu_device, gate_margin=TAU, reproducible=True, **kw) for kw in kws]
    a = ests[0]
    cloud = a.prepare(fx["pts"], queries=fx["jittered"])
    a.net.set_x8_guard(-1.0)
    norms = np.linalg.norm(_np(a.run(cloud))[0], axis=1)
    thr = float(np.sort(norms[norms > 0])[8])
    for e in ests:
        e.net.set_x8_guard(thr)
        e.net.reproducible_stats(reset=True)
    return ests, cloud


def test_identity_positions_equal_to_cloud_points(fx, frozen, gpu_device):
    """queries = pts[pidx] gives the bits pidx gives: the four patch outputs, and normals / expert / probs in reproducible f16x8c."""
    from nesti_net_amd.provider import CloudPatches
    pidx = np.arange(5, 20000, 40)[:500]
    by_idx = CloudPatches(fx["pts"], fx["cfg"], device=gpu_device, pidx=pidx)
    by_pos = CloudPatches(fx["pts"], fx["cfg"], device=gpu_device, queries=fx["pts"][pidx])
    assert by_pos.patch_count == 500 and by_pos.r_abs == by_idx.r_abs
    a, b = _np(by_idx.build(0, 500, want_idx=True)), _np(by_pos.build(0, 500, want_idx=True))
    assert _bits_equal(a, b)
    assert (a[3] >= 1).all() and (a[3][:, -1] > F.P).any()          # a cloud point is in its own balls; the subsample is exercised
    est = frozen[0][0]
    assert _bits_equal(_np(est.run(by_idx)), _np(est.run(by_pos)))
    # a sub-range keeps the row key
    lo = _np(by_pos.build(123, 77, want_idx=True))
    assert _bits_equal(lo, [x[123:200] for x in b])


@pytest.mark.parametrize("name", ["jittered", "faces"])
def test_patches_against_scipy(fx, gpu_device, name):
    from nesti_net_amd.provider import CloudPatches
    o_pts, o_neff, o_nbr, o_ball = fx["ref_" + name]
    cls = fx["cls_" + name]
    print(name, {k: int(v.sum()) for k, v in cls.items()})
    for k, v in cls.items():
        assert v.any(), "class %s is not populated in the %s set" % (k, name)
    cp = CloudPatches(fx["pts"], fx["cfg"], device=gpu_device, queries=fx[name])
    assert cp.r_abs == fx["r_abs"]                                  # from the CLOUD's bounding box, not the queries'
    p, n_eff, nbr, n_ball = _np(cp.build(0, cp.patch_count, want_idx=True))
    assert np.array_equal(n_ball, o_ball) and np.array_equal(n_eff, o_neff) and np.array_equal(nbr, o_nbr)
    assert np.array_equal(_bits(p), _bits(o_pts))
    if name == "faces":
        lo, hi = fx["pts"].min(0), fx["pts"].max(0)
        outside = ((fx[name] < lo) | (fx[name] > hi)).any(axis=1)
        assert outside.all() and (n_ball[outside].sum(axis=1) > 0).any()     # centres outside the grid's box still find their balls


def _lost_positions(fx, device):
    """Rows 0 and 9: two cloud points.  Rows 1 .. 8: +inf, NaN, a position 1e6 bounding-box diagonals away, mixed non-finite, and
    positions with ONE non-finite coordinate whose other two are a cloud point's (they clamp to a cell block that holds points)."""
    far, inf, nan = 1e6 * fx["bbdiag"], float("inf"), float("nan")
    a, b = (float(v) for v in fx["pts"][1234]), (float(v) for v in fx["pts"][4321])
    a, b = list(a), list(b)
    rows = [a, [inf, 0.0, 0.0], [nan] * 3, [far, -far, far], [0.0, -inf, nan], [nan, a[1], a[2]], [a[0], nan, a[2]], [a[0], a[1], -nan],
            [b[0], inf, b[2]], b]
    lost = np.array([False] + [True] * 8 + [False])
    return torch.tensor(rows, dtype=torch.float32, device=device), lost


def test_far_and_non_finite_positions_have_empty_balls(fx, gpu_device):
    """Through a device tensor (the host check refuses them): a defined cell or none, then an empty ball at every scale, on the
    parity kernel, on the fused kernel (built with -fno-honor-nans: nothing may depend on how a NaN compares) and through
    run_many; the calls return normally, the rows carry the sentinel and the cloud points next to them are served."""
    from nesti_net_amd.pipeline import NormalEstimator
    from nesti_net_amd.provider import CloudPatches
    q, lost = _lost_positions(fx, gpu_device)
    cp = CloudPatches(fx["pts"], fx["cfg"], device=gpu_device, queries=q)
    p, n_eff, nbr, n_ball = _np(cp.build(0, len(q), want_idx=True))
    assert not n_ball[lost].any() and not n_eff[lost].any() and (nbr[lost] == -1).all() and not _bits(p[lost]).any()
    assert (n_ball[~lost] >= 1).all()
    est = NormalEstimator(fx["cfg"], fx["W"], dtype="f16x3", device=gpu_device, batch=4)       # three library batches
    normals, expert, probs, fused_ball = _np(_estimate_at(est, cp))
    assert np.array_equal(fused_ball, n_ball)
    assert not _bits(normals[lost]).any() and (expert[lost] == -1).all() and not _bits(probs[lost]).any()
    assert (expert[~lost] >= 0).all() and np.isfinite(normals).all() and (np.linalg.norm(normals[~lost], axis=1) > 0).all()
    many = est.run_many([(cp, 0, 3), (cp, 3, 7)])
    joined = [np.concatenate([x, y]) for x, y in zip(_np(many[0]), _np(many[1]))]
    assert _bits_equal(joined, [normals, expert, probs])


def test_run_many_refuses_a_mix_of_query_kinds(fx, gpu_device):
    from nesti_net_amd.pipeline import NormalEstimator
    est = NormalEstimator(fx["cfg"], fx["W"], dtype="f16", device=gpu_device, batch=16)
    by_pos = est.prepare(fx["pts"], queries=fx["jittered"][:8])
    by_idx = est.prepare(fx["pts"], pidx=np.arange(8))
    with pytest.raises(ValueError, match="cannot share one call"):
        est.run_many([(by_pos, 0, 8), (by_idx, 0, 8)])


@pytest.fixture(scope="module")
def f32_runs(fx, gpu_device):
    """The jittered set in f32 through the fused entry and through the unfused path -- shared by the next tests."""
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.pipeline import NormalEstimator
    out = {}
    for dtype in ("f32", "f16x3"):
        est = NormalEstimator(fx["cfg"], fx["W"], dtype=dtype, device=gpu_device, batch=192)      # 500 rows: three library batches
        cloud = est.prepare(fx["pts"], queries=fx["jittered"])
        fused = _np(_estimate_at(est, cloud))
        run = _np(est.run(cloud))
        net = NestiNet(fx["cfg"], fx["W"], dtype=dtype, device=gpu_device, max_batch=500)
        out[dtype] = {"fused": fused, "run": run, "unfused": _np(_unfused(net, cloud))}
        del est, net
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_fused_equals_unfused(fx, f32_runs, dtype):
    r = f32_runs[dtype]
    assert _bits_equal(r["fused"][:3], r["unfused"][:3])
    assert _bits_equal(r["run"], r["fused"][:3])
    assert np.array_equal(r["fused"][3], fx["ref_jittered"][3])                # the fused entry's uncapped ball sizes
    assert np.array_equal(r["unfused"][3], fx["ref_jittered"][1])


def test_sentinel_rows(fx, f32_runs, gpu_device):
    """Exactly the rows whose n_eff is 0 at every scale carry (0,0,0) / -1 / 0; nobody else does.  ss_norm_est: normals only."""
    from nesti_net_amd import weights
    from nesti_net_amd.config import ARCH_SINGLE, NestiConfig
    from nesti_net_amd.pipeline import NormalEstimator
    empty = fx["cls_jittered"]["all_empty"]
    assert 0 < empty.sum() < len(empty)
    for dtype in ("f32", "f16x3"):
        normals, expert, probs = f32_runs[dtype]["fused"][:3]
        assert not _bits(normals[empty]).any() and (expert[empty] == -1).all() and not _bits(probs[empty]).any()
        assert (expert[~empty] >= 0).all() and (np.linalg.norm(normals[~empty], axis=1) > 0).all()
        assert np.allclose(probs[~empty].sum(axis=1), 1.0, atol=1e-5) and np.isfinite(normals).all()
    # single tower (expert and probs NULL), fused, on the face set: a single scale, so 'partly empty' does not exist
    cfg1 = NestiConfig(patch_radius=[0.05], num_point=F.P, n_experts=1, expert_dict={0: [0]}, arch=ARCH_SINGLE)
    q = fx["faces"][::3]
    ball = fx["ref_faces"][3][::3, 2]
    assert (ball == 0).any() and (ball > 0).any()
    est = NormalEstimator(cfg1, weights.synthetic_weights(cfg1), dtype="f16x3", device=gpu_device, batch=128)
    normals, expert, probs = est.estimate(fx["pts"], queries=q)
    assert expert is None and probs is None and np.isfinite(normals).all()
    assert np.array_equal((normals == 0).all(axis=1), ball == 0)


def test_partitions_agree_bit_for_bit(fx, frozen):
    """Reproducible f16x8c: one call, 2 streams x 192-row batches, run_many over two items, and a captured graph at batch 256."""
    ests, cloud = frozen
    a = ests[0]
    whole = _np(a.run(cloud))
    empty = fx["cls_jittered"]["all_empty"]
    assert np.array_equal(whole[1] == -1, empty) and len(np.unique(whole[1][~empty])) >= 5
    many = a.run_many([(cloud, 0, 230), (cloud, 230, 270)])
    joined = [np.concatenate([x, y]) for x, y in zip(_np(many[0]), _np(many[1]))]
    assert _bits_equal(joined, whole), "run_many 230 / 270"
    halves = [np.concatenate([x, y]) for x, y in zip(_np(a.run(cloud, 0, 301)), _np(a.run(cloud, 301, 199)))]
    assert _bits_equal(halves, whole), "two calls"
    for e, name in zip(ests[1:], ("batch 192 on two streams", "batch 256, captured graph")):
        assert _bits_equal(_np(e.run(cloud)), whole), name
    many2 = ests[1].run_many([(cloud, 0, 230), (cloud, 230, 270)])
    joined2 = [np.concatenate([x, y]) for x, y in zip(_np(many2[0]), _np(many2[1]))]
    assert _bits_equal(joined2, whole), "run_many on two streams"
    assert _bits_equal(_np(a.run_verified(cloud)), _np(ests[2].run_verified(cloud))), "run_verified"


def test_reference_order_is_refused_for_positions(fx, gpu_device):
    from nesti_net_amd import _lib
    from nesti_net_amd.pipeline import NormalEstimator
    est = NormalEstimator(fx["cfg"], fx["W"], dtype="f16", device=gpu_device, batch=64, subsample="reference")
    cloud = est.prepare(fx["pts"], queries=fx["jittered"][:8])
    with pytest.raises(_lib.NestiError, match="index queries only"):
        est.run(cloud)
    with pytest.raises(_lib.NestiError, match="index queries only"):
        cloud.count_balls(0, 8)


def test_f32_against_the_fp64_oracle(fx, gpu_device):
    """96 jittered rows, partly-empty and over-P rows among them, gate calibrated on them; the oracle's channels of an empty scale
    are zero (the documented convention; the reference divides by zero there).  Rules of tests/test_gpu_fixtures.py; at most one
    row may be excused as a tie."""
    from nesti_net_amd import parity, weights
    from nesti_net_amd.calibrate import calibrate_gate
    from nesti_net_amd.pipeline import NormalEstimator
    from nesti_net_amd.provider import CloudPatches
    from oracle import mups_ref, net_ref
    cfg = fx["cfg"]
    sel = np.arange(0, 480, 5)
    q = fx["jittered"][sel]
    o_pts, o_neff, _, o_ball = F.extract_at(fx["pts"], q, fx["r_abs"], F.P, SEED)
    cls = F.classes(o_ball)
    print({k: int(v.sum()) for k, v in cls.items()})
    assert len(q) == 96 and cls["partly_empty"].any() and cls["over_P"].any()
    cp = CloudPatches(fx["pts"], cfg, device=gpu_device, queries=q)
    p_d, n_d = cp.build(0, 96)
    assert np.array_equal(_bits(p_d.cpu().numpy()), _bits(o_pts))
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), p_d, n_d, device=gpu_device)
    normals, expert, probs = NormalEstimator(cfg, W, dtype="f32", device=gpu_device, batch=64).estimate(fx["pts"], queries=q)
    # ---- oracle: fp64 MuPS with the channels of an empty scale set to zero, then the fp64 network ------------------------------
    mups = mups_ref.mups_assemble(o_pts, np.maximum(o_neff, 1), cfg.n_scales)
    for s in range(cfg.n_scales):
        mups[o_neff[:, s] == 0, ..., 20 * s:20 * (s + 1)] = 0.0
    assert np.isfinite(mups).all()
    keep = ~cls["all_empty"]
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    outs = net_ref.over_chunks(lambda sl: net_ref.moe_forward(mups[keep][sl], W, expert_dict=cfg.expert_dict, dtype=torch.float64, top1_only=True),
                               int(keep.sum()))
    ref = {k: torch.cat([o[k] for o in outs]).numpy() for k in ("probs", "expert", "normals")}
    # all-empty rows: the sentinel
    assert not _bits(normals[~keep]).any() and (expert[~keep] == -1).all() and not _bits(probs[~keep]).any()
    ex, pr, nr = expert[keep], probs[keep], normals[keep].astype(np.float64)
    srt = np.sort(ref["probs"], axis=1)
    margin = srt[:, -1] - srt[:, -2]
    agree = ex == ref["expert"]
    perr = np.abs(pr - ref["probs"]).max()
    cos = (nr[agree] * ref["normals"][agree]).sum(1) / (np.linalg.norm(nr[agree], axis=1) * np.linalg.norm(ref["normals"][agree], axis=1))
    print("rows", int(keep.sum()), "routing", np.bincount(ex, minlength=cfg.n_experts), "prob err", perr, "flips", int((~agree).sum()),
          "min margin", margin.min(), "1-cos max", (1 - cos).max())
    assert len(np.unique(ex)) >= 5
    assert perr <= parity.F32_PROB_ERR_BOUND
    assert np.all(agree | (margin < parity.TIE_MARGIN))
    assert int((~agree).sum()) <= 1
    assert np.all(1 - cos <= 1e-5)


def test_3_gaussian_grid_equals_the_unfused_path(fx, gpu_device):
    from nesti_net_amd import weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.pipeline import NormalEstimator
    cfg3 = NestiConfig(num_point=F.P, n_gaussians=3)
    W3 = weights.synthetic_weights(cfg3)
    q = fx["jittered"][:64]
    cls = {k: v[:64] for k, v in fx["cls_jittered"].items()}
    assert cls["partly_empty"].any() and cls["over_P"].any()
    est = NormalEstimator(cfg3, W3, dtype="f32", device=gpu_device, batch=24)          # 64 rows: three library batches
    cloud = est.prepare(fx["pts"], queries=q)
    fused = _np(_estimate_at(est, cloud))
    net = NestiNet(cfg3, W3, dtype="f32", device=gpu_device, max_batch=64)
    unf = _np(_unfused(net, cloud))
    assert _bits_equal(fused[:3], unf[:3]) and _bits_equal(_np(est.run(cloud)), fused[:3])
    assert np.array_equal(fused[3], fx["ref_jittered"][3][:64])
    assert np.array_equal(fused[1] == -1, cls["all_empty"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_world(out, world):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        if world == 1:
            for k in ("RANK", "WORLD_SIZE", "MASTER_PORT"):
                env.pop(k)
        procs.append(subprocess.Popen([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        o, _ = p.communicate(timeout=600)
        assert p.returncode == 0, o.decode()[-3000:]


def test_two_ranks_equal_one_rank(fx, tmp_path, gpu_device):
    """Position queries sharded by row over two ranks on one GPU (a fresh child process per rank), reproducible f16x8c: both ranks
    hold the one-process result bit for bit, sentinel rows included."""
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    _run_world(one, 1)
    _run_world(two, 2)
    ref = np.load(one + ".rank0.npz")
    empty = fx["cls_jittered"]["all_empty"]
    assert ref["normals"].shape == (500, 3) and np.array_equal(ref["expert"] == -1, empty)
    assert len(np.unique(ref["expert"][~empty])) >= 5
    for r in range(2):
        got = np.load(two + ".rank%d.npz" % r)
        for k in ("normals", "expert", "probs"):
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), "rank %d %s" % (r, k)
        assert got["passes"] == ref["passes"] and got["tau"] == ref["tau"] and got["thr"] == ref["thr"]


def test_command_line_with_query_positions(fx, tmp_path, gpu_device):
    """Two small shapes with .qxyz files: M rows per output file, byte-identical at two library batch sizes with --reproducible 1,
    sentinel rows written as they are, and the log counts them."""
    from nesti_net_amd import synth
    from nesti_net_amd.cli import main
    d = tmp_path / "pcp"
    d.mkdir()
    M, expect_empty = {}, {}
    for name, shape, seed in (("shapeA", "ellipsoid", 50), ("shapeB", "torus", 51)):
        pts, _ = synth.make_cloud(shape, n=3000, seed=seed)
        np.savetxt(str(d / (name + ".xyz")), pts, fmt="%.9g")
        pts = np.loadtxt(str(d / (name + ".xyz"))).astype(np.float32)
        bbdiag = float(np.linalg.norm(pts.max(0) - pts.min(0), 2))
        q = pts[::9] + np.random.RandomState(seed).normal(0, 0.02 * bbdiag, size=pts[::9].shape)
        q = np.concatenate([q, pts.max(0)[None] + bbdiag]).astype(np.float32)          # the last one is certainly alone
        np.savetxt(str(d / (name + ".qxyz")), q, fmt="%.9g")
        q = np.loadtxt(str(d / (name + ".qxyz"))).astype(np.float32)
        M[name] = len(q)
        ball = F.extract_at(pts, q, [bbdiag * r for r in (0.01, 0.03, 0.05)], 512, SEED)[3]
        expect_empty[name] = (ball == 0).all(axis=1)
        assert expect_empty[name][-1] and not expect_empty[name].all()
    (d / "testset.txt").write_text("shapeA\nshapeB\n")
    files = []
    for lib_batch in (256, 448):
        results = str(tmp_path / ("log%d" % lib_batch)) + os.sep
        assert main(["--results_path", results, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt",
                     "--synthetic_weights", "--reproducible", "1", "--query_positions", "1", "--lib_batch", str(lib_batch)]) == 0
        out = os.path.join(results, "synth_results")
        files.append({(n, ext): open(os.path.join(out, n + ext), "rb").read() for n in M for ext in (".normals", ".experts", ".experts_probs")})
        log = open(os.path.join(out, "log.txt")).read()
        print(log)
        for n in M:
            assert "query positions of %s: %d, of which %d had no neighbourhood" % (n, M[n], int(expect_empty[n].sum())) in log
    assert files[0] == files[1]
    for n in M:
        normals = np.loadtxt(os.path.join(out, n + ".normals")).reshape(-1, 3)
        experts = np.loadtxt(os.path.join(out, n + ".experts")).reshape(-1)
        probs = np.loadtxt(os.path.join(out, n + ".experts_probs")).reshape(len(experts), -1)
        assert len(normals) == len(experts) == len(probs) == M[n]
        e = expect_empty[n]
        assert np.array_equal(experts == -1, e) and not normals[e].any() and not probs[e].any()
        assert (np.linalg.norm(normals[~e], axis=1) > 0).all()
