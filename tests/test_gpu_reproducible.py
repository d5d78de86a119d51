"""Reproducible mode (nesti_model_set_reproducible, NormalEstimator(..., reproducible=True), --reproducible 1) on real kernels:
with the gate margin and the conditioning guard's threshold frozen, a query's three outputs are a function of the weights, the
thresholds, the cloud, the seed and its patch row -- not of the batch, the stream, a captured graph or the calls before; what the
default mode would have acted on is counted; run_verified turns the counts into the default mode's 1.5 x guarantee by running the
whole range again with wider thresholds."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

Q = 1536
TAU = 0.02          # far below the f16 filter's error on a logit difference (~0.1 on this cloud): the default mode would widen
WORKER = os.path.join(REPO, "tests", "_dist_repro_worker.py")


def _f32(v):
    return float(np.float32(v))


def _np(triple):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in triple]


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def case(gpu_device):
    """The cloud, 1536 strided queries, a gate calibrated to route to every expert, and -- computed once, shared, never changed --
    the f16x3 results of those queries and the FILTER pass's top-2 logit margin (from a tau = 0 pass, as tests/test_gpu_cascade.py
    derives it: softmax is shift-invariant)."""
    from nesti_net_amd import synth, weights
    from nesti_net_amd.calibrate import calibrate_gate
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.pipeline import NormalEstimator
    from nesti_net_amd.provider import CloudPatches
    cfg = NestiConfig()
    pts = synth.make_cloud("ellipsoid", n=20000, seed=1234)[0]
    q = np.arange(3, 20000, 20000 // Q)[:Q]
    assert len(q) == Q
    cp = CloudPatches(pts, cfg, device=gpu_device, pidx=q)
    sp, sn = cp.build(0, 512)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), sp, sn, device=gpu_device)
    del cp, sp, sn
    x3 = NormalEstimator(cfg, W, dtype="f16x3", device=gpu_device, batch=Q)
    ref = x3.estimate(pts, pidx=q)
    fl = NormalEstimator(cfg, W, dtype="f16x3c", device=gpu_device, batch=Q, gate_margin=0.0)
    pfl = fl.estimate(pts, pidx=q)[2]
    srt = np.sort(np.log(pfl.astype(np.float64)), axis=1)
    margin16 = srt[:, -1] - srt[:, -2]
    del x3, fl
    torch.cuda.empty_cache()
    return {"cfg": cfg, "W": W, "pts": pts, "q": q, "ref": ref, "margin16": margin16}


@pytest.fixture(scope="module")
def trio(case, gpu_device):
    """Three f16x8c estimators (default x8 format) that batch differently: one call per run; two streams of 384-row batches; a
    captured hipGraph of 512 rows.  tau = 0.02; thr = the 9th smallest |n| of the 1536 outputs, measured with the guard off."""
    from nesti_net_amd.pipeline import NormalEstimator
    kws = ({"batch": Q}, {"batch": 384, "n_streams": 2}, {"batch": 512, "use_graph": True})
    ests = [NormalEstimator(case["cfg"], case["W"], dtype="f16x8c", device=gpu_device, gate_margin=TAU, reproducible=True, **kw)
            for kw in kws]
    a = ests[0]
    cloud = a.prepare(case["pts"], pidx=case["q"])
    a.net.set_x8_guard(-1.0)
    norms = np.linalg.norm(_np(a.run(cloud))[0], axis=1)
    thr = float(np.sort(norms)[8])
    for e in ests:
        e.net.set_x8_guard(thr)
        e.net.reproducible_stats(reset=True)
    return ests, cloud, thr


def _partitions(est, cloud):
    """The same 1536 rows, cut four ways."""
    outs = {"whole": _np(est.run(cloud))}
    lo, hi = _np(est.run(cloud, 0, 500)), _np(est.run(cloud, 500, Q - 500))
    outs["two calls"] = [np.concatenate([x, y]) for x, y in zip(lo, hi)]
    hi, lo = _np(est.run(cloud, 500, Q - 500)), _np(est.run(cloud, 0, 500))
    outs["two calls, reversed"] = [np.concatenate([x, y]) for x, y in zip(lo, hi)]
    many = est.run_many([(cloud, 0, 700), (cloud, 700, Q - 700)])
    outs["run_many 700 / 836"] = [np.concatenate([x, y]) for x, y in zip(_np(many[0]), _np(many[1]))]
    return outs


def test_frozen_means_frozen(case, gpu_device):
    """f16x3c at tau = 0.02: nothing widens, the violations are counted, and the rows decided by the f16x3 gate are EXACTLY the rows
    whose filter margin is below tau -- in the first run and in the second, whatever the first one measured."""
    from nesti_net_amd.pipeline import NormalEstimator
    est = NormalEstimator(case["cfg"], case["W"], dtype="f16x3c", device=gpu_device, batch=Q, gate_margin=TAU, reproducible=True)
    cloud = est.prepare(case["pts"], pidx=case["q"])
    first = _np(est.run(cloud))
    cs, rs = est.net.cascade_stats(), est.net.reproducible_stats()
    print("cascade", cs, "reproducible", rs)
    assert cs["widened"] == 0 and cs["widen_events"] == 0 and cs["tau_eff"] == cs["tau"] == _f32(TAU)
    assert rs["on"] and rs["gate_violations"] > 0 and rs["max_margin_err"] > TAU / 1.5 and rs["tau"] == _f32(TAU)
    assert rs["max_margin_err"] == cs["max_margin_err"] and rs["thr"] == -1.0 and rs["guard_violations"] == 0
    decided_twice = (first[2].view(np.uint32) == case["ref"][2].view(np.uint32)).all(axis=1)
    m = case["margin16"]
    clear = np.abs(m - TAU) > 1e-4
    assert np.array_equal(decided_twice[clear], (m < TAU)[clear])
    assert cs["rechecked"] == int(decided_twice.sum()) and 0 < cs["rechecked"] < Q
    second = _np(est.run(cloud))
    assert _bits_equal(first, second)
    cs2 = est.net.cascade_stats()
    assert cs2["tau_eff"] == _f32(TAU) and cs2["widened"] == 0 and cs2["rechecked"] == 2 * cs["rechecked"]


def test_partition_independence(case, trio, gpu_device):
    """f16x8c with both thresholds inside the measured errors' reach: one call, two calls in either order, run_many, two streams of
    small batches and a captured graph write the same bits."""
    from nesti_net_amd import _lib
    ests, cloud, thr = trio
    a = ests[0]
    a.net.reproducible_stats(reset=True)
    outs = _partitions(a, cloud)
    for name, o in outs.items():
        assert _bits_equal(o, outs["whole"]), name
    for e, name in zip(ests[1:], ("batch 384 on two streams", "batch 512, captured graph")):
        assert _bits_equal(_np(e.run(cloud)), outs["whole"]), name
    # the violation counter agrees with the maximum it is derived from
    a.net.reproducible_stats(reset=True)
    a.run(cloud)
    rs, gs = a.net.reproducible_stats(), a.net.x8_guard_stats()
    print("reproducible", rs, "guard", gs)
    scale = np.float32(_lib.X8_GUARD_WIDEN) / np.sqrt(np.float32(2.0) * np.float32(_lib.X8_GUARD_BAR))
    assert (rs["guard_violations"] > 0) == bool(scale * np.float32(rs["max_dn"]) > np.float32(thr))
    assert rs["guard_violations"] <= gs["rechecked"] and gs["dropped"] == 0 and gs["queries"] == Q
    assert gs["rechecked"] in (8, 9) and gs["thr_eff"] == gs["thr"] == _f32(thr)      # |n| < thr: the 8 smallest (9 if sqrtf rounds the 9th down)
    assert (rs["gate_violations"] > 0) == (np.float32(1.5) * np.float32(rs["max_margin_err"]) > np.float32(TAU))
    # the default mode on the same partitions: reported, not asserted (it depends on where the largest error falls)
    a.net.set_reproducible(False)
    try:
        a.net.reproducible_stats(reset=True)
        whole = _np(a.run(cloud))
        a.net.reproducible_stats(reset=True)
        lo, hi = _np(a.run(cloud, 0, 500)), _np(a.run(cloud, 500, Q - 500))
        split = [np.concatenate([x, y]) for x, y in zip(lo, hi)]
        rows = np.zeros(Q, bool)
        for x, y in zip(whole, split):
            rows |= (x.reshape(Q, -1).view(np.uint32) != y.reshape(Q, -1).view(np.uint32)).any(axis=1)
        print("default mode, one call vs two calls: %d of %d rows differ in some bit" % (int(rows.sum()), Q))
    finally:
        a.net.set_reproducible(True)
        a.net.reproducible_stats(reset=True)


def test_run_verified(case, trio, gpu_device):
    """From tau = 0.02 the first pass violates; run_verified raises the thresholds from the measured maxima and runs the whole range
    again until nothing violates: the default mode's guarantee, as a function of (model, thresholds, cloud, query set)."""
    ests, cloud, thr = trio
    outs = []
    for e in ests:
        e.last_verified = None
        outs.append(_np(e.run_verified(cloud)))
    a, lv = ests[0], ests[0].last_verified
    rs = a.net.reproducible_stats()
    print("last_verified", lv, "final stats", rs)
    assert 2 <= lv["passes"] <= 4 and lv["tau"] > TAU and lv["thr"] >= _f32(thr)
    assert rs["gate_violations"] == 0 and rs["guard_violations"] == 0 and rs["guard_dropped"] == 0
    assert lv["max_margin_err"] == rs["max_margin_err"] and lv["max_dn"] == rs["max_dn"]
    assert np.float32(1.5) * np.float32(lv["max_margin_err"]) <= np.float32(lv["tau"])
    normals, expert, probs = outs[0]
    assert np.array_equal(expert, case["ref"][1])
    below = case["margin16"] < lv["tau"] - 1e-4
    assert below.sum() > 0 and np.array_equal(probs[below].view(np.uint32), case["ref"][2][below].view(np.uint32))
    # the calibrated thresholds are back in place
    assert a.net.cascade_stats()["tau"] == _f32(TAU) and a.net.x8_guard_stats()["thr"] == _f32(thr)
    for e, o in zip(ests[1:], outs[1:]):
        assert _bits_equal(o, outs[0]) and e.last_verified == lv
        assert e.net.cascade_stats()["tau"] == _f32(TAU) and e.net.x8_guard_stats()["thr"] == _f32(thr)
    # and it refuses what it cannot verify
    a.reproducible = False
    try:
        with pytest.raises(ValueError, match="reproducible=True"):
            a.run_verified(cloud)
    finally:
        a.reproducible = True


def test_command_line_files_do_not_depend_on_the_library_batch(tmp_path, gpu_device):
    from nesti_net_amd import synth
    from nesti_net_amd.cli import main
    d = tmp_path / "pcp"
    d.mkdir()
    pts, _ = synth.make_cloud("ellipsoid", n=3000, seed=50)
    np.savetxt(str(d / "shapeA.xyz"), pts, fmt="%.9g")
    (d / "testset.txt").write_text("shapeA\n\n")
    files = []
    for lib_batch in (1024, 1792):
        results = str(tmp_path / ("log%d" % lib_batch)) + os.sep
        assert main(["--results_path", results, "--dataset_name", "synth", "--dataset_path", str(d) + os.sep, "--testset", "testset.txt",
                     "--synthetic_weights", "--reproducible", "1", "--lib_batch", str(lib_batch)]) == 0
        out = os.path.join(results, "synth_results")
        files.append([open(os.path.join(out, "shapeA" + ext), "rb").read() for ext in (".normals", ".experts", ".experts_probs")])
        log = open(os.path.join(out, "log.txt")).read()
        print(log)
        assert "reproducible run of shapeA:" in log and " pass" in log and "violations == 0: True" in log
    assert len(files[0][0].splitlines()) == 3000
    for x, y in zip(*files):
        assert x == y


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
        o, _ = p.communicate(timeout=900)
        assert p.returncode == 0, o.decode()[-3000:]


def test_two_ranks_equal_one_rank_in_the_headline_dtype(tmp_path, gpu_device):
    """f16x8c, reproducible, deterministic calibration: both ranks of a world-2 job on one GPU end up with the one-rank result bit
    for bit in all three arrays (the loop of run_verified over the global maxima, dist.estimate_sharded)."""
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    _run_world(one, 1)
    _run_world(two, 2)
    ref = np.load(one + ".rank0.npz")
    assert ref["normals"].shape == (2001, 3) and len(np.unique(ref["expert"])) >= 5
    print("one rank: passes %d tau %.6g thr %.6g" % (ref["passes"], ref["tau"], ref["thr"]))
    for r in range(2):
        got = np.load(two + ".rank%d.npz" % r)
        for k in ("normals", "expert", "probs"):
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), "rank %d %s" % (r, k)
        assert got["passes"] == ref["passes"] and got["tau"] == ref["tau"] and got["thr"] == ref["thr"]
