"""NESTI_F16X8 / NESTI_F16X8C (round 6): the expert towers' tap layers at 8^3 (default: all four; mask 0xA: the 5^3 ones) with their
two cross terms through ONE FP8 MFMA (conv8n.hip X8) and the conditioning guard behind them (decide.hip: x8_guard_*) -- pinned to
f16x3 on 10k queries of the bench's cloud shape with a calibrated gate:
  * arg-max IDENTICAL to f16x3's on every query (the gating net is untouched) and probabilities bit-identical,
  * normals within 1 - cos <= 2.5e-6 of f16x3's on every query (the emulation that preceded the kernel: profiles/r06_fp8_cross_step0.txt;
    the tolerance of the north star is 1e-5),
  * every expert used, so all seven towers' X8 layers and their producers' e4m3 planes are exercised (Expert_6 has 42 -> 64 padded
    input channels in inception1),
  * layer mask 0 == f16x3 bit for bit, every layer alone and the 5^3 pair (mask 0xA) inside the same bar,
  * f16x8c == f16x8 in arg-max and normals once its gate margin is calibrated (the cascade is orthogonal to the expert arithmetic),
The fp64 oracle holds the mode on the six fixture clouds in tests/test_gpu_fixtures.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _omc(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)


@pytest.mark.parametrize("fmt", [6, 8])
def test_x8_experts_pinned_to_f16x3(gpu_device, fmt):
    """fmt 6 (the default): the cross terms as block-scaled FP6 e2m3 (one scale per 16-channel block of a row, conv8n.hip X6); fmt 8: FP8
    e4m3 with one scale per layer (X8).  Same assertions for both; the FP6 residual is ~1.15x the FP8 one."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import parity, synth, weights
    from nesti_net_amd.calibrate import calibrate_gate, calibrate_gate_margin
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.provider import CloudPatches
    cfg = NestiConfig()
    N, Q = 100000, 10000
    pts = synth.make_cloud("ellipsoid", n=N, seed=1234)[0]
    q = np.arange(0, N, N // Q)[:Q]
    cp = CloudPatches(pts, cfg, device=gpu_device, pidx=q)
    p_d, n_d = cp.build(0, Q)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), p_d[:512], n_d[:512], device=gpu_device)
    n3, e3, p3 = NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=Q)(p_d, n_d)
    net8 = NestiNet(cfg, W, dtype="f16x8", device=gpu_device, max_batch=Q)
    net8.set_x8_format(fmt)
    net8.set_x8_guard(-1.0)          # the bare loop: every row carries the 6 / 8-bit cross terms (the guard has its own test below)
    n8, e8, p8 = net8(p_d, n_d)
    torch.cuda.synchronize()
    n3, e3, n8, e8 = n3.cpu().numpy(), e3.cpu().numpy(), n8.cpu().numpy(), e8.cpu().numpy()
    assert np.array_equal(e8, e3) and torch.equal(p8, p3)
    assert len(np.unique(e3)) == cfg.n_experts
    omc = _omc(n8, n3)
    dn = np.linalg.norm(n8.astype(np.float64) - n3, axis=1)
    print("format %d:" % fmt, "f16x8 vs f16x3 on %d queries: 1-cos p50 %.3g p99 %.3g max %.3g, |dn| p50 %.3g max %.3g, routing %s"
          % (Q, np.quantile(omc, .5), np.quantile(omc, .99), omc.max(), np.quantile(dn, .5), dn.max(), np.bincount(e3).tolist()))
    assert omc.max() <= 2.5e-6
    assert dn.max() > 0            # the FP8 loop really ran (mask 0 below is the bit-identical case)
    # per expert: every tower within the bound (a wrong plane / scale in ONE tower must not hide behind the others)
    for e in range(cfg.n_experts):
        assert omc[e3 == e].max() <= 2.5e-6
    # mask 0: f16x3 proper
    net8.set_x8_layers(0)
    n0, e0, _ = net8(p_d, n_d)
    assert np.array_equal(n0.cpu().numpy(), n3) and np.array_equal(e0.cpu().numpy(), e3)
    # the 5^3 layers only
    net8.set_x8_layers(0xA)
    nf, _, _ = net8(p_d, n_d)
    omc_f = _omc(nf.cpu().numpy(), n3)
    print("mask 0xA (5^3 layers only): 1-cos p99 %.3g max %.3g" % (np.quantile(omc_f, .99), omc_f.max()))
    assert omc_f.max() <= 2.5e-6
    if fmt == 8:          # the per-layer and cascade checks below run once, in the default form
        return
    # one layer at a time: each bit alone moves the result, and stays inside the bound
    for bit in range(4):
        net8.set_x8_layers(1 << bit)
        nb, _, _ = net8(p_d[:2000], n_d[:2000])
        ob = _omc(nb.cpu().numpy(), n3[:2000])
        assert 0 < ob.max() <= 2.5e-6, (bit, ob.max())
    net8.set_x8_layers(0xF)
    del net8
    # the cascade on top: f16x8c == f16x8 once the margin is calibrated
    net_c = NestiNet(cfg, W, dtype="f16x8c", device=gpu_device, max_batch=Q)
    net_c.set_x8_format(fmt)
    net_c.set_x8_guard(-1.0)
    tau = calibrate_gate_margin(net_c, p_d[:2048], n_d[:2048])
    nc, ec, _ = net_c(p_d, n_d)
    st = net_c.cascade_stats()
    print("f16x8c: tau %.4g" % tau, st)
    assert 0 < st["rechecked"] < Q
    assert np.array_equal(ec.cpu().numpy(), e8) and np.array_equal(nc.cpu().numpy(), n8)
    with pytest.raises(Exception):
        NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=8).set_x8_layers(0xA)
    with pytest.raises(Exception):
        NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=8).set_x8_format(6)
    with pytest.raises(Exception):
        net_c.set_x8_format(4)


def test_x8_prescale_follows_the_batch_norm_and_saturates_gracefully(gpu_device):
    """The e4m3 planes' pre-scale is 2^sc with (|beta| + 8 |gamma|) 2^sc in (128, 256], from the PRODUCING layer's folded batch-norm.
    (a) A tower whose conv1 layers have 16x larger gamma (activations 16x larger) must stay inside the bound: the scale adapts.
    (b) Batch-norm statistics that LIE about the data (variance 1000x too small: activations ~30x the bound, most of them beyond
    e4m3's 448 after scaling) saturate the planes: the cross terms of those elements are lost, nothing else -- the result stays
    finite and degrades to single-product quality at worst (1 - cos of order 1e-5 .. 1e-3), it does not blow up."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth, weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.provider import CloudPatches
    cfg = NestiConfig()
    pts = synth.make_cloud("ellipsoid", n=20000, seed=5)[0]
    q = np.arange(0, 20000, 10)[:2000]
    cp = CloudPatches(pts, cfg, device=gpu_device, pidx=q)
    p_d, n_d = cp.build(0, len(q))
    W0 = weights.synthetic_weights(cfg)
    expert = torch.full((len(q),), 3, dtype=torch.int32, device=gpu_device)       # one expert: Expert_3

    def run(W):
        """-> the experts' normals in f16x3, in the e4m3 form (whose pre-scale this test is about) and in the FP6 form (which scales every
        block by itself)."""
        net3 = NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=len(q))
        o3 = net3.experts(net3.mups(p_d, n_d), expert).cpu().numpy()
        del net3
        net = NestiNet(cfg, W, dtype="f16x8", device=gpu_device, max_batch=len(q))
        m = net.mups(p_d, n_d)
        net.set_x8_format(8)
        o8 = net.experts(m, expert).cpu().numpy()
        net.set_x8_format(6)
        return o3, o8, net.experts(m, expert).cpu().numpy()

    Wa = dict(W0)
    for blk in ("inception1", "inception2"):
        k = blk + "Expert_3_conv1/bn/"
        Wa[k + "gamma"] = (W0[k + "gamma"] * 16).astype(np.float32)
        Wa[k + "beta"] = (W0[k + "beta"] * 16).astype(np.float32)
    a3, a8, a6 = run(Wa)
    oa = _omc(a8, a3)
    print("16x larger conv1 activations: 1-cos max %.3g" % oa.max())
    assert oa.max() <= 2.5e-6
    Wb = dict(W0)
    for blk in ("inception1", "inception2"):
        k = blk + "Expert_3_conv1/bn/"
        Wb[k + "var"] = (W0[k + "var"] / 1000).astype(np.float32)
    n3, n8, b6 = run(Wb)
    ob = _omc(n8, n3)
    print("batch-norm variance 1000x too small (saturating planes): 1-cos p50 %.3g max %.3g" % (np.quantile(ob, .5), ob.max()))
    assert np.all(np.isfinite(n8)) and ob.max() <= 5e-3
    # the FP6 form carries one scale per 16-channel block, taken from the data: neither case can push it out of range
    o6a, o6b = _omc(a6, a3), _omc(b6, n3)
    print("FP6 form: 16x larger activations 1-cos max %.3g, lying batch-norm 1-cos max %.3g" % (o6a.max(), o6b.max()))
    assert o6a.max() <= 2.5e-6 and o6b.max() <= 2.5e-6


def test_x8_conditioning_guard(gpu_device):
    """Outputs of small norm are re-evaluated in f16x3 proper (decide.hip: x8_guard_*): threshold infinity == f16x3 bit for bit and
    measures |dn|; threshold < 0 == the bare FP8 loop; in between exactly the rows below the threshold carry f16x3's bits, the others
    the FP8 loop's; the threshold follows the measured |dn| (thr_eff), calibrate_x8_guard sets it from a sample, and with the guard in
    place the largest 1 - cos against f16x3 among the un-re-evaluated rows respects the bound 2.5e-6 / 1.5^2."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib, synth, weights
    from nesti_net_amd.calibrate import calibrate_gate, calibrate_x8_guard
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.provider import CloudPatches
    cfg = NestiConfig()
    N, Q = 100000, 9000          # threshold infinity re-evaluates every row: an expert's share must fit its guard list (2 048 rows)
    pts = synth.make_cloud("ellipsoid", n=N, seed=1234)[0]
    q = np.arange(3, N, N // Q)[:Q]
    cp = CloudPatches(pts, cfg, device=gpu_device, pidx=q)
    p_d, n_d = cp.build(0, Q)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), p_d[:512], n_d[:512], device=gpu_device)
    n3, e3, _ = NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=Q)(p_d, n_d)
    n3 = n3.cpu().numpy()
    net = NestiNet(cfg, W, dtype="f16x8", device=gpu_device, max_batch=Q)
    theta = (2 * _lib.X8_GUARD_BAR) ** 0.5
    # off: the bare FP8 loop
    net.set_x8_guard(-1.0)
    bare = net(p_d, n_d)[0].cpu().numpy()
    assert net.x8_guard_stats()["rechecked"] == 0
    rb = np.linalg.norm(bare.astype(np.float64), axis=1)
    dn_true = np.linalg.norm(bare.astype(np.float64) - n3, axis=1)
    # infinity: every row twice
    net.x8_guard_stats(reset=True)
    net.set_x8_guard(float("inf"))
    allr = net(p_d, n_d)[0].cpu().numpy()
    st = net.x8_guard_stats(reset=True)
    assert np.array_equal(allr, n3) and st["rechecked"] == Q and st["queries"] == Q and st["dropped"] == 0
    assert abs(st["max_dn"] - dn_true.max()) <= 1e-6 * max(1.0, dn_true.max()) + 1e-9, (st["max_dn"], dn_true.max())
    # a threshold in the bulk of the |n| distribution: exactly the rows below it are f16x3's
    thr = float(np.quantile(rb, 0.2))
    net.set_x8_guard(thr)
    mid = net(p_d, n_d)[0].cpu().numpy()
    st = net.x8_guard_stats(reset=True)
    below = rb < thr
    assert thr > _lib.X8_GUARD_WIDEN * dn_true.max() / theta          # so the measured |dn| does not widen it
    assert st["rechecked"] == int(below.sum()) and st["dropped"] == 0 and st["thr_eff"] == pytest.approx(thr)
    assert np.array_equal(mid[below], n3[below]) and np.array_equal(mid[~below], bare[~below])
    # a threshold BELOW what the measured |dn| asks for: the call widens itself -- rows up to 1.5 x |dn| / theta of the error it measured
    # in its first pass are re-evaluated in its second pass
    small = float(np.sort(rb)[2])                                     # two rows below it
    net.set_x8_guard(small)
    wid = net(p_d, n_d)[0].cpu().numpy()
    st = net.x8_guard_stats(reset=True)
    dn_first = dn_true[rb < small].max()
    upper = max(small, _lib.X8_GUARD_WIDEN * dn_first / theta)
    covered = rb < upper
    print("widening: thr %.4g -> %.4g, %d rows re-evaluated (%d below thr), thr_eff now %.4g" % (small, upper, st["rechecked"], int((rb < small).sum()), st["thr_eff"]))
    assert st["rechecked"] >= int(covered.sum()) and np.array_equal(wid[covered], n3[covered])
    # calibration, then the enforced bound on the rows that keep the FP8 result
    thr_c = calibrate_x8_guard(net, p_d[:2048], n_d[:2048])
    out = net(p_d, n_d)[0].cpu().numpy()
    st = net.x8_guard_stats()
    keep = ~np.all(out == n3, axis=1)
    omc = _omc(out[keep], n3[keep])
    print("calibrated thr %.4g, thr_eff %.4g, re-evaluated %d of %d, max 1-cos of the rest %.3g (bound %.3g)"
          % (thr_c, st["thr_eff"], st["rechecked"], Q, omc.max(), _lib.X8_GUARD_BAR / _lib.X8_GUARD_WIDEN ** 2))
    assert 0 < st["rechecked"] < 0.05 * Q
    assert omc.max() <= _lib.X8_GUARD_BAR / _lib.X8_GUARD_WIDEN ** 2 * 1.05
    with pytest.raises(Exception):
        NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=8).set_x8_guard(0.1)
