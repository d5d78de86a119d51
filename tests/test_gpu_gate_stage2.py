"""Recheck stage 2 of the f16x8c gate (include/nesti_hip.h): the rows the plain-f16 filter flags first go through the gating net with
its six k^3 tap layers at 8^3 in the FP6 cross-term form; only those whose stage-2 top-2 margin is below tau2_eff go on to the f16x3
gate (stage 3).  Checked against the f16x3 gate and against the same model with the stage switched off -- the parent's two-pass
recheck -- never against the stage's own output."""
import ctypes

import numpy as np
import pytest
import torch

import layer_ref

pytestmark = pytest.mark.gpu

B = 4096      # the calibrated-margin case: enough rows for a non-empty residual; <= 4096, so one recheck round and two stage-2 rounds
Q = 256       # the slice of the other cases


@pytest.fixture(scope="module")
def case(gpu_device):
    from nesti_net_amd import synth, weights
    from nesti_net_amd.calibrate import calibrate_gate
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from nesti_net_amd.provider import CloudPatches
    cfg = NestiConfig()
    pts = synth.make_cloud("torus", n=20000, seed=5, noise=0.001)[0]
    q = np.arange(3, 20000, 20000 // B)[:B]
    cp = CloudPatches(pts, cfg, device=gpu_device, pidx=q)
    points, n_eff = cp.build(0, B)
    W = calibrate_gate(cfg, weights.synthetic_weights(cfg), points[:512], n_eff[:512], device=gpu_device)
    x3 = NestiNet(cfg, W, dtype="f16x3", device=gpu_device, max_batch=B)
    p3, e3 = [t.clone() for t in x3.gate(x3.mups(points, n_eff))]
    l3 = torch.log(p3.double())                                        # the f16x3 gate's logits up to a shift per row
    top = torch.sort(l3, dim=1, descending=True).values
    margin3 = (top[:, 0] - top[:, 1]).cpu().numpy()                    # its top-2 margins
    torch.cuda.synchronize()
    del x3
    torch.cuda.empty_cache()
    return {"cfg": cfg, "W": W, "points": points, "n_eff": n_eff, "e3": e3, "p3": p3, "margin3": margin3}


def _net(case, dev, n):
    from nesti_net_amd.model import NestiNet
    net = NestiNet(case["cfg"], case["W"], dtype="f16x8c", device=dev, max_batch=n)
    net.set_x8_guard(-1.0)               # the experts' conditioning guard follows its own measurements: out of the comparison
    return net


def _bits(ts):
    return [t.cpu().numpy().view(np.uint32) for t in ts]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _filter_margins(net, points, n_eff):
    """Top-2 logit margins of the filter pass (tau = 0: it alone decides), from its probabilities."""
    net.set_gate_margin(0.0)
    p, _ = net.gate(net.mups(points, n_eff))
    s = torch.sort(torch.log(p.double()), dim=1, descending=True).values
    return (s[:, 0] - s[:, 1]).cpu().numpy()


def test_stage2_off_and_tau2_infinite_equal_the_two_pass_recheck(case, gpu_device):
    """256 rows, a filter margin that flags about half of them: with the stage switched off the gate's outputs are those of an
    f16x3c model (the parent's gate) bit for bit; with tau2 = +inf every flagged row falls through to stage 3 and all three outputs
    of a forward call equal the switched-off ones bit for bit, while the counters show every flagged row in the residual."""
    from nesti_net_amd.model import NestiNet
    pts, ne = case["points"][:Q], case["n_eff"][:Q]
    net = _net(case, gpu_device, Q)
    assert not net.cascade_stats()["stage2"]                           # no second margin set yet: the stage does not run
    tau = float(np.median(_filter_margins(net, pts, ne)))
    net.set_gate_margin(tau)
    net.cascade_stats(reset=True)
    unset = [t.clone() for t in net(pts, ne)]                          # ... and the call is the two-pass recheck
    assert net.cascade_stats(reset=True)["stage2_rows"] == 0
    net.set_gate_margin2(1e-3)
    assert net.cascade_stats()["stage2"]
    net.set_gate_stage2(False)
    off = [t.clone() for t in net(pts, ne)]
    assert _same(unset, off)
    st_off = net.cascade_stats(reset=True)
    assert not st_off["stage2"] and st_off["stage2_rows"] == 0 and 0 < st_off["rechecked"] < Q
    c3 = NestiNet(case["cfg"], case["W"], dtype="f16x3c", device=gpu_device, max_batch=Q)
    c3.set_gate_margin(tau)
    pc, ec = c3.gate(c3.mups(pts, ne))
    assert _same([off[2], off[1]], [pc, ec]), "stage off: the gate differs from the f16x3c model's"
    net.set_gate_stage2(True)
    net.set_gate_margin2(1e30)
    inf = [t.clone() for t in net(pts, ne)]
    st = net.cascade_stats(reset=True)
    assert _same(inf, off), "tau2 = +inf: outputs differ from the switched-off model's"
    assert st["stage2"] and st["rechecked"] == st_off["rechecked"] == st["stage2_rows"] == st["stage2_residual"]
    assert st["stage2_decided"] == 0 and st["changed"] == st_off["changed"]
    assert st["max_margin_err"] == st_off["max_margin_err"]            # the filter is measured against the f16x3 gate, as before
    assert 0 < st["max_margin_err2"] < st["max_margin_err"]
    net.set_x8_format(8)                                               # format 8: no stage, whatever the switch says
    assert not net.cascade_stats()["stage2"]
    assert _same([t.clone() for t in net.gate(net.mups(pts, ne))], [pc, ec])


def test_tau2_zero_lets_stage2_decide_every_row(case, gpu_device):
    """Every row flagged (tau = +inf) and tau2 = 0: stage 2 decides all of them.  Its arg-max is the f16x3 gate's on every row whose
    f16x3 top-2 margin exceeds the stage's largest error on a logit difference (measured beforehand with tau2 = +inf, where both
    stages decide every row); rows with equal arg-max have the normals the two-pass recheck routes to, bit for bit; the counters
    add up."""
    pts, ne = case["points"][:Q], case["n_eff"][:Q]
    net = _net(case, gpu_device, Q)
    net.set_gate_margin(1e30)
    net.set_gate_margin2(1e30)
    net.cascade_stats(reset=True)
    ref = [t.clone() for t in net(pts, ne)]                            # stage 3 decides: the f16x3 gate's routing
    err2 = net.cascade_stats(reset=True)["max_margin_err2"]
    assert 0 < err2 < 0.05 and np.array_equal(ref[1].cpu().numpy(), case["e3"][:Q].cpu().numpy())
    net.set_gate_margin2(0.0)
    out = [t.clone() for t in net(pts, ne)]
    st = net.cascade_stats(reset=True)
    print("tau2 = 0:", st, "measured stage-2 error", err2)
    assert st["rechecked"] == Q and st["stage2_rows"] == Q and st["stage2_decided"] + st["stage2_residual"] == st["stage2_rows"]
    assert st["stage2_residual"] == 0 and st["stage2_decided"] == Q and st["stage2_widened"] == 0 and st["stage2_dropped"] == 0
    e, e3 = out[1].cpu().numpy(), case["e3"][:Q].cpu().numpy()
    safe = case["margin3"][:Q] > err2
    assert safe.sum() > Q // 2 and np.array_equal(e[safe], e3[safe])
    same = e == ref[1].cpu().numpy()
    assert np.array_equal(_bits([out[0]])[0][same], _bits([ref[0]])[0][same])
    # the probabilities now carry stage 2's error instead of none: small against the filter's 0.0136 that unrechecked rows carry
    dp = float((out[2] - ref[2]).abs().max())
    print("largest |probs(stage 2) - probs(f16x3)| over %d rows: %.3g" % (Q, dp))
    assert dp < 0.0136


@pytest.mark.parametrize("k", [0, 1, 3, 4, 5, 9])
def test_awkward_list_sizes_leave_everything_else_alone(case, gpu_device, k):
    """The filter margin and the batch chosen so that exactly k rows are flagged (a tap-kernel tile holds 4 points), the workspace
    filled with a pattern beforehand.  tau2 = +inf: stage 2 runs k rows, the residual list holds the same k, and the gate's outputs are the
    two-pass recheck's bit for bit; tau2 = 0: stage 2 decides them, with the f16x3 arg-max wherever the f16x3 margin exceeds the
    measured error.  Behind the k rows the block of FP6 planes, the residual list, its logits and the margins still hold the pattern."""
    from nesti_net_amd import _lib
    from nesti_net_amd.config import DTYPES
    net = _net(case, gpu_device, Q)
    fm = _filter_margins(net, case["points"][:Q], case["n_eff"][:Q])
    # the threshold sits in the first gap of the sorted margins wider than 1e-4 with at least k rows below it (the probabilities
    # give the margins to ~1e-6); k of the rows below the gap stay in the batch, the others leave it
    order = np.argsort(fm)
    srt = fm[order]
    j = next(i for i in range(max(k, 1), Q) if srt[i] - srt[i - 1] > 1e-4)
    tau = 0.0 if k == 0 else float((srt[j - 1] + srt[j]) / 2)
    idx = np.arange(Q) if k == 0 else np.sort(np.concatenate([order[:k], order[j:]]))
    n = len(idx)
    assert n > Q // 2
    sel = torch.as_tensor(idx, device=gpu_device)
    pts, ne = case["points"][:Q][sel].contiguous(), case["n_eff"][:Q][sel].contiguous()
    margin3 = case["margin3"][:Q][idx]
    net.set_gate_margin(tau)
    net.set_reproducible(True)           # the threshold is tau itself: a margin this small would otherwise widen itself (and the list)
    mups = net.mups(pts, ne)
    net.set_gate_stage2(False)
    off = [t.clone() for t in net.gate(mups)]
    assert net.cascade_stats(reset=True)["rechecked"] == k
    net.set_gate_stage2(True)
    S, c = _lib.CDebugStage2(), case["cfg"].to_c()
    _lib.check(net.lib.nesti_debug_gate_stage2_plan(ctypes.byref(c), DTYPES["f16x8c"], n, ctypes.byref(S)), "nesti_debug_gate_stage2_plan")
    _, _, ws_pair = layer_ref.tower_ops(net.lib, c, DTYPES["f16x8c"], -1, S.cap, 0, 0)
    arena = net._ws[S.arena_offset:S.arena_offset + S.arena_bytes]
    PAT = 0x7B
    for tau2 in (1e30, 0.0):
        net.set_gate_margin2(tau2)
        torch.cuda.synchronize()
        net._ws.fill_(PAT)
        out = [t.clone() for t in net.gate(mups)]
        st = net.cascade_stats(reset=True)
        assert st["rechecked"] == k == st["stage2_rows"] == st["stage2_decided"] + st["stage2_residual"]
        if tau2 > 1:
            assert st["stage2_residual"] == k and _same(out, off)
        else:
            assert st["stage2_decided"] == k
            e, e0 = out[1].cpu().numpy(), off[1].cpu().numpy()
            flagged = e != e0
            assert flagged.sum() <= k and np.all(margin3[flagged] <= 0.05)
            moved = (out[0] != off[0]).any(dim=1).cpu().numpy()
            assert moved.sum() <= k                                    # only flagged rows can carry stage 2's probabilities
        res_n = k if tau2 > 1 else 0
        side = arena[ws_pair:S.tower_bytes]                            # the planes: 512 voxels x 256 channels x 2 bytes per row
        assert side.numel() == ((S.cap * 512 * 256 * 2 + 255) // 256) * 256
        assert bool((side[k * 512 * 512:] == PAT).all()), "FP6 planes written behind row %d" % k
        if k:
            assert not bool((side[:k * 512 * 512] == PAT).all())
        assert bool((arena[S.residual + 4 * res_n:S.logits2] == PAT).all()), "residual list written behind entry %d" % res_n
        assert bool((arena[S.logits2 + 32 * res_n:S.margin2] == PAT).all()), "stage-2 logits written behind row %d" % res_n
        assert bool((arena[S.margin2 + 4 * k:S.end] == PAT).all()), "margins written behind entry %d" % k


def test_calibrated_margins_reproduce_the_f16x3_decisions(case, gpu_device):
    """Both margins calibrated on the first 1024 rows, then the filter margin forced wide open so that all 4096 rows reach stage 2
    (two stage-2 rounds): the residual is not empty, every arg-max is the f16x3 gate's, tau2_eff covers 1.5 x the error the call
    measured; in the reproducible mode one call and two calls over the halves write the same bits."""
    from nesti_net_amd.calibrate import GATE_MARGIN2_FLOOR, calibrate_gate_margin
    pts, ne = case["points"], case["n_eff"]
    net = _net(case, gpu_device, B)
    tau = calibrate_gate_margin(net, pts[:1024], ne[:1024])
    cal = net.cascade_stats()
    assert 0 < tau < 2.0 and GATE_MARGIN2_FLOOR <= cal["tau2"] < tau and cal["stage2"]
    net.set_gate_margin(1e30)
    normals, expert, probs = net(pts, ne)
    st = net.cascade_stats()
    print("calibrated: tau %.4g tau2 %.4g" % (tau, cal["tau2"]), st)
    assert st["stage2_rows"] == B == st["stage2_decided"] + st["stage2_residual"] + 0 and st["stage2_dropped"] == 0
    assert 0 < st["stage2_residual"] < B // 10                         # a residual, not a second full pass
    assert np.array_equal(expert.cpu().numpy(), case["e3"].cpu().numpy())
    assert st["tau2_eff"] >= 1.5 * st["max_margin_err2"] * (1 - 1e-6) and st["tau2_eff"] >= st["tau2"]
    # reproducible mode: both margins frozen, a row's outputs do not depend on the call it is part of
    net.set_reproducible(True)
    whole = [t.clone() for t in net(pts, ne)]
    halves = [[t.clone() for t in net(pts[lo:lo + B // 2], ne[lo:lo + B // 2])] for lo in (B // 2, 0)]
    joined = [torch.cat([halves[1][i], halves[0][i]]) for i in range(3)]
    assert _same(whole, joined)
    thirds = [[t.clone() for t in net(pts[lo:hi], ne[lo:hi])] for lo, hi in ((0, 1000), (1000, 3001), (3001, B))]
    assert _same(whole, [torch.cat([t[i] for t in thirds]) for i in range(3)])
    assert np.array_equal(whole[1].cpu().numpy(), case["e3"].cpu().numpy())
