"""Per-layer fp64 conformance of every conv and pool launch (tests/layer_ref.py): each launch of a tower runs alone
(nesti_debug_tower_step) and is compared with an fp64 evaluation of the same layer on its own input buffer, under a bound
derived from the number format; pools are bit-exact; every k^3 layer proves it would see a missing tap.  Also: live rows do
not depend on what the workspace held before (fills 0x00 / 0x7B), the routed / walking launches compute the same rows as the
plain ones, and stepping a tower op by op is exactly the product's tower pass.

Ragged batch: B = 37 queries (9 full 4-point groups + 1, 2 full 16-point groups + 5, a partial 512-row tile at 2^3)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_patch_files, load_golden_patches

import layer_ref

pytestmark = pytest.mark.gpu

B = 37
STATS = {}


def _report():
    for k in sorted(STATS, key=str):
        print("layer-conformance", k, "%.4g" % STATS[k])


@pytest.fixture(scope="module")
def experts_setup(gpu_device):
    from nesti_net_amd import weights
    from nesti_net_amd.config import NestiConfig
    cfg = NestiConfig()
    W = weights.synthetic_weights(cfg)
    pts, neff = [], []
    for p in golden_patch_files():
        g = load_golden_patches(p)
        if g["points"].shape[1] == 3 * 512 and g["n_eff"].shape[1] == 3:
            pts.append(g["points"])
            neff.append(g["n_eff"])
    pts, neff = np.concatenate(pts)[:B], np.concatenate(neff)[:B]
    assert len(pts) == B
    return cfg, W, torch.as_tensor(pts, device=gpu_device), torch.as_tensor(neff, device=gpu_device)


def _cloud_inputs(cfg, dev, n):
    from nesti_net_amd import synth
    from nesti_net_amd.provider import CloudPatches
    pts = synth.make_cloud("torus", n=20000, seed=5, noise=0.001)[0]
    q = np.arange(3, 20000, 20000 // n)[:n]
    cp = CloudPatches(pts, cfg, device=dev, pidx=q)
    return cp.build(0, n)


def _model_form(dtype):
    return {"f16x3c": "f16x3", "f16x8c": "f16x3", "f16x8": "f16x3"}.get(dtype, dtype)


def _check_tower(net, W, dtype, tower, mups, nb, **kw):
    """Every launch checked on a 0x00 workspace, then the same launches on a 0x7B workspace: bit-identical live rows."""
    lib = net.lib
    a = layer_ref.TowerChecker(lib, net, W, _model_form(dtype), tower, nb, mups, fill=0x00, stats=STATS, **kw)
    snaps_a = []
    a.run(check=True, snapshots=snaps_a)
    b = layer_ref.TowerChecker(lib, net, W, _model_form(dtype), tower, nb, mups, fill=0x7B, stats=STATS, **kw)
    snaps_b = []
    b.run(check=False, snapshots=snaps_b)
    for i, (sa, sb) in enumerate(zip(snaps_a, snaps_b)):
        for ta, tb in zip(sa, sb):
            if not torch.equal(ta, tb):
                bad = int((ta != tb).sum())
                raise AssertionError("%s, op %d %s: %d live output elements depend on what the workspace held (0x00 vs 0x7B fill)"
                                     % (a.where, i, layer_ref.op_name(a.ops[i]), bad))
    return a


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16", "f16x3", "bf16x3"])
def test_experts_model_every_launch(experts_setup, gpu_device, dtype):
    """experts_n_est on the 8^3 grid: the gating net and all seven experts, launch by launch; the stepped towers give the
    product's outputs exactly (experts: bitwise; gate: the arg-max, and the probabilities up to the fp32 softmax's own rounding)."""
    from nesti_net_amd.config import DTYPES
    from nesti_net_amd.model import NestiNet
    cfg, W, pts, neff = experts_setup
    net = NestiNet(cfg, W, dtype=dtype, device=gpu_device, max_batch=B)
    mups = net.mups(pts, neff)
    g = _check_tower(net, W, dtype, -1, mups, B)
    probs, expert = net.gate(mups)
    torch.cuda.synchronize()
    # nesti_gate_forward leaves the gating net's logits in its tower workspace, the tail of the forward workspace (plan.cpp:
    # ws_layout): they must be the stepped tower's, bit for bit
    c = cfg.to_c()
    tower_bytes = max(net.lib.nesti_tower_workspace_bytes(ctypes.byref(c), DTYPES[dtype], t, B) for t in range(-1, cfg.n_experts))
    ob = g.bufs[g.ops[-1]["out_buf"]]
    off = net._ws.numel() - tower_bytes + ob["offset"]
    logits = net._ws[off:off + B * ob["C"] * 4].view(torch.float32).reshape(B, ob["C"])
    assert torch.equal(logits, g.output()), "stepped gate: logits differ from nesti_gate_forward's (%s)" % dtype
    assert torch.equal(expert.long(), torch.argmax(logits[:, :cfg.n_experts], dim=1)), "nesti_gate_forward: arg-max of its own logits"
    # the probabilities against an fp64 softmax of those same logits: what remains is the fp32 softmax's own rounding (an exp of
    # ~1 ulp, a 7-term sum, a division), a few ulp -- 2^-20 relative
    p_ref = torch.softmax(logits[:, :cfg.n_experts].double(), dim=1)
    rel = float(((probs.double() - p_ref).abs() / p_ref.clamp_min(1e-30)).max())
    assert rel <= 2.0 ** -20, "stepped gate: probabilities differ from the softmax of the stepped logits by %.3g relative" % rel
    n_all = net.experts(mups, None)
    torch.cuda.synchronize()
    for e in range(cfg.n_experts):
        t = _check_tower(net, W, dtype, e, mups, B)
        assert torch.equal(t.output()[:, :3], n_all[e]), "stepped expert %d differs from nesti_experts_forward (%s)" % (e, dtype)
    _report()


@pytest.mark.parametrize("fmt", [6, 8])
def test_x8_experts_every_launch(experts_setup, gpu_device, fmt):
    """f16x8c (the bench's headline mode): the experts' four 8^3 tap layers with their cross terms in FP6 blocks (6, the default) or
    e4m3 (8), and the producer planes their blocks' conv1 writes, launch by launch; the stepped towers give nesti_experts_forward's
    normals bit for bit."""
    from nesti_net_amd.model import NestiNet
    cfg, W, pts, neff = experts_setup
    net = NestiNet(cfg, W, dtype="f16x8c", device=gpu_device, max_batch=B)
    net.set_x8_format(fmt)
    mups = net.mups(pts, neff)
    n_all = net.experts(mups, None)
    torch.cuda.synchronize()
    form = layer_ref.FORM_X6 if fmt == 6 else layer_ref.FORM_X8
    # FP6 (the product's form): every expert; FP8: one expert per scale and the three-scale one (its producer check runs the
    # e4m3 encoder on the host, which costs the suite's time budget)
    for e in (range(cfg.n_experts) if fmt == 6 else (0, 3, 6)):
        t = _check_tower(net, W, "f16x8c", e, mups, B, x8_mask=0xF, x8_fmt=fmt)
        assert sum(o["form"] == form for o in t.ops) == 4 and sum(o["aux_out_buf"] >= 0 for o in t.ops) == 2
        assert torch.equal(t.output()[:, :3], n_all[e]), "stepped expert %d differs from nesti_experts_forward (f16x8c, FP%d)" % (e, fmt)
    _report()


def test_filter_pass_every_launch(experts_setup, gpu_device):
    """The two-stage gate's plain-f16 filter pass (f16x3c): f16 tap layers, X2 one-tap layers on the pair packing."""
    from nesti_net_amd.model import NestiNet
    cfg, W, pts, neff = experts_setup
    net = NestiNet(cfg, W, dtype="f16x3c", device=gpu_device, max_batch=B)
    mups = net.mups(pts, neff)
    t = _check_tower(net, W, "f16x3c", -1, mups, B, fast=1)
    forms = {o["form"] for o in t.ops if o["kind"] == layer_ref.OP_CONV}
    assert forms == {layer_ref.FORM_PLAIN, layer_ref.FORM_X2}
    _report()


@pytest.mark.parametrize("dtype", ["f32", "f16", "f16x3", "f16x8c"])
def test_routed_walking_launches(experts_setup, gpu_device, dtype):
    """One expert tower per arithmetic family (f16x8c: the FP6 cross terms) over a gapped permutation of the batch with a live
    count below capacity: every launch checked at walk 8 (every tap launch's workgroups iterate 2-4 times) and 64 (the wide 1x1x1
    launches iterate), and the output rows bit-identical to the plain run's for walk 0, 1, 8 and 64."""
    from nesti_net_amd.model import NestiNet
    cfg, W, pts, neff = experts_setup
    net = NestiNet(cfg, W, dtype=dtype, device=gpu_device, max_batch=B)
    mups = net.mups(pts, neff)
    x8 = {"x8_mask": 0xF} if dtype == "f16x8c" else {}
    plain = layer_ref.TowerChecker(net.lib, net, W, _model_form(dtype), 2, B, mups, **x8)
    plain.run(check=False)
    ref_rows = plain.output()[:, :3].clone()
    rng = np.random.default_rng(11)
    lst = rng.permutation(B)[:29]                      # a gapped permutation: 29 of 37 rows, shuffled
    cap = 40
    idx = np.full(cap, 0, np.int32)
    idx[:29] = lst
    for walk in (8, 64, 0, 1):
        t = layer_ref.TowerChecker(net.lib, net, W, _model_form(dtype), 2, cap, mups, fill=0x7B, point_index=idx, count=29, walk=walk,
                                   stats=STATS, **x8)
        t.run(check=walk in (8, 64))
        assert torch.equal(t.output()[:, :3], ref_rows[torch.as_tensor(lst, device=gpu_device).long()]), \
            "routed expert 2 (%s, walk %d): rows differ from the plain run" % (dtype, walk)
    _report()


def _other_configs():
    from nesti_net_amd.config import NestiConfig
    four = NestiConfig(patch_radius=[0.01, 0.02, 0.04, 0.06], num_point=128, n_experts=8, expert_dict=None)
    four.expert_dict = four.default_expert_dict()
    return {"ss_norm_est": NestiConfig.for_model("ss_norm_est"), "ms_norm_est": NestiConfig.for_model("ms_norm_est"),
            "ms_sw_n_est": NestiConfig.for_model("ms_sw_n_est"), "grid3": NestiConfig(n_gaussians=3, gmm_variance=0.111),
            "four_scales": four}


@pytest.mark.parametrize("model", ["ss_norm_est", "ms_norm_est", "ms_sw_n_est", "grid3", "four_scales"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "f16x3"])
def test_other_models_every_launch(gpu_device, model, dtype):
    """The ablation models, the 3^3 grid and four scales / eight experts: every tower, launch by launch (s_real, the 3^3
    max-pool, conv4n at 4^3, the remapped 2^3 layers)."""
    from nesti_net_amd import weights
    from nesti_net_amd.model import NestiNet
    cfg = _other_configs()[model]
    W = weights.synthetic_weights(cfg)
    n = 21
    pts, neff = _cloud_inputs(cfg, gpu_device, n)
    net = NestiNet(cfg, W, dtype=dtype, device=gpu_device, max_batch=n)
    mups = net.mups(pts, neff)
    towers = ([-1] if cfg.arch in (0, 3) else []) + list(range(cfg.n_towers))
    for tw in towers:
        _check_tower(net, W, dtype, tw, mups, n)
    _report()
