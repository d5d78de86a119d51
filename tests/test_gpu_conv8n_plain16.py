"""The plain 16-bit tap loop of conv8n_kernel (MODE 0: v_mfma_f32_16x16x32 for f16, 32x32x16 for bf16) against the fp64 oracle.

Every k^3 tap layer at 8^3 of a plain f16 / bf16 model runs this loop: 3^3 and 5^3, 64-column tiles, the fused 2^3 max-pool
epilogue of the experts' inception blocks, the routed experts' device-side point counts and walking launches.  The bounds are
the ones tests/test_gpu_net.py states for these modes; the batch sizes are not multiples of the kernel's 4-point groups."""
import numpy as np
import pytest
import torch

from conftest import golden_patch_files, load_golden_patches

pytestmark = pytest.mark.gpu

TOL = {"f16": (5e-3, 6e-2), "bf16": (1e-1, 4e-1)}     # (1 - cos of the normals, |probs| error)


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _queries(n100k, n20k):
    g = load_golden_patches([p for p in golden_patch_files() if "ellipsoid100k" in p][0])
    g2 = load_golden_patches([p for p in golden_patch_files() if "ellipsoid20k" in p][0])
    pts = np.concatenate([g["points"][:n100k], g2["points"][:n20k]])
    n_eff = np.concatenate([g["n_eff"][:n100k], g2["n_eff"][:n20k]])
    return pts, n_eff


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_gate_and_every_expert_match_oracle_on_a_ragged_batch(dtype, gpu_device):
    """13 queries (three full 4-point groups and one with a single point): the gating tower and all seven expert towers."""
    from nesti_net_amd import weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from oracle import mups_ref, net_ref
    cos_tol, prob_tol = TOL[dtype]
    cfg = NestiConfig()
    W = weights.synthetic_weights(cfg)
    pts, n_eff = _queries(8, 5)
    mups = mups_ref.mups_assemble(pts, n_eff, 3)
    ref = net_ref.moe_forward(mups, W, dtype=torch.float64, top1_only=False)
    net = NestiNet(cfg, W, dtype=dtype, device=gpu_device, max_batch=16)
    p, n = torch.as_tensor(pts, device=gpu_device), torch.as_tensor(n_eff, device=gpu_device)
    normals, expert, probs = net(p, n)
    n_all = net.experts(net.mups(p, n), None).cpu().numpy()               # [E, 13, 3]
    torch.cuda.synchronize()
    pe = np.abs(probs.cpu().numpy() - ref["probs"].numpy()).max()
    c = _cos(n_all, ref["n_est"].numpy())
    print(dtype, "prob err", pe, "all-experts max 1 - cos", (1 - c).max())
    assert pe < prob_tol
    assert np.all(1 - c < cos_tol)
    srt = np.sort(ref["probs"].numpy(), axis=1)
    agree = expert.cpu().numpy() == ref["probs"].numpy().argmax(1)
    assert np.all(agree | (srt[:, -1] - srt[:, -2] < 2 * prob_tol))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_routed_top1_forward_matches_oracle(dtype, gpu_device):
    """A gate calibrated to spread its arg-max over the experts: each expert tower sees a ragged, device-side count of the
    45 queries (npoints_ptr), and the rounds after the first are walking launches."""
    from nesti_net_amd import weights
    from nesti_net_amd.calibrate import calibrate_gate
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    from oracle import mups_ref, net_ref
    cos_tol, prob_tol = TOL[dtype]
    cfg = NestiConfig()
    pts, n_eff = _queries(24, 21)
    p, n = torch.as_tensor(pts, device=gpu_device), torch.as_tensor(n_eff, device=gpu_device)
    Wc = calibrate_gate(cfg, weights.synthetic_weights(cfg), p, n, device=gpu_device)
    net = NestiNet(cfg, Wc, dtype=dtype, device=gpu_device, max_batch=48)
    normals, expert, probs = net(p, n)
    torch.cuda.synchronize()
    ex = expert.cpu().numpy()
    assert len(np.unique(ex)) >= 4
    ref = net_ref.moe_forward(mups_ref.mups_assemble(pts, n_eff, 3), Wc, dtype=torch.float64, top1_only=True)
    pe = np.abs(probs.cpu().numpy() - ref["probs"].numpy()).max()
    srt = np.sort(ref["probs"].numpy(), axis=1)
    agree = ex == ref["expert"].numpy()
    print(dtype, "routing", np.bincount(ex, minlength=7), "prob err", pe, "agree", agree.mean())
    assert pe < prob_tol
    assert np.all(agree | (srt[:, -1] - srt[:, -2] < 2 * prob_tol))
    c = _cos(normals.cpu().numpy()[agree], ref["normals"].numpy()[agree])
    assert np.all(1 - c < cos_tol)
