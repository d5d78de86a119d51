"""The three MuPS kernels (csrc/mups.hip: mups_kernel, mups3_kernel, patches_mups_kernel) and their five store types on the crafted
cases of tests/_mups_fixture.py, judged per output -- (row, scale, channel, Gaussian) -- against the float64 restatement with the
bound 4 e32 + 2^-22 the fixture derives from the restatement's own float32 error (tests/test_mups_cases.py checks the fixture).
Every output buffer is filled with the byte 0x7B before the call, so an element a kernel does not write is seen.

  f32 against the bound   every (grid, kind): within the bound, finite, empty scales exact zeros; the failure names the row, the scale,
                          the statistic and the Gaussian.  The 3^3 grid also through NestiNet.mups in the 4^3-embedded layout: the 27
                          live rows equal the dense run bit for bit, dead rows and pad columns are zero bits
  masked garbage          NaN / inf in the rows beyond n_eff change no bit
  store types             f16 / bf16 (tight and padded stride) and the hi plane of f16x3 / bf16x3 equal the f32 run of the same input
                          rounded to nearest even on the CPU, bit for bit; every pad column of both planes and both groups is zero
                          bits; the lo plane is NOT bit-equal (the pair instantiations fuse the kernel's last product into the
                          subtraction): it is within 1 ulp of the 16-bit type of the rounding of v - hi, except bf16x3 elements whose
                          ulp is below ulp32(v), which are held to |hi + lo - v| <= ulp32(v) instead (``_check_store``);
                          on the 3^3 grid the embedded layout of a model of that dtype equals the dense run
  fused kernel            a cloud of 1154 points whose position queries see balls of 0, 1, 63, 64, 65, P and more points:
                          patches_mups_kernel's MuPS tensor and the network's outputs equal the unfused path's bit for bit"""
import ctypes

import numpy as np
import pytest
import torch

import _mups_fixture as F

pytestmark = pytest.mark.gpu

FILL = 0x7B
ALL = [(g, k) for g in F.GRIDS for k in F.KINDS]
_ids = ["%d-%s" % gk for gk in ALL]
_f32, _weights = {}, {}


def _filled(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(FILL)
    return t


def _bits(t):
    """Bit pattern of a CPU tensor as a signed integer array of its element width."""
    a = t.contiguous()
    return a.view(torch.int32 if a.element_size() == 4 else torch.int16).numpy()


def _case(grid, kind):
    return F.layout_case(grid) if kind == "layout" else F.case(grid, kind)


def _dense(c, dev, dtype="f32", cstride=None, pts=None):
    """``mups_forward`` into a 0x7B-filled buffer -> CPU tensor [B, R, R, R, cstride]."""
    from nesti_net_amd.model import _TORCH_DT, mups_forward
    g, B = c["grid"], len(c["n_eff"])
    out = _filled((B, g, g, g, cstride or 20 * c["S"]), _TORCH_DT[dtype], dev)
    got = mups_forward(F.config(g, c["S"], c["P"]), torch.as_tensor(c["pts"] if pts is None else pts, device=dev),
                       torch.as_tensor(c["n_eff"], device=dev), out_dtype=dtype, out_cstride=cstride, out=out)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu()


def _run_f32(grid, kind, dev):
    """The dense f32 run of a case (on ``pts``, masked garbage included), once; shared and never changed."""
    if (grid, kind) not in _f32:
        _f32[(grid, kind)] = _dense(_case(grid, kind), dev)
    return _f32[(grid, kind)]


def _net(grid, n_scales, num_point, dtype, dev, B):
    from nesti_net_amd import weights
    from nesti_net_amd.model import NestiNet
    cfg = F.config(grid, n_scales, num_point)
    if (grid, n_scales) not in _weights:
        _weights[(grid, n_scales)] = weights.synthetic_weights(cfg)
    return NestiNet(cfg, _weights[(grid, n_scales)], dtype=dtype, device=dev, max_batch=B)


def _embedded(c, dtype, dev):
    """``NestiNet.mups`` of a model of ``dtype`` on the 3^3 grid into a 0x7B-filled buffer: (CPU tensor [B,4,4,4,cstride], cstride)."""
    from nesti_net_amd.model import _TORCH_DT
    B = len(c["n_eff"])
    net = _net(3, c["S"], c["P"], dtype, dev, B)
    out = _filled((B, 4, 4, 4, net.mups_cstride), _TORCH_DT[dtype], torch.device(dev))
    got = net.mups(torch.as_tensor(c["pts"], device=dev), torch.as_tensor(c["n_eff"], device=dev), out=out)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu(), net.mups_cstride


def _check_embedded(emb, dense):
    """The 27 live rows are the dense run's bits; dead rows (a coordinate of 3) are zero bits."""
    assert np.array_equal(_bits(emb[:, :3, :3, :3]), _bits(dense))
    e = _bits(emb)
    assert not e[:, 3].any() and not e[:, :, 3].any() and not e[:, :, :, 3].any()


@pytest.mark.parametrize("grid,kind", ALL, ids=_ids)
def test_f32_within_the_bound(grid, kind, gpu_device):
    c = F.case(grid, kind)
    got = _run_f32(grid, kind, gpu_device).numpy()
    assert got.shape == (7, grid, grid, grid, 20 * F.S)
    assert np.isfinite(got).all()
    dead = ~c["live"]
    assert not np.moveaxis(got.view(np.uint32).reshape(7, grid, grid, grid, F.S, 20), 4, 1)[dead].any()      # empty scales: +0.0 bits
    r = F.ratios(got, c)
    well = ~c["ill"][:, None, None, None, :, :] & np.ones(r.shape, bool)
    print("%d^3 %s: largest error / bound %.3f (well-conditioned cells %.3f), largest e32 %.3g, ill-conditioned cells %.4f"
          % (grid, kind, r.max(), r[well].max(), c["e32"].max(), c["ill"].mean()))
    lines = F.violations(got, c)
    assert not lines, "\n".join(lines)


def test_f32_layout_case_within_the_bound(gpu_device):
    for grid in F.GRIDS:
        c = F.layout_case(grid)
        got = _run_f32(grid, "layout", gpu_device).numpy()
        assert got.shape == (3, grid, grid, grid, 80) and np.isfinite(got).all()
        assert not np.moveaxis(got.view(np.uint32).reshape(3, grid, grid, grid, 4, 20), 4, 1)[~c["live"]].any()
        lines = F.violations(got, c)
        assert not lines, "\n".join(lines)


@pytest.mark.parametrize("kind", F.KINDS + ("layout",))
def test_f32_embedded_layout_of_the_3_grid(kind, gpu_device):
    c = _case(3, kind)
    emb, cs = _embedded(c, "f32", gpu_device)
    assert cs >= 20 * c["S"] and emb.shape == (len(c["n_eff"]), 4, 4, 4, cs)
    _check_embedded(emb[..., :20 * c["S"]], _run_f32(3, kind, gpu_device))
    assert not _bits(emb[..., 20 * c["S"]:]).any()                       # pad columns of every row


@pytest.mark.parametrize("grid,kind", ALL, ids=_ids)
def test_masked_rows_never_reach_the_output(grid, kind, gpu_device):
    c = F.case(grid, kind)
    assert not np.isfinite(c["pts"]).all() and np.isfinite(c["pts_clean"]).all()
    clean = _dense(c, gpu_device, pts=c["pts_clean"])
    assert np.array_equal(_bits(clean), _bits(_run_f32(grid, kind, gpu_device)))


def _rounded(v, tdt):
    """(hi, lo) of the f32 CPU tensor v: hi = v rounded to nearest even, lo = (v - hi) in float32, rounded."""
    hi = v.to(tdt)
    return hi, (v - hi.float()).to(tdt)


def _pair_layout(hi, lo, cs):
    """[..., C] planes -> [..., cs] physical rows of [hi 64 | lo 64] per 64-channel group, zeros elsewhere."""
    C = hi.shape[-1]
    out = torch.zeros(hi.shape[:-1] + (cs,), dtype=hi.dtype)
    for g0 in range(0, C, 64):
        n = min(64, C - g0)
        out[..., 2 * g0:2 * g0 + n] = hi[..., g0:g0 + n]
        out[..., 2 * g0 + 64:2 * g0 + 64 + n] = lo[..., g0:g0 + n]
    return out


def _ulp16(x, tdt):
    """One unit in the last place of the 16-bit type at |x| (float64 array); the subnormal step below its normal range."""
    bits, emin = (10, -14) if tdt == torch.float16 else (7, -126)
    ex = np.frexp(np.abs(x))[1] - 1                                   # |x| = m 2^ex with m in [1, 2)
    return np.ldexp(1.0, np.maximum(np.where(x == 0, emin, ex), emin) - bits)


def _check_store(got, v, dtype, cs, label):
    """A 16-bit or pair-plane run ``got`` [B,R,R,R,cs] against the f32 run ``v`` of the same input.

    f16 / bf16 and the hi plane: the bits of v rounded to nearest even; every pad column, in both planes of every group: zero bits.
    lo plane: the bits of rne(v - hi) are NOT reproduced, so the template instantiations differ in float32: split_pack2
    (csrc/common.h) states lo = rne(v - hi), but the compiler fuses the kernel's last product (v = raw x 1/norm) into that
    subtraction (v_pk_fma_f32 raw, 1/norm, -hi), so lo = rne(p - hi) with p the unrounded product, |p - v| <= 1/2 ulp32(v), while
    the f32 and 16-bit instantiations store v.  The test reports how many lo elements differ and by how much, then asserts
      * 1 ulp of the 16-bit type on every lo element of f16x3, and on every lo element of bf16x3 whose ulp is at least ulp32(v),
        that is except where v - hi cancels to a few float32 ulps of v;
      * on those remaining bf16x3 elements, where 1/2 ulp32(v) is itself several ulps of lo, the reconstructed value instead:
        |hi + lo - v| <= ulp32(v).  This second clause is a deviation from the 1-ulp bound, which such an element cannot meet
        while lo is formed from the unrounded product."""
    from nesti_net_amd.model import _TORCH_DT
    tdt, C = _TORCH_DT[dtype], v.shape[-1]
    hi, lo = _rounded(v, tdt)
    if not dtype.endswith("x3"):
        want = torch.cat([hi, torch.zeros(hi.shape[:-1] + (cs - C,), dtype=tdt)], dim=-1)
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), label
        return
    want = _pair_layout(hi, lo, cs)
    is_lo = _pair_layout(torch.zeros_like(v), torch.ones_like(v), cs).numpy().astype(bool)
    assert got.shape == want.shape
    same = _bits(got) == _bits(want)
    assert same[~is_lo].all(), label + ": hi plane or a pad column"
    g, w = got.double().numpy()[is_lo], want.double().numpy()[is_lo]
    vv = _pair_layout(torch.zeros_like(v), v, cs).numpy()[is_lo]
    h = want.double().numpy()[np.roll(is_lo, -64, axis=-1)]             # the hi element 64 columns before each lo element
    ulp16, ulp32 = _ulp16(w, tdt), np.spacing(np.abs(vv)).astype(np.float64)
    big = (ulp16 >= ulp32) | (tdt == torch.float16)                     # f16x3: the 1-ulp bound on every element
    err, rec = np.abs(g - w), np.abs((h + g) - vv.astype(np.float64))
    print("%s: lo plane differs from rne(v - hi) in %d of %d elements; %d elements held to 1 ulp of the 16-bit type (largest %.2f), "
          "%d to |hi + lo - v| <= ulp32(v) (largest %.2f; they are up to %.1f ulp of the 16-bit type off)"
          % (label, (~same[is_lo]).sum(), is_lo.sum(), big.sum(), (err / ulp16)[big].max(), (~big).sum(),
             (rec / ulp32)[~big].max() if (~big).any() else 0.0, (err / ulp16)[~big].max() if (~big).any() else 0.0))
    assert np.abs(w).max() > 0, label
    assert (err[big] <= ulp16[big]).all(), label + ": lo plane, 1 ulp of the 16-bit type"
    assert (rec[~big] <= ulp32[~big]).all(), label + ": lo plane, reconstructed value"


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f16x3", "bf16x3"])
@pytest.mark.parametrize("kind", ["uniform", "octant", "layout"])
@pytest.mark.parametrize("grid", list(F.GRIDS))
def test_store_types_are_the_rounded_f32_run(grid, kind, dtype, gpu_device):
    c = _case(grid, kind)
    C = 20 * c["S"]
    v = _run_f32(grid, kind, gpu_device)
    label = "%d^3 %s %s" % (grid, kind, dtype)
    strides = (128 if c["S"] <= 3 else 256,) if dtype.endswith("x3") else (C, 64 if C <= 60 else 96)
    for cs in strides:
        _check_store(_dense(c, gpu_device, dtype=dtype, cstride=cs), v, dtype, cs, "%s stride %d" % (label, cs))
    if grid == 3:                       # the embedded layout of a model of this dtype: the same kernel instantiation, so the same bits
        emb, cs = _embedded(c, dtype, gpu_device)
        dense = _dense(c, gpu_device, dtype=dtype, cstride=cs)
        assert emb.shape == (len(c["n_eff"]), 4, 4, 4, cs)
        _check_embedded(emb, dense)
        _check_store(dense, v, dtype, cs, "%s model stride %d" % (label, cs))


def test_out_is_checked(gpu_device):
    from nesti_net_amd.model import mups_forward
    c = F.layout_case(3)
    p, n = torch.as_tensor(c["pts"], device=gpu_device), torch.as_tensor(c["n_eff"], device=gpu_device)
    cfg = F.config(3, 4, 64)
    for bad in (torch.empty((3, 3, 3, 3, 84), device=gpu_device), torch.empty((3, 3, 3, 3, 80), dtype=torch.float16, device=gpu_device),
                torch.empty((3, 3, 3, 3, 160), device=gpu_device)[..., ::2], torch.empty((3, 3, 3, 3, 80))):
        with pytest.raises(ValueError, match="out: contiguous"):
            mups_forward(cfg, p, n, out=bad)


# ---- the fused kernel ---------------------------------------------------------------------------------------------------------------
def _arena_mups(est, M, dtype):
    """The MuPS tensor of the last library batch of a fused call: the head of the forward workspace (nesti_forward's own X0), which
    is the tail of the estimator's arena -- its offset is the difference of the two sizes the library reports."""
    from nesti_net_amd.model import _TORCH_DT
    cs = est.net.mups_cstride
    esz = torch.empty((), dtype=_TORCH_DT[dtype]).element_size()
    lib, h = est.net.lib, est.net._handle
    off = lib.nesti_estimate_workspace_bytes(h, est.batch) - lib.nesti_workspace_bytes(h, est.batch)
    assert 0 < off < est._arena.numel() and est._arena.numel() == lib.nesti_estimate_workspace_bytes(h, est.batch)
    torch.cuda.synchronize()
    return est._arena[off:off + M * 512 * cs * esz].cpu().view(_TORCH_DT[dtype]).view(M, 8, 8, 8, cs)


@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_fused_kernel_equals_the_unfused_path_on_edge_counts(dtype, gpu_device):
    from nesti_net_amd import _lib
    from nesti_net_amd.pipeline import NormalEstimator
    cl = F.make_cloud()
    cfg, M = cl["cfg"], len(cl["queries"])
    if (8, 3) not in _weights:
        from nesti_net_amd import weights
        _weights[(8, 3)] = weights.synthetic_weights(cfg)
    W = _weights[(8, 3)]
    est = NormalEstimator(cfg, W, dtype=dtype, device=gpu_device, batch=M, seed=3627473)
    assert est._fused
    cloud = est.prepare(cl["pts"], queries=cl["queries"])
    assert cloud.r_abs == cl["r_abs"]
    est._arena.fill_(FILL)
    E = cfg.n_gate_out
    normals, expert, probs = _filled((M, 3), torch.float32, est.device), _filled((M,), torch.int32, est.device), _filled((M, E), torch.float32, est.device)
    n_ball = _filled((M, 3), torch.int32, est.device)
    _lib.check(est.net.lib.nesti_estimate_normals_at(
        est.net._handle, _lib.ptr(cloud.cloud), cloud.n_points, _lib.ptr(cloud.queries), M, cloud._r, ctypes.c_uint64(cloud.seed), 0,
        est.batch, 0, _lib.ptr(cloud._ws), cloud._ws.numel(), _lib.ptr(est._arena), est._arena.numel(), _lib.ptr(normals),
        _lib.ptr(expert), _lib.ptr(probs), _lib.ptr(n_ball), _lib.stream_ptr(torch.cuda.current_stream(est.device))), "nesti_estimate_normals_at")
    fused_mups = _arena_mups(est, M, dtype)
    fused = [t.cpu() for t in (normals, expert, probs)]
    assert np.array_equal(n_ball.cpu().numpy(), F.cloud_ball_sizes())
    # the unfused path: patch tensors -> mups_kernel -> towers -> the sentinel of queries without a neighbourhood
    net = est.net                      # the same model (one weight upload); its own workspace, not the arena read above
    p, n = cloud.build(0, M)
    assert np.array_equal(n.cpu().numpy(), np.minimum(F.cloud_ball_sizes(), F.CLOUD_P))
    mups = net.mups(p, n, out=_filled((M, 8, 8, 8, net.mups_cstride), fused_mups.dtype, net.device))
    un = net.forward(p, n)
    _lib.check(net.lib.nesti_mask_empty_queries(_lib.ptr(n), M, cfg.n_scales, _lib.ptr(un[0]), _lib.ptr(un[1]), _lib.ptr(un[2]), un[2].shape[1],
                                                _lib.stream_ptr(torch.cuda.current_stream(net.device))), "nesti_mask_empty_queries")
    torch.cuda.synchronize()
    assert fused_mups.shape == mups.shape and np.array_equal(_bits(fused_mups), _bits(mups.cpu()))
    assert _bits(mups.cpu()).any() and not _bits(mups.cpu()[4]).any()              # the query without a neighbourhood: zeros, written
    for x, y in zip(fused, un):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y.cpu()))
    assert (fused[1][4] == -1) and (np.delete(fused[1].numpy(), 4) >= 0).all() and np.isfinite(fused[0].numpy()).all()
