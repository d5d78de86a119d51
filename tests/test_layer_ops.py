"""CPU checks of the per-layer test hook (nesti_debug_tower_ops) and of tests/layer_ref.py's emulation of the packer's value
rules and number formats -- no device needed."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import layer_ref


def _configs():
    from nesti_net_amd.config import NestiConfig
    four = NestiConfig(patch_radius=[0.01, 0.02, 0.04, 0.06], num_point=128, n_experts=8, expert_dict=None)
    four.expert_dict = four.default_expert_dict()
    return {"experts": NestiConfig(), "grid3": NestiConfig(n_gaussians=3, gmm_variance=0.111), "four_scales": four,
            "ss_norm_est": NestiConfig.for_model("ss_norm_est"), "ms_norm_est": NestiConfig.for_model("ms_norm_est"),
            "ms_sw_n_est": NestiConfig.for_model("ms_sw_n_est")}


def _passes(model, dtype):
    """(tower, fast, x8_mask) of every pass a model of this dtype runs."""
    cfg = _configs()[model]
    gate = cfg.arch in (0, 3)
    out = [(-1, 0, 0)] if gate else []
    if gate and dtype in ("f16x3c", "f16x8c"):
        out.append((-1, 1, 0))
    for e in range(cfg.n_towers):
        out.append((e, 0, 0))
        if dtype in ("f16x8", "f16x8c") and model == "experts":
            out.append((e, 0, 0xF))
    return out


DTYPES_OF = {m: ["f32", "f16", "bf16", "f16x3", "bf16x3"] + (["f16x3c", "f16x8", "f16x8c"] if m == "experts" else [])
             for m in _configs()}


@pytest.mark.parametrize("model", sorted(DTYPES_OF))
def test_tower_ops_cover_the_graph_and_keep_buffers_apart(model):
    """Every conv scope nesti_model_describe lists is the scope (or fused scope2) of exactly one conv launch of the towers;
    every buffer lies inside nesti_tower_workspace_bytes; buffers whose lifetimes overlap never share bytes; every launch
    reads buffers that are live and already written."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib, weights
    from nesti_net_amd.config import DTYPES
    lib = _lib.load()
    cfg = _configs()[model]
    c = cfg.to_c()
    scopes = sorted({k.rsplit("/", 1)[0] for k in weights.describe(cfg) if k.endswith("/weights")})
    for dtype in DTYPES_OF[model]:
        seen = {}
        for tower, fast, x8 in _passes(model, dtype):
            for batch in (37, 1000):
                bufs, ops, wsb = layer_ref.tower_ops(lib, c, DTYPES[dtype], tower, batch, fast, x8)
                # nesti_tower_workspace_bytes quotes the filter pass for the gating net of the two-stage models
                if fast or not (tower < 0 and dtype in ("f16x3c", "f16x8c")):
                    assert wsb == lib.nesti_tower_workspace_bytes(ctypes.byref(c), DTYPES[dtype], tower, batch)
                used = [b for b in bufs[1:] if b["bytes"] > 0]
                for b in used:
                    assert 0 <= b["offset"] and b["offset"] + b["bytes"] <= wsb, (model, dtype, tower, b)
                    esz = 2 if b["aux8"] else 4 if b["elem"] == 0 or b["f32"] else 2 * b["planes"]
                    assert b["bytes"] >= (batch << (3 * b["log2S"])) * b["C"] * esz
                for i, x in enumerate(used):
                    for y in used[i + 1:]:
                        if x["first"] <= y["last"] and y["first"] <= x["last"]:
                            assert x["offset"] + x["bytes"] <= y["offset"] or y["offset"] + y["bytes"] <= x["offset"], \
                                (model, dtype, tower, x, y)
                for k, op in enumerate(ops):
                    for b in (op["in_buf"], op["aux_in_buf"]):
                        if b >= 1:
                            assert bufs[b]["first"] < k <= bufs[b]["last"], (model, dtype, tower, k, b)
                    if op["kind"] == layer_ref.OP_CONV:
                        assert len(op["in_pos"]) == op["cin"] and np.all(op["in_pos"] < op["Cin_p"])
                        assert len(set(op["in_pos"].tolist())) == op["cin"]
                        if op["is_fc"] and op["in_buf"] >= 1:      # fc1's flattened view stays inside its buffer
                            assert op["in_cstride"] * op["in_planes"] * (2 if op["elem"] else 4) * batch <= bufs[op["in_buf"]]["bytes"]
                        if batch == 37 and not fast:
                            for s in (op["scope"], op["scope2"]):
                                if s:
                                    seen[s] = seen.get(s, 0) + (0 if x8 else 1)
        assert sorted(seen) == scopes, (model, dtype, set(scopes) ^ set(seen))
        assert all(v == 1 for v in seen.values()), (model, dtype, [k for k, v in seen.items() if v != 1])


PLAN_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests.json")
# both sides of cascade_cap's 4096, expert_cap's 8192 and guard_cap's 2048; 100000: a whole cloud as one batch
PLAN_BATCHES = (1, 37, 1000, 2048, 2049, 4096, 4097, 8192, 8193, 100000)


def plan_digests(lib):
    """{key: SHA-256} of every plan the library makes, folded over PLAN_BATCHES: per (model, dtype) the fused entry's workspace size
    ("size/..."), per pass of a tower ("plan/...") every field nesti_debug_tower_ops reports for every buffer and launch in the
    structs' field order, in_pos, the tower workspace and nesti_tower_workspace_bytes.  scripts/record_plan_digests.py writes the
    golden file from this function and the library of the commit BEFORE the planner was carved out of model.hip."""
    from nesti_net_amd.config import DTYPES
    out = {}
    for model, cfg in sorted(_configs().items()):
        c = cfg.to_c()
        for dtype in DTYPES_OF[model]:
            h = hashlib.sha256()
            for batch in PLAN_BATCHES:
                h.update(b"%d=%d;" % (batch, lib.nesti_estimate_workspace_bytes_for_config(ctypes.byref(c), DTYPES[dtype], batch)))
            out["size/%s/%s" % (model, dtype)] = h.hexdigest()
            for tower, fast, x8 in _passes(model, dtype):
                for fmt in ((6, 8) if x8 else (0,)):
                    h = hashlib.sha256()
                    for batch in PLAN_BATCHES:
                        bufs, ops, wsb = layer_ref.tower_ops(lib, c, DTYPES[dtype], tower, batch, fast, x8, fmt)
                        h.update(b"batch %d ws %d tower %d;" % (batch, wsb, lib.nesti_tower_workspace_bytes(
                            ctypes.byref(c), DTYPES[dtype], tower, batch)))
                        for d in bufs + ops:
                            for k, v in d.items():       # the struct's field order (layer_ref.tower_ops), then in_pos
                                h.update(("%s=%s;" % (k, v.tolist() if isinstance(v, np.ndarray) else v)).encode())
                    out["plan/%s/%s/tower%d/fast%d/x8_%x/fmt%d" % (model, dtype, tower, fast, x8, fmt)] = h.hexdigest()
    return out


def test_plans_equal_the_recorded_ones():
    """Every plan -- buffer placement, launch description, workspace sizes; all six models, every dtype, every pass, ten batch sizes --
    is the one recorded in tests/golden/plan_digests.json.  No tolerance, no excluded case."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    got = plan_digests(_lib.load())
    want = json.load(open(PLAN_GOLDEN))
    assert sorted(got) == sorted(want)
    assert [k for k in sorted(want) if got[k] != want[k]] == []


def test_tower_ops_forms_follow_the_pass():
    """The filter pass runs its tap layers in plain f16 and its one-tap conv_igemm layers in the X2 form; the x8 mask switches
    exactly the four 8^3 tap layers of an expert to X6 (default) or X8 and turns their block's conv1 into producers."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    from nesti_net_amd.config import DTYPES, NestiConfig
    lib, c = _lib.load(), NestiConfig().to_c()
    _, ops, _ = layer_ref.tower_ops(lib, c, DTYPES["f16x3c"], -1, 37, 1, 0)
    for o in ops:
        if o["kind"] == layer_ref.OP_CONV:
            assert o["form"] == (layer_ref.FORM_X2 if o["family"] == 0 and o["n_taps"] == 1 else layer_ref.FORM_PLAIN) and o["elem"] == 2
    for fmt, form in ((0, layer_ref.FORM_X6), (6, layer_ref.FORM_X6), (8, layer_ref.FORM_X8)):
        bufs, ops, _ = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], 3, 37, 0, 0xF, fmt)
        x = [o for o in ops if o["form"] == form]
        assert [o["scope"] for o in x] == ["inception%dExpert_3_conv%d" % (b, k) for b in (1, 2) for k in (2, 3)]
        assert all(o["family"] == 2 and bufs[o["aux_in_buf"]]["aux8"] for o in x)
        prod = [o for o in ops if o["aux_out_buf"] >= 0]
        assert [o["scope"] for o in prod] == ["inception1Expert_3_conv1", "inception2Expert_3_conv1"]
    _, ops, _ = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], 3, 37, 0, 0)
    assert all(o["form"] == layer_ref.FORM_PAIR and o["aux_out_buf"] < 0 for o in ops if o["kind"] == layer_ref.OP_CONV)
    ps = _lib.CDebugPass(1, 0, 0)
    n = ctypes.c_int()
    assert lib.nesti_debug_tower_ops(ctypes.byref(c), DTYPES["f16x3"], -1, 8, ctypes.byref(ps), None, 0, ctypes.byref(n), None, 0,
                                     ctypes.byref(n), None, 0, None, None) != 0
    assert b"filter pass" in lib.nesti_last_error()


def test_weight_rules_hand_cases():
    """The emulated packer on values worked out by hand: BN folding in double cast to float, f16 / bf16 rounding of the
    folded weight, the f16x3 power-of-two scale and the pair split W_lo = rne(W - W_hi)."""
    W = {"s/weights": np.array([[[[[1.0, 3.0]]]]], np.float32), "s/biases": np.array([0.5, -1.0], np.float32),
         "s/bn/gamma": np.array([2.0, 1.0], np.float32), "s/bn/beta": np.array([0.25, 0.0], np.float32),
         "s/bn/mean": np.array([0.5, 1.0], np.float32), "s/bn/var": np.array([1.0 - 1e-3, 4.0 - 1e-3], np.float32)}
    w, b = layer_ref.fold(W, "s", True)
    inv = np.array([2.0 / np.sqrt(np.float64(np.float32(1.0 - 1e-3)) + 1e-3), 1.0 / np.sqrt(np.float64(np.float32(4.0 - 1e-3)) + 1e-3)])
    assert np.array_equal(w.reshape(-1), np.array([1.0, 3.0], np.float32) * inv.astype(np.float32))
    assert abs(b[0] - 0.25) < 1e-6 and abs(b[1] - (-2.0 / 2.0)) < 1e-6
    assert layer_ref.pair_exponent(1.0) == 13 and layer_ref.pair_exponent(3.0) == 12 and layer_ref.pair_exponent(0.0) == 0
    x = np.float32(1.0 + 2.0 ** -11)                    # a tie between two f16 neighbours: to even (1.0)
    assert layer_ref.f16_rne(x) == 1.0 and layer_ref.f16_rne(np.float32(1.0 + 3 * 2.0 ** -11)) == np.float32(1.0 + 2.0 ** -9)
    assert layer_ref.bf16_rne(np.float32(1.0 + 2.0 ** -8)) == 1.0 and layer_ref.bf16_rne(np.float32(1.0 + 3 * 2.0 ** -8)) == np.float32(1 + 2.0 ** -6)
    op = {"scope": "s", "scope2": "", "bn": True, "is_fc": False, "k": 1, "s_real": 0, "log2S": 3, "form": layer_ref.FORM_PAIR,
          "elem": layer_ref.F16}
    (p,) = layer_ref.effective_weights(W, op, "f16x3")
    v = (w * np.float32(2.0 ** 12)).astype(np.float32).reshape(-1)   # largest folded weight ~2.83: scale 2^12
    assert p["acc"] == 2.0 ** -12
    hi = v.astype(np.float16).astype(np.float32)
    assert np.array_equal(p["hi"].reshape(-1), hi) and np.array_equal(p["lo"].reshape(-1), (v - hi).astype(np.float16).astype(np.float32))
    assert np.all(np.abs(p["hi"] + p["lo"] - v.reshape(p["hi"].shape)) <= 2.0 ** -22 * np.abs(v.reshape(p["hi"].shape)))


def test_vectorised_encoders_match_the_library_and_the_format():
    """layer_ref.e2m3_encode against the library's nesti_f32_to_e2m3 on every code, every midpoint and scaled values;
    layer_ref.e4m3_encode against the e4m3 definition: every code round-trips, midpoints go to the even code, 448 saturates."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    grid = layer_ref.e2m3_grid()
    mids = 0.5 * (grid[1:] + grid[:-1])
    vals = np.concatenate([grid, -grid, mids, -mids, grid * 1.01, mids * 0.999, [7.6, 9.0, 1e30, -1e30, 0.06, 0.0626]])
    for s in (1.0, 0.25, 2.0 ** -7):
        x = (vals / s).astype(np.float32)
        want = np.array([lib.nesti_f32_to_e2m3(float(v), s) for v in x])
        assert np.array_equal(layer_ref.e2m3_encode(x, s), want), s
    codes = np.array([c for c in range(256) if (c & 0x7F) != 0x7F])
    dec = layer_ref.e4m3_decode(codes)
    enc = layer_ref.e4m3_encode(dec)
    assert np.array_equal(enc[codes != 0x80], codes[codes != 0x80]) and layer_ref.e4m3_decode(0x7E) == 448.0
    pos = layer_ref.e4m3_decode(np.arange(0x7F))
    m = 0.5 * (pos[1:] + pos[:-1])
    assert np.array_equal(layer_ref.e4m3_encode(m), np.where(np.arange(1, 0x7F) % 2 == 0, np.arange(1, 0x7F), np.arange(0, 0x7E)))
    assert layer_ref.e4m3_encode(1000.0) == 0x7E and layer_ref.e4m3_encode(-1000.0) == 0xFE


def test_side_buffer_decoding():
    """layer_ref.aux_decode on side-buffer rows built by hand: e4m3 planes [lo8 64 B | hi8 64 B] per 64-channel group, and FP6 blocks --
    32 six-bit elements packed little-endian (pack.cpp: cross_rows' bit layout), slot 2i = lo, 2i + 1 = hi, E8M0 scale in byte 24,
    the block's first 16 bytes where lo8 went and its second 16 where hi8 went."""
    import torch
    rng = np.random.default_rng(3)
    C = 128
    lo8, hi8 = rng.integers(0, 0x7F, (2, C)), rng.integers(0x80, 0xFF, (2, C))
    raw = np.zeros((2, 2 * C), np.uint8)
    for g in range(C // 64):
        raw[:, g * 128:g * 128 + 64] = lo8[:, g * 64:(g + 1) * 64]
        raw[:, g * 128 + 64:g * 128 + 128] = hi8[:, g * 64:(g + 1) * 64]
    a0, a1, _ = layer_ref.aux_decode(torch.as_tensor(raw), 8)
    assert np.array_equal(a0.numpy(), layer_ref.e4m3_decode(lo8)) and np.array_equal(a1.numpy(), layer_ref.e4m3_decode(hi8))
    codes = rng.integers(0, 64, (2, C // 16, 32))
    sb = rng.integers(120, 135, (2, C // 16))
    raw = np.zeros((2, 2 * C), np.uint8)
    for r in range(2):
        for q in range(C // 16):
            blk = np.zeros(32, np.int64)
            for j in range(32):
                pos = 6 * j
                w = int(codes[r, q, j]) << (pos & 7)
                blk[pos >> 3] |= w & 0xFF
                blk[(pos >> 3) + 1] |= w >> 8
            blk[24] = sb[r, q]
            g, c = q // 4, q % 4
            raw[r, g * 128 + 16 * c:g * 128 + 16 * c + 16] = blk[:16]
            raw[r, g * 128 + 64 + 16 * c:g * 128 + 64 + 16 * c + 16] = blk[16:]
    a0, a1, (dc, ds) = layer_ref.aux_decode(torch.as_tensor(raw), 6)
    assert np.array_equal(dc.numpy(), codes) and np.array_equal(ds.numpy(), sb)
    scale = np.ldexp(1.0, sb - 127)[..., None]
    assert np.array_equal(a0.numpy(), (layer_ref.e2m3_decode(codes[..., 0::2]) * scale).reshape(2, C))
    assert np.array_equal(a1.numpy(), (layer_ref.e2m3_decode(codes[..., 1::2]) * scale).reshape(2, C))


def test_cross_weights_reproduce_the_split():
    """The emulated cross-term weights stand for W_hi and W_lo = v - W_hi (FP8: within e4m3's 2^-4; FP6: within e2m3's 2^-4 of
    the block's largest |W_hi|)."""
    rng = np.random.default_rng(5)
    v = np.clip(rng.standard_normal((3, 3, 3, 40, 24)) * 4000, -16000, 16000).astype(np.float32)   # W_hi 2^-6 below e4m3's 448
    hi = layer_ref.f16_rne(v)
    pos = np.arange(40)
    for fmt in (8, 6):
        b0, b1 = layer_ref.x8_cross_weights(hi, v, pos, fmt)
        if fmt == 8:
            # relative 2^-4 for normal e4m3 codes, plus half the subnormal quantum (2^-10 before the 2^6 block scale)
            assert np.all(np.abs(b0 - hi) <= 2.0 ** -4 * np.abs(hi) + 2.0 ** -4)
            assert np.all(np.abs(b1 - (v - hi) * 2048.0) <= 2.0 ** -4 * np.abs(v - hi) * 2048 + 2.0 ** -4)
        else:
            blk = np.abs(np.pad(hi, [(0, 0)] * 3 + [(0, 8), (0, 0)])).reshape(3, 3, 3, 3, 16, 24).max(axis=4)[..., pos // 16, :]
            assert np.all(np.abs(b0 * 2048.0 - hi) <= 2.0 ** -4 * blk) and np.all(np.abs(b1 - (v - hi)) <= 2.0 ** -4 * blk)
