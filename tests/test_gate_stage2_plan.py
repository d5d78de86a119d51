"""Recheck stage 2 of the f16x8c gate, without a device: the gating net with its six k^3 tap layers at 8^3 in the FP6 cross-term form
(include/nesti_hip.h).  The plans of the new launch forms, the FP6 pack image of one of those tap layers against a byte-level
restatement written here, and the stage's place inside the forward workspace, whose size stays the parent's."""
import ctypes
import hashlib

import numpy as np

import layer_ref

# every batch size tests/test_layer_ops.py folds into its size digests (both sides of cascade_cap's 4096)
BATCHES = (1, 37, 1000, 2048, 2049, 4096, 4097, 8192, 8193, 100000)
GATE_TAPS = ["inception%dgating_conv_conv%d" % (b, k) for b in (1, 2, 3) for k in (2, 3)]
GATE_PRODUCERS = ["inception%dgating_conv_conv1" % b for b in (1, 2, 3)]
SIDE_C = (128, 256, 256)     # F of the three 8^3 inception blocks of the gating net: the channels of their side buffers


def _a256(n):
    return (n + 255) // 256 * 256


def _lib_cfg():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    from nesti_net_amd.config import DTYPES, NestiConfig
    return _lib, _lib.load(), NestiConfig(), DTYPES


def test_stage2_plan_forms_and_placement():
    """Mask 0x3F: the six 8^3 tap layers run FORM_X6 on conv8n's family and read the side buffer their block's conv1 | conv4 launch
    writes; every other launch, and every buffer of the plain pass, is unchanged; the three side buffers share one block right
    behind the plain pass's bytes.  Sub-masks switch whole blocks' producers and single layers."""
    _lib, lib, cfg, DTYPES = _lib_cfg()
    c = cfg.to_c()
    for batch in (5, 37, 1000):
        b0, o0, ws0 = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], -1, batch, 0, 0)
        b2, o2, ws2 = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], -1, batch, 0, 0x3F, 6)
        assert len(o2) == len(o0) and len(b2) == len(b0) + 3
        assert b2[:len(b0)] == b0                                       # the plain pass's buffers, where they were
        side = b2[len(b0):]
        assert [s["C"] for s in side] == list(SIDE_C) and all(s["aux8"] and s["log2S"] == 3 for s in side)
        assert all(s["offset"] == ws0 for s in side)                    # one block behind everything else
        assert [s["bytes"] for s in side] == [_a256((batch << 9) * C * 2) for C in SIDE_C]
        assert ws2 == ws0 + max(s["bytes"] for s in side)
        for i, s in enumerate(side):                                    # lifetimes apart: they may share the block
            for t in side[i + 1:]:
                assert s["last"] < t["first"]
        x6 = [o for o in o2 if o["form"] == layer_ref.FORM_X6]
        assert [o["scope"] for o in x6] == GATE_TAPS
        assert all(o["family"] == 2 and o["log2S"] == 3 and b2[o["aux_in_buf"]]["aux8"] for o in x6)
        prod = [o for o in o2 if o["aux_out_buf"] >= 0]
        assert [o["scope"] for o in prod] == GATE_PRODUCERS and all(o["form"] == layer_ref.FORM_PAIR and o["n_taps"] == 1 for o in prod)
        for blk in range(3):                                            # a block's tap layers read what its own producer writes
            assert x6[2 * blk]["aux_in_buf"] == x6[2 * blk + 1]["aux_in_buf"] == prod[blk]["aux_out_buf"] == len(b0) + blk
            assert x6[2 * blk]["aux_layer"] == x6[2 * blk + 1]["aux_layer"] == prod[blk]["layer"]
        for a, b in zip(o0, o2):                                        # nothing else moved
            for k in a:
                if k in ("form", "aux_in_buf", "aux_out_buf", "aux_layer", "in_pos", "scope", "scope2"):
                    continue
                assert a[k] == b[k], (a["scope"], k)
            if b["scope"] not in GATE_TAPS:
                assert a["form"] == b["form"]
            assert a["scope"] == b["scope"] and a["form"] == (layer_ref.FORM_PAIR if a["kind"] == layer_ref.OP_CONV else a["form"])
    _, o, _ = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], -1, 8, 0, 0b001000, 6)
    assert [x["scope"] for x in o if x["form"] == layer_ref.FORM_X6] == [GATE_TAPS[3]]
    assert [x["scope"] for x in o if x["aux_out_buf"] >= 0] == [GATE_PRODUCERS[1]]
    # refused: a model without the stage, format 8, the filter pass, a seventh bit
    n = ctypes.c_int()
    for dtype, fast, mask, fmt in (("f16x3c", 0, 0x3F, 6), ("f16x8", 0, 0x3F, 6), ("f16x8c", 0, 0x3F, 8), ("f16x8c", 1, 0x3F, 6),
                                   ("f16x8c", 0, 0x40, 6)):
        ps = _lib.CDebugPass(fast, mask, fmt)
        assert lib.nesti_debug_tower_ops(ctypes.byref(c), DTYPES[dtype], -1, 8, ctypes.byref(ps), None, 0, ctypes.byref(n), None, 0,
                                         ctypes.byref(n), None, 0, None, None) != 0, (dtype, fast, mask, fmt)


def _cascade_cap(nb):
    return nb if nb <= 4096 else _a256((nb + 3) // 4)


def test_stage2_lives_inside_the_tower_arena():
    """The stage takes no workspace: nesti_estimate_workspace_bytes_for_config(f16x8c) is the parent's at ten batch sizes (its recorded
    digest), and nesti_debug_gate_stage2_plan puts [stage-2 gating net of a round | residual list | its logits | margins] inside the
    arena, each part the size restated here, with the recheck's own round above 4096 rows and a round of at least 3/4 of the batch
    below (one that could not be a tile larger and still fit only when it is the recheck's own)."""
    _lib, lib, cfg, DTYPES = _lib_cfg()
    c = cfg.to_c()
    h = hashlib.sha256()
    for nb in BATCHES:
        h.update(b"%d=%d;" % (nb, lib.nesti_estimate_workspace_bytes_for_config(ctypes.byref(c), DTYPES["f16x8c"], nb)))
    assert h.hexdigest() == PARENT_F16X8C_SIZE_DIGEST
    for nb in BATCHES + (2, 3, 4, 5, 9, 256):
        S = _lib.CDebugStage2()
        _lib.check(lib.nesti_debug_gate_stage2_plan(ctypes.byref(c), DTYPES["f16x8c"], nb, ctypes.byref(S)), "nesti_debug_gate_stage2_plan")
        ecap = nb if nb <= 8192 else _a256((nb + 3) // 4)
        arena = max([lib.nesti_tower_workspace_bytes(ctypes.byref(c), DTYPES["f16x8c"], -1, nb),
                     lib.nesti_tower_workspace_bytes(ctypes.byref(c), DTYPES["f16x3"], -1, _cascade_cap(nb))] +
                    [lib.nesti_tower_workspace_bytes(ctypes.byref(c), DTYPES["f16x8c"], t, ecap) for t in range(cfg.n_experts)])
        assert S.arena_bytes == arena and S.arena_offset + arena == lib.nesti_estimate_workspace_bytes_for_config(
            ctypes.byref(c), DTYPES["f16x8c"], nb) - _a256(nb * cfg.n_scales * 4)
        if nb == 1:
            assert S.cap == 0 and S.rounds == 0          # the planes of one row do not fit beside its own f16x3 gate
            continue
        assert 0 < S.cap <= _cascade_cap(nb) and S.rounds == -(-nb // S.cap) and S.rounds <= 24
        assert S.cap == _cascade_cap(nb) if nb > 4096 else S.cap >= (3 * nb) // 4
        _, _, ws2 = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], -1, S.cap, 0, 0x3F, 6)
        assert S.tower_bytes == ws2 and S.residual == ws2
        assert S.logits2 == S.residual + _a256(S.cap * 4) and S.margin2 == S.logits2 + _a256(S.cap * 8 * 4)
        assert S.end == S.margin2 + _a256(nb * 4) and S.end <= S.arena_bytes
    for dt in ("f16x3c", "f16x8", "f16x3"):
        S = _lib.CDebugStage2()
        _lib.check(lib.nesti_debug_gate_stage2_plan(ctypes.byref(c), DTYPES[dt], 1000, ctypes.byref(S)), "nesti_debug_gate_stage2_plan")
        assert S.cap == 0


# SHA-256 over "batch=bytes;" of nesti_estimate_workspace_bytes_for_config(experts, f16x8c) at BATCHES as the commit BEFORE the stage
# reported it: what tests/golden/plan_digests.json holds under "size/experts/f16x8c"
PARENT_F16X8C_SIZE_DIGEST = "d52f9bd50d6384748e0a048c08fa2fc5c6547300b1bb9535c46c2f4b66b6fc22"


def _slot(row, s):
    """pack.cpp weight_slot for conv8n_kernel: 64-byte rows, 16-byte slots XOR-swizzled by (row >> 2) & 3."""
    return row * 64 + ((s ^ ((row >> 2) & 3)) << 4)


def x6_image(w, in_pos, Cin_p):
    """The FP6-form image of a k^3 tap layer at 8^3 with cout <= 64, restated from the format's description: per (16-channel chunk,
    tap) a tile of 64 rows (output columns) x 64 bytes -- [W_hi f16 x 16 | 32 e2m3 codes (W_hi / s, W_lo 2^11 / s interleaved per
    channel, 6 bits each, little-endian) , byte 24 of that half: the E8M0 code of s 2^-11, s = 2^(E - 2), E the exponent of the chunk's
    largest |W_hi|], slots swizzled.  w: BN-folded weights [k, k, k, cin, cout] float32."""
    k, cin, cout = w.shape[0], w.shape[3], w.shape[4]
    e = layer_ref.pair_exponent(float(np.abs(w).max()))
    v = (w * np.float32(2.0 ** e)).astype(np.float32).reshape(k ** 3, cin, cout)
    hi16 = v.astype(np.float16)
    hi = hi16.astype(np.float32)
    lo = (v - hi).astype(np.float32)
    n_chunks, n_taps = Cin_p // 16, k ** 3
    img = np.zeros((n_chunks, n_taps, 64 * 64), np.uint8)
    inv = np.full(Cin_p, -1)
    inv[np.asarray(in_pos)] = np.arange(cin)
    for ch in range(n_chunks):
        cr = inv[ch * 16:ch * 16 + 16]
        live = cr >= 0
        for t in range(n_taps):
            H = np.zeros((16, 64), np.float32)
            L = np.zeros((16, 64), np.float32)
            B16 = np.zeros((16, 64), np.uint16)
            H[live, :cout], L[live, :cout], B16[live, :cout] = hi[t, cr[live]], lo[t, cr[live]], hi16[t, cr[live]].view(np.uint16)
            tile = img[ch, t]
            for nl in range(64):
                hb = B16[:, nl].astype("<u2").tobytes()
                tile[_slot(nl, 0):_slot(nl, 0) + 16] = np.frombuffer(hb[:16], np.uint8)
                tile[_slot(nl, 1):_slot(nl, 1) + 16] = np.frombuffer(hb[16:], np.uint8)
                amax = float(np.abs(H[:, nl]).max())
                if not amax > 0:
                    continue
                sexp = int(np.frexp(np.float32(amax))[1]) - 3
                inv_s = np.float32(2.0 ** -sexp)
                codes = np.empty(32, np.int64)
                codes[0::2] = layer_ref.e2m3_encode(H[:, nl], inv_s)
                codes[1::2] = layer_ref.e2m3_encode(L[:, nl] * np.float32(2048.0), inv_s)
                bits = 0
                for i, cde in enumerate(codes):
                    bits |= int(cde) << (6 * i)
                blk = bytearray(bits.to_bytes(24, "little") + bytes(8))
                blk[24] = sexp - 11 + 127
                tile[_slot(nl, 2):_slot(nl, 2) + 16] = np.frombuffer(bytes(blk[:16]), np.uint8)
                tile[_slot(nl, 3):_slot(nl, 3) + 16] = np.frombuffer(bytes(blk[16:]), np.uint8)
    return img.reshape(-1), e


def test_fp6_pack_image_of_a_gate_tap_layer():
    """inception1gating_conv_conv2 (3^3 taps, 128 -> 64 channels) packed for the stage (FORM_X6) equals the restatement byte for
    byte, with the pair packing's accumulator scale and bias; its W_hi halves are the pair image's, which the stage leaves alone."""
    _lib, lib, cfg, DTYPES = _lib_cfg()
    from nesti_net_amd import weights
    W = weights.synthetic_weights(cfg, bn="random")
    keep = [np.ascontiguousarray(W[k], dtype=np.float32) for k in W]
    arr = (_lib.CTensor * len(keep))()
    for i, (k, a) in enumerate(zip(W, keep)):
        arr[i].name, arr[i].data, arr[i].ndim = k.encode(), a.ctypes.data, a.ndim
        for d in range(a.ndim):
            arr[i].dims[d] = a.shape[d]
    c = cfg.to_c()
    _, ops, _ = layer_ref.tower_ops(lib, c, DTYPES["f16x8c"], -1, 8, 0, 0x3F, 6)
    op = [o for o in ops if o["scope"] == GATE_TAPS[0]][0]
    assert op["k"] == 3 and op["cin"] == 128 and op["cout"] == 64 and op["Cin_p"] == 128

    def pack(form):
        info = _lib.CDebugPack()
        w, b = np.empty(1 << 21, np.uint8), np.empty(64, np.float32)
        _lib.check(lib.nesti_debug_pack_layer(ctypes.byref(c), arr, len(keep), DTYPES["f16x8c"], form, op["layer"], ctypes.byref(info),
                                              w.ctypes.data, w.size, b.ctypes.data, b.size), "nesti_debug_pack_layer")
        return info, w[:info.w_bytes], b[:info.n_bias]

    info, w6, b6 = pack(layer_ref.FORM_X6)
    wf, bias = layer_ref.fold(W, op["scope"], True)
    want, e = x6_image(wf, op["in_pos"], op["Cin_p"])
    assert (info.kind, info.TN, info.n_tiles, info.n_chunks, info.n_taps) == (2, 64, 1, 8, 27) and info.w_bytes == want.size
    assert info.acc_scale == 2.0 ** -e and np.array_equal(b6, bias)
    assert np.array_equal(w6, want), "%d of %d bytes differ" % (int((w6 != want).sum()), want.size)
    infop, wp, bp = pack(layer_ref.FORM_PAIR)
    assert infop.w_bytes == info.w_bytes and np.array_equal(bp, b6)
    t6, tp = w6.reshape(-1, 64, 4, 16), wp.reshape(-1, 64, 4, 16)
    key = (np.arange(64) >> 2) & 3
    for s in (0, 1):                                                    # the W_hi halves (logical slots 0, 1) are shared
        assert np.array_equal(t6[:, np.arange(64), s ^ key], tp[:, np.arange(64), s ^ key])
