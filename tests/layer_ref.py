"""Per-launch fp64 reference of the conv and pool launches of one tower (tests/test_gpu_layers.py, tests/test_layer_ops.py).

``tower_ops`` reads a tower's buffers and launches from the library (``nesti_debug_tower_ops``).  ``TowerChecker`` compares
ONE launch, run alone by ``nesti_debug_tower_step``, with an fp64 evaluation of the same layer on the launch's own input
buffer, decoded from the workspace.  The effective weights are emulated here from the TF tensors with the packer's VALUE rules
(pack.cpp: fold_layer, pack_layer), not read back from the packed buffers, so a packing bug and a kernel bug both show up.

Bound per output element: ``|gpu - ref| <= r_out(ref) + c 2^-24 S`` with ``S = sum |a w| + |b|`` over the products the form
multiplies, r_out the rounding of the output format, and ``c`` one constant per (kernel family, arithmetic form) -- ``C_BOUND``,
set from the measurements in profiles/layer_conformance.txt.  Pools must be bit-exact.  For every k^3 layer the check also
proves that it could see a missing tap: the effect of removing any single tap must exceed 8x the bound somewhere."""
import ctypes

import numpy as np
import torch

from oracle import net_ref

OP_CONV, OP_MAX, OP_MAX3 = 0, 1, 2                     # NESTI_DEBUG_OP_*
FORM_PLAIN, FORM_PAIR, FORM_X2, FORM_X8, FORM_X6 = range(5)   # NESTI_DEBUG_FORM_*
FORM_NAMES = {FORM_PLAIN: "plain", FORM_PAIR: "pair", FORM_X2: "x2", FORM_X8: "x8", FORM_X6: "x6"}
FAMILY_NAMES = {0: "conv_igemm", 2: "conv8n", 3: "conv4n", -1: "pool"}
F32, BF16, F16 = 0, 1, 2                               # NESTI_F32 / NESTI_BF16 / NESTI_F16 (include/nesti_hip.h)
BN_EPS = 1e-3
U = 2.0 ** -24
DETECT_RATIO = 8.0

# c of the bound per (kernel family, form, element type): >= 4x the largest max|err| / (2^-24 S) measured on an MI355X
# (profiles/layer_conformance.txt)
C_BOUND = {
    ("conv8n", "plain", "f32"): 40, ("conv8n", "plain", "f16"): 8, ("conv8n", "plain", "bf16"): 4,
    ("conv8n", "pair", "f16"): 40, ("conv8n", "pair", "bf16"): 16,
    ("conv4n", "plain", "f32"): 32, ("conv4n", "plain", "f16"): 8, ("conv4n", "plain", "bf16"): 4,
    ("conv4n", "pair", "f16"): 24, ("conv4n", "pair", "bf16"): 8,
    ("conv_igemm", "plain", "f32"): 48, ("conv_igemm", "plain", "f16"): 8, ("conv_igemm", "plain", "bf16"): 6,
    ("conv_igemm", "pair", "f16"): 24, ("conv_igemm", "pair", "bf16"): 12, ("conv_igemm", "x2", "f16"): 8,
    ("conv8n", "x8", "f16"): 32, ("conv8n", "x6", "f16"): 24,
}


def c_bound(family, form, elem):
    key = (FAMILY_NAMES[family], FORM_NAMES[form], {F32: "f32", F16: "f16", BF16: "bf16"}[elem])
    if key not in C_BOUND:
        raise KeyError("no measured bound constant for %s: measure it and add it to C_BOUND" % (key,))
    return C_BOUND[key]


# ---- number formats ---------------------------------------------------------------------------------------------------
def f16_rne(x):
    """float32 array -> float32 values rounded to f16 (IEEE RNE, as the host packer's _Float16 cast)."""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bf16_rne(x):
    """float32 array -> float32 values rounded to bf16 (RNE; pack.cpp: host_f32_to_bf16)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = np.where(nan, (u >> 16) | 0x40, r).astype(np.uint32) << 16
    return r.view(np.float32)


def round16(x, elem):
    return f16_rne(x) if elem == F16 else bf16_rne(x)


def e2m3_grid():
    """The 32 non-negative e2m3 values by code (sign in bit 5)."""
    return np.array([(m / 8.0) if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8)])


def e2m3_encode(x, inv_scale=1.0):
    """Vectorised pack.cpp host_f32_to_e2m3: code of x * inv_scale (float32 product), RNE on the piecewise-uniform grid,
    saturating at 7.5, sign in bit 5, NaN -> 31."""
    x = np.asarray(x, np.float32)
    a = np.abs(x) * np.float32(inv_scale)
    a = a.astype(np.float32)
    with np.errstate(invalid="ignore"):
        c_lo = np.rint(a * np.float32(8.0))
        c_mid = 16 + np.rint((a - np.float32(2.0)) * np.float32(4.0))
        c_hi = 24 + np.rint((np.minimum(a, np.float32(8.0)) - np.float32(4.0)) * np.float32(2.0))
        code = np.where(a < 2, c_lo, np.where(a < 4, c_mid, c_hi))
        code = np.where(np.isnan(a), 31, np.minimum(code, 31)).astype(np.int64)
    return code | np.where(np.signbit(x), 32, 0)


def e4m3_decode(code):
    """OCP e4m3 (bias 7, no infinities, 0x7f / 0xff = NaN) -> float64."""
    code = np.asarray(code, np.int64)
    s = np.where(code & 0x80, -1.0, 1.0)
    e, m = (code >> 3) & 15, code & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    return np.where((code & 0x7F) == 0x7F, np.nan, s * v)


def e4m3_encode(x):
    """Vectorised OCP e4m3 encoder: round to nearest even on the format's grid, saturating at 448, NaN -> 0x7f
    (pack.cpp: host_f32_to_e4m3)."""
    x = np.asarray(x, np.float64)
    pos = e4m3_decode(np.arange(0x7F))                                  # codes 0 .. 126, increasing
    a = np.minimum(np.abs(x), 448.0)
    i = np.clip(np.searchsorted(pos, a), 1, 126)
    lo, hi = pos[i - 1], pos[i]
    pick_hi = (a - lo > hi - a) | ((a - lo == hi - a) & ((i & 1) == 0))
    code = np.where(a <= 0, 0, np.where(pick_hi, i, i - 1))
    code = np.where(np.isnan(x), 0x7F, code | np.where(np.signbit(x), 0x80, 0))
    return code.astype(np.int64)


# ---- the packer's value rules -----------------------------------------------------------------------------------------
def fold(W, scope, bn):
    """(w float32 [..., cin, cout] * scale, bias) as pack.cpp fold_layer + pack_layer: scale and bias in double cast to
    float, the weight times the scale in float."""
    w = np.asarray(W[scope + "/weights"], np.float32)
    b = np.asarray(W[scope + "/biases"], np.float32)
    if not bn:
        return w * np.float32(1.0), b.astype(np.float32)
    g, v = np.asarray(W[scope + "/bn/gamma"], np.float64), np.asarray(W[scope + "/bn/var"], np.float64)
    inv = g / np.sqrt(v + BN_EPS)
    bias = ((b.astype(np.float64) - np.asarray(W[scope + "/bn/mean"], np.float64)) * inv
            + np.asarray(W[scope + "/bn/beta"], np.float64)).astype(np.float32)
    return w * inv.astype(np.float32), bias


def pair_exponent(wmax):
    """pack_layer (NESTI_F16X3): the power of two that brings the largest folded weight into [2^13, 2^14)."""
    if not (wmax > 0 and np.isfinite(wmax)):
        return 0
    _, e = np.frexp(np.float32(wmax))
    return int(min(24, max(-8, 14 - int(e))))


def kept_taps(k, S):
    lo = (k - 1) // 2
    return [(a, b, c) for a in range(k) for b in range(k) for c in range(k)
            if abs(a - lo) < S and abs(b - lo) < S and abs(c - lo) < S]


def effective_weights(W, op, model_dtype):
    """The weights one launch multiplies, per part (scope, scope2), as float64 tensors [k, k, k, cin, cout] plus the
    accumulator scale and the f32 bias: {'hi': W_hi, 'lo': W_lo or None, 'acc': acc_scale, 'bias': [...]}.
    model_dtype: the model's main element form -- 'f32', 'f16', 'bf16', 'f16x3', 'bf16x3'."""
    scopes = [op["scope"]] + ([op["scope2"]] if op["scope2"] else [])
    folded = [fold(W, s, op["bn"]) for s in scopes]
    if op["is_fc"]:
        folded = [(w.reshape(1, 1, 1, *w.shape), b) for w, b in folded]
    S = op["s_real"] or (1 << op["log2S"])
    taps = kept_taps(op["k"], S)
    form, elem = op["form"], op["elem"]
    pair_packed = form in (FORM_PAIR, FORM_X2, FORM_X8, FORM_X6)
    e = 0
    if pair_packed and model_dtype == "f16x3":
        wmax = max(float(np.max(np.abs(np.stack([w[t] for t in taps])))) for w, _ in folded)
        e = pair_exponent(wmax)
    out = []
    for w, b in folded:
        v = (w * np.float32(2.0 ** e)).astype(np.float32)
        mask = np.zeros(w.shape[:3], bool)
        for t in taps:
            mask[t] = True
        if elem == F32:
            hi, lo = v, None
        elif pair_packed:
            el = F16 if model_dtype == "f16x3" else BF16
            hi = round16(v, el)
            lo = round16(v - hi, el)
        else:
            hi, lo = round16(v, elem), None
        hi = np.where(mask[..., None, None], hi, 0)
        lo = None if lo is None else np.where(mask[..., None, None], lo, 0)
        out.append({"hi": hi.astype(np.float64), "lo": None if lo is None else lo.astype(np.float64),
                    "acc": 2.0 ** -e, "bias": b.astype(np.float64), "hi32": hi, "v": np.where(mask[..., None, None], v, 0)})
    return out


# ---- the library's description of a tower -----------------------------------------------------------------------------
def tower_ops(lib, cfg_c, dtype_code, tower, batch, fast=0, x8_mask=0, x8_fmt=0):
    """nesti_debug_tower_ops -> (bufs: list of dicts, ops: list of dicts with 'in_pos' arrays, workspace bytes)."""
    from nesti_net_amd import _lib
    ps = _lib.CDebugPass(fast, x8_mask, x8_fmt)
    nb, no, npos, wsb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _lib.check(lib.nesti_debug_tower_ops(ctypes.byref(cfg_c), dtype_code, tower, batch, ctypes.byref(ps), None, 0, ctypes.byref(nb),
                                         None, 0, ctypes.byref(no), None, 0, ctypes.byref(npos), ctypes.byref(wsb)),
               "nesti_debug_tower_ops")
    B, O = (_lib.CDebugBuf * nb.value)(), (_lib.CDebugOp * no.value)()
    P = np.zeros(max(1, npos.value), np.int32)
    _lib.check(lib.nesti_debug_tower_ops(ctypes.byref(cfg_c), dtype_code, tower, batch, ctypes.byref(ps), B, nb.value,
                                         ctypes.byref(nb), O, no.value, ctypes.byref(no), P.ctypes.data, npos.value,
                                         ctypes.byref(npos), ctypes.byref(wsb)), "nesti_debug_tower_ops")
    bufs = [{f: getattr(b, f) for f, _ in _lib.CDebugBuf._fields_} for b in B]
    ops = []
    for o in O:
        d = {f: getattr(o, f) for f, _ in _lib.CDebugOp._fields_}
        d["scope"] = (d["scope"] or b"").decode()
        d["scope2"] = (d["scope2"] or b"").decode()
        d["in_pos"] = P[d["in_pos_off"]:d["in_pos_off"] + d["cin"]].copy() if d["kind"] == OP_CONV else None
        ops.append(d)
    return bufs, ops, wsb.value


def op_name(op):
    if op["kind"] != OP_CONV:
        return "%s(C=%d, S=2^%d)" % ({OP_MAX: "maxpool2", OP_MAX3: "maxpool3s2"}[op["kind"]], op["C"], op["log2S"])
    return "%s%s [%s/%s k=%d]" % (op["scope"], "|" + op["scope2"] if op["scope2"] else "", FAMILY_NAMES[op["family"]],
                                  FORM_NAMES[op["form"]], op["k"])


# ---- workspace decoding -----------------------------------------------------------------------------------------------
def split_cols(cols):
    """Logical column -> physical element of its hi plane in the pair layout (common.h: split_col)."""
    cols = np.asarray(cols)
    return (cols >> 6) * 128 + (cols & 63)


_TD = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


class Decoder:
    """Typed views of the buffers of one tower in a workspace (torch uint8 on the device) and the MuPS tensor."""

    def __init__(self, bufs, ws, x0, nb):
        self.bufs, self.ws, self.nb = bufs, ws, nb
        self.x0 = x0.contiguous().reshape(-1).view(torch.uint8)    # the MuPS tensor, as bytes

    def raw(self, b, cstride=None, rows=None):
        """[rows, cstride * planes] elements of buffer b (a flattened view when cstride / rows are given)."""
        d = self.bufs[b]
        cs = (cstride or d["C"]) * d["planes"]
        rows = rows if rows is not None else self.nb << (3 * d["log2S"])
        esz = 4 if d["elem"] == F32 else 2
        if b == 0:
            return self.x0[:rows * cs * esz].view(_TD[d["elem"]]).reshape(rows, cs)
        off = d["offset"]
        return self.ws[off:off + rows * cs * esz].view(_TD[d["elem"]]).reshape(rows, cs)

    def cols(self, b, cols, hi_only=False, cstride=None, rows=None):
        """float64 [rows, len(cols)] of logical columns (pair layout: hi + lo, or the hi plane alone)."""
        r = self.raw(b, cstride, rows)
        cols = torch.as_tensor(np.asarray(cols), device=r.device, dtype=torch.long)
        if self.bufs[b]["planes"] == 1:
            return r[:, cols].double()
        pc = torch.as_tensor(split_cols(cols.cpu().numpy()), device=r.device)
        v = r[:, pc].double()
        return v if hi_only else v + r[:, pc + 64].double()

    def phys(self, b, cols):
        """Physical element indices (every plane) of logical columns of buffer b."""
        cols = np.asarray(cols)
        if self.bufs[b]["planes"] == 1:
            return cols
        pc = split_cols(cols)
        return np.concatenate([pc, pc + 64])


# ---- fp64 evaluation: oracle/net_ref.py's SAME taps and pools, on the device --------------------------------------------
def r_out_rel(op):
    """Relative rounding of the output format."""
    if op["out_f32"] or op["elem"] == F32:
        return 0.0, 0.0
    if op["planes"] == 2:     # the pair split: lo = rne(v - hi) leaves half an ulp of lo
        return (2.0 ** -22, 2.0 ** -25) if op["elem"] == F16 else (2.0 ** -16, 1e-38)
    return (2.0 ** -11, 2.0 ** -25) if op["elem"] == F16 else (2.0 ** -8, 1e-38)


class ConvRef:
    """fp64 reference of one conv launch as a sum of terms (activations X, weights W) -- one term per product the form
    multiplies: per part the pre-activation, S (sum of |products| + |b|), and the contribution of each tap."""

    def __init__(self, op, parts, dev):
        """parts: per part {'terms': [(X float64 [P, S, S, S, cin] on dev, W [k, k, k, cin, cout])], 'acc': scale, 'bias': [cout]}."""
        self.op, self.terms, self.acc = op, [], []
        self.pre, self.S = [], []
        for p in parts:
            terms = [(x, torch.as_tensor(w, device=dev)) for x, w in p["terms"]]
            b = torch.as_tensor(p["bias"], device=dev)
            pre = sum(net_ref.conv3d_same_taps(x, w, 0.0) for x, w in terms) * p["acc"]
            sab = sum(net_ref.conv3d_same_taps(x.abs(), w.abs(), 0.0) for x, w in terms) * p["acc"]
            if op["pool_k"] > 1 and p is parts[-1] and len(parts) == 2:
                pre, sab = net_ref.avg_pool3d_same(pre, op["pool_k"]), net_ref.avg_pool3d_same(sab, op["pool_k"])
            self.terms.append(terms)
            self.acc.append(p["acc"])
            self.pre.append(pre + b)
            self.S.append(sab + b.abs())

    def tap_effects(self, post, bound):
        """min over taps of max over outputs |post(pre) - post(pre - contribution of the tap)| / bound (part 0: the tap layers
        are single-part) -> (ratio, tap)."""
        terms, acc, pre = self.terms[0], self.acc[0], self.pre[0]
        ref = post(pre)
        worst = (np.inf, None)
        for slices in zip(*[net_ref.same_taps(x, self.op["k"]) for x, _ in terms]):
            t = slices[0][0]
            if not any(bool((w[t] != 0).any()) for _, w in terms):
                continue                                  # a tap that never lands inside the volume (not packed)
            c = sum(xs @ w[t] for (_, xs), (_, w) in zip(slices, terms))
            r = float(((ref - post(pre - c.reshape(pre.shape) * acc)).abs() / bound).max())
            if r < worst[0]:
                worst = (r, t)
        return worst


# ---- the cross terms of the X8 / X6 forms ---------------------------------------------------------------------------------
def e2m3_decode(code):
    code = np.asarray(code) if not torch.is_tensor(code) else code
    g = e2m3_grid()
    if torch.is_tensor(code):
        g = torch.as_tensor(g, device=code.device)
        return torch.where((code & 32) != 0, -1.0, 1.0).double() * g[(code & 31).long()]
    return np.where(code & 32, -1.0, 1.0) * g[code & 31]


def x8_activation_exponent(W, scope, bn):
    """pack.cpp x8_activation_exponent: the pre-scale 2^sc of a producer's planes, from its batch norm."""
    amax = np.float32(16.0)
    if bn:
        beta, gamma = np.asarray(W[scope + "/bn/beta"], np.float32), np.asarray(W[scope + "/bn/gamma"], np.float32)
        amax = np.max(np.abs(beta) + np.float32(8.0) * np.abs(gamma)).astype(np.float32)
    if not (amax > 0 and np.isfinite(amax)):
        amax = np.float32(16.0)
    _, e = np.frexp(np.float32(amax))
    return int(min(20, max(-8, 8 - int(e))))


def x8_cross_weights(hi, v, in_pos, fmt):
    """The two cross-term weight operands of pack.cpp cross_rows as the values the MFMA multiplies, per real input channel:
    (B0 ~ W_hi, paired with the activations' lo; B1 ~ W_lo, paired with the activations' full value), each with its block scale
    folded in and in the units the decoded activation operands below use.  hi = f16(v), v = the pair packing's scaled weight."""
    if fmt == 8:                                          # W_hi8 = e4m3(W_hi 2^-6), W_lo8 = e4m3((v - W_hi) 2^5), block scale 2^6
        b0 = e4m3_decode(e4m3_encode((hi * np.float32(2.0 ** -6)).astype(np.float32))) * 2.0 ** 6
        b1 = e4m3_decode(e4m3_encode(((v - hi) * np.float32(2.0 ** 5)).astype(np.float32))) * 2.0 ** 6
        return b0, b1
    # FP6: per (tap, 16-channel block of padded input positions, column) s = 2^(E - 2), E = exponent of the block's largest |W_hi|;
    # slots W_hi / s and (v - W_hi) 2^11 / s, the scale byte s 2^-11
    k, cout = hi.shape[0], hi.shape[4]
    nblk = (int(np.max(in_pos)) // 16) + 1
    hp = np.zeros((k, k, k, nblk * 16, cout), np.float32)
    hp[..., in_pos, :] = hi
    amax = np.abs(hp).reshape(k, k, k, nblk, 16, cout).max(axis=4)
    _, e = np.frexp(amax)
    sexp = np.where(amax > 0, e - 3, 0)
    sexp_c = sexp[..., np.asarray(in_pos) // 16, :]      # [k, k, k, cin, cout]
    inv_s = np.ldexp(np.float32(1.0), -sexp_c).astype(np.float32)
    scale = np.where(amax[..., np.asarray(in_pos) // 16, :] > 0, np.ldexp(1.0, sexp_c - 11), 0.0)
    lo11 = ((v - hi) * np.float32(2048.0)).astype(np.float32)
    b0 = e2m3_decode(e2m3_encode(hi * inv_s, 1.0)) * scale
    b1 = e2m3_decode(e2m3_encode(lo11 * inv_s, 1.0)) * scale
    return b0, b1


def aux_decode(raw, fmt):
    """Side-buffer rows [rows, 2 C] uint8 -> (A0, A1) float64 [rows, C]: the activation operands of the cross terms, pre-scales
    undone -- FP8: A0 = dec(lo8) (the activation's lo 2^sa), A1 = dec(hi8) (its value 2^sc); FP6: A0 = dec(slot 2i) s (lo 2^11),
    A1 = dec(slot 2i + 1) s (hi), s the block's E8M0 scale -- and for FP6 the block scale bytes [rows, C / 16]."""
    rows, C = raw.shape[0], raw.shape[1] // 2
    g = raw.reshape(rows, C // 64, 2, 64).long()
    if fmt == 8:
        lo8, hi8 = g[:, :, 0].reshape(rows, C), g[:, :, 1].reshape(rows, C)
        return (torch.as_tensor(e4m3_decode(lo8.cpu().numpy()), device=raw.device),
                torch.as_tensor(e4m3_decode(hi8.cpu().numpy()), device=raw.device), None)
    blk = torch.cat([g[:, :, 0].reshape(rows, C // 64, 4, 16), g[:, :, 1].reshape(rows, C // 64, 4, 16)], dim=3)   # [.., 32 B]
    sbyte = blk[..., 24]
    j = torch.arange(32, device=raw.device)
    byte, sh = (6 * j) >> 3, (6 * j) & 7
    word = blk[..., byte] | (blk[..., (byte + 1).clamp_max(31)] << 8)
    codes = (word >> sh) & 63                                                  # [rows, C/64, 4, 32]
    scale = torch.ldexp(torch.ones_like(sbyte, dtype=torch.float64), sbyte - 127)[..., None]
    a0 = (e2m3_decode(codes[..., 0::2]) * scale).reshape(rows, C)
    a1 = (e2m3_decode(codes[..., 1::2]) * scale).reshape(rows, C)
    return a0, a1, (codes.reshape(rows, C // 16, 32), sbyte.reshape(rows, C // 16))


def code_match(got, want, x, unc, mag_mask, dec):
    """Codes equal, or (both zero of either sign), or one magnitude step apart where the encoded value x lies within its own
    uncertainty `unc` of the boundary between the two codes' values."""
    gm, wm = got & mag_mask, want & mag_mask
    ok = (got == want) | ((gm == 0) & (wm == 0))
    step = (np.abs(gm - wm) == 1) & ((got & ~mag_mask) == (want & ~mag_mask))
    mid = 0.5 * (np.abs(dec(got)) + np.abs(dec(want)))
    return ok | (step & (np.abs(np.abs(x) - mid) <= unc))


class TowerChecker:
    """Runs one tower launch by launch on a fresh workspace and checks every launch (see the module docstring)."""

    def __init__(self, lib, net, W, model_dtype, tower, nb, x0, fast=0, x8_mask=0, x8_fmt=0, fill=0x00,
                 point_index=None, count=None, walk=0, stats=None):
        from nesti_net_amd import _lib
        from nesti_net_amd.config import DTYPES
        self.lib, self.net, self.W, self.model_dtype, self.tower, self.nb = lib, net, W, model_dtype, tower, nb
        self.dev = net.device
        self.pass_ = _lib.CDebugPass(fast, x8_mask, x8_fmt)
        self.bufs, self.ops, wsb = tower_ops(lib, net._c, DTYPES[net.dtype], tower, nb, fast, x8_mask, x8_fmt)
        self.ws = torch.full((max(wsb, 256),), fill, dtype=torch.uint8, device=self.dev)
        self.x0, self.x0_points = x0, x0.shape[0]
        self.point_index, self.count, self.walk = point_index, count, walk
        self.live = nb if count is None else int(count)
        self.cnt_dev = None if count is None else torch.tensor([int(count)], dtype=torch.int32, device=self.dev)
        self.idx_dev = None if point_index is None else torch.as_tensor(np.asarray(point_index, np.int32), device=self.dev)
        self.dec = Decoder(self.bufs, self.ws, x0, nb)
        self.stats = stats if stats is not None else {}
        self.where = "tower %s, %s" % ("gate" if tower < 0 else "expert %d" % tower, net.dtype + (" filter pass" if fast else ""))

    def step(self, i):
        from nesti_net_amd import _lib
        st = torch.cuda.current_stream(self.dev)
        _lib.check(self.lib.nesti_debug_tower_step(self.net._handle, self.tower, ctypes.byref(self.pass_), i, _lib.ptr(self.x0), self.nb,
                                                   _lib.ptr(self.idx_dev), _lib.ptr(self.cnt_dev), self.walk, _lib.ptr(self.ws),
                                                   self.ws.numel(), ctypes.c_void_p(st.cuda_stream)),
                   "nesti_debug_tower_step(%s, op %d)" % (self.where, i))

    def written(self, i):
        """(buffer, logical columns, rows per point) of everything launch i writes."""
        op = self.ops[i]
        out = []
        if op["kind"] != OP_CONV:
            out.append((op["out_buf"], np.arange(op["out_coff"], op["out_coff"] + op["C"])))
            return out
        nparts = 2 if op["scope2"] else 1
        width = op["Cout_p"] // nparts
        c1 = np.arange(op["out_coff"], op["out_coff"] + width)
        if op["mp_mode"] != 1:
            out.append((op["out_buf"], c1))
        if op["mp_buf"] >= 0:
            out.append((op["mp_buf"], c1))
        if nparts == 2:
            c2 = np.arange(op["out_coff2"], op["out_coff2"] + width)
            out.append((op["mp_buf"] if op["mp_mode2"] == 1 else op["out_buf"], c2))
        return out

    def snapshot(self, i):
        """Raw bits of every element launch i wrote on live rows."""
        snap = []
        if self.ops[i]["kind"] == OP_CONV and self.ops[i]["aux_out_buf"] >= 0:
            snap.append(self._aux_raw(self.ops[i]["aux_out_buf"]).clone())
        for b, cols in self.written(i):
            d = self.bufs[b]
            rows = self.live << (3 * d["log2S"])
            r = self.dec.raw(b)[:rows]
            v = r[:, torch.as_tensor(self.dec.phys(b, cols), device=self.dev)]
            snap.append(v.view(torch.int16) if v.element_size() == 2 else v.view(torch.int32))
        return snap

    # ---- input of a launch -------------------------------------------------------------------------------------------
    def _input(self, op):
        S = 1 << op["log2S"]
        b = op["in_buf"]
        hi_only = op["form"] in (FORM_PLAIN, FORM_X2) and op["in_planes"] == 2
        cols = op["in_coff"] + op["in_pos"]
        if op["is_fc"]:
            xa = self.dec.cols(b, cols, hi_only, cstride=op["in_cstride"], rows=self.nb)
            xa = xa[:self.live].reshape(self.live, 1, 1, 1, -1)
            xh = self.dec.cols(b, cols, True, cstride=op["in_cstride"], rows=self.nb)[:self.live].reshape(self.live, 1, 1, 1, -1)
            return xa, xh
        rows_pp = S ** 3
        xa = self.dec.cols(b, cols, hi_only, rows=self._rows(b))
        xh = self.dec.cols(b, cols, True, rows=self._rows(b))
        if b == 0 and self.idx_dev is not None:
            idx = self.idx_dev[:self.live].long()
            xa = xa.reshape(-1, rows_pp, xa.shape[-1])[idx]
            xh = xh.reshape(-1, rows_pp, xh.shape[-1])[idx]
        xa = xa[:self.live * rows_pp].reshape(self.live, S, S, S, -1)
        xh = xh[:self.live * rows_pp].reshape(self.live, S, S, S, -1)
        sr = op["s_real"]
        if sr:
            xa, xh = xa[:, :sr, :sr, :sr].contiguous(), xh[:, :sr, :sr, :sr].contiguous()
        return xa, xh

    def _rows(self, b):
        d = self.bufs[b]
        if b == 0:
            return self.x0_points << (3 * d["log2S"])
        return self.nb << (3 * d["log2S"])

    def _out(self, b, cols, log2S, sr=0):
        """GPU output of logical columns, float64 [live, S, S, S, n] (dead voxels of the 3^3 grid cut away)."""
        S = 1 << log2S
        v = self.dec.cols(b, cols)[:self.live << (3 * log2S)].reshape(self.live, S, S, S, -1)
        return v[:, :sr, :sr, :sr] if sr else v

    def _fail(self, i, what, err, bound, shape_cols):
        op = self.ops[i]
        r = (err / bound)
        j = int(torch.argmax(r))
        idx = np.unravel_index(j, tuple(r.shape))
        raise AssertionError("%s, op %d %s: %s -- worst element point %d voxel %s channel %d: |err| %.4g, bound %.4g (ratio %.3g)"
                             % (self.where, i, op_name(op), what, idx[0], tuple(int(v) for v in idx[1:4]), int(shape_cols[idx[4]]),
                                float(err.reshape(-1)[j]), float(bound.reshape(-1)[j]), float(r.reshape(-1)[j])))

    def _aux_raw(self, b):
        d = self.bufs[b]
        rows, rb = self.live << (3 * d["log2S"]), 2 * d["C"]
        return self.ws[d["offset"]:d["offset"] + rows * rb].reshape(rows, rb)

    def _producer(self, op):
        return next(o for o in self.ops if o["kind"] == OP_CONV and o["layer"] == op["aux_layer"])

    def _cross_input(self, op, fmt):
        """The cross-term activation operands a consumer reads from its side buffer, [live, 8, 8, 8, cin]."""
        a0, a1, _ = aux_decode(self._aux_raw(op["aux_in_buf"]), fmt)
        if fmt == 8:                                          # the block scale 2^-sa, sa = sc + 11, undoes both pre-scales
            prod = self._producer(op)
            sa = x8_activation_exponent(self.W, prod["scope"], prod["bn"]) + 11
            a0, a1 = a0 * 2.0 ** -sa, a1 * 2.0 ** -sa
        cols = torch.as_tensor(op["in_coff"] + op["in_pos"], device=self.dev).long()
        S = 1 << op["log2S"]
        return tuple(a[:, cols].reshape(self.live, S, S, S, -1) for a in (a0, a1))

    def check_producer(self, i):
        """The side buffer a producer wrote holds the encoding, under the documented pre-scale / block-scale rule, of the values the
        same launch wrote: one code step allowed only where the value lies within 2^-20 relative of a rounding boundary.  The lo
        operand is the exception: the launch's pair output holds v - f16(v) rounded to f16 (half an ulp: 2^-11 relative, 2^-25
        absolute below f16's normal range), while the planes encode it exact, so its boundary band is that rounding."""
        op = self.ops[i]
        fmt = 8 if self.pass_.x8_fmt == 8 else 6
        b = op["aux_out_buf"]
        C = self.bufs[b]["C"]
        cols = np.arange(op["out_coff"], op["out_coff"] + C)
        rows = self.live << (3 * op["log2S"])
        hi = self.dec.cols(op["out_buf"], cols, hi_only=True)[:rows].cpu().numpy()
        v = self.dec.cols(op["out_buf"], cols)[:rows].cpu().numpy()
        lo = v - hi
        raw = self._aux_raw(b)
        bad = []
        if fmt == 8:
            sc = x8_activation_exponent(self.W, op["scope"], op["bn"])
            g = raw.reshape(rows, C // 64, 2, 64).long().cpu().numpy()
            got_lo, got_hi = g[:, :, 0].reshape(rows, C), g[:, :, 1].reshape(rows, C)
            xl, xv = lo * 2.0 ** (sc + 11), v * 2.0 ** sc
            unc_l = (2.0 ** -11 * np.abs(lo) + 2.0 ** -25) * 2.0 ** (sc + 11)
            unc_v = (2.0 ** -20 * np.abs(v) + 2.0 ** -25) * 2.0 ** sc
            bad.append(("lo8", ~code_match(got_lo, e4m3_encode(xl), xl, unc_l, 0x7F, e4m3_decode)))
            bad.append(("hi8", ~code_match(got_hi, e4m3_encode(xv), xv, unc_v, 0x7F, e4m3_decode)))
        else:
            _, _, (codes, sbyte) = aux_decode(raw, 6)
            codes, sbyte = codes.cpu().numpy(), sbyte.cpu().numpy()
            amax = np.abs(hi).reshape(rows, C // 16, 16).max(axis=2).astype(np.float32)
            want_sb = np.maximum((amax.view(np.uint32) >> 23).astype(np.int64) - 2, 1)
            if not np.array_equal(sbyte, want_sb):
                r, q = np.argwhere(sbyte != want_sb)[0]
                raise AssertionError("%s, op %d %s: producer block scale byte %d at row %d block %d, expected %d"
                                     % (self.where, i, op_name(op), sbyte[r, q], r, q, want_sb[r, q]))
            inv = np.ldexp(1.0, 127 - want_sb)[..., None]
            xh = (hi.reshape(rows, C // 16, 16) * inv)
            xl = (lo.reshape(rows, C // 16, 16) * 2048.0 * inv)
            unc_l = (2.0 ** -11 * np.abs(lo.reshape(rows, C // 16, 16)) + 2.0 ** -25) * 2048.0 * inv
            bad.append(("FP6 hi slot", ~code_match(codes[..., 1::2], e2m3_encode(xh.astype(np.float32)), xh, 2.0 ** -20 * np.abs(xh), 31,
                                                   e2m3_decode)))
            bad.append(("FP6 lo slot", ~code_match(codes[..., 0::2], e2m3_encode(xl.astype(np.float32)), xl, unc_l, 31, e2m3_decode)))
        for what, m in bad:
            if m.any():
                r = np.argwhere(m)[0]
                raise AssertionError("%s, op %d %s: %d producer %s codes differ from the encoding of the launch's own outputs (first at %s)"
                                     % (self.where, i, op_name(op), int(m.sum()), what, tuple(int(t) for t in r)))
        key = ("producer", "x%d" % fmt)
        self.stats[key] = self.stats.get(key, 0) + int(m.size)

    # ---- the checks --------------------------------------------------------------------------------------------------
    def check_pool(self, i):
        op = self.ops[i]
        cols = np.arange(op["in_coff"], op["in_coff"] + op["C"])
        ocols = np.arange(op["out_coff"], op["out_coff"] + op["C"])
        S = 1 << op["log2S"]
        x = self.dec.cols(op["in_buf"], cols)[:self.live * S ** 3].reshape(self.live, S, S, S, -1)
        if op["kind"] == OP_MAX3:
            ref = net_ref.max_pool3d_3s2_same(x[:, :3, :3, :3])
            got = self._out(op["out_buf"], ocols, 1)
        else:
            ref = net_ref.max_pool3d_2(x)
            got = self._out(op["out_buf"], ocols, op["log2S"] - 1)
        bad = got != ref
        if bool(bad.any()):
            self._fail(i, "pool output is not bit-exact against the pooling of its own input", (got - ref).abs(),
                       torch.full_like(got, 1e-300), ocols)

    def check_conv(self, i):
        op = self.ops[i]
        parts = effective_weights(self.W, op, self.model_dtype)
        xa, xh = self._input(op)
        form = op["form"]
        for p in parts:
            if form == FORM_PLAIN:
                p["terms"] = [(xa, p["hi"])]
            elif form == FORM_X2:                             # hi (W_hi + W_lo): plain activations, the pair-packed weights
                p["terms"] = [(xa, p["hi"]), (xa, p["lo"])]
            elif form == FORM_PAIR:                           # hi W_hi + lo W_hi + hi W_lo
                p["terms"] = [(xa, p["hi"]), (xh, p["lo"])]
            else:                                             # hi W_hi in f16, then lo W_hi + v W_lo through the narrow codes
                fmt = 8 if form == FORM_X8 else 6
                a0, a1 = self._cross_input(op, fmt)
                b0, b1 = x8_cross_weights(p["hi32"], p["v"], op["in_pos"], fmt)
                p["terms"] = [(xh, p["hi"]), (a0, b0), (a1, b1)]
        ref = ConvRef(op, parts, self.dev)
        rel, tiny = r_out_rel(op)
        c = c_bound(op["family"], op["form"], op["elem"])
        key = (FAMILY_NAMES[op["family"]], FORM_NAMES[op["form"]], {F32: "f32", F16: "f16", BF16: "bf16"}[op["elem"]])
        relu = (lambda t: torch.relu(t)) if op["relu"] else (lambda t: t)
        sr = op["s_real"]
        nparts = len(parts)
        lg = op["log2S"]
        for part in range(nparts):
            pre, Sab = ref.pre[part], ref.S[part]
            cout = pre.shape[-1]
            acc_b = c * U * Sab
            bound = rel * (pre.abs() + acc_b) + tiny + acc_b
            ref_post = relu(pre)
            coff = op["out_coff"] if part == 0 else op["out_coff2"]
            cols = np.arange(coff, coff + cout)
            pooled_only = op["mp_mode"] == 1 if part == 0 else op["mp_mode2"] == 1
            pooled = op["mp_buf"] >= 0 and (part == 0 or op["mp_mode2"] == 1)
            checks = []
            if not pooled_only:
                if op["is_fc"]:
                    got = self.dec.cols(op["out_buf"], cols)[:self.live].reshape(self.live, 1, 1, 1, -1)
                else:
                    got = self._out(op["out_buf"], cols, lg, sr)
                checks.append(("full resolution", got, ref_post, bound, Sab))
            if pooled:
                gotp = self._out(op["mp_buf"], cols, lg - 1)
                checks.append(("fused max-pool", gotp, net_ref.max_pool3d_2(ref_post), net_ref.max_pool3d_2(bound), net_ref.max_pool3d_2(Sab)))
                if not pooled_only:
                    full = self._out(op["out_buf"], cols, lg, sr)
                    if not bool(torch.equal(net_ref.max_pool3d_2(full), gotp)):
                        self._fail(i, "mp_mode 2: the pooled tensor differs from the pooling of the launch's own full-resolution output",
                                   (net_ref.max_pool3d_2(full) - gotp).abs(), torch.full_like(gotp, 1e-300), cols)
            for what, got, r, bnd, sab in checks:
                err = (got - r).abs()
                finite = torch.isfinite(got)
                if not bool(finite.all()):
                    self._fail(i, what + ": non-finite output", torch.where(finite, err, torch.full_like(err, 1e30)), bnd, cols)
                meas = float(((err - rel * r.abs() - tiny).clamp_min(0) / (U * sab)).max())
                self.stats[key] = max(self.stats.get(key, 0.0), meas)
                if bool((err > bnd).any()):
                    self._fail(i, what + " outside the bound (c = %g; measured max |err| / (2^-24 S) %.3g)" % (c, meas), err, bnd, cols)
            # detectability of a missing tap, on the tensor the launch writes
            if op["n_taps"] > 1 and part == 0:
                if pooled_only:
                    post, bnd = (lambda t: net_ref.max_pool3d_2(relu(t))), net_ref.max_pool3d_2(bound)
                else:
                    post, bnd = relu, bound
                ratio, tap = ref.tap_effects(post, bnd)
                dkey = key + ("detect",)
                self.stats[dkey] = min(self.stats.get(dkey, np.inf), ratio)
                assert ratio >= DETECT_RATIO, ("%s, op %d %s: removing tap %s changes no output by more than %.3g x the bound (need %g): "
                                               "the bound of this form is too loose to see a missing tap"
                                               % (self.where, i, op_name(op), tap, ratio, DETECT_RATIO))

    def run(self, check=True, snapshots=None):
        """Every launch in order; check each (check=True) and/or collect the raw bits it wrote (snapshots: a list)."""
        for i, op in enumerate(self.ops):
            self.step(i)
            if snapshots is not None:
                snapshots.append(self.snapshot(i))
            if not check:
                continue
            torch.cuda.synchronize(self.dev)
            if op["kind"] == OP_CONV:
                self.check_conv(i)
                if op["aux_out_buf"] >= 0:
                    self.check_producer(i)
            else:
                self.check_pool(i)
        torch.cuda.synchronize(self.dev)

    def output(self):
        """The tower's final f32 output [live, n] (the last launch's output buffer)."""
        op = self.ops[-1]
        d = self.bufs[op["out_buf"]]
        return self.dec.raw(op["out_buf"])[:self.live, :d["C"]]
