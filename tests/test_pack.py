"""The weight packer's bytes, pinned on the CPU: nesti_debug_pack_layer packs one layer on the host with the code nesti_model_create
uploads from, and a SHA-256 over everything a launch gets from the packer -- metadata, tap table, weight image, padded bias -- must
equal the digest recorded from the commit BEFORE the packer was carved out of model.hip (tests/golden/pack_digests.json; how they
were recorded: profiles/refactor_pack.txt).  No tolerance, no excluded case: a change of the packed layout changes these digests
and has to say so.  tests/layer_ref.py stays independent of this: it emulates the packer's values and never reads them back."""
import ctypes
import functools
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import layer_ref
from test_layer_ops import _configs, _passes

# model -> the dtypes packed for it.  grid3 adds the 3^3 grid's dropped taps and conv4n's even-kernel rule in the pair modes, ms_sw_n_est
# the ablation towers; the gating net, expert 0 and the last expert of each (the other experts have the same shapes)
MODELS = {"experts": ["f32", "f16", "bf16", "f16x3", "bf16x3", "f16x3c", "f16x8", "f16x8c"], "grid3": ["f16", "f16x3"],
          "ms_sw_n_est": ["f16"]}
MAIN = {"f16x3c": "f16x3", "f16x8": "f16x3", "f16x8c": "f16x3"}      # main_dtype: what the packings of a model are made for
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")
INFO_INTS = ("kind", "TN", "n_tiles", "split_tile", "n_chunks", "n_taps", "x3n", "x8_sb")


def _lib():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    return _lib, _lib.load()


@functools.lru_cache(maxsize=None)
def _tensors(model):
    """(cfg struct, CTensor array, count, the arrays it points into) of the model's synthetic weights."""
    from nesti_net_amd import weights
    L, _ = _lib()
    cfg = _configs()[model]
    W = weights.synthetic_weights(cfg, bn="random")
    keep = [np.ascontiguousarray(W[k], dtype=np.float32) for k in W]
    arr = (L.CTensor * len(keep))()
    for i, (k, a) in enumerate(zip(W, keep)):
        arr[i].name, arr[i].data, arr[i].ndim = k.encode(), a.ctypes.data, a.ndim
        for d in range(a.ndim):
            arr[i].dims[d] = a.shape[d]
    return cfg.to_c(), arr, len(keep), keep


@functools.lru_cache(maxsize=None)
def _cases(model, dtype):
    """{key: (layer, packing form, producer)} of every packing the covered towers of a model of this dtype launch on."""
    from nesti_net_amd.config import DTYPES
    _, lib = _lib()
    c = _tensors(model)[0]
    last = _configs()[model].n_towers - 1
    out = {}
    for tower, fast, x8 in _passes(model, dtype):
        if tower not in (-1, 0, last):
            continue
        for fmt in ((6, 8) if x8 else (0,)):
            _, ops, _ = layer_ref.tower_ops(lib, c, DTYPES[dtype], tower, 8, fast, x8, fmt)
            for o in ops:
                if o["kind"] != layer_ref.OP_CONV:
                    continue
                form = layer_ref.FORM_PAIR if o["form"] == layer_ref.FORM_X2 else o["form"]
                producer = o["aux_out_buf"] >= 0
                key = "%s/%s/%s/%s%s" % (model, MAIN.get(dtype, dtype), layer_ref.FORM_NAMES[form], o["scope"], "/producer" if producer else "")
                out[key] = (o["layer"], form, producer)
    return out


_scratch = {"w": np.empty(1 << 24, np.uint8), "b": np.empty(1 << 12, np.float32)}


def _pack(model, dtype, form, layer):
    """nesti_debug_pack_layer -> (info, weight bytes, bias float32).  One call when the scratch arrays are large enough (packing a
    layer twice to learn its size first doubles the run time); the hook fills info before it refuses small arrays."""
    from nesti_net_amd.config import DTYPES
    L, lib = _lib()
    c, arr, n, _ = _tensors(model)
    info = L.CDebugPack()
    for _ in range(2):
        w, b = _scratch["w"], _scratch["b"]
        rc = lib.nesti_debug_pack_layer(ctypes.byref(c), arr, n, DTYPES[dtype], form, layer, ctypes.byref(info), w.ctypes.data, w.size,
                                        b.ctypes.data, b.size)
        if rc == 0 or b"output arrays too small" not in lib.nesti_last_error():
            break
        _scratch["w"], _scratch["b"] = np.empty(max(w.size, info.w_bytes), np.uint8), np.empty(max(b.size, info.n_bias), np.float32)
    L.check(rc, "nesti_debug_pack_layer")
    return info, w[:info.w_bytes], b[:info.n_bias]


def _digest(info, w, b, producer):
    """SHA-256 of the canonical record: the info fields as little-endian int32 (x8_sc for producers only, else 0), acc_scale's
    bits, n_taps x 4 tap bytes, the weight bytes, the bias bytes."""
    h = hashlib.sha256()
    h.update(struct.pack("<9i", *[getattr(info, f) for f in INFO_INTS], info.x8_sc if producer else 0))
    h.update(struct.pack("<f", info.acc_scale))
    h.update(bytes(np.ctypeslib.as_array(info.tap)[:info.n_taps].astype(np.int8).tobytes()))
    h.update(w.tobytes())
    h.update(b.astype("<f4").tobytes())
    return h.hexdigest()


_done = {}      # key -> digest: a packing several model dtypes share (f16x3 / f16x3c / f16x8 / f16x8c) is packed once


@pytest.mark.parametrize("model,dtype", [(m, d) for m in MODELS for d in MODELS[m]])
def test_packed_bytes_match_the_recorded_digests(model, dtype):
    golden = json.load(open(GOLDEN))
    cases = _cases(model, dtype)
    assert cases
    bad = []
    for key, (layer, form, producer) in cases.items():
        assert key in golden, "no recorded digest for " + key
        if key not in _done:
            info, w, b = _pack(model, dtype, form, layer)
            assert w.size == info.n_tiles * info.n_chunks * info.n_taps * info.TN * (128 if info.kind == 0 else 64)
            assert b.size == info.n_tiles * info.TN
            _done[key] = _digest(info, w, b, producer)
        if _done[key] != golden[key]:
            bad.append(key)
    assert not bad, "%d of %d packings differ from the recorded bytes: %s" % (len(bad), len(cases), bad[:8])


def test_golden_file_holds_exactly_the_enumerated_cases():
    """Every form the models launch is covered (plain, pair, X8, X6, the filter pass's plain-f16 tap layers, producers), all three
    kernel families, and the file holds no digest nobody checks."""
    golden = json.load(open(GOLDEN))
    keys = set()
    for m in MODELS:
        for d in MODELS[m]:
            keys |= set(_cases(m, d))
    assert keys == set(golden)
    forms = {k.split("/")[2] for k in keys}
    assert forms == {"plain", "pair", "x8", "x6"} and any(k.endswith("/producer") for k in keys)
    assert "experts/f16x3/plain/inception1gating_conv_conv2" in keys      # the two-stage gate's filter pass


def _refused(model, dtype, form, layer, tensors=None):
    from nesti_net_amd.config import DTYPES
    L, lib = _lib()
    c, arr, n, _ = _tensors(model)
    if tensors is not None:
        arr, n = tensors
    info = L.CDebugPack()
    rc = lib.nesti_debug_pack_layer(ctypes.byref(c), arr, n, DTYPES[dtype], form, layer, ctypes.byref(info), None, 0, None, 0)
    assert rc != 0
    return lib.nesti_last_error().decode()


def test_hook_refuses_forms_the_layer_cannot_take():
    cases = _cases("experts", "f16x8c")
    x6 = [v for k, v in cases.items() if "/x6/" in k]
    fc = [v for k, v in cases.items() if "/pair/fc1Expert_0" in k]
    conv1 = [v for k, v in cases.items() if k.endswith("/pair/inception1Expert_0_conv1/producer")]
    assert x6 and fc and conv1
    for layer in (fc[0][0], conv1[0][0]):                      # not k^3 tap layers at 8^3
        for form in (layer_ref.FORM_X8, layer_ref.FORM_X6):
            assert "X8 / X6 packings are for the k^3 tap layers at 8^3" in _refused("experts", "f16x8c", form, layer)
    assert "X8 / X6" in _refused("experts", "f16x3", layer_ref.FORM_X6, x6[0][0])       # not an x8 model
    assert "pair packing is for the pair dtypes" in _refused("experts", "f16", layer_ref.FORM_PAIR, fc[0][0])
    assert "form is NESTI_DEBUG_FORM_" in _refused("experts", "f16", 5, fc[0][0])
    assert "layer index outside the model" in _refused("experts", "f16", layer_ref.FORM_PLAIN, 10 ** 6)
    # X2 launches run on the pair packing
    a, b = _pack("experts", "f16x3", layer_ref.FORM_X2, fc[0][0]), _pack("experts", "f16x3", layer_ref.FORM_PAIR, fc[0][0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_hook_reports_missing_and_misshaped_tensors_and_small_arrays():
    L, lib = _lib()
    c, arr, n, _ = _tensors("experts")
    cases = _cases("experts", "f16")
    layer = cases["experts/f16/plain/inception1Expert_0_conv2"][0]
    scope = "inception1Expert_0_conv2"

    def edited(name, edit):
        cp = (L.CTensor * n)()
        ctypes.memmove(cp, arr, ctypes.sizeof(arr))
        (i,) = [i for i in range(n) if cp[i].name == name.encode()]
        edit(cp[i])
        return cp, n

    def rename(t):
        t.name = b"elsewhere"

    def reshape(t):
        t.dims[0] += 1

    assert _refused("experts", "f16", 0, layer, edited(scope + "/weights", rename)) == "missing or mis-shaped tensor %s/weights" % scope
    assert _refused("experts", "f16", 0, layer, edited(scope + "/weights", reshape)) == "missing or mis-shaped tensor %s/weights" % scope
    assert _refused("experts", "f16", 0, layer, edited(scope + "/biases", reshape)) == "missing or mis-shaped tensor %s/biases" % scope
    assert _refused("experts", "f16", 0, layer, edited(scope + "/bn/var", rename)) == \
        "missing or mis-shaped batch-norm tensors under %s/bn/" % scope
    info = L.CDebugPack()
    from nesti_net_amd.config import DTYPES
    assert lib.nesti_debug_pack_layer(ctypes.byref(c), arr, n, DTYPES["f16"], 0, layer, ctypes.byref(info), None, 0, None, 0) == 0
    w = np.empty(info.w_bytes, np.uint8)
    assert lib.nesti_debug_pack_layer(ctypes.byref(c), arr, n, DTYPES["f16"], 0, layer, ctypes.byref(info), w.ctypes.data, w.size - 1,
                                      None, 0) != 0
    assert b"output arrays too small" in lib.nesti_last_error()
