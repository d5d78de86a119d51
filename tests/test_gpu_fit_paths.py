"""Patch rows [first, first + count) with ``first != 0`` through every method of ``provider.CloudPatches`` that takes them, for the three
kinds of centre (all points, ``pidx``, positions) and both argument layouts of the C entries (the ball entries pass ``query_row0`` in
both forms, the k-NN and list-fit entries only in the index form): two pieces on two streams equal one call, bit for bit, within one
``CloudPatches``.  ``pca`` and ``quadric`` over all points are ``test_partition`` of test_gpu_pca.py and test_gpu_quadric.py."""
import numpy as np
import pytest
import torch

import _pca_fixture as fx

pytestmark = pytest.mark.gpu

M, CUT = 301, 129                     # 129 is no multiple of the four rows of a workgroup
KS = (8, 16)
KINDS = ("all", "pidx", "positions")
METHODS = ("pca", "quadric", "knn", "pca_knn", "quadric_knn", "build", "count_balls")
_clouds = {}


def _cloud(kind, dev):
    """One ``CloudPatches`` per kind over the first 2 000 points of the fixture's ellipsoid, prepared once."""
    if kind not in _clouds:
        import nesti_net_amd  # noqa: F401
        from nesti_net_amd.config import NestiConfig
        from nesti_net_amd.provider import CloudPatches
        pts = fx.cloud("ellipsoid")["pts"][:2000]
        rows = np.arange(5, 2000, 6)[:M]
        off = (pts[rows] + np.float32(0.004) * np.random.RandomState(3).normal(size=(M, 3))).astype(np.float32)
        assert len(rows) == M
        _clouds[kind] = CloudPatches(pts, NestiConfig(), device=dev, pidx=rows if kind == "pidx" else None,
                                     queries=off if kind == "positions" else None)
    return _clouds[kind]


def _call(cp, method, first, count, out=None, stream=None):
    if method in ("pca", "quadric", "build"):
        return getattr(cp, method)(first, count, out=out, stream=stream)
    if method == "knn":
        return cp.knn(first, count, 16, stream=stream)
    if method == "count_balls":
        return (cp.count_balls(first, count, stream=stream),)
    return getattr(cp, method)(first, count, KS, stream=stream)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


CELLS = [(k, m) for k in KINDS for m in METHODS
         if not (k == "all" and m in ("pca", "quadric"))         # test_gpu_pca.py / test_gpu_quadric.py::test_partition
         and not (k == "positions" and m == "count_balls")]      # the reference-order entries serve index queries only


@pytest.mark.parametrize("kind,method", CELLS, ids=["%s-%s" % c for c in CELLS])
def test_two_pieces_equal_one_call(kind, method, gpu_device):
    cp = _cloud(kind, gpu_device)
    whole = _call(cp, method, 0, M)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)]
    takes_out = method in ("pca", "quadric", "build")
    if takes_out:
        got = tuple(torch.full_like(t, 7) for t in whole)
        for (a, b), st in zip(((0, CUT), (CUT, M)), streams):
            with torch.cuda.stream(st):          # the method's temporaries are then allocated for the stream that uses them
                ret = _call(cp, method, a, b - a, out=tuple(t[a:b] for t in got), stream=st)
            assert all(r.data_ptr() == t[a:b].data_ptr() for r, t in zip(ret, got))
    else:
        pieces = []
        for (a, b), st in zip(((0, CUT), (CUT, M)), streams):
            with torch.cuda.stream(st):          # the method's temporaries are then allocated for the stream that uses them
                pieces.append(_call(cp, method, a, b - a, stream=st))
        torch.cuda.synchronize()
        got = tuple(torch.cat(p) for p in zip(*pieces))
    torch.cuda.synchronize()
    assert len(got) == len(whole)
    for w, g in zip(whole, got):
        assert w.shape == g.shape and w.dtype == g.dtype and torch.equal(_bits(w), _bits(g))
    # the rows are the cloud's own: a first piece mistaken for the second would still be equal to itself, not to these
    assert not torch.equal(_bits(whole[0][:CUT]), _bits(whole[0][CUT:2 * CUT]))


@pytest.mark.parametrize("kind", KINDS)
def test_centre_positions(kind, gpu_device):
    from nesti_net_amd import orient
    cp = _cloud(kind, gpu_device)
    want = {"all": lambda: cp.cloud, "pidx": lambda: cp.cloud[cp.pidx.long()].contiguous(),
            "positions": lambda: orient.harmless_positions(cp.queries)}[kind]()
    got = cp.centre_positions()
    assert tuple(got.shape) == (cp.patch_count, 3) and got.is_contiguous() and torch.equal(got.view(torch.int32), want.view(torch.int32))
