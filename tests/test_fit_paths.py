"""The call path the model-free estimators share, without a GPU: the ``out=`` helper of ``provider`` on CPU tensors, and the log lines of
``--estimator pca / quadric`` and of the orientation pass against the strings written out here."""
import pytest
import torch

SPECS = (((5, 4, 3), torch.float32), ((5, 4, 2), torch.float32), ((5, 4), torch.int32))
WHAT = "(a [5,4,3] f32, b [5,4,2] f32, n [5,4] int32)"
CPU = torch.device("cpu")


def _good():
    return tuple(torch.zeros(shape, dtype=dt) for shape, dt in SPECS)


def _check_out(*args):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.provider import check_out
    return check_out(*args)


def test_out_helper_returns_the_callers_tensors():
    out = _good()
    got = _check_out(out, SPECS, CPU, WHAT)
    assert isinstance(got, tuple) and len(got) == 3 and all(a is b for a, b in zip(got, out))
    got = _check_out(list(out), SPECS, CPU, WHAT)
    assert isinstance(got, tuple) and all(a is b for a, b in zip(got, out))
    # a slice of rows of a larger buffer, as the batched callers pass it, is contiguous
    big = tuple(torch.zeros((9,) + shape[1:], dtype=dt) for shape, dt in SPECS)
    assert all(a.data_ptr() == b[2:7].data_ptr() for a, b in zip(_check_out(tuple(t[2:7] for t in big), SPECS, CPU, WHAT), big))


def test_out_helper_allocates():
    got = _check_out(None, SPECS, CPU, WHAT)
    assert [(tuple(t.shape), t.dtype, t.device) for t in got] == [(shape, dt, CPU) for shape, dt in SPECS]
    assert all(t.is_contiguous() for t in got)
    assert [tuple(t.shape) for t in _check_out(None, (((0, 4, 3), torch.float32),), CPU, WHAT)] == [(0, 4, 3)]


def _bad_outs():
    a, b, n = _good()
    yield "too short", (a, b)
    yield "too long", (a, b, n, n)
    yield "one wrong shape", (a, torch.zeros((5, 4, 3)), n)
    yield "one row short", (a, b, torch.zeros((4, 4), dtype=torch.int32))
    yield "wrong dtype", (a, b, torch.zeros((5, 4), dtype=torch.int64))
    yield "float64", (torch.zeros((5, 4, 3), dtype=torch.float64), b, n)
    yield "a non-contiguous view", (a, torch.zeros((5, 4, 4))[:, :, :2], n)
    yield "a transposed view", (a, b, torch.zeros((4, 5), dtype=torch.int32).t())
    yield "another device", (a, b, torch.zeros((5, 4), dtype=torch.int32, device="meta"))


@pytest.mark.parametrize("what,out", list(_bad_outs()), ids=[w for w, _ in _bad_outs()])
def test_out_helper_refuses(what, out):
    with pytest.raises(ValueError) as e:
        _check_out(out, SPECS, CPU, WHAT)
    assert str(e.value) == "out: contiguous " + WHAT + " on cpu"


def test_orientation_line():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    stats = {"n_eligible": 790, "n_flipped": 12, "n_components": 1, "n_edges": 3000}
    assert cli.orient_line("ell", "mst", stats, 800) == \
        "orientation of ell (mst): 790 of 800 rows oriented, 12 flipped, 1 connected piece, 3000 edges"
    assert cli.orient_line("ell", "mst", dict(stats, n_components=2), 800) == \
        "orientation of ell (mst): 790 of 800 rows oriented, 12 flipped, 2 connected pieces, 3000 edges"


@pytest.mark.parametrize("estimator,args,want", [
    ("pca", dict(n_scales=4, scale=3, radius=0.0123456789),
     "plane fit of ell: 800 rows, radius 0.0123457 (scale 3 of 4); 5 rows with fewer than 3 points in that ball (written as 0 0 0)"),
    ("pca", dict(n_scales=2, scale=1, k=16),
     "plane fit of ell: 800 rows, 16 nearest neighbours (scale 1 of 2); 5 rows without a fit (written as 0 0 0)"),
    ("quadric", dict(n_scales=4, scale=3, radius=0.0123456789),
     "quadric fit of ell: 800 rows, radius 0.0123457 (scale 3 of 4); 5 rows without a fit in that ball (fewer than 6 points or a "
     "singular system: written as 0 0 0 and 0 0)"),
    ("quadric", dict(n_scales=2, scale=1, k=16),
     "quadric fit of ell: 800 rows, 16 nearest neighbours (scale 1 of 2); 5 rows without a fit (fewer than 6 points or a "
     "singular system: written as 0 0 0 and 0 0)"),
], ids=["pca ball", "pca knn", "quadric ball", "quadric knn"])
def test_fit_lines(estimator, args, want):
    """The four lines as the two runners formatted them before they became one, for name ell, 800 rows of which 5 have no fit."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    assert cli.fit_line(estimator, "ell", 800, missing=5, **args) == want
