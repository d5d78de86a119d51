"""Orientation of estimated normals without a GPU: the tests' own restatement (tests/_orient_fixture.py) orients the fixture clouds
the way the definition promises, and the C entries refuse bad arguments before any device call."""
import ctypes

import numpy as np
import pytest

import _orient_fixture as F


@pytest.mark.parametrize("name", F.SANITY)
def test_restatement_orients_the_fixture_clouds(name):
    """After orientation no eligible row points against the analytic normal, there is one tree per surface, and the reference's
    oriented RMS (utils/evaluate.py:151) equals the unoriented one."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.evaluate import shape_metrics
    c, p = F.case(name), F.predicted(name)
    el = F.eligible(c["normals"])
    assert F.inward(p["out"], c["gt"], c["normals"]) == 0
    assert p["stats"]["n_components"] == c["surfaces"] and p["stats"]["n_eligible"] == int(el.sum())
    m = shape_metrics(p["out"][el], c["gt"][el])
    assert m["rms_o"] == m["rms"]
    # ineligible rows untouched, every other row +input or -input
    assert np.array_equal(p["out"][~el].view(np.uint32), c["normals"][~el].view(np.uint32))
    assert np.array_equal(p["out"].view(np.uint32) & 0x7fffffff, c["normals"].view(np.uint32) & 0x7fffffff)
    if name == "ellipsoid3001_zero10":
        assert 200 < int((~el).sum()) < 400


def test_fixture_conditions():
    """What the GPU tests rely on: the helix tree is deep, K = 1 falls apart (the documented limit), the lattice has exact ties
    and duplicates."""
    assert F.predicted("helix2000")["depth"] >= 1000 and F.predicted("helix2000")["stats"]["n_components"] == 1
    k1 = F.predicted("ellipsoid3001_k1")
    assert k1["stats"]["n_components"] > 100
    assert F.inward(k1["out"], F.case("ellipsoid3001_k1")["gt"], F.case("ellipsoid3001_k1")["normals"]) > 0
    lat = F.case("lattice")
    x = lat["xyz"].astype(np.float64)
    nb = F.predicted("lattice")["g"]["nbr"]
    d2 = ((x[nb[:100, 0]] - x[:100]) ** 2).sum(1)
    assert (d2 == 0).all() and (nb[:100, 0] == np.arange(1728, 1828)).all()      # a duplicate is an ordinary neighbour at d2 = 0
    # position noise 0.006, tilt 0.3: one tree.  The pass undoes the random signs the fixture drew except where a tilted normal is
    # over 90 degrees from its tree parent's: two independent tilts of sigma 0.3 per component differ by sigma 0.42, so that takes a
    # > 2.3 sigma excursion along the parent's direction on top of the cosine -- of the order of 1e-3 per row; 0.5 % is the bar
    c, p = F.case("ellipsoid3001_noisy"), F.predicted("ellipsoid3001_noisy")
    wrong = int((p["flipped"] != (c["signs"] < 0)).sum())
    assert p["stats"]["n_components"] == 1 and min(wrong, 3001 - wrong) <= 15


def _lib():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    return _lib.load()


def test_orient_workspace_bytes():
    lib = _lib()
    ws = lib.nesti_orient_workspace_bytes
    assert ws(0, 8) == 0 and ws(-5, 8) == 0
    assert ws(1, 1) > 0
    sizes = [ws(m, 8) for m in (1, 100, 3001, 100000, 1 << 24)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    by_k = [ws(3001, k) for k in range(1, 17)]
    assert by_k == sorted(by_k) and by_k[0] > 0 and by_k[-1] > by_k[0]
    assert ws(3001, 8) >= 3001 * 8 * 4            # at least the neighbour lists


def test_orient_entries_refuse_bad_arguments_before_any_device_call():
    """Every refusal of include/nesti_hip.h, with pointers that are never dereferenced: no device is touched."""
    lib = _lib()
    M, K, R = 1000, 8, 0.1
    p = ctypes.c_void_p(0x1000)                   # non-null, never read: the checks come first
    gws, ows = lib.nesti_patches_workspace_bytes(M), lib.nesti_orient_workspace_bytes(M, K)
    big = ctypes.c_size_t(1 << 62)
    vp = (ctypes.c_double * 3)(0.0, 0.0, 5.0)

    def graph(xyz=p, m=M, n=p, r=R, k=K, g=p, gb=gws, w=p, wb=ows):
        return lib.nesti_orient_graph(xyz, m, n, ctypes.c_double(r), k, g, gb, w, wb, None, None, None, None, None, None)

    def normals(xyz=p, m=M, n=p, mode=0, r=R, k=K, v=None, g=p, gb=gws, w=p, wb=ows):
        return lib.nesti_orient_normals(xyz, m, n, mode, ctypes.c_double(r), k, v, g, gb, w, wb, None, None, None)

    def refused(rc, *words):
        msg = lib.nesti_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    for call, who in ((graph, "nesti_orient_graph"), (normals, "nesti_orient_normals")):
        for kw in ({"xyz": None}, {"n": None}, {"g": None}, {"w": None}):
            refused(call(**kw), who, "null")
        for k in (0, -1, 17):
            refused(call(k=k), who, "K")
        for r in (0.0, -1.0, float("inf"), float("nan")):
            refused(call(r=r), who, "radius")
        refused(call(wb=ows - 1), who, "workspace too small")
        refused(call(gb=gws - 1), who, "grid workspace too small")
        refused(call(m=1 << 28, k=16, gb=big, wb=big), who, "2^32")          # M K = 2^32
        refused(call(m=-1), who, "M")
        assert call(m=0) == 0 and call(m=0, xyz=None, n=None, g=None, w=None, gb=0, wb=0) == 0      # the no-op
    refused(normals(mode=2), "unknown mode")
    refused(normals(mode=-1), "unknown mode")
    refused(normals(mode=1), "viewpoint")
    for bad in (float("nan"), float("inf")):
        refused(normals(mode=0, v=(ctypes.c_double * 3)(0.0, bad, 1.0)), "viewpoint", "finite")
        refused(normals(mode=1, v=(ctypes.c_double * 3)(bad, 0.0, 1.0)), "viewpoint", "finite")
    del vp


def test_python_layer_refuses_non_finite_positions_of_eligible_rows():
    """``orient_normals`` checks its input on the host before it asks for a device."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.orient import orient_normals
    xyz = np.zeros((4, 3), np.float32)
    n = np.ones((4, 3), np.float32)
    xyz[2, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        orient_normals(xyz, n, 0.1)
    with pytest.raises(ValueError):
        orient_normals(xyz[:, :2], n, 0.1)
    with pytest.raises(ValueError):
        orient_normals(np.zeros((4, 3), np.float32), n, 0.1, mode="viewpoint")
    with pytest.raises(ValueError):
        orient_normals(np.zeros((4, 3), np.float32), n, 0.1, mode="hoppe")
    with pytest.raises(ValueError):
        orient_normals(np.zeros((4, 3), np.float32), n, 0.1, k=17)
