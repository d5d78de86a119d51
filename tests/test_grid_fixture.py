"""The conditions the search-grid tests on the device (tests/test_gpu_grid.py) rely on, checked on the host: the fixture clouds
(tests/_grid_fixture.py) really reach the regimes they are named after."""
import numpy as np
import pytest

import _grid_fixture as G


def test_lattice_radii_are_exact_and_the_centre_counts_are_the_known_ones():
    for name, unit in (("lattice_exact", 1.0), ("lattice_shifted", 0.25)):
        c = G.case(name)
        assert c["bbdiag"] == 42.0 * unit and c["r_abs"] == [3.0 * unit, 5.0 * unit, 7.0 * unit]
        assert c["pts"].shape == (9139, 3) and len(np.unique(c["pts"], axis=0)) == 9139
        # the float32 cloud is the lattice itself: every coordinate difference, and with it every d2, is exact
        ints = np.stack(np.meshgrid(*[np.arange(n) for n in G.LATTICE], indexing="ij"), -1).reshape(-1, 3)
        assert np.array_equal((c["pts"].astype(np.float64) - c["pts"][0].astype(np.float64)) / unit, ints)
    centre = [G.lattice_index(*G.LATTICE_CENTRE)]
    closed, on = G.lattice_counts(centre, (9, 25, 49))
    assert closed.tolist() == [[123, 515, 1417]] and on.all()
    assert G.lattice_counts(centre, (9, 25, 49), strict=True)[0].tolist() == [[93, 485, 1365]]
    cfg = G.case("lattice_exact")["cfg"]
    assert closed[0, 1] > cfg.num_point > G.lattice_counts(centre, (9, 25, 49), strict=True)[0][0, 1]   # 515 > P = 512 > 485
    assert closed[0, 2] > G.K_LIST_CAP
    rows = G.case("lattice_exact")["rows"]
    assert centre[0] in rows and len(rows) <= 400
    # the inclusive test matters on hundreds of (row, scale) pairs: a point at d2 == r^2 exactly
    _, on = G.lattice_counts(rows, (9, 25, 49))
    strict = G.lattice_counts(rows, (9, 25, 49), strict=True)[0]
    assert on.sum() >= 100 and ((G.ball_sizes("lattice_exact") != strict) == on).all()


def test_lattice_brute_force_agrees_with_scipy():
    """The two references of the lattice's ball sizes, one of them independent of scipy, agree."""
    from scipy import spatial
    c = G.case("lattice_exact")
    tree = spatial.cKDTree(c["pts"], 10)
    got = np.stack([tree.query_ball_point(c["pts"][c["rows"]], r, return_length=True) for r in c["r_abs"]], 1)
    assert np.array_equal(got, G.ball_sizes("lattice_exact"))


@pytest.mark.parametrize("name", G.CASES)
def test_grid_regime_and_ball_sizes(name):
    """The clamp cases take the ``ext / 127`` arm of the cell edge with an axis of at least 127 cells; in every case one scale has a
    ball of at most P and a ball of more than P points among the rows."""
    c, h, n_ball = G.case(name), G.case(name)["header"], G.ball_sizes(name)
    P = c["cfg"].num_point
    print("%s: N %d, %d rows, P %d, dims %s, ncells %d, cell / (1.0001 r_max) %.4f; balls per scale min %s mean %s max %s"
          % (name, len(c["pts"]), len(c["rows"]), P, h["dims"], h["ncells"], h["cell"] / (1.0001 * max(c["r_abs"])),
             n_ball.min(0).tolist(), n_ball.mean(0).round(1).tolist(), n_ball.max(0).tolist()))
    assert c["pts"].dtype == np.float32 and len(c["rows"]) <= 400 and c["rows"].max() < len(c["pts"])
    assert h["clamped"] == (name in G.CLAMPED)
    if name in G.CLAMPED:
        assert max(h["dims"]) >= 127 and h["cell"] > 1.0001 * max(c["r_abs"])
    assert any((n_ball[:, s] <= P).any() and (n_ball[:, s] > P).any() for s in range(n_ball.shape[1]))
    assert (n_ball >= 1).all()                                  # a cloud point is in its own balls
    if name == "plate":
        assert h["dims"] == [128, 64, 3]
    if name == "needle_x":
        assert h["dims"][1:] == [1, 1]
    if name == "needle_diag":
        assert h["ncells"] > 2000000 and len(np.unique(G.cells(c["pts"], h))) < 0.001 * h["ncells"]     # almost every cell is empty
    if name == "offset":
        assert len(np.unique(c["pts"], axis=0)) == len(c["pts"]) and np.abs(c["pts"]).min(0).tolist() >= [1000.0, 1999.0, 500.0]
    if name == "duplicates":
        assert len(c["heavy"]) == 1500 and len(np.unique(c["pts"][c["heavy"]], axis=0)) == 1
        assert len(np.unique(c["pts"], axis=0)) == 2001 and np.isin(c["heavy"][:8], c["rows"]).all()
        assert n_ball[:, 0].max() > G.K_LIST_CAP and n_ball.max() < 16384        # above kListCap at distance 0, below the reference-order sort
        assert (n_ball >= 4).all()


@pytest.mark.parametrize("name", G.WITH_POSITIONS)
def test_positions_lie_outside_the_box_and_inside_empty_cells(name):
    from scipy import spatial
    c, h = G.case(name), G.case(name)["header"]
    pos, n_out = c["positions"], c["n_outside"]
    p64 = c["pts"].astype(np.float64)
    lo, hi = p64.min(0), p64.max(0)
    assert pos.dtype == np.float32 and n_out == (14 + 6 * G.EXTREME) * len(G.PUSH) and len(pos) <= 400
    outside = ((pos[:n_out] < lo) | (pos[:n_out] > hi)).any(axis=1)
    assert outside.all()
    inside = pos[n_out:].astype(np.float64)
    assert len(inside) >= 40 and ((inside >= lo) & (inside <= hi)).all()
    occupied = np.zeros(h["ncells"], bool)
    occupied[G.cells(c["pts"], h)] = True
    assert not occupied[G.cells(pos[n_out:], h)].any()
    tree = spatial.cKDTree(p64)
    sizes = np.stack([tree.query_ball_point(pos.astype(np.float64), r, return_length=True) for r in c["r_abs"]], 1)
    print("%s: %d positions outside the box, %d of them with a non-empty ball; %d inside empty cells, %d of them with a non-empty ball; "
          "largest ball %d" % (name, n_out, int((sizes[:n_out, -1] > 0).sum()), len(inside), int((sizes[n_out:, -1] > 0).sum()), sizes.max()))
    assert (sizes[:n_out, -1] > 0).sum() >= 50 and (sizes[:n_out, -1] == 0).sum() >= 50
    assert (sizes[n_out:, -1] > 0).sum() >= 20 and (sizes[n_out:, 0] == 0).sum() >= 20
    near = tree.query(inside)[0]
    ratio = near[:, None] / np.asarray(c["r_abs"])[None, :]
    close = (np.abs(ratio - 0.9) < 0.03).any(axis=1)
    far = (np.abs(ratio - 1.1) < 0.035).any(axis=1)
    assert (close | far).all() and close.sum() >= 20 and far.sum() >= 20
