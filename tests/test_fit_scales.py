"""The premises of tests/test_gpu_fit_scales.py without a GPU: what the restatements give on the clouds, rows, radii and neighbour
counts of tests/_fit_scales_fixture.py.  The GPU test allows no ill-conditioned plane fit and holds every quadric fit with n >= 6 to its
bounds; these tests pin that the inputs deserve it -- the ball sizes that interleave sentinel rows, failed fits and live rows at the
smallest radius of the ellipsoid, an ill-conditioned share of 0 at every scale of every case, a solvable system wherever n >= 6 -- so
that a later change of ``synth`` cannot hollow the GPU test out unnoticed.  Also the parser errors of ``--patch_radius``."""
import numpy as np
import pytest

import _fit_scales_fixture as sx
import _hough_fixture as hx


def _plane_premises(ref, label):
    """No live pair is ill-conditioned; -> (smallest gap w1 - w0 of a live pair, live mask)."""
    bound, live = sx.plane_bound(ref)
    assert (bound[live] <= 1e-3).all(), label
    assert (ref["normals"][live] != 0).any(axis=-1).all() and not ref["normals"][~live].any(), label
    return float((ref["w"][..., 1] - ref["w"][..., 0])[live].min()), live


def _quadric_premises(ref, label):
    """Ill-conditioned share 0 at every scale and a solved system wherever n >= 6; -> (largest kappa of a fitted pair, fit mask)."""
    ill, fit = sx.quadric_ill(ref)
    assert not ill.any(), (label, ill.sum(0))
    assert ref["ok"][fit].all() and not ref["ok"][~fit].any(), label
    return float(ref["kappa"][fit].max()), fit


def test_inputs():
    """250 rows of each cloud; every scale set has 1 to 4 positive radii drawn from A4 / T4, and the sub-configurations name every
    single column, two pairs (one out of order) and a triple."""
    for name in sx.CLOUDS:
        c = sx.cloud(name)
        assert len(c["rows"]) == 250 and c["pts"].dtype == np.float32
    assert sorted(len(r) for _, r in sx.SCALE_SETS.values()) == [1, 2, 4, 4, 4]
    for name, radii in sx.SCALE_SETS.values():
        assert set(radii) <= set(sx.A4 if name == "ellipsoid" else sx.T4)
        assert sx.SCALE_SETS[sx.FULL_SET[name]] == (name, sx.A4 if name == "ellipsoid" else sx.T4)
    assert sorted(len(s) for s in sx.SUB_CONFIGS) == [1, 1, 1, 1, 2, 2, 3] and (3, 1) in sx.SUB_CONFIGS
    assert [len(ks) for ks in sx.KS_SETS] == [4, 2, 1] and sx.KS_SETS[0][-1] == 256 and sx.KS_SETS[1][-1] % 64


def test_ellipsoid_balls_interleave_sentinels_failed_fits_and_live_rows():
    """At 0.01 the balls hold 1 to 6 points: 107 of the 250 rows have n >= 3 and 7 have n >= 6; the sentinel rows, the rows whose plane
    fit is live but whose quadric fit fails, and the rows with both are found inside one workgroup's four rows."""
    ref = sx.plane_balls("ellipsoid_4")
    n = ref["n_ball"]
    assert n[:, 0].min() == 1 and n[:, 0].max() == 6
    assert int((n[:, 0] >= 3).sum()) == 107 and int((n[:, 0] >= 6).sum()) == 7
    assert (n[:, 1:] >= 3).all() and int((n[:, 1] >= 6).sum()) == 248 and (n[:, 2:] >= 6).all()
    assert (np.diff(n, axis=1) >= 0).all() and n[:, 3].max() > 64                          # more than one trip per lane at 0.08
    kinds = np.where(n[:, 0] < 3, 0, np.where(n[:, 0] < 6, 1, 2)).reshape(-1, 2)           # 250 = 125 pairs of neighbouring rows
    assert (kinds[:, 0] != kinds[:, 1]).sum() > 40
    # the repeated, out-of-order set holds the same balls in other columns
    rep = sx.plane_balls("ellipsoid_4_repeated")["n_ball"]
    assert np.array_equal(rep[:, 0], rep[:, 1]) and np.array_equal(rep[:, [2, 3, 0]], n[:, [0, 1, 2]])


def test_torus_balls():
    """Balls of 17 to 679 points; curvatures of both signs at every radius."""
    ref = sx.plane_balls("torus_4")
    n = ref["n_ball"]
    assert n.min() == 17 and n.max() == 679 and n[:, 0].max() > 64
    q = sx.quadric_balls("torus_4", ref["normals"])
    assert q["ok"].all()
    assert ((q["k"][..., 0] > 0) & (q["k"][..., 1] < 0)).any(axis=0).all()                 # saddle points on the inner half of the tube
    assert ((q["k"][..., 0] * q["k"][..., 1]) > 0).any(axis=0).all()                       # ... and elliptic ones on the outer half


@pytest.mark.parametrize("key", list(sx.SCALE_SETS))
def test_ball_fits_are_well_conditioned(key):
    """Plane fits: 0 ill-conditioned pairs (the smallest gap w1 - w0 of a live pair is 6.0e-5, on the ellipsoid at 0.01).  Quadric fits
    from the restatement's plane normals: ill-conditioned share 0 at every scale, ``ok`` everywhere n >= 6 (the largest kappa is
    2.3e7, on the ellipsoid at 0.03)."""
    ref = sx.plane_balls(key)
    gap, live = _plane_premises(ref, key)
    kappa, fit = _quadric_premises(sx.quadric_balls(key, ref["normals"]), key)
    print("%s: %d live plane fits of %d pairs, smallest gap %.3g; %d pairs with n >= 6, largest kappa %.3g"
          % (key, live.sum(), live.size, gap, fit.sum(), kappa))
    assert gap > 5e-5 and kappa < 1e8
    if sx.SCALE_SETS[key][0] == "torus_clean":
        assert live.all() and fit.all()
    if key == "ellipsoid_4":
        assert 5.9e-5 < gap < 6.1e-5 and 2.2e7 < kappa < 2.4e7 and fit.sum(0).tolist() == [7, 248, 250, 250]


@pytest.mark.parametrize("ks", sx.KS_SETS)
@pytest.mark.parametrize("name", sx.CLOUDS)
def test_list_fits_are_well_conditioned(name, ks):
    """The same over the lists: every pair is live (n = k_s >= 8), 0 ill-conditioned plane fits, ill-conditioned share 0 of the quadric
    fits (the largest kappa is 1.3e6, on the torus at k = 8)."""
    idx, d2, count = sx.lists(name)
    assert (count == 256).all() and (idx[:, 0] == sx.cloud(name)["rows"]).all() and (np.diff(d2, axis=1) >= 0).all()
    ref = sx.plane_lists(name, ks)
    assert (ref["n_ball"] == np.array(ks)).all() and (ref["radius"] > 0).all()
    gap, live = _plane_premises(ref, (name, ks))
    kappa, fit = _quadric_premises(sx.quadric_lists(name, ks, ref["normals"]), (name, ks))
    print("%s, ks = %s: smallest gap %.3g, largest kappa %.3g" % (name, ks, gap, kappa))
    assert live.all() and fit.all() and gap > 1e-2 and kappa < 2e6
    if name == "torus_clean" and ks[0] == 8:
        assert 1.2e6 < kappa < 1.4e6


def _rot(R):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import hough
    return hough.rotation_table(R)


@pytest.mark.parametrize("ks", sx.HOUGH_KS_SETS)
def test_hough_restatement_scales_are_independent(ks):
    """The restatement keys its hash with scale 0, as the header of csrc/hough.hip promises: column s of a run over ``ks`` is the single
    column of a run over ``(ks[s],)``.  Every row has a winner at every scale from 9 neighbours up."""
    import _knn_fixture as kx
    pts = sx.box()
    nbr = kx.searched(("fit_scales", "box"), pts, pts, sx.HOUGH_K)[0]
    T = sx.HOUGH_T[0]
    whole = hx.restate(pts, pts, nbr, ks, T, sx.HOUGH_B, sx.HOUGH_R, _rot(sx.HOUGH_R), sx.HOUGH_SEED)
    assert (whole["count"] == np.array(ks)).all()
    for s, k in enumerate(ks):
        one = hx.restate(pts, pts, nbr, (k,), T, sx.HOUGH_B, sx.HOUGH_R, _rot(sx.HOUGH_R), sx.HOUGH_SEED)
        for key in whole:
            assert np.array_equal(np.ascontiguousarray(whole[key][:, s:s + 1]).view(np.uint8), one[key].view(np.uint8)), (key, k)
        if k >= 9:
            assert (whole["votes"][:, s, 0] > 0).all()
    assert len({whole["normals"][:, s].tobytes() for s in range(len(ks))}) == len(ks)      # the columns differ from one another


@pytest.mark.parametrize("args, word", [
    (["--estimator", "net", "--patch_radius", "0.05"], "--patch_radius belongs to --estimator pca / --estimator quadric"),
    (["--estimator", "hough", "--knn", "8", "--patch_radius", "0.05"], "--patch_radius belongs to"),
    (["--estimator", "pca", "--knn", "8", "--patch_radius", "0.05"], "--patch_radius belongs to"),
    (["--estimator", "pca", "--patch_radius", "0.01", "0.02", "0.03", "0.04", "0.05"], "1 to 4 positive finite numbers"),
    (["--estimator", "quadric", "--patch_radius", "0.01", "0"], "1 to 4 positive finite numbers"),
    (["--estimator", "pca", "--patch_radius", "inf"], "1 to 4 positive finite numbers"),
    (["--estimator", "pca", "--patch_radius", "nan"], "1 to 4 positive finite numbers")])
def test_patch_radius_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    assert e.value.code == 2 and word in capsys.readouterr().err
    assert not (tmp_path / "out").exists()                      # refused while parsing: nothing was created


def test_patch_radius_scale_is_checked_against_the_given_radii(tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    assert cli.build_parser().parse_args([]).patch_radius is None
    with pytest.raises(SystemExit, match="--pca_scale"):        # four radii: scales -4 .. 3
        cli.main(["--estimator", "pca", "--patch_radius", "0.01", "0.03", "0.05", "0.08", "--pca_scale", "4",
                  "--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
