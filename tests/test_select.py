"""The scale-selected plane fit without a GPU: every refusal of ``nesti_pca_select_nbr`` and ``nesti_pca_select_nbr_at`` through ctypes
(each returns before any device call), the ``ValueError``s of the Python layer, the parser errors of ``--knn_ladder`` and
``--select_slack``, the properties of the tests' restatement of the selection step (tests/_select_fixture.py), and the accuracy
conditions of the rule on the six clouds of DESIGN.md's table, in float64 reference arithmetic."""
import ctypes

import numpy as np
import pytest

import _select_fixture as sx

ENTRIES = ("nesti_pca_select_nbr", "nesti_pca_select_nbr_at")


# ---- 1. argument refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_need_no_device():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    dummy = np.zeros(8, np.float32)                                          # never dereferenced: the checks come first
    p = ctypes.c_void_p(dummy.ctypes.data)
    N, M, K = 1000, 100, 64
    good = tuple(range(1, 11))

    def ladder_arg(ks):
        return None if ks is None else (ctypes.c_int32 * max(1, len(ks)))(*ks)

    for entry in ENTRIES:
        at = entry.endswith("_at")

        def call(cloud=p, n=N, q=p, m=M, row0=0, nbr=p, K=K, ks=good, L=None, slack=0.0, outs=(p,) * 10):
            head = (cloud, n, q, m) + (() if at else (row0,))
            return getattr(lib, entry)(*head, nbr, K, ladder_arg(ks), len(ks) if L is None else L, slack, *outs, None)

        def refused(rc, word):
            msg = lib.nesti_last_error() or b""
            assert rc != 0 and word.encode() in msg and msg.startswith((entry + ":").encode()), (entry, rc, msg, word)

        # the errors of nesti_pca_normals_nbr
        refused(call(cloud=None), "null")
        refused(call(nbr=None), "null")
        refused(call(ks=None, L=3), "null")
        refused(call(n=0), "empty cloud")
        refused(call(n=-7), "empty cloud")
        refused(call(K=0), "K must be in 1 .. 256")
        refused(call(K=257), "K must be in 1 .. 256")
        refused(call(m=-1), "M must be")
        if at:
            refused(call(q=None), "null query_xyz_dev")
        else:
            refused(call(row0=-1), "query_row0")
            refused(call(q=None, row0=N - M + 1), "exceed the cloud")
        # the entry's own: the length of the ladder, its order and range, the slack
        for L in (0, -1, 33):
            refused(call(ks=tuple(range(1, 34)), L=L), "L must be in 1 .. 32")
        for ks in ((0, 16, 32), (-4,), (8, 32, 16), (8, 16, 16), (8, 16, K + 1), (K + 1,)):
            refused(call(ks=ks), "the ladder must be strictly ascending and in 1 .. K")
        for s in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
            refused(call(slack=s), "slack must be finite and >= 0")
        # M = 0 is a no-op at the ends of every range, with every output NULL too, and an argument error is still one
        assert call(q=None, m=0, ks=(1,)) == 0 and call(q=None, m=0, ks=tuple(range(33, 65)), slack=1e300) == 0
        assert call(q=None, m=0, K=256, ks=(255, 256), outs=(None,) * 10) == 0
        if not at:
            assert call(q=None, m=0, row0=N) == 0
        refused(call(q=None, m=0, ks=(8, 4)), "the ladder must be")
        refused(call(q=None, m=0, slack=np.nan), "slack")


# ---- 2. the Python layer ---------------------------------------------------------------------------------------------------------------

def test_python_layer_validates():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib, select
    assert select.DEFAULT_LADDER == (12, 16, 24, 32, 48, 64, 96, 128, 192, 256) == sx.DEFAULT_LADDER
    assert _lib.SELECT_MAX_L == 32
    assert select.check_ladder(select.DEFAULT_LADDER) == select.DEFAULT_LADDER and select.check_ladder(7) == (7,)
    assert select.check_ladder(np.arange(1, 33)) == tuple(range(1, 33)) and select.check_ladder([256]) == (256,)
    assert select.check_slack(0) == 0.0 and select.check_slack(1e300) == 1e300 and select.check_slack(np.float32(0.5)) == 0.5
    pts = np.zeros((10, 3), np.float32)
    for bad, word in (((), "1 .. 32 neighbour counts"), (tuple(range(1, 34)), "1 .. 32 neighbour counts"), ((8, 8), "strictly ascending"),
                      ((16, 8), "strictly ascending"), ((0, 8), "k must be an integer in 1 .. 256"), ((8, 257), "k must be"),
                      ((8, 12.5), "k must be"), ((True, 8), "k must be"), ("auto", "ladder must be an int or a sequence"),
                      (None, "ladder must be an int or a sequence"), (0, "k must be")):
        with pytest.raises(ValueError, match=word):
            select.check_ladder(bad)
        with pytest.raises(ValueError, match=word):
            select.select_normals(pts, ladder=bad)
    for bad in (-1e-9, -1, float("nan"), float("inf"), "loose", None, True):
        with pytest.raises(ValueError, match="slack must be a finite number >= 0"):
            select.check_slack(bad)
        with pytest.raises(ValueError, match="slack must be"):
            select.select_normals(pts, slack=bad)
    # the other arguments, all before any GPU work (this test runs without a GPU)
    with pytest.raises(ValueError, match="mutually exclusive"):
        select.select_normals(pts, pidx=[0, 1], queries=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="orient must be"):
        select.select_normals(pts, orient="up")
    with pytest.raises(ValueError):
        select.select_normals(pts, orient="viewpoint")                       # no viewpoint
    with pytest.raises(ValueError):
        select.select_normals(pts, orient="mst", orient_k=0)
    with pytest.raises(ValueError, match="smooth needs all points"):
        select.select_normals(pts, pidx=[0, 1], smooth=2)
    with pytest.raises(ValueError, match="smooth needs all points"):
        select.select_normals(pts, queries=np.zeros((2, 3), np.float32), smooth={"iters": 1})
    with pytest.raises(ValueError, match="iters"):
        select.select_normals(pts, smooth=0)
    with pytest.raises(ValueError, match="angle"):
        select.select_normals(pts, smooth={"angle": 91.0})
    v = select.selected_variation(np.array([[0.1, 0.2], [0.3, 0.4], [0.0, 0.0]], np.float32), np.array([1, 0, -1], np.int32))
    assert v.dtype == np.float32 and np.array_equal(v, np.array([0.2, 0.3, 0.0], np.float32))


# ---- 3. the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, word", [
    (["--knn_ladder", "auto"], "--knn_ladder belongs to --estimator pca"),
    (["--estimator", "net", "--knn_ladder", "16,32"], "--knn_ladder belongs to --estimator pca"),
    (["--estimator", "quadric", "--knn_ladder", "16,32"], "--knn_ladder belongs to --estimator pca"),
    (["--estimator", "hough", "--knn", "64", "--knn_ladder", "16,32"], "--knn_ladder belongs to --estimator pca"),
    (["--select_slack", "0.5"], "--select_slack belongs to --estimator pca --knn_ladder"),
    (["--estimator", "pca", "--select_slack", "0.5"], "--select_slack belongs to --estimator pca --knn_ladder"),
    (["--estimator", "pca", "--knn", "16", "--select_slack", "0.5"], "--select_slack belongs to --estimator pca --knn_ladder"),
    (["--estimator", "quadric", "--select_slack", "0"], "--select_slack belongs to --estimator pca --knn_ladder"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--knn", "16"], "--knn_ladder and --knn are mutually exclusive"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--patch_radius", "0.05"], "--knn_ladder and --patch_radius are mutually exclusive"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--pca_scale", "0"], "--knn_ladder and --pca_scale are mutually exclusive"),
    (["--estimator", "pca", "--knn_ladder", "32,16"], "strictly ascending"),
    (["--estimator", "pca", "--knn_ladder", "16,16"], "strictly ascending"),
    (["--estimator", "pca", "--knn_ladder", "0,16"], "k must be an integer in 1 .. 256"),
    (["--estimator", "pca", "--knn_ladder", "16,300"], "k must be an integer in 1 .. 256"),
    (["--estimator", "pca", "--knn_ladder", ",".join(map(str, range(1, 34)))], "1 .. 32 neighbour counts"),
    (["--estimator", "pca", "--knn_ladder", "16,many"], "--knn_ladder 16,many"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--select_slack", "-0.1"], "slack must be a finite number >= 0"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--select_slack", "nan"], "slack must be a finite number >= 0"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--select_slack", "inf"], "slack must be a finite number >= 0"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--depth_images", "1"], "--estimator pca does not take --depth_images 1"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--reproducible", "1"], "--estimator pca does not take --reproducible 1"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--subsample", "reference"], "--estimator pca does not take --subsample reference"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--subsample", "reference_host"], "does not take --subsample reference_host"),
    (["--estimator", "pca", "--knn_ladder", "auto", "--smooth", "1", "--sparse_patches", "1"], "--smooth does not go with --sparse_patches 1"),
])
def test_command_line_refusals(args, word, capsys, tmp_path):
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--results_path", str(tmp_path / "out"), "--dataset_path", str(tmp_path)])
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err and not (tmp_path / "out").exists()       # refused while parsing: nothing was created


def test_log_line_counts_the_chosen_neighbour_counts():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import cli
    line = cli.select_line("cube", 7, (12, 16, 24), 0.5, np.array([0, 2, 2, -1, 1, 2, 0], np.int32))
    assert line == ("scale-selected plane fit of cube: 7 rows, slack 0.5; chosen neighbour counts: 12: 2, 16: 1, 24: 3; "
                    "1 rows without a fit (written as 0 0 0)")


# ---- 4. the selection step ---------------------------------------------------------------------------------------------------------------

def _eig(v, total=0.5):
    """float32 eigenvalues (e0, e1, e2) whose score is close to v: the tests compare scores the fixture computes itself."""
    return np.array([v * total, 0.4 * (1 - v) * total, 0.6 * (1 - v) * total], np.float32)


def test_ties_go_to_the_larger_count_and_slack_widens_the_choice():
    # one row, five candidates; candidates 1 and 3 share the smallest score exactly (the same float32 eigenvalues)
    eig = np.stack([_eig(0.05), _eig(0.01), _eig(0.02), _eig(0.01), _eig(0.03)])[None]
    cnt = np.array([[12, 16, 24, 32, 48]], np.int32)
    rad = np.array([[0.1, 0.2, 0.3, 0.4, 0.5]], np.float32)
    nrm = np.arange(15, dtype=np.float32).reshape(1, 5, 3)
    v, ok = sx.scores(eig, cnt, rad)
    assert ok.all() and v[0, 1] == v[0, 3] == v[0].min()
    r = sx.select(eig, cnt, rad, 0.0, nrm)
    assert r["sel"][0] == 3 and r["k"][0] == 32 and r["radius"][0] == np.float32(0.4)
    assert np.array_equal(r["eig"][0], eig[0, 3]) and np.array_equal(r["normals"][0], nrm[0, 3])
    assert np.array_equal(r["variation_all"], v.astype(np.float32))
    # thr = v_min + v_min * slack: a slack of 1.5 reaches the score 0.02 but not 0.03; 2.5 reaches 0.03; a huge one everything
    assert sx.select(eig, cnt, rad, 0.5)["sel"][0] == 3
    assert sx.select(eig, cnt, rad, 1.5)["sel"][0] == 3 and v[0, 2] <= v[0, 1] + v[0, 1] * 1.5 < v[0, 4]
    assert sx.select(eig, cnt, rad, 2.5)["sel"][0] == 4
    assert sx.select(eig, cnt, rad, 1e300)["sel"][0] == 4
    # the threshold is the product then the sum, in float64: a score one ulp above it is not taken
    vmin = v[0, 1]
    slack = 0.3
    thr = vmin + vmin * slack
    assert sx.select(eig, cnt, rad, slack)["sel"][0] == 3 and not (v[0, 2] <= thr)


def test_short_prefixes_ineligible_candidates_and_rows_without_a_fit():
    # row 0: the prefix holds 20 entries, so the candidates from 24 on are the same fit (duplicate n_c): the largest of them is chosen
    # row 1: candidates with fewer than 3 neighbours, a radius of 0 or a zero sum are skipped even where their score would be the smallest
    # row 2: nothing is eligible
    L = 5
    eig = np.zeros((3, L, 3), np.float32)
    cnt = np.zeros((3, L), np.int32)
    rad = np.zeros((3, L), np.float32)
    eig[0] = [_eig(0.04), _eig(0.03), _eig(0.02), _eig(0.02), _eig(0.02)]
    cnt[0] = [12, 16, 20, 20, 20]
    rad[0] = [0.1, 0.2, 0.3, 0.3, 0.3]
    eig[1] = [_eig(0.001), _eig(0.002), np.zeros(3), _eig(0.2), _eig(0.3)]
    cnt[1] = [2, 16, 24, 32, 48]
    rad[1] = [0.1, 0.0, 0.3, 0.4, 0.5]
    cnt[2] = [1, 2, 2, 2, 2]
    rad[2] = [0.0, 0.1, 0.1, 0.1, 0.1]
    r = sx.select(eig, cnt, rad, 0.0)
    assert r["sel"].tolist() == [4, 3, -1] and r["k"].tolist() == [20, 32, 0]
    assert np.array_equal(r["variation_all"][1] > 0, [False, False, False, True, True])
    assert not r["variation_all"][2].any() and not r["eig"][2].any() and r["radius"][2] == 0
    # a huge finite slack picks the largest ELIGIBLE candidate: the product overflows to +inf, nothing becomes NaN
    big = sx.select(eig, cnt, rad, 1e300)
    assert big["sel"].tolist() == [4, 4, -1]
    # a score of exactly 0 (a perfect plane): thr = 0 + 0 * slack = 0 for every finite slack
    eig[1, 3] = [0.0, 0.2, 0.3]
    assert sx.select(eig, cnt, rad, 1e300)["sel"][1] == 3 and sx.select(eig, cnt, rad, 0.0)["sel"][1] == 3


def test_prefix_fits_agree_with_the_list_fixture():
    """``prefix_fits`` (running sums, vectorised) against tests/_knn_fixture.py's plane_lists (one sum per prefix) on lists with a -1, an
    index beyond the cloud, a shuffled row and a non-finite centre: the same counts and radii, eigenvalues to 1e-6 relative to the
    largest, normals to 1e-5."""
    import _knn_fixture as kx
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    pts, _ = synth.make_cloud("torus", n=400, seed=9, noise=0.003)
    centres = pts[::7].copy()
    nbr = kx.search(pts, centres, 64)[0]
    nbr[1, 20] = -1
    nbr[2, 2] = len(pts)
    nbr[3] = nbr[3, np.random.RandomState(1).permutation(64)]
    centres[4, 1] = np.nan
    ladder = (2, 3, 8, 21, 40, 64)
    mine, theirs = sx.prefix_fits(pts, centres, nbr, ladder), kx.plane_lists(pts, centres, nbr, ladder)
    assert np.array_equal(mine["count_all"], theirs["n_ball"]) and np.array_equal(mine["radius_all"], theirs["radius"])
    assert mine["count_all"][1].tolist() == [2, 3, 8, 20, 20, 20] and mine["count_all"][2].tolist() == [2] * 6 and not mine["count_all"][4].any()
    assert np.abs(mine["eig_all"] - theirs["eig"]).max() <= 1e-6 * theirs["eig"].max()
    cos = np.abs((mine["normals_all"].astype(np.float64) * theirs["normals"]).sum(-1))
    live = (theirs["normals"] != 0).any(-1)
    assert np.array_equal(live, (mine["normals_all"] != 0).any(-1)) and (1 - cos[live]).max() < 1e-5


# ---- 5. the accuracy conditions of the rule --------------------------------------------------------------------------------------------

def test_accuracy_conditions_in_reference_arithmetic():
    """The rule itself, in float64 ``eigh`` arithmetic over exact lists: on ``synth.make_cloud(shape, n=20000, seed=3, noise)``, every
    8th row as a centre against the full cloud, ladder (12, 16, 24, 32, 48, 64, 96, 128, 192, 256), slack 0, the share of rows within
    10 degrees of the analytic normal.  Conditions: selected >= best fixed count - 2.0 points on all six clouds; selected >= worst fixed
    count + 20 points on the five clouds other than the clean torus.

    Measured with this fixture on the 2500 centres (best fixed k: share / worst fixed k: share / selected); the worst margins are
    -1.16 points against the best fixed count (box 0.006) and +26.20 points over the worst (box 0.002):
      box 0          12: 92.48 / 256: 64.88 / 92.92
      box 0.002      16: 90.04 / 256: 65.12 / 91.32
      box 0.006      48: 83.12 /  12: 23.16 / 81.96
      torus 0       any: 100.00 / any: 100.00 / 100.00
      torus 0.002    48: 100.00 /  12: 68.00 / 99.32
      torus 0.006   192: 98.40 /  12: 12.12 / 97.80"""
    for shape, noise in sx.TABLE_CLOUDS:
        t = sx.table_cloud(shape, noise)
        fits = t["fits"]
        fixed = [sx.within_deg(fits["normals_all"][:, c], t["gt"]) for c in range(len(sx.DEFAULT_LADDER))]
        chosen = sx.select(fits["eig_all"], fits["count_all"], fits["radius_all"], 0.0, fits["normals_all"])
        selected = sx.within_deg(chosen["normals"], t["gt"])
        best, worst = int(np.argmax(fixed)), int(np.argmin(fixed))
        print("%s %g: best fixed %d: %.2f / worst fixed %d: %.2f / selected %.2f"
              % (shape, noise, sx.DEFAULT_LADDER[best], fixed[best], sx.DEFAULT_LADDER[worst], fixed[worst], selected))
        assert (chosen["sel"] >= 0).all()
        assert selected >= fixed[best] - 2.0, (shape, noise, selected, fixed)
        if (shape, noise) != ("torus", 0.0):
            assert selected >= fixed[worst] + 20.0, (shape, noise, selected, fixed)
