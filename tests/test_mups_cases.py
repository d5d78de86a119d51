"""The case table of tests/_mups_fixture.py on the CPU: what the GPU tests (tests/test_gpu_mups_cases.py) rely on is checked here, where
no kernel runs -- the inputs are deterministic, the two forms of the restatement agree at float64, the separable float32 restatement
(the form the kernels use) is finite on every case, few cells are ill-conditioned, and every edge the table claims is in it."""
import numpy as np
import pytest

import _mups_fixture as F

ALL = [(g, k) for g in F.GRIDS for k in F.KINDS]
_ids = ["%d-%s" % gk for gk in ALL]


def _cases():
    return [F.case(g, k) for g, k in ALL] + [F.layout_case(g) for g in F.GRIDS]


def test_fixture_is_deterministic():
    for g, k in ALL:
        a, a_clean = F.make_points(g, k, F.N_EFF, F.P)
        c = F.case(g, k)
        assert np.array_equal(a.view(np.uint32), c["pts"].view(np.uint32))
        assert np.array_equal(a_clean.view(np.uint32), c["pts_clean"].view(np.uint32))
    g, k = 3, "centres"
    again = F.expect(F.case(g, k)["pts_clean"], F.N_EFF, g)
    for name in ("ref", "e32", "bound"):
        assert np.array_equal(again[name], F.case(g, k)[name])
    cloud = F.make_cloud()
    assert np.array_equal(cloud["pts"], F.make_cloud()["pts"])


def test_padding_and_masked_fill():
    """Zero rows from n_eff on; strictly beyond n_eff of rows 3 and 4 only, every row holds a NaN or an infinity (next to the odd
    finite 3e38); nothing of it in the clean copy."""
    for c in _cases():
        B, S, P = len(c["n_eff"]), c["S"], c["P"]
        x, clean = c["pts"].reshape(B, S, P, 3), c["pts_clean"].reshape(B, S, P, 3)
        assert np.isfinite(clean).all()
        for b in range(B):
            for s in range(S):
                m = c["n_eff"][b, s]
                assert not clean[b, s, m:].any()
                assert np.array_equal(x[b, s, :m + 1], clean[b, s, :m + 1])          # row n_eff itself stays 0: the reference counts it
                if b in F.GARBAGE_ROWS and m + 1 < P:
                    assert (~np.isfinite(x[b, s, m + 1:])).any(axis=1).all()           # every filled row has a non-finite coordinate
                    if m + 4 < P:
                        assert np.isnan(x[b, s, m + 1:]).any() and np.isinf(x[b, s, m + 1:]).any()
                else:
                    assert np.array_equal(x[b, s], clean[b, s])
    masked = F.P - F.nrows(F.N_EFF, F.P)[list(F.GARBAGE_ROWS)]
    assert (masked > 0).all()                      # every scale of the two rows has a masked row to fill


def test_kinds_are_what_the_table_says():
    for g in F.GRIDS:
        live = (np.arange(F.P)[None, None, :] < F.N_EFF[:, :, None])
        x = {k: F.case(g, k)["pts_clean"].reshape(7, F.S, F.P, 3)[live] for k in F.KINDS}
        assert np.abs(x["uniform"]).max() <= 0.7
        assert np.abs(np.linalg.norm(x["ball_surface"].astype(np.float64), axis=1) - 1).max() < 1e-6
        values = np.concatenate([F.axis_centres(g), [-1.0, 0.0, 1.0]]).astype(np.float32)
        assert np.isin(x["centres"], values).all() and set(np.unique(x["centres"])) == set(values)
        ident = F.case(g, "identical")["pts_clean"].reshape(7, F.S, F.P, 3)
        for b in range(7):
            for s in range(F.S):
                m = F.N_EFF[b, s]
                assert (ident[b, s, :m] == ident[b, s, 0]).all()
        assert x["octant"].min() >= 0.5 and x["octant"].max() <= 1.0
        assert np.abs(x["outside"]).max() == 2.0 and (np.abs(x["outside"]) > 1.0).mean() > 0.4
        assert np.abs(x["tiny"]).max() <= 1e-3 and x["tiny"].any()


def test_every_claimed_n_eff_pattern_is_present():
    n = F.nrows(F.N_EFF, F.P)
    for want in (2, 3, 64, 65, 66, F.P):
        assert (n == want).any(), want
    assert F.P % 64 and F.P > 128
    assert ((F.N_EFF == F.P - 2) & (n == F.P - 1)).any()                    # the only masked row is row P-1
    assert (((n > 0) & (n < F.P)).any() and (F.N_EFF == F.P).any() and (F.N_EFF == F.P - 1).any())   # with and without masked rows
    assert ((F.N_EFF == 0).any(axis=1) & (F.N_EFF > 0).any(axis=1)).sum() >= 2                       # an empty scale beside a live one
    ln = F.nrows(F.LAYOUT_N_EFF, F.LAYOUT_P)
    assert F.LAYOUT_S == 4 and 20 * F.LAYOUT_S > 64 and (F.LAYOUT_N_EFF[:, 3] > 0).all()             # live channels in the second group
    assert (ln == F.LAYOUT_P).any() and (ln == 2).any() and (ln == 0).any() and (ln == 34).any()


@pytest.mark.parametrize("g,k", ALL, ids=_ids)
def test_forms_agree_at_float64(g, k):
    assert F.case(g, k)["forms_gap64"] <= 1e-12


def test_forms_agree_at_float64_on_the_layout_case():
    for g in F.GRIDS:
        assert F.layout_case(g)["forms_gap64"] <= 1e-12


def test_separable_float32_is_finite_everywhere_the_literal_one_is_not():
    for c in _cases():
        assert c["sep32_finite"].all(), (c["grid"], c["kind"])
        assert np.isfinite(c["ref"]).all() and np.isfinite(c["bound"]).all()
    lit = F.case(8, "outside")["lit32_finite"]
    print("8^3 outside: literal float32 finite per (row, scale):", lit.tolist())
    assert not lit[F.case(8, "outside")["live"]].any()          # every live patch holds a corner of [-2, 2]^3: 0 / 0 in the literal form
    for g, k in ALL:
        if (g, k) != (8, "outside"):
            assert F.case(g, k)["lit32_finite"].all(), (g, k)


def test_empty_scales_expect_exact_zeros_and_the_bound_has_its_floor():
    for c in _cases():
        dead = ~c["live"]
        assert dead.any()
        assert not np.moveaxis(c["ref"], 4, 1)[dead].any() and not c["e32"][dead].any()
        assert (c["bound"] >= F.FLOOR).all() and np.array_equal(c["bound"], 4 * c["e32"] + 2.0 ** -22)


def test_ill_conditioned_cells_are_few():
    worst = 0.0
    for c in _cases():
        share = c["ill"].mean()
        print("%d^3 %-12s S=%d largest e32 %.3g, median bound %.3g, largest bound %.3g, ill-conditioned %.4f"
              % (c["grid"], c["kind"], c["S"], c["e32"].max(), np.median(c["bound"]), c["bound"].max(), share))
        assert share <= F.ILL_CAP, (c["grid"], c["kind"])
        worst = max(worst, share)
        if c["kind"] in ("uniform", "ball_surface"):
            assert not c["ill"].any(), (c["grid"], c["kind"], np.argwhere(c["ill"]).tolist())
    assert worst > 0              # the crafted cases do reach cells the fixed 5e-6 tolerance could not have judged


def test_violations_name_the_cell():
    """The checker the GPU tests use, on a perturbed copy of the expected values: one output moved by twice its bound is the one named."""
    c = F.case(3, "octant")
    assert F.violations(c["ref"].reshape(7, 3, 3, 3, 20 * F.S), c) == []
    bad = c["ref"].copy()
    bad[1, 2, 0, 1, 1, 6] += 2 * c["bound"][1, 1, 6]
    lines = F.violations(bad.reshape(7, 3, 3, 3, 20 * F.S), c)
    assert len(lines) == 2 and lines[0].startswith("1 of ")
    assert "row 1 (n_eff %d) scale 1 min of mu y, Gaussian (2, 0, 1)" % F.N_EFF[1, 1] in lines[1]
    bad[0, 0, 0, 0, 0, 0] = np.nan
    assert len(F.violations(bad.reshape(7, 3, 3, 3, 20 * F.S), c)) == 3
    assert F.STATS[0] == "max Q" and F.STATS[1] == "sum Q" and F.STATS[11] == "max of sigma x" and len(F.STATS) == 20


def test_cloud_of_the_fused_test_has_the_claimed_ball_sizes():
    """Brute force in float64: the position queries see balls of 0, 1, 63, 64, 65, P and more than P points, empty scales beside live
    ones and one query with no neighbourhood at all; no point within 15 % of a ball's surface."""
    cl = F.make_cloud()
    assert 200 < len(cl["pts"]) < 2000
    assert cl["pts"].min() == 0.0 and cl["pts"].max() == 1.0 and abs(cl["bbdiag"] - np.sqrt(3.0)) < 1e-6
    d = np.linalg.norm(cl["pts"].astype(np.float64)[None] - cl["queries"].astype(np.float64)[:, None], axis=2)
    n_ball = np.stack([(d <= r).sum(axis=1) for r in cl["r_abs"]], axis=1)
    assert np.array_equal(n_ball, F.cloud_ball_sizes())
    for r in cl["r_abs"]:
        assert not ((d > 0.85 * r) & (d < 1.15 * r)).any()
    n_eff = np.minimum(n_ball, F.CLOUD_P)
    for want in (0, 1, 63, 64, 65, F.CLOUD_P):
        assert (n_eff == want).any(), want
    assert (n_ball > F.CLOUD_P).any() and (n_ball == F.CLOUD_P).any()          # P by the cap and P exactly
    assert not n_ball[4].any() and ((n_ball == 0).any(axis=1) & (n_ball > 0).any(axis=1)).any()
