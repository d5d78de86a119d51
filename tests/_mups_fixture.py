"""The case table of the MuPS kernel tests (tests/test_mups_cases.py on the CPU, tests/test_gpu_mups_cases.py on the GPU) and the
yardstick they are judged by.  Everything here is numpy on seeded inputs: no GPU, no file.

A case is (grid, kind): grid 8 (variance 0.0156) or 3 (variance 0.111), kind one of ``KINDS``.  Every case has the same B = 7 rows of
S = 2 scales with P = 130 patch rows (not a multiple of the kernels' 64-row chunk, more than two chunks):

    n_eff = [[P, P], [P-1, P-2], [1, 2], [63, 64], [65, 127], [0, 5], [3, 0]]

The kernels sweep ``nrows = min(n_eff + 1, P)`` rows (row n_eff, the first padding row, counts as a point: ``mask = r > n_eff``), so
these give: no masked row (P, P-1); a masked row that is exactly row P-1 (P-2); nrows of 2 and 3 (the pair loop's shortest even and
odd sweeps); nrows of 64, 65 and 66 (a whole chunk, a chunk and an odd tail of one, a chunk and a pair); empty scales beside live ones.
Rows at or beyond n_eff hold the reference's zero padding, except in ``pts`` of batch rows 3 and 4, where the rows STRICTLY beyond
n_eff hold NaN and +-inf: the reference masks them and the kernels never stage them.  ``pts_clean`` is the same input without that
fill; the expected values are computed from it (the numpy restatement multiplies a masked row by 0, which a NaN survives).

The layout case (``layout_case``) is S = 4, P = 64, B = 3: 80 channels, into the second 64-channel group of the pair layouts.

Expected value: ``oracle.mups_ref.mups_assemble`` at float64; exact zeros where n_eff == 0.

Yardstick ``e32[row, scale, channel]``: the maximum over the Gaussians of the larger of the errors, against float64, of the two float32
restatements the oracle has -- ``mups_literal(dtype=float32)`` and ``mups_separable(dtype=float32)``; where the literal one is not
finite on a (row, scale) (its three-axis exponent underflows for points outside the 8^3 grid), the separable one alone.  The bound
of a kernel output is ``4 e32 + 2^-22``: the kernel is a third float32 evaluation order (64-row chunks, rows in pairs, four wave
partials in the L2 norm, the device's expf and division), the two restatements already differ by up to 16x in single channels, and
the floor covers channels where both happen to be exact.  The yardstick never sees a kernel's output.

A cell (row, scale, channel) whose bound exceeds ``ILL`` = 5e-6 (the tolerance of tests/test_gpu_mups.py) is ill-conditioned: a
statistic that cancels to ~0, where the signed square root turns an error of 1e-8 into 1e-4.  No case may have more than ``ILL_CAP``
of its cells so; if a seed breaks that, the seed changes, not the cap."""
import numpy as np

GRIDS = {8: 0.0156, 3: 0.111}
KINDS = ("uniform", "ball_surface", "centres", "identical", "octant", "outside", "tiny")
S, P = 2, 130
N_EFF = np.array([[P, P], [P - 1, P - 2], [1, 2], [63, 64], [65, 127], [0, 5], [3, 0]], np.int32)
GARBAGE_ROWS = (3, 4)
LAYOUT_S, LAYOUT_P = 4, 64
LAYOUT_N_EFF = np.array([[64, 64, 64, 64], [1, 63, 0, 33], [5, 0, 0, 64]], np.int32)
FACTOR, FLOOR = 4.0, 2.0 ** -22
ILL, ILL_CAP = 5e-6, 0.10
SEED = 5          # must leave uniform and ball_surface without an ill-conditioned cell and every case under ILL_CAP (tests/test_mups_cases.py)
STATS = (["max Q", "sum Q"] + ["%s of mu %s" % (r, a) for r in ("max", "min", "sum") for a in "xyz"]
         + ["%s of sigma %s" % (r, a) for r in ("max", "min", "sum") for a in "xyz"])      # the 20 channels of a scale, in order

_cache = {}


def axis_centres(grid_n):
    """The grid's per-axis Gaussian centres (float64, ascending)."""
    from oracle import mups_ref
    return mups_ref.grid_gmm(grid_n, GRIDS[grid_n])[1][::grid_n * grid_n, 0].copy()


def config(grid_n, n_scales=S, num_point=P):
    """The ``NestiConfig`` of a case: the published experts model on ``grid_n``^3 Gaussians with ``n_scales`` radii."""
    from nesti_net_amd.config import NestiConfig
    if n_scales == 3:
        return NestiConfig(num_point=num_point, n_gaussians=grid_n, gmm_variance=GRIDS[grid_n])
    return NestiConfig(patch_radius=[0.01 * (i + 1) for i in range(n_scales)], num_point=num_point, n_gaussians=grid_n,
                       gmm_variance=GRIDS[grid_n], n_experts=1, expert_dict={0: list(range(n_scales))})


def nrows(n_eff, num_point):
    """Rows the kernels sweep per (row, scale): min(n_eff + 1, P), 0 for an empty scale."""
    n_eff = np.asarray(n_eff)
    return np.where(n_eff > 0, np.minimum(n_eff + 1, num_point), 0)


def _coords(rng, kind, grid_n, shape):
    """[B, S, P, 3] float64 coordinates of ``kind`` (the float32 cast comes later)."""
    full = tuple(shape) + (3,)
    if kind == "uniform":
        return rng.uniform(-0.7, 0.7, full)
    if kind == "ball_surface":              # unit vectors: the largest norm the product path's (p - c) / r produces
        v = rng.normal(size=full)
        return v / np.linalg.norm(v, axis=-1, keepdims=True)
    if kind == "centres":                   # on the Gaussian centres, the origin and the cube's faces: statistics cancel by symmetry
        values = np.concatenate([axis_centres(grid_n), [-1.0, 0.0, 1.0]])
        return values[rng.randint(0, len(values), full)]
    if kind == "identical":                 # one point per patch, repeated: max = min, sum = n x that
        return np.broadcast_to(rng.uniform(-0.7, 0.7, (shape[0], shape[1], 1, 3)), full).copy()
    if kind == "octant":                    # most Gaussians see every d with one sign: the masked rows' 0 decides the min or max
        return rng.uniform(0.5, 1.0, full)
    if kind == "outside":                   # beyond the grid, inside the stated domain (include/nesti_hip.h: nesti_mups_forward) ...
        x = rng.uniform(-2.0, 2.0, full)
        x[:, :, 0, :] = 2.0 * rng.choice([-1.0, 1.0], (shape[0], shape[1], 3))      # ... and one corner of that domain per patch
        return x
    if kind == "tiny":
        return rng.uniform(-1e-3, 1e-3, full)
    raise KeyError(kind)


def make_points(grid_n, kind, n_eff, num_point, seed=SEED):
    """(pts, pts_clean) [B, S*P, 3] float32 for ``n_eff`` [B, S]: zero padding from row n_eff on; in ``pts`` the rows beyond n_eff of
    ``GARBAGE_ROWS`` hold NaN / +inf / -inf instead."""
    n_eff = np.asarray(n_eff)
    B, n_scales = n_eff.shape
    rng = np.random.RandomState([seed, grid_n, KINDS.index(kind), n_scales, num_point])
    x = _coords(rng, kind, grid_n, (B, n_scales, num_point)).astype(np.float32)
    r = np.arange(num_point)[None, None, :]
    x[r >= n_eff[:, :, None]] = 0.0
    clean = x.copy()
    fill = np.array([np.nan, np.inf, -np.inf, np.nan, 3.0e38, -np.inf, np.inf], np.float32)
    junk = fill[(np.arange(num_point * 3) % len(fill))].reshape(num_point, 3)
    for b in GARBAGE_ROWS:
        if b < B:
            for s in range(n_scales):
                x[b, s, n_eff[b, s] + 1:] = junk[n_eff[b, s] + 1:]
    return x.reshape(B, n_scales * num_point, 3), clean.reshape(B, n_scales * num_point, 3)


def expect(pts_clean, n_eff, grid_n):
    """ref [B,R,R,R,S,20] float64, e32 / bound [B,S,20], the float64 gap between the two forms, and the finiteness of the float32
    restatements per (row, scale)."""
    from oracle import mups_ref as M
    n_eff = np.asarray(n_eff)
    B, n_scales = n_eff.shape
    live = n_eff > 0
    n1 = np.maximum(n_eff, 1)          # an empty scale divides by n_eff = 0 in the reference; the kernels write zeros
    var = GRIDS[grid_n]

    def run(fn, dtype):
        with np.errstate(all="ignore"):
            o = M.mups_assemble(pts_clean, n1, n_scales, grid_n=grid_n, variance=var, dtype=dtype, fn=fn, workers=1)      # one thread: errstate is per thread
        o = o.reshape(B, grid_n, grid_n, grid_n, n_scales, 20).astype(np.float64)
        np.moveaxis(o, 4, 1)[~live] = 0.0          # a view indexed [row, scale]
        return o

    ref, sep64 = run(M.mups_literal, np.float64), run(M.mups_separable, np.float64)
    lit32, sep32 = run(M.mups_literal, np.float32), run(M.mups_separable, np.float32)
    lit_finite = np.isfinite(lit32).all(axis=(1, 2, 3, 5))          # [B, S]
    sep_finite = np.isfinite(sep32).all(axis=(1, 2, 3, 5))
    with np.errstate(invalid="ignore"):
        e_lit = np.abs(lit32 - ref).max(axis=(1, 2, 3))             # [B, S, 20]
        e_sep = np.abs(sep32 - ref).max(axis=(1, 2, 3))
    e_lit = np.where(lit_finite[:, :, None], e_lit, 0.0)
    e32 = np.maximum(e_lit, e_sep)
    return {"ref": ref, "e32": e32, "bound": FACTOR * e32 + FLOOR, "forms_gap64": float(np.abs(sep64 - ref).max()),
            "lit32_finite": lit_finite, "sep32_finite": sep_finite, "live": live}


def _build(grid_n, kind, n_eff, num_point):
    pts, clean = make_points(grid_n, kind, n_eff, num_point)
    c = {"grid": grid_n, "kind": kind, "n_eff": n_eff.copy(), "S": n_eff.shape[1], "P": num_point, "pts": pts, "pts_clean": clean}
    c.update(expect(clean, n_eff, grid_n))
    c["ill"] = c["bound"] > ILL
    return c


def case(grid_n, kind):
    """The case, built once per process and shared: treat it as read-only."""
    key = (grid_n, kind)
    if key not in _cache:
        _cache[key] = _build(grid_n, kind, N_EFF, P)
    return _cache[key]


def layout_case(grid_n):
    """S = 4, P = 64, uniform coordinates."""
    key = (grid_n, "layout")
    if key not in _cache:
        _cache[key] = _build(grid_n, "uniform", LAYOUT_N_EFF, LAYOUT_P)
    return _cache[key]


def gaussian_view(got, c):
    """A kernel's dense f32 output [B,R,R,R,20 S] as [B,R,R,R,S,20] float64."""
    g = c["grid"]
    return np.asarray(got, np.float64).reshape(len(c["n_eff"]), g, g, g, c["S"], 20)


def ratios(got, c):
    """error / bound per (row, Gaussian i, j, k, scale, channel); NaN-safe (a non-finite output gives inf)."""
    with np.errstate(invalid="ignore"):
        err = np.abs(gaussian_view(got, c) - c["ref"])
    err = np.where(np.isfinite(err), err, np.inf)
    return err / c["bound"][:, None, None, None, :, :]


def violations(got, c, limit=8):
    """[] if every output is within its bound, else up to ``limit`` lines naming row, scale, statistic and Gaussian, worst first."""
    r = ratios(got, c)
    bad = np.argwhere(r > 1.0)
    if not len(bad):
        return []
    order = np.argsort(-r[tuple(bad.T)], kind="stable")[:limit]
    g, lines = gaussian_view(got, c), []
    for b, i, j, k, s, ch in bad[order]:
        lines.append("row %d (n_eff %d) scale %d %s, Gaussian (%d, %d, %d): got %.9g, expected %.9g, error %.3g > bound %.3g"
                     % (b, c["n_eff"][b, s], s, STATS[ch], i, j, k, g[b, i, j, k, s, ch], c["ref"][b, i, j, k, s, ch],
                        abs(g[b, i, j, k, s, ch] - c["ref"][b, i, j, k, s, ch]), c["bound"][b, s, ch]))
    return ["%d of %d outputs beyond 4 e32 + 2^-22:" % (len(bad), r.size)] + lines


# ---- the small cloud of the fused-kernel test ------------------------------------------------------------------------------------
# Position queries at the centres of well-separated clusters inside the unit cube (two corner points pin the bounding box, so the
# radii are 0.01 / 0.03 / 0.05 x sqrt(3)).  Cluster q has a_q points within 0.8 r_0 of its centre, b_q between 1.2 r_0 and 0.8 r_1
# and c_q between 1.2 r_1 and 0.8 r_2: ball sizes (a, a + b, a + b + c), nothing near a ball's surface.
CLOUD_P = 130
CLOUD_COUNTS = np.array([[0, 1, 62], [1, 62, 1], [0, 0, 64], [63, 2, 200], [0, 0, 0], [64, 66, 70], [130, 1, 0], [0, 65, 300]], np.int32)


def cloud_ball_sizes():
    return np.cumsum(CLOUD_COUNTS, axis=1).astype(np.int32)


def make_cloud(seed=SEED):
    """{cfg, pts [N,3] f32, queries [M,3] f32, r_abs}: see above."""
    from oracle import patches_ref
    cfg = config(8, 3, CLOUD_P)
    rng = np.random.RandomState([seed, 99])
    r = [np.sqrt(3.0) * rad for rad in cfg.patch_radius]
    lo, hi = [0.0, 1.2 * r[0], 1.2 * r[1]], [0.8 * r[0], 0.8 * r[1], 0.8 * r[2]]
    centres = np.array([[x, y, z] for x in (0.2, 0.5, 0.8) for y in (0.25, 0.75) for z in (0.3, 0.7)])[:len(CLOUD_COUNTS)]
    rows = [np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])]
    for c, counts in zip(centres, CLOUD_COUNTS):
        for s, n in enumerate(counts):
            v = rng.normal(size=(n, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            rows.append(c + v * rng.uniform(lo[s], hi[s], (n, 1)))
    pts = np.ascontiguousarray(np.concatenate(rows).astype(np.float32))
    pts = pts[np.random.RandomState([seed, 100]).permutation(len(pts))]
    bbdiag, r_abs = patches_ref.patch_radii(pts, cfg.patch_radius)
    return {"cfg": cfg, "pts": pts, "queries": np.ascontiguousarray(centres.astype(np.float32)), "r_abs": r_abs, "bbdiag": bbdiag}
