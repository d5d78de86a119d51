"""The fixture of the position-query tests (tests/test_gpu_query_positions.py and its two-rank worker), and the tests' OWN
restatement of a position query on the CPU: ``cKDTree(pts, 10).query_ball_point(position, r)`` as the reference's line
``utils/pcpnet_dataset.py:304`` would answer for a position, keys from ``oracle.patches_ref.subsample_hash`` on the patch row,
``(pts[inds] - position) / float32(r)``.

Cloud: the 20 000-point noisy torus.  Two query sets:
  jittered  pts[::40] (500 rows) + N(0, 0.02 x bbdiag): rows with every ball empty, rows whose smallest ball is empty but not the
            largest, rows whose largest ball holds more than P points, rows whose largest ball holds 1 .. P points;
  faces     the 20 extreme points of each bounding-box face pushed outward by {0.25, 0.9, 1.0, 1.1, 2.5, 50} x r_max (720 rows):
            centres outside the search grid's bounding box, one cell out and further."""
import numpy as np

P = 64
PUSH = (0.25, 0.9, 1.0, 1.1, 2.5, 50.0)


def make():
    """{cfg, pts, bbdiag, r_abs, jittered [500,3], faces [720,3]}; everything float32 / Python floats like the product computes them."""
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import synth
    from nesti_net_amd.config import NestiConfig
    from oracle import patches_ref
    cfg = NestiConfig(num_point=P)
    pts = synth.make_cloud("torus", n=20000, seed=77, noise=0.00125)[0]
    bbdiag, r_abs = patches_ref.patch_radii(pts, cfg.patch_radius)
    base = pts[::40]
    jit = np.random.RandomState(5).normal(0, 0.02 * bbdiag, size=base.shape)
    jittered = np.ascontiguousarray((base + jit).astype(np.float32))
    r_max = max(r_abs)
    rows = []
    for axis in range(3):
        order = np.argsort(pts[:, axis], kind="stable")
        for sign, ext in ((-1.0, order[:20]), (1.0, order[-20:])):
            for f in PUSH:
                q = pts[ext].astype(np.float64)
                q[:, axis] += sign * f * r_max
                rows.append(q)
    faces = np.ascontiguousarray(np.concatenate(rows).astype(np.float32))
    assert jittered.shape == (500, 3) and faces.shape == (720, 3)
    return {"cfg": cfg, "pts": pts, "bbdiag": bbdiag, "r_abs": r_abs, "jittered": jittered, "faces": faces}


def extract_at(pts, positions, r_abs, n_keep, seed, rows=None, tree=None):
    """Patches at ``positions`` [M,3] f32 -> points [M,S*P,3] f32, n_eff [M,S], nbr [M,S*P] (-1 padded), n_ball [M,S].  A scale
    with an empty ball: n_eff 0, rows zero."""
    from scipy import spatial
    from oracle.patches_ref import subsample_hash
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    tree = tree or spatial.cKDTree(pts, 10)
    M, S = len(positions), len(r_abs)
    points = np.zeros((M, S * n_keep, 3), np.float32)
    n_eff = np.zeros((M, S), np.int32)
    nbr = np.full((M, S * n_keep), -1, np.int32)
    n_ball = np.zeros((M, S), np.int32)
    for q in range(M):
        c = positions[q]
        for s, rad in enumerate(r_abs):
            inds = np.array(tree.query_ball_point(c, rad), dtype=np.int64)
            n_ball[q, s] = len(inds)
            count = min(n_keep, len(inds))
            n_eff[q, s] = count
            if not count:
                continue
            h = subsample_hash(seed, q if rows is None else int(rows[q]), s, inds)
            inds = inds[np.lexsort((inds, h))[:count]]
            nbr[q, s * n_keep:s * n_keep + count] = inds
            points[q, s * n_keep:s * n_keep + count] = (pts[inds] - c) / np.float32(rad)
    return points, n_eff, nbr, n_ball


def classes(n_ball, n_keep=P):
    """Row masks: every ball empty / smallest empty but not the largest / largest above P / largest in 1 .. P."""
    largest, smallest = n_ball[:, -1], n_ball[:, 0]
    return {"all_empty": (n_ball == 0).all(axis=1), "partly_empty": (smallest == 0) & (largest > 0),
            "over_P": largest > n_keep, "under_P": (largest >= 1) & (largest <= n_keep)}
