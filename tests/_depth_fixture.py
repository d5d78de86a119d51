"""The fixture of the depth-image tests (tests/test_depth.py, tests/test_gpu_depth.py) and the tests' OWN restatement of the three
depth entries on the CPU, written from their definition (include/nesti_hip.h, DESIGN.md 2 "Depth images") in numpy float64:

  valid pixel      z = float64(raw) * depth_scale finite, > 0 and inside [z_near, z_far]
  back-projection  xc = ((u - cx) * z) / fx, yc = ((v - cy) * z) / fy, zc = z; with a pose T [3,4]
                   X_r = ((T[r,0] * xc + T[r,1] * yc) + T[r,2] * zc) + T[r,3]; then .astype(float32)
  order            np.flatnonzero(valid): row-major pixel order; pix = v W + u, rank = cloud row of a pixel or -1,
                   qidx = rank of the valid pixels with v % stride == 0 and u % stride == 0
  projection       camera coordinates (through T if given), u = floor(((xc * fx) / zc + cx) + 0.5), v likewise; a row lands iff its
                   floats and zc are finite, zc > 0 and the pixel is inside; per pixel the smallest (bits of float32(zc), row) wins

numpy evaluates every product, quotient and sum of an expression on its own, which is the rounding the definition asks for: every
step below is a separate numpy operation on float64 arrays.  0-based pixels: u = column, v = row.

The scene is analytic: a sphere of radius 0.6 at (0, 0, 2.2) in front of the plane z = 3 + 0.3 x, seen by fx = fy = 120, cx = 63.5,
cy = 47.5 on 96 x 128 pixels, stored as uint16 millimetres (depth_scale 1e-3) and as float32 metres (depth_scale 1).  Holes: a
9 x 13 rectangle of zeros, every 97th pixel zero, rows 40 .. 43 entirely zero; the float version also has one NaN, one +inf and one
negative depth."""
import numpy as np

H, W = 96, 128
FX = FY = 120.0
CX, CY = 63.5, 47.5
SPHERE_C, SPHERE_R = (0.0, 0.0, 2.2), 0.6
HOLE = (slice(20, 29), slice(30, 43))          # 9 x 13
EMPTY_ROWS = slice(40, 44)
NAN_AT, INF_AT, NEG_AT = (5, 7), (50, 100), (90, 3)


def camera(kind, pose=None, z_near=0.0, z_far=np.inf):
    """The fixture's camera as a plain dict (the tests build ``depth.Camera(**d)`` from it)."""
    return {"fx": FX, "fy": FY, "cx": CX, "cy": CY, "depth_scale": 1e-3 if kind == "u16" else 1.0, "z_near": z_near, "z_far": z_far,
            "pose": pose}


def scene_z():
    """Analytic depth [H,W] float64 in metres: the nearer of the sphere and the plane along each pixel's ray (x/z, y/z, 1)."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = (u - CX) / FX, (v - CY) / FY
    plane = 3.0 / (1.0 - 0.3 * dx)                                   # z = 3 + 0.3 x with x = z dx
    c = np.array(SPHERE_C)
    dd = dx * dx + dy * dy + 1.0
    dc = dx * c[0] + dy * c[1] + c[2]
    disc = dc * dc - dd * (c @ c - SPHERE_R ** 2)
    sphere = np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0.0))) / dd, np.inf)
    return np.minimum(plane, sphere)


def scene(kind):
    """The depth image: ``'u16'`` millimetres or ``'f32'`` metres, holes cut."""
    z = scene_z()
    d = np.round(z * 1000.0).astype(np.uint16) if kind == "u16" else z.astype(np.float32)
    d = d.copy()
    d[HOLE] = 0
    d.reshape(-1)[::97] = 0
    d[EMPTY_ROWS] = 0
    if kind == "f32":
        d[NAN_AT], d[INF_AT], d[NEG_AT] = np.nan, np.inf, -1.5
    return d


def rigid_pose(seed):
    """A random rotation (QR of a Gaussian matrix, det +1) and a translation of a few metres -> float64 [3,4]."""
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.ascontiguousarray(np.concatenate([q, rs.uniform(-3.0, 3.0, size=(3, 1))], axis=1))


def inverse_pose(T):
    R, t = T[:, :3], T[:, 3]
    return np.ascontiguousarray(np.concatenate([R.T, -(R.T @ t)[:, None]], axis=1))


def rigid(T, x, y, z):
    out = []
    for r in range(3):
        a = T[r, 0] * x
        b = T[r, 1] * y
        s = a + b
        c = T[r, 2] * z
        s = s + c
        out.append(s + T[r, 3])
    return out


def back_project(depth, cam, stride=1):
    """{xyz [n,3] f32, pix [n] i32, rank [H W] i32, qidx [q] i32, n_valid, n_queries} of ``depth`` [H,W] through the dict ``cam``."""
    h, w = depth.shape
    with np.errstate(invalid="ignore", over="ignore"):
        z = depth.astype(np.float64) * np.float64(cam["depth_scale"])
        valid = np.isfinite(depth.astype(np.float64)) & np.isfinite(z) & (z > 0) & (z >= cam["z_near"]) & (z <= cam["z_far"])
    pix = np.flatnonzero(valid.reshape(-1))
    v, u = pix // w, pix % w
    zz = z.reshape(-1)[pix]
    xn = (u.astype(np.float64) - cam["cx"]) * zz
    yn = (v.astype(np.float64) - cam["cy"]) * zz
    x = xn / cam["fx"]
    y = yn / cam["fy"]
    if cam.get("pose") is not None:
        x, y, zz = rigid(np.asarray(cam["pose"], np.float64), x, y, zz)
    xyz = np.stack([x, y, zz], axis=1).astype(np.float32).reshape(-1, 3)
    rank = np.full(h * w, -1, np.int32)
    rank[pix] = np.arange(len(pix), dtype=np.int32)
    on = (v % stride == 0) & (u % stride == 0)
    qidx = rank[pix[on]]
    return {"xyz": np.ascontiguousarray(xyz), "pix": pix.astype(np.int32), "rank": rank, "qidx": qidx.astype(np.int32),
            "n_valid": len(pix), "n_queries": int(on.sum())}


def scatter(rows, pix, h, w, fill):
    """rows [M] / [M,C] at the pixels pix [M] of an image of ``fill``; an entry outside [0, h w) is skipped."""
    rows = np.asarray(rows)
    C = 1 if rows.ndim == 1 else rows.shape[1]
    img = np.empty((h * w, C), rows.dtype)
    img[:] = np.asarray(fill, rows.dtype)
    ok = (pix >= 0) & (pix < h * w)
    img[pix[ok]] = rows.reshape(len(rows), C)[ok]
    return img.reshape((h, w) if rows.ndim == 1 else (h, w, C))


def project(xyz, cam, h, w):
    """index_image [h,w] i32 of the cloud ``xyz`` [M,3] f32 through the dict ``cam`` (``pose`` = world -> camera): the winning row
    of each pixel, or -1.  A lexsort on (row, bits of float32(zc)) per pixel gives the nearest-wins rule."""
    p = np.asarray(xyz, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fin = np.isfinite(p).all(axis=1)
        x, y, z = (p[:, k].astype(np.float64) for k in range(3))
        if cam.get("pose") is not None:
            x, y, z = rigid(np.asarray(cam["pose"], np.float64), x, y, z)
        ok = fin & np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > 0)
        xf = x * cam["fx"]
        yf = y * cam["fy"]
        uq = xf / z
        vq = yf / z
        uc = uq + cam["cx"]
        vc = vq + cam["cy"]
        uf = np.floor(uc + 0.5)
        vf = np.floor(vc + 0.5)
        ok &= np.isfinite(uf) & np.isfinite(vf) & (uf >= 0) & (uf < w) & (vf >= 0) & (vf < h)
        zbits = z.astype(np.float32).view(np.uint32)
    rows = np.flatnonzero(ok)
    pixel = vf[rows].astype(np.int64) * w + uf[rows].astype(np.int64)
    order = np.lexsort((rows, zbits[rows], pixel))              # by pixel, then z bits, then row
    pixel, rows = pixel[order], rows[order]
    first = np.ones(len(rows), bool)
    first[1:] = pixel[1:] != pixel[:-1]
    index = np.full(h * w, -1, np.int32)
    index[pixel[first]] = rows[first]
    return index.reshape(h, w)


def resolve(index, values, fill):
    """The value image of an index image: values[row] where a row won, else ``fill``."""
    values = np.asarray(values)
    C = 1 if values.ndim == 1 else values.shape[1]
    img = np.empty((index.size, C), values.dtype)
    img[:] = np.asarray(fill, values.dtype)
    hit = index.reshape(-1) >= 0
    img[hit] = values.reshape(len(values), C)[index.reshape(-1)[hit]]
    return img.reshape(index.shape if values.ndim == 1 else index.shape + (C,))
