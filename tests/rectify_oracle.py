"""numpy oracle of K34 (include/mi355x_match_rectify.h): the section's atan and tan, the forward camera models, the sampling map
and its mask, the remap in its three element types and two interpolations, the undistortion of points and the rectifying
rotations of a stereo rig -- the header's arithmetic, operation by operation in float64 (float32 and integers for the taps), so
that csrc/rectify_math.h on the host and on the device gives the same bits.  Also the cameras, frames and points the tests of
K34 share."""
import functools

import numpy as np

COEFFS, SUBPIXEL_BITS, OUTSIDE, MAX_DIM, MAX_BATCH, MAX_POINTS, MAX_ITERATIONS, MAX_THETA = 8, 5, -(1 << 31), 16384, 65536, 1 << 24, 64, 1.5
PINHOLE, FISHEYE = 0, 1
U8, U16, F32 = 0, 1, 2
NEAREST, LINEAR = 0, 1
DTYPES = {U8: np.uint8, U16: np.uint16, F32: np.float32}
IDENTITY = np.eye(3)


def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
    return wrapped


@_quiet
def atan(x):
    x = np.asarray(x, np.float64)
    neg = x < 0.0
    a = np.where(neg, -x, x)
    recip = a > 1.0
    a = np.where(recip, 1.0 / a, a)
    a = a / (1.0 + np.sqrt(1.0 + a * a))
    a = a / (1.0 + np.sqrt(1.0 + a * a))
    z = a * a
    p = np.full_like(z, 1.0 / 23.0)
    for m in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = 1.0 / m - z * p
    p = 1.0 - z * p
    v = 4.0 * (a * p)
    v = np.where(recip, 1.5707963267948966 - v, v)
    return np.where(neg, -v, v)


@_quiet
def tan(t):
    t = np.asarray(t, np.float64)
    z = t * t
    s, c = np.ones_like(z), np.ones_like(z)
    for m in range(22, 1, -2):
        s = 1.0 - z / float(m * (m + 1)) * s
        c = 1.0 - z / float((m - 1) * m) * c
    return t * s / c


def _camera(k):
    k = np.asarray(k, np.float64).reshape(3, 3)
    return k[0, 0], k[1, 1], k[0, 2], k[1, 2]


@_quiet
def distort(model, dist, x, y):
    """the forward model of normalised points -> (xd, yd, has_image)"""
    d = np.asarray(dist, np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r2 = x * x + y * y
    if model == FISHEYE:
        rr = np.sqrt(r2)
        th = atan(rr)
        t2 = th * th
        thd = th * (1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3]))))
        s = np.where(rr > 0.0, thd / rr, 1.0)
        return x * s, y * s, np.ones(x.shape, bool)
    num = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))
    den = 1.0 + r2 * (d[5] + r2 * (d[6] + r2 * d[7]))
    radial = num / den
    a = (2.0 * x) * y
    xd = x * radial + (d[2] * a + d[3] * (r2 + (2.0 * x) * x))
    yd = y * radial + (d[2] * (r2 + (2.0 * y) * y) + d[3] * a)
    return xd, yd, den > 0.0


@_quiet
def rectify_map(model, k, dist, r, k_new, src_h, src_w, h, w):
    """-> (map (h, w, 2) int32, mask (h, w) uint8)"""
    fx, fy, cx, cy = _camera(k)
    nfx, nfy, ncx, ncy = _camera(k_new)
    r = (IDENTITY if r is None else np.asarray(r, np.float64)).reshape(9)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    xp, yp = (u - ncx) / nfx, (v - ncy) / nfy
    X0, X1, X2 = (r[0] * xp + r[3] * yp) + r[6], (r[1] * xp + r[4] * yp) + r[7], (r[2] * xp + r[5] * yp) + r[8]
    ok = X2 > 0.0
    xd, yd, has = distort(model, dist, X0 / X2, X1 / X2)
    ok &= has
    sx, sy = fx * xd + cx, fy * yd + cy
    tx, ty = np.floor(sx * 32.0 + 0.5), np.floor(sy * 32.0 + 0.5)
    ok &= (tx >= -64.0) & (tx < 32.0 * float(src_w + 1)) & (ty >= -64.0) & (ty < 32.0 * float(src_h + 1))
    ix, iy = np.where(ok, tx, 0.0).astype(np.int64), np.where(ok, ty, 0.0).astype(np.int64)
    X, Y = ix >> 5, iy >> 5
    ok &= (X >= -1) & (X < src_w) & (Y >= -1) & (Y < src_h)
    lastx, lasty = np.where(ix & 31, X + 1, X), np.where(iy & 31, Y + 1, Y)
    mask = ok & (X >= 0) & (lastx <= src_w - 1) & (Y >= 0) & (lasty <= src_h - 1)
    out = np.stack([np.where(ok, ix, OUTSIDE), np.where(ok, iy, OUTSIDE)], -1).astype(np.int32)
    return out, mask.astype(np.uint8)


@_quiet
def remap(src, map_, interpolation, border):
    """src (B, sh, sw) uint8 / uint16 / float32, map (h, w, 2) int32 -> (B, h, w) of src's type"""
    src = np.asarray(src)
    dtype = src.dtype
    _, sh, sw = src.shape
    qx, qy = map_[..., 0].astype(np.int64), map_[..., 1].astype(np.int64)
    outside = (qx == OUTSIDE) | (qy == OUTSIDE)
    border = dtype.type(border)

    def tap(Y, X):
        inside = (X >= 0) & (X < sw) & (Y >= 0) & (Y < sh)
        return np.where(inside, src[:, np.clip(Y, 0, sh - 1), np.clip(X, 0, sw - 1)], border)
    if interpolation == NEAREST:
        out = tap((qy + 16) >> 5, (qx + 16) >> 5)
    else:
        assert dtype != np.uint16
        X, Y, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
        p00, p01, p10, p11 = tap(Y, X), tap(Y, X + 1), tap(Y + 1, X), tap(Y + 1, X + 1)
        if dtype == np.uint8:
            p00, p01, p10, p11 = (p.astype(np.int64) for p in (p00, p01, p10, p11))
            out = (p00 * (32 - ax) * (32 - ay) + p01 * ax * (32 - ay) + p10 * (32 - ax) * ay + p11 * ax * ay + 512) >> 10
        else:
            wx, wy = ax.astype(np.float32) / np.float32(32.0), ay.astype(np.float32) / np.float32(32.0)
            top = np.where(ax != 0, p00 + (p01 - p00) * wx, p00)
            bot = np.where(ax != 0, p10 + (p11 - p10) * wx, p10)
            out = np.where(ay != 0, top + (bot - top) * wy, top)
            out = np.where(np.isnan(out) & ((ax != 0) | (ay != 0)), np.float32(np.nan), out)       # the quiet NaN 0x7FC00000
            assert out.dtype == np.float32
    return np.where(outside, border, out).astype(dtype)


@_quiet
def undistort_points(pts, model, k, dist, r=None, k_new=None, iterations=10, max_residual_px=0.5):
    """pts (..., 2) float32 pixels -> (out (..., 2) float32, ok (...) uint8)"""
    pts = np.asarray(pts, np.float32)
    d = np.asarray(dist, np.float64)
    fx, fy, cx, cy = _camera(k)
    u, v = pts[..., 0].astype(np.float64), pts[..., 1].astype(np.float64)
    xd, yd = (u - cx) / fx, (v - cy) / fy
    ok = np.ones(u.shape, bool)
    if model == FISHEYE:
        thd = np.sqrt(xd * xd + yd * yd)
        th = thd
        for _ in range(iterations):
            t2 = th * th
            f = th * (1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3])))) - thd
            g = 1.0 + t2 * (3.0 * d[0] + t2 * (5.0 * d[1] + t2 * (7.0 * d[2] + t2 * (9.0 * d[3]))))
            th = th - f / g
        ok &= (th >= 0.0) & (th <= MAX_THETA)
        s = np.where(thd > 0.0, tan(th) / thd, 1.0)
        x, y = xd * s, yd * s
    else:
        x, y = xd, yd
        for _ in range(iterations):
            r2 = x * x + y * y
            num = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))
            den = 1.0 + r2 * (d[5] + r2 * (d[6] + r2 * d[7]))
            icd = den / num
            a = (2.0 * x) * y
            x, y = (xd - (d[2] * a + d[3] * (r2 + (2.0 * x) * x))) * icd, (yd - (d[2] * (r2 + (2.0 * y) * y) + d[3] * a)) * icd
    bx, by, has = distort(model, d, x, y)
    ok &= has
    ex, ey = (fx * bx + cx) - u, (fy * by + cy) - v
    ok &= ex * ex + ey * ey <= max_residual_px * max_residual_px
    r = (IDENTITY if r is None else np.asarray(r, np.float64)).reshape(9)
    X0, X1, X2 = (r[0] * x + r[1] * y) + r[2], (r[3] * x + r[4] * y) + r[5], (r[6] * x + r[7] * y) + r[8]
    ok &= X2 > 0.0
    px, py = X0 / X2, X1 / X2
    if k_new is not None:
        nfx, nfy, ncx, ncy = _camera(k_new)
        px, py = nfx * px + ncx, nfy * py + ncy
    out = np.stack([px, py], -1).astype(np.float32)
    ok &= np.isfinite(out).all(-1)
    out[~ok] = 0.0
    return out, ok.astype(np.uint8)


def camera_ok(k):
    k = np.asarray(k, np.float64).reshape(9)
    return bool(np.isfinite(k).all() and k[0] > 0 and k[4] > 0 and k[1] == 0 and k[3] == 0 and k[6] == 0 and k[7] == 0 and k[8] == 1)


@_quiet
def stereo_rig(k1, k2, r, t, h, w):
    """-> (r1, r2, k_new (3, 3 each), baseline, fb), or None where the entry returns MI_E_PARAM"""
    k1, k2 = np.asarray(k1, np.float64).reshape(9), np.asarray(k2, np.float64).reshape(9)
    r, t = np.asarray(r, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)
    if not (camera_ok(k1) and camera_ok(k2) and np.isfinite(r).all() and np.isfinite(t).all()):
        return None
    b = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    if not (b > 0.0 and np.isfinite(b)):
        return None
    x = np.array([-((r[i] * t[0] + r[3 + i] * t[1]) + r[6 + i] * t[2]) / b for i in range(3)])
    if not (x[0] > 0.0 and x[0] >= abs(x[1])):
        return None
    zm = np.array([r[6], r[7], 1.0 + r[8]])
    y = np.array([zm[1] * x[2] - zm[2] * x[1], zm[2] * x[0] - zm[0] * x[2], zm[0] * x[1] - zm[1] * x[0]])
    ny, nz = np.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]), np.sqrt((zm[0] * zm[0] + zm[1] * zm[1]) + zm[2] * zm[2])
    if not ny > 1e-6 * nz:
        return None
    y = y / ny
    z = np.array([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]])
    r1 = np.stack([x, y, z])
    r2 = np.array([[(r1[i, 0] * r[3 * j] + r1[i, 1] * r[3 * j + 1]) + r1[i, 2] * r[3 * j + 2] for j in range(3)] for i in range(3)])
    f = (k1[4] + k2[4]) / 2.0
    k_new = np.array([[f, 0.0, (float(w) - 1.0) / 2.0], [0.0, f, (float(h) - 1.0) / 2.0], [0.0, 0.0, 1.0]])
    return r1, r2, k_new, float(b), float(f * b)


# ---- what the tests share ---------------------------------------------------------------------------------------------------------------
def rotation(rx, ry, rz):
    """a rotation from three small angles (numpy's trigonometry: an input of the tests, not part of the arithmetic under test)"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def camera(src_h, src_w, f=0.8):
    """a plausible camera of a (src_h, src_w) frame: focal length f * src_w (at least 8 pixels), the principal point on the pixel
    next to the middle (so that the optical axis is an exact-integer hit of an unrotated map)"""
    fl = max(f * src_w, 8.0)
    return np.array([[fl, 0.0, float(src_w // 2)], [0.0, fl * 1.01, float(src_h // 2)], [0.0, 0.0, 1.0]])


# strong enough that a destination of the size of the source holds sentinels, partly-outside footprints and interior pixels
DIST = {PINHOLE: np.array([-0.28, 0.09, 0.004, -0.003, -0.01, 0.02, 0.01, 0.002]),
        FISHEYE: np.array([-0.03, 0.01, -0.004, 0.001, 0.0, 0.0, 0.0, 0.0])}
ROTATION = rotation(0.04, -0.07, 0.02)
# (src_h, src_w, h, w): the issue's four and one whose width is a multiple of 4 (the kernel's vector path)
MAP_SHAPES = [(41, 90, 37, 83), (41, 90, 1, 70), (41, 90, 70, 1), (24, 60, 50, 130), (41, 90, 20, 72)]


def new_camera(src_h, src_w, h, w, model):
    """the ideal camera of a (h, w) destination that looks a little WIDER than the source, so that the border of the destination
    has no source pixel; its principal point sits on a pixel"""
    k = camera(src_h, src_w)
    scale = 0.8 * min(max(w, 8) / src_w, max(h, 8) / src_h) if model == PINHOLE else 0.6 * min(max(w, 8) / src_w, max(h, 8) / src_h)
    return np.array([[k[0, 0] * scale, 0.0, float(w // 2)], [0.0, k[1, 1] * scale, float(h // 2)], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def map_case(model, rotated, shape):
    """(k, dist, r or None, k_new, map, mask) of one of MAP_SHAPES, cached and read-only"""
    src_h, src_w, h, w = shape
    k, dist, r, k_new = camera(src_h, src_w), DIST[model], (ROTATION if rotated else None), new_camera(src_h, src_w, h, w, model)
    m, mask = rectify_map(model, k, dist, r, k_new, src_h, src_w, h, w)
    m.setflags(write=False)
    mask.setflags(write=False)
    return k, dist, r, k_new, m, mask


def map_classes(map_, mask):
    """how many destination pixels are sentinels, partly outside (a source pixel exists, the mask is 0) and exact-integer hits"""
    outside = map_[..., 0] == OUTSIDE
    exact = ~outside & ((map_[..., 0] & 31) == 0) & ((map_[..., 1] & 31) == 0)
    return int(outside.sum()), int((~outside & (mask == 0)).sum()), int(exact.sum())


def frames(seed, batch, src_h, src_w, type_):
    """a batch of textured frames of one element type: smooth enough to interpolate, with full-range extremes"""
    rng = np.random.default_rng(seed)
    top = {U8: 255, U16: 65535, F32: 255}[type_]
    g = rng.integers(0, top + 1, (batch, src_h, src_w))
    if type_ == F32:
        return (g + rng.uniform(-0.5, 0.5, g.shape)).astype(np.float32)
    return g.astype(DTYPES[type_])


def hostile_frames(seed, batch, src_h, src_w):
    """float32 frames with NaN, both infinities and +-1e30 in a tenth of the pixels"""
    rng = np.random.default_rng(seed)
    g = frames(seed, batch, src_h, src_w, F32)
    pick = rng.random(g.shape) < 0.1
    g[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), int(pick.sum()))
    return g


def points(seed, batch, n, src_h, src_w, hostile=True):
    """raw pixel coordinates (batch, n, 2) float32: most inside the frame, some far outside it (no undistorted point within the
    residual exists for them) and, with `hostile`, a NaN and a 1e30 among them when n allows"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0, src_w - 1, (batch, n)), rng.uniform(0, src_h - 1, (batch, n))], -1)
    far = rng.random((batch, n)) < 0.15
    p[far] = p[far] * 40.0 - 15.0 * src_w
    p = p.astype(np.float32)
    if hostile and n >= 3:
        p[:, 1, 0] = np.nan
        p[:, 2, 1] = 1e30
    return p


def bilinear_exact(src, sx, sy):
    """float64 bilinear sample of one (sh, sw) frame at real coordinates inside it: the yardstick of the analytic-image test"""
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    ax, ay = sx - x0, sy - y0
    x1, y1 = np.minimum(x0 + 1, src.shape[1] - 1), np.minimum(y0 + 1, src.shape[0] - 1)
    return (src[y0, x0] * (1 - ax) + src[y0, x1] * ax) * (1 - ay) + (src[y1, x0] * (1 - ax) + src[y1, x1] * ax) * ay
