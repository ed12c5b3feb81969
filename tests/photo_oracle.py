"""numpy restatement of K21, direct RGB-D refinement (include/mi355x_match.h, "direct RGB-D refinement"): intensity maps, one
photometric linearisation, the joint sums and the scheduled joint refinement, with icp_oracle for the geometric half, the
solve and the pose update; and the textured scenes the K21 tests use.

Every function takes `dtype` as icp_oracle's do: np.float64 is the oracle; np.float32 runs the per-pixel arithmetic of the
header in float32, operation by operation, and sums in float32 (numpy's pairwise order, not the kernels'), with the joint
system, the solve and the pose in float64 as the header has them."""
import numpy as np

import icp_oracle as IO

PHOTO_WEIGHT, INTENSITY_THRESHOLD = 0.003, 30.0


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------

def intensity_maps(gray, dtype=np.float64):
    """gray (h, w) uint8 / float32 -> (record (h, w, 3) = (I, gx, gy) in `dtype`, valid (h, w))"""
    T = dtype
    h, w = gray.shape
    g = gray.astype(np.float32).astype(T)
    ok = np.zeros((h, w), bool)
    rec = np.zeros((h, w, 3), T)
    c, l, r, u, d = g[1:-1, 1:-1], g[1:-1, :-2], g[1:-1, 2:], g[:-2, 1:-1], g[2:, 1:-1]
    inner = np.isfinite(c) & np.isfinite(l) & np.isfinite(r) & np.isfinite(u) & np.isfinite(d)
    with np.errstate(invalid="ignore", over="ignore"):
        gx, gy = T(0.5) * (r - l), T(0.5) * (d - u)
    ok[1:-1, 1:-1] = inner
    rec[1:-1, 1:-1] = np.where(inner[..., None], np.stack([c, gx, gy], axis=-1), T(0))
    return rec, ok


def blend(c00, c01, c10, c11, a, b):
    top, bot = c00 + a * (c01 - c00), c10 + a * (c11 - c10)
    return top + b * (bot - top)


def rows(maps1, int1, maps2, int2, R, t, cam, stride=1, dist=IO.DIST, int_thr=INTENSITY_THRESHOLD, dtype=np.float64):
    """the surviving rows of one photometric linearisation: (J (m, 6), r (m,)) in `dtype`.  maps: icp_oracle.surfel_maps'
    tuples (only the vertices are used), int: intensity_maps' pairs."""
    T = dtype
    v1, vok1 = maps1[0], maps1[1]
    v2, vok2 = maps2[0], maps2[1]
    (rec1, gok1), (rec2, gok2) = int1, int2
    h, w = vok1.shape
    fx, fy, cx, cy = (T(c) for c in cam)
    R = np.asarray(R, T)
    t = np.asarray(t, T)
    sel = (vok1 & gok1)[::stride, ::stride]
    p, i1 = v1[::stride, ::stride][sel].astype(T), rec1[::stride, ::stride, 0][sel].astype(T)
    q = np.stack([(R[j, 0] * p[:, 0] + R[j, 1] * p[:, 1]) + R[j, 2] * p[:, 2] for j in range(3)], axis=-1) + t
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = fx * (q[:, 0] / q[:, 2]) + cx
        v = fy * (q[:, 1] / q[:, 2]) + cy
        px, py, x0, y0 = np.floor(u + T(0.5)), np.floor(v + T(0.5)), np.floor(u), np.floor(v)
        a, b = u - x0, v - y0
        keep = (q[:, 2] > 0) & (x0 >= 0) & (x0 <= w - 2) & (y0 >= 0) & (y0 <= h - 2)
    q, i1, a, b = q[keep], i1[keep], a[keep], b[keep]
    ix, iy, nx, ny = (z[keep].astype(np.int64) for z in (x0, y0, px, py))
    keep = gok2[iy, ix] & gok2[iy, ix + 1] & gok2[iy + 1, ix] & gok2[iy + 1, ix + 1] & vok2[ny, nx]
    keep &= np.abs(q[:, 2] - v2[ny, nx, 2].astype(T)) <= T(dist)
    q, i1, a, b, ix, iy = q[keep], i1[keep], a[keep], b[keep], ix[keep], iy[keep]
    c00, c01, c10, c11 = (rec2[iy + dy, ix + dx].astype(T) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
    i2, gx, gy = (blend(c00[:, k], c01[:, k], c10[:, k], c11[:, k], a, b) for k in range(3))
    res = i2 - i1
    keep = np.abs(res) <= T(int_thr)
    q, gx, gy, res = q[keep], gx[keep], gy[keep], res[keep]
    k0, k1 = (fx * gx) / q[:, 2], (fy * gy) / q[:, 2]
    k2 = -((k0 * q[:, 0] + k1 * q[:, 1]) / q[:, 2])
    J = np.stack([q[:, 1] * k2 - q[:, 2] * k1, q[:, 2] * k0 - q[:, 0] * k2, q[:, 0] * k1 - q[:, 1] * k0, k0, k1, k2], axis=-1)
    return J.astype(T), res.astype(T)


def sums_of(J, r, dtype):
    """icp_oracle.linearise's 29 sums of given rows"""
    s = np.zeros(29)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            s[k] = (J[:, i] * J[:, j]).sum(dtype=dtype)
            k += 1
    for i in range(6):
        s[21 + i] = (J[:, i] * r).sum(dtype=dtype)
    s[27] = (r * r).sum(dtype=dtype)
    s[28] = len(r)
    return s


def linearise(maps1, int1, maps2, int2, R, t, cam, stride=1, dist=IO.DIST, int_thr=INTENSITY_THRESHOLD, dtype=np.float64):
    return sums_of(*rows(maps1, int1, maps2, int2, R, t, cam, stride, dist, int_thr, dtype), dtype)


def weight2(weight):
    """w * w in float64 of the float32 weight the kernels are given"""
    return np.float64(np.float32(weight)) * np.float64(np.float32(weight))


def joint(g, p, weight):
    """the joint sums: g + w^2 p for A, b and sum r^2, the counts added; p = None: g"""
    if p is None:
        return np.asarray(g, np.float64).copy()
    s = np.zeros(29)
    s[:28] = g[:28] + weight2(weight) * p[:28]
    s[28] = g[28] + p[28]
    return s


def refine(maps1, int1, maps2, int2, R0, t0, cam, schedule=IO.SCHEDULE, dist=IO.DIST, angle=np.deg2rad(IO.ANGLE_DEG),
           weight=PHOTO_WEIGHT, int_thr=INTENSITY_THRESHOLD, min_count=IO.MIN_CORR, dtype=np.float64):
    """icp_oracle.refine with the photometric term joined to every step -> its dict, `information` the joint A, and
    count_photo, rmse_photo, sums_photo"""
    R, t = np.asarray(R0, np.float64).copy(), np.asarray(t0, np.float64).copy()
    lin = (lambda a: a.astype(np.float32)) if dtype == np.float32 else (lambda a: a)
    photo = float(np.float32(weight)) != 0.0

    def both(stride):
        g = IO.linearise(maps1, maps2, lin(R), lin(t), cam, stride, dist, angle, dtype)
        p = linearise(maps1, int1, maps2, int2, lin(R), lin(t), cam, stride, dist, int_thr, dtype) if photo else None
        return g, p

    frozen, steps, last, min_ratio = False, 0, np.inf, np.inf
    for stride, iters in schedule:
        for _ in range(iters):
            if frozen:
                continue
            x, ratio = IO.solve(joint(*both(stride), weight), min_count)
            min_ratio = min(min_ratio, ratio)
            if x is None:
                frozen = True
                continue
            Rn, tn = IO.update(R, t, x)
            if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
                frozen = True
                continue
            R, t, steps, last = Rn, tn, steps + 1, float(np.abs(x).max())
    g, p = both(schedule[-1][0])
    s = joint(g, p, weight)
    count, count_p = int(g[28]), int(p[28]) if photo else 0
    return dict(R=lin(R), t=lin(t), information=lin(IO.full_matrix(s)), rmse=float(lin(np.sqrt(g[27] / count))) if count else 0.0,
                count=count, rmse_photo=float(lin(np.sqrt(p[27] / count_p))) if count_p else 0.0, count_photo=count_p, steps=steps,
                ok=(not frozen) and count + count_p >= min_count, last_step=last, min_ratio=min_ratio, sums=g, sums_photo=p)


# ---- the textured scenes -----------------------------------------------------------------------------------------------------------

def texture(X):
    """the gray value of the surface point X (..., 3), in frame 1's coordinates"""
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    tau = 2.0 * np.pi
    return (128.0 + 40.0 * np.sin(tau * (x / 0.9 + y / 1.3) + 0.3) + 30.0 * np.sin(tau * (y / 0.7 - z / 1.1) + 1.1)
            + 25.0 * np.sin(tau * (x / 0.5 + z / 0.8) + 2.0))


def rays(h, w):
    xn, yn = IO._rays(h, w)
    return np.stack([xn, yn, np.ones_like(xn)], axis=-1)


def render(depth1, depth2, R, t):
    """the two gray frames (float32) of the textured surface seen in both depth frames: float64, rounded to float32"""
    ray = rays(*depth1.shape)
    X1 = ray * depth1.astype(np.float64)[..., None]
    X2 = ray * depth2.astype(np.float64)[..., None]
    return texture(X1).astype(np.float32), texture((X2 - t) @ R).astype(np.float32)      # (X2 - t) @ R = R^T (X2 - t)


def as_u8(gray):
    return np.rint(gray).astype(np.uint8)


def plane_pair(seed, h, w):
    """icp_oracle.plane_depth's plane seen from synth_depth_room(seed, h, w)'s two cameras: (depth1, depth2, R, t); the
    second view is analytic: n2 = R n, c2 = c + n2 . t"""
    from onnx_image_processing_amd.synth import synth_depth_room
    R, t = synth_depth_room(seed, h, w)[2:]
    n2 = R @ np.array([0.2, 0.1, 1.0])
    c2 = 2.0 + n2 @ t
    return IO.plane_depth(h, w), (c2 / (rays(h, w) @ n2)).astype(np.float32), R, t


def scene(kind, seed, h, w, dtype=np.float64, u8=False):
    """kind "plane" (the textured plane), "room" (synth_depth_room with the sphere) or "flat" (without) -> dict(maps1, maps2,
    int1, int2 in `dtype`, R, t, cam, depth1, depth2, gray1, gray2)"""
    from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room
    d1, d2, R, t = plane_pair(seed, h, w) if kind == "plane" else synth_depth_room(seed, h, w, sphere=kind == "room")
    g1, g2 = render(d1, d2, R, t)
    if u8:
        g1, g2 = as_u8(g1), as_u8(g2)
    K = rgbd_camera(h, w)
    ki = IO.k_inv32(K)
    cam = tuple(float(np.float32(c)) for c in IO.camera_of(K))
    return dict(maps1=IO.surfel_maps(d1, ki, dtype=dtype), maps2=IO.surfel_maps(d2, ki, dtype=dtype), int1=intensity_maps(g1, dtype),
                int2=intensity_maps(g2, dtype), R=R, t=t, cam=cam, depth1=d1, depth2=d2, gray1=g1, gray2=g2)


def refine_scene(s, R0=None, t0=None, dtype=np.float64, **kw):
    R0 = np.eye(3) if R0 is None else R0
    t0 = np.zeros(3) if t0 is None else t0
    return refine(s["maps1"], s["int1"], s["maps2"], s["int2"], R0, t0, s["cam"], dtype=dtype, **kw)
