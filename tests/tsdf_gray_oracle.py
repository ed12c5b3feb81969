"""numpy restatement of K22, TSDF intensity (include/mi355x_match.h, "TSDF intensity"): the intensity volume's reset, the joint
integration of depth and gray frames, the gather at points, the model's intensity map and direct frame-to-model tracking
through tests/tsdf_oracle.py (raycast, composition) and tests/photo_oracle.py (the joint refinement).

Every function takes `dtype` as tsdf_oracle's do: np.float64 is the oracle; np.float32 is the header's arithmetic operation by
operation (numpy fuses nothing), so the float32 integration and the float32 samples are the kernels' bits.  Host parameters
are rounded to float32 first in both runs.

A volume is tsdf_oracle's pair (tsdf, weight), an intensity volume the pair (gray, gweight) of (nz, ny, nx) arrays."""
import functools

import numpy as np

import icp_oracle as IO
import photo_oracle as PO
import tsdf_oracle as TO

F32, F64 = np.float32, np.float64


def reset(dims, dtype=F64):
    nx, ny, nz = dims
    return np.zeros((nz, ny, nx), dtype), np.zeros((nz, ny, nx), dtype)


def integrate(volume, ivolume, depth, gray, Rs, ts, cam, grid, max_weight=TO.MAX_WEIGHT, z_scale=1.0, min_depth=TO.MIN_DEPTH,
              max_depth=TO.MAX_DEPTH, active=None, dtype=F64):
    """depth (frames, h, w) float32 / uint16, gray (frames, h, w) float32 / uint8 -> the new ((tsdf, weight), (gray, gweight)).
    The (tsdf, weight) half is tsdf_oracle.integrate's, statement for statement."""
    T = dtype
    tsdf, weight = (x.astype(T, copy=True) for x in volume)
    gry, gwt = (x.astype(T, copy=True) for x in ivolume)
    nz, ny, nx = tsdf.shape
    _, _, trunc = grid
    trunc, mw, zs, lo, hi = T(F32(trunc)), T(F32(max_weight)), T(F32(z_scale)), T(F32(min_depth)), T(F32(max_depth))
    fx, fy, cx, cy = (T(F32(c)) for c in cam)
    cxs, cys, czs = TO.centres((nx, ny, nz), grid, T)
    p = [cxs[None, None, :], cys[None, :, None], czs[:, None, None]]
    frames, h, w = depth.shape
    for f in range(frames):
        if active is not None and not active[f]:
            continue
        R, t = np.asarray(Rs[f], F32).astype(T), np.asarray(ts[f], F32).astype(T)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            q = [((R[j, 0] * p[0] + R[j, 1] * p[1]) + R[j, 2] * p[2]) + t[j] for j in range(3)]
            u = fx * (q[0] / q[2]) + cx
            v = fy * (q[1] / q[2]) + cy
            px, py = np.floor(u + T(0.5)), np.floor(v + T(0.5))
            keep = (q[2] > 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
            ix, iy = np.where(keep, px, 0).astype(np.int64), np.where(keep, py, 0).astype(np.int64)
            d = depth[f][iy, ix].astype(F32).astype(T)
            z = d * zs
            keep &= np.isfinite(d) & (z >= lo) & (z <= hi)
            sdf = z - q[2]
            keep &= sdf >= -trunc
            fv = np.minimum(T(1), sdf / trunc)
            new_t = (tsdf * weight + fv) / (weight + T(1))
            new_w = np.minimum(weight + T(1), mw)
            g = gray[f][iy, ix].astype(F32).astype(T)
            gkeep = keep & (sdf <= trunc) & np.isfinite(g)
            new_g = (gry * gwt + g) / (gwt + T(1))
            new_gw = np.minimum(gwt + T(1), mw)
        tsdf = np.where(keep, new_t, tsdf).astype(T)
        weight = np.where(keep, new_w, weight).astype(T)
        gry = np.where(gkeep, new_g, gry).astype(T)
        gwt = np.where(gkeep, new_gw, gwt).astype(T)
    return (tsdf, weight), (gry, gwt)


def world(points, R, t, dtype=F64):
    """camera-frame points (N, 3) under the world-to-camera pose -> world points (N, 3): c = p - t, R^T c as (a + b) + c"""
    T = dtype
    R, t = np.asarray(R, F32).astype(T), np.asarray(t, F32).astype(T)
    pts = np.asarray(points).astype(T)
    c = [pts[:, 0] - t[0], pts[:, 1] - t[1], pts[:, 2] - t[2]]
    return np.stack([(R[0, j] * c[0] + R[1, j] * c[1]) + R[2, j] * c[2] for j in range(3)], axis=-1).astype(T)


def sample(ivolume, points, flags, grid, R=None, t=None, dtype=F64):
    """the intensity volume at points (N, 3) with flags (N,) (the records' f) -> (I (N,), valid (N,)); I = 0 where not valid"""
    T = dtype
    gry, gwt = (x.astype(T) for x in ivolume)
    nz, ny, nx = gry.shape
    origin, vs, _ = grid
    pts = np.asarray(points).astype(T)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.asarray(flags) != 0) & np.isfinite(pts).all(axis=1)
        xw = pts if R is None else world(pts, R, t, T)
        g = np.stack([(xw[:, a] - T(F32(origin[a]))) / T(F32(vs)) - T(0.5) for a in range(3)], axis=-1).astype(T)
        for a, n in enumerate((nx, ny, nz)):
            valid &= (g[:, a] >= 0) & (g[:, a] <= n - 1)
    g = np.where(valid[:, None], g, T(0)).astype(T)
    b = np.minimum(np.floor(g), np.array([nx - 2, ny - 2, nz - 2], T)).astype(T)
    a = (g - b).astype(T)
    ix, iy, iz = (b[:, k].astype(np.int64) for k in range(3))
    num, den = np.zeros(len(g), T), np.zeros(len(g), T)
    for m in range(8):
        dx, dy, dz = m & 1, (m >> 1) & 1, (m >> 2) & 1
        wx = a[:, 0] if dx else T(1) - a[:, 0]
        wy = a[:, 1] if dy else T(1) - a[:, 1]
        wz = a[:, 2] if dz else T(1) - a[:, 2]
        wm = (wx * wy) * wz
        seen = gwt[iz + dz, iy + dy, ix + dx] > 0
        num = np.where(seen, num + wm * gry[iz + dz, iy + dy, ix + dx], num).astype(T)
        den = np.where(seen, den + wm, den).astype(T)
    valid &= den > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        I = num / den
    return np.where(valid, I, T(0)).astype(T), valid


def raycast(volume, ivolume, R, t, k_inv, h, w, grid, dtype=F64, **kw):
    """tsdf_oracle.raycast and the intensity volume at its vertices -> (maps (vertex, vertex valid, normal, normal valid), the
    model's intensity map (record (h, w, 3) = (I, 0, 0), valid (h, w)): photo_oracle.intensity_maps' tuple)"""
    maps = TO.raycast(volume, R, t, k_inv, h, w, grid, dtype=dtype, **kw)
    I, ok = sample(ivolume, maps[0].reshape(-1, 3), maps[1].ravel(), grid, R, t, dtype)
    rec = np.zeros((h, w, 3), dtype)
    rec[..., 0] = I.reshape(h, w)
    return maps, (rec, ok.reshape(h, w))


def track(volume, ivolume, grid, depth, gray, R_pred, t_pred, h, w, dtype=F64, **kw):
    """direct frame-to-model: (raycast, model intensity) at the prediction as frame 1, the live frame's surfel and intensity
    maps as frame 2, photo_oracle.refine from the identity, composed onto the prediction -> (R, t, the refinement's dict)"""
    cam, ki = TO.camera(h, w)
    maps1, int1 = raycast(volume, ivolume, R_pred, t_pred, ki, h, w, grid, dtype=dtype)
    maps2 = IO.surfel_maps(depth, ki, dtype=dtype)
    int2 = PO.intensity_maps(gray, dtype)
    o = PO.refine(maps1, int1, maps2, int2, np.eye(3), np.zeros(3), cam, dtype=dtype, **kw)
    if dtype == F32:
        R, t = TO.compose(o["R"], o["t"], R_pred, t_pred)
    else:
        Rp, tp = np.asarray(R_pred, F32).astype(F64), np.asarray(t_pred, F32).astype(F64)
        R, t = o["R"] @ Rp, o["R"] @ tp + o["t"]
    return R, t, o


@functools.lru_cache(maxsize=None)
def plane_model(seed, h, w, spec=TO.ROOM, dtype=F64, u8=False):
    """the textured plane of photo_oracle.scene("plane", seed, h, w): frame 1 fused at the identity into `spec` -> (volume,
    intensity volume, grid, the scene's dict)"""
    s = PO.scene("plane", seed, h, w, dtype=dtype, u8=u8)
    dims, grid = TO.grid_of(spec)
    vol, ivol = integrate(TO.reset(dims, dtype), reset(dims, dtype), s["depth1"][None], s["gray1"][None], np.eye(3)[None],
                          np.zeros((1, 3)), TO.camera(h, w)[0], grid, dtype=dtype)
    return vol, ivol, grid, s


# ---- the tests' scenes -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def views_gray(h, w, seeds=(0, 1, 2)):
    """the gray frames (float32) of photo_oracle.texture on the room's surface, seen in the frames of tsdf_oracle.views(h, w)"""
    depth, R, t = TO.views(h, w, seeds)
    ray = PO.rays(h, w)
    return np.stack([PO.texture((ray * depth[f].astype(F64)[..., None] - t[f]) @ R[f]) for f in range(len(depth))]).astype(F32)


@functools.lru_cache(maxsize=None)
def fused_room(h, w, spec=TO.ROOM, dtype=F64):
    """the four views of tsdf_oracle.views(h, w) with views_gray(h, w) fused into `spec` -> ((tsdf, weight), (gray, gweight))"""
    dims, grid = TO.grid_of(spec)
    depth, R, t = TO.views(h, w)
    return integrate(TO.reset(dims, dtype), reset(dims, dtype), depth, views_gray(h, w), R, t, TO.camera(h, w)[0], grid, dtype=dtype)


def synthetic(dims, seed=0):
    """an intensity volume with every kind of cell: random gray, about a third of the records unobserved, the eight corner
    records of the volume observed and -- where the volume is large enough -- the block [2, 5)^3 unobserved with the x = 1
    layer beside it observed -> (gray, gweight) float32"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    gry = rng.uniform(0.0, 255.0, (nz, ny, nx)).astype(F32)
    gwt = np.where(rng.uniform(size=(nz, ny, nx)) < 0.33, 0.0, rng.integers(1, 5, (nz, ny, nx))).astype(F32)
    for k in (0, nz - 1):
        for j in (0, ny - 1):
            for i in (0, nx - 1):
                gwt[k, j, i] = 1.0
    if min(dims) >= 6:
        gwt[2:5, 2:5, 2:5] = 0.0
        gwt[2:5, 2:5, 1] = 2.0
    gry[gwt == 0] = 0.0
    return gry, gwt


def hand_points(dims, grid, seed=0):
    """point records (N, 4) float32 in the world frame, placed by grid coordinate (exact where origin and voxel_size are
    dyadic, as ROOM's are) -> (points, names of the first rows).  g = 0 and g = n - 1 on every axis; the last layer on one
    axis; just outside on either side; NaN and inf coordinates; f = 0, f = -1, f = 2; a cell with no observed corner and one
    with some (synthetic()'s block); then 200 random points in and around the box, a tenth of them with f = 0"""
    nx, ny, nz = dims
    origin, vs, _ = grid
    o64 = origin.astype(F64)

    def at(gx, gy, gz, f=1.0):
        return [*((np.array([gx, gy, gz], F64) + 0.5) * F64(vs) + o64).astype(F32), F32(f)]
    lo, hi = at(0, 0, 0), at(nx - 1, ny - 1, nz - 1)
    below, above = list(lo), list(hi)
    below[0], above[2] = np.nextafter(F32(lo[0]), F32(-np.inf)), np.nextafter(F32(hi[2]), F32(np.inf))
    rows = {"g = 0": lo, "g = n - 1": hi, "last x layer": at(nx - 1, 0.25, 0.5), "below": below, "above": above,
            "far outside": at(-3.0, 0.5, 0.5), "nan": [np.nan, lo[1], lo[2], 1.0], "inf": [lo[0], np.inf, lo[2], 1.0],
            "f = 0": at(0.5, 0.5, 0.5, 0.0), "f = -1": at(0.5, 0.5, 0.5, -1.0), "f = 2": at(0.5, 0.5, 0.5, 2.0)}
    if min(dims) >= 6:
        rows["no observed corner"] = at(2.5, 3.25, 3.75)
        rows["some observed corners"] = at(1.5, 2.5, 3.5)
    rng = np.random.default_rng(seed + 1)
    g = rng.uniform(-0.1, 1.05, (200, 3)) * (np.array(dims) - 1)
    rand = np.concatenate([(g + 0.5) * F64(vs) + o64, np.where(rng.uniform(size=(200, 1)) < 0.1, 0.0, 1.0)], axis=1)
    return np.concatenate([np.array(list(rows.values()), F32), rand.astype(F32)]), list(rows)
