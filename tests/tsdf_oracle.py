"""numpy restatement of K19, TSDF fusion (include/mi355x_match.h, "TSDF fusion"): reset, integration, raycast, the
composition of poses and frame-to-model tracking through tests/icp_oracle.py.

Every function takes `dtype`: np.float64 is the oracle; np.float32 is the header's arithmetic operation by operation (numpy
fuses nothing), so the float32 integration and the float32 samples are the kernels' bits.  Host parameters are rounded to
float32 first in both runs, as the C ABI receives them: the deviation of the float32 run from the float64 run is then that of
the arithmetic alone, and it is what the GPU tests' tolerances are derived from.

A volume is the pair (tsdf, weight) of (nz, ny, nx) arrays; a grid is (origin (3,), voxel_size, truncation).  Poses are world
(volume) to camera, X_c = R X_w + t."""
import functools

import numpy as np

import icp_oracle as IO

F32, F64 = np.float32, np.float64
MIN_DEPTH, MAX_DEPTH, MAX_WEIGHT, STEP_FRACTION = 0.1, 10.0, 64.0, 0.5
# the volumes of the tests, (nx, ny, nz), origin, voxel_size, truncation: the room of synth_depth_room in 6.25 cm voxels; one
# with every dimension odd that cuts the room; the smallest legal one
ROOM = ((72, 44, 56), (-2.25, -1.75, 0.5), 0.0625, 0.25)
ODD = ((41, 29, 37), (-1.3, -1.05, 0.9), 0.07, 0.28)
TINY = ((2, 2, 2), (-1.0, -0.8, 1.2), 1.0, 1.0)


def grid_of(spec):
    """(dims (nx, ny, nz), (origin float32 (3,), voxel_size, truncation)) of one of the specifications above"""
    dims, origin, vs, trunc = spec
    return tuple(dims), (np.asarray(origin, F32), float(F32(vs)), float(F32(trunc)))


def reset(dims, dtype=F64):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), dtype), np.zeros((nz, ny, nx), dtype)


def centres(dims, grid, dtype):
    T = dtype
    origin, vs, _ = grid
    return [((np.arange(n, dtype=T) + T(0.5)) * T(F32(vs))) + T(F32(origin[a])) for a, n in enumerate(dims)]


def integrate(volume, depth, Rs, ts, cam, grid, max_weight=MAX_WEIGHT, z_scale=1.0, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
              active=None, dtype=F64):
    """depth (frames, h, w) float32 / uint16, Rs (frames, 3, 3), ts (frames, 3) -> the new (tsdf, weight)"""
    T = dtype
    tsdf, weight = (x.astype(T, copy=True) for x in volume)
    nz, ny, nx = tsdf.shape
    _, _, trunc = grid
    trunc, mw, zs, lo, hi = T(F32(trunc)), T(F32(max_weight)), T(F32(z_scale)), T(F32(min_depth)), T(F32(max_depth))
    fx, fy, cx, cy = (T(F32(c)) for c in cam)
    cxs, cys, czs = centres((nx, ny, nz), grid, T)
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
        tsdf = np.where(keep, new_t, tsdf).astype(T)
        weight = np.where(keep, new_w, weight).astype(T)
    return tsdf, weight


def sample(volume, g, dtype=F64):
    """trilinear tsdf at the grid coordinates g (N, 3) -> (f (N,), valid (N,)); f = 0 where not valid"""
    T = dtype
    tsdf, weight = volume
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        inside = ((g[:, 0] >= 0) & (g[:, 0] < nx - 1) & (g[:, 1] >= 0) & (g[:, 1] < ny - 1) & (g[:, 2] >= 0) & (g[:, 2] < nz - 1))
    gs = np.where(inside[:, None], g, T(0)).astype(T)
    b = np.floor(gs)
    a = gs - b
    ix, iy, iz = (b[:, k].astype(np.int64) for k in range(3))
    valid = inside.copy()
    c = {}
    for dz in (0, 1):
        for dy in (0, 1):
            t0, t1 = tsdf[iz + dz, iy + dy, ix].astype(T), tsdf[iz + dz, iy + dy, ix + 1].astype(T)
            valid &= (weight[iz + dz, iy + dy, ix] > 0) & (weight[iz + dz, iy + dy, ix + 1] > 0)
            c[dy, dz] = t0 + a[:, 0] * (t1 - t0)
    c0 = c[0, 0] + a[:, 1] * (c[1, 0] - c[0, 0])
    c1 = c[0, 1] + a[:, 1] * (c[1, 1] - c[0, 1])
    f = c0 + a[:, 2] * (c1 - c0)
    return np.where(valid, f, T(0)).astype(T), valid


def grid_point(xn, yn, s, R, t, grid, dtype):
    T = dtype
    origin, vs, _ = grid
    c = [xn * s - t[0], yn * s - t[1], s - t[2]]
    return np.stack([((R[0, j] * c[0] + R[1, j] * c[1]) + R[2, j] * c[2] - T(F32(origin[j]))) / T(F32(vs)) - T(0.5)
                     for j in range(3)], axis=-1).astype(T)


def sample_count(truncation, step_fraction=STEP_FRACTION, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """(step, last k), float32 as the header has them"""
    step = F32(step_fraction) * F32(truncation)
    return step, int(np.ceil((F32(max_depth) - F32(min_depth)) / step))


def hit(s_prev, step, f_prev, f):
    return s_prev + step * (f_prev / (f_prev - f))


def raycast(volume, R, t, k_inv, h, w, grid, step_fraction=STEP_FRACTION, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, dtype=F64):
    """-> (vertex (h, w, 3), vertex valid (h, w), normal (h, w, 3), normal valid (h, w)): the tuple of icp_oracle.surfel_maps"""
    T = dtype
    volume = tuple(x.astype(T) for x in volume)
    step32, last = sample_count(grid[2], step_fraction, min_depth, max_depth)
    step = T(step32)
    R, t = np.asarray(R, F32).astype(T), np.asarray(t, F32).astype(T)
    ki = np.asarray(k_inv, F32).astype(T).ravel()
    y, x = np.meshgrid(np.arange(h, dtype=T), np.arange(w, dtype=T), indexing="ij")
    xn = ((x * ki[0] + y * ki[1]) + ki[2]).ravel()
    yn = ((x * ki[3] + y * ki[4]) + ki[5]).ravel()
    n = h * w
    done, prev_ok, is_hit = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    f_prev, s_prev, s_hit = np.zeros(n, T), np.zeros(n, T), np.zeros(n, T)
    for k in range(last + 1):
        s = np.full(n, (T(k) * step) + T(F32(min_depth)), T)
        f, ok = sample(volume, grid_point(xn, yn, s, R, t, grid, T), T)
        end = ok & (f <= 0) & ~done
        now = end & prev_ok & (f_prev > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            s_hit = np.where(now, hit(s_prev, step, f_prev, f), s_hit).astype(T)
        is_hit |= now
        done |= end
        prev_ok, f_prev, s_prev = ok, f, s
        if done.all():
            break
    sh = np.where(is_hit, s_hit, T(0))
    v = np.stack([xn * sh, yn * sh, sh], axis=-1).astype(T)
    g = grid_point(xn, yn, sh, R, t, grid, T)
    grad, nok = [], is_hit.copy()
    for a in range(3):
        hi_g, lo_g = g.copy(), g.copy()
        hi_g[:, a] = g[:, a] + T(1)
        lo_g[:, a] = g[:, a] - T(1)
        fh, okh = sample(volume, hi_g, T)
        fl, okl = sample(volume, lo_g, T)
        nok &= okh & okl
        grad.append(fh - fl)
    m = np.stack([(R[j, 0] * grad[0] + R[j, 1] * grad[1]) + R[j, 2] * grad[2] for j in range(3)], axis=-1)
    len2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
    nok &= (len2 > 0) & np.isfinite(len2)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = m / np.sqrt(len2)[:, None]
    facing = (e[:, 0] * v[:, 0] + e[:, 1] * v[:, 1]) + e[:, 2] * v[:, 2]
    with np.errstate(invalid="ignore"):
        e = np.where((facing > 0)[:, None], -e, e)
    nrm = np.where(nok[:, None], e, T(0)).astype(T)
    v = np.where(is_hit[:, None], v, T(0)).astype(T)
    return v.reshape(h, w, 3), is_hit.reshape(h, w), nrm.reshape(h, w, 3), nok.reshape(h, w)


def compose(Ra, ta, Rb, tb):
    """(Ra, ta) o (Rb, tb): float32 in, float64 products and (a + b) + c sums, float32 out"""
    Ra, ta, Rb, tb = (np.asarray(x, F32).astype(F64) for x in (Ra, ta, Rb, tb))
    R = np.array([[(Ra[i, 0] * Rb[0, j] + Ra[i, 1] * Rb[1, j]) + Ra[i, 2] * Rb[2, j] for j in range(3)] for i in range(3)])
    t = np.array([((Ra[i, 0] * tb[0] + Ra[i, 1] * tb[1]) + Ra[i, 2] * tb[2]) + ta[i] for i in range(3)])
    return R.astype(F32), t.astype(F32)


# ---- the tests' scenes -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def views(h, w, seeds=(0, 1, 2)):
    """the room's frames with known world-to-camera poses: synth_depth_room's first view (the identity; the same for every
    seed) and the second views of `seeds` -> (depth (1 + len(seeds), h, w) float32, R (.., 3, 3), t (.., 3) float64)"""
    from onnx_image_processing_amd.synth import synth_depth_room
    rooms = [synth_depth_room(s, h, w) for s in seeds]
    depth = np.stack([rooms[0][0]] + [r[1] for r in rooms])
    R = np.stack([np.eye(3)] + [r[2] for r in rooms])
    t = np.stack([np.zeros(3)] + [r[3] for r in rooms])
    return depth, R, t


def camera(h, w):
    """(cam (fx, fy, cx, cy) as float32-exact floats, k_inv float32 (3, 3)) of rgbd_camera(h, w)"""
    from onnx_image_processing_amd.synth import rgbd_camera
    K = rgbd_camera(h, w)
    return tuple(float(F32(c)) for c in IO.camera_of(K)), IO.k_inv32(K)


@functools.lru_cache(maxsize=None)
def fused_room(h, w, spec=ROOM, dtype=F64):
    """the four views of views(h, w) fused into the volume `spec` -> (tsdf, weight)"""
    dims, grid = grid_of(spec)
    depth, R, t = views(h, w)
    return integrate(reset(dims, dtype), depth, R, t, camera(h, w)[0], grid, dtype=dtype)


def track(volume, grid, depth, R_pred, t_pred, h, w, dtype=F64, **icp):
    """frame-to-model: the raycast at the prediction as maps1, the live frame's surfel maps as maps2, icp_oracle.refine from
    the identity, composed onto the prediction -> (R, t, the refinement's dict)"""
    cam, ki = camera(h, w)
    maps1 = raycast(volume, R_pred, t_pred, ki, h, w, grid, dtype=dtype)
    maps2 = IO.surfel_maps(depth, ki, dtype=dtype)
    o = IO.refine(maps1, maps2, np.eye(3), np.zeros(3), cam, dtype=dtype, **icp)
    if dtype == F32:
        R, t = compose(o["R"], o["t"], R_pred, t_pred)
    else:
        Rp, tp = np.asarray(R_pred, F32).astype(F64), np.asarray(t_pred, F32).astype(F64)
        R, t = o["R"] @ Rp, o["R"] @ tp + o["t"]
    return R, t, o
