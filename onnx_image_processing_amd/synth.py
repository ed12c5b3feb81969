"""Deterministic synthetic gray image pairs.

The generator is a pure integer hash (splitmix64 finaliser), so the same
pixels come out of numpy here, on the GPU box, and in any later re-run; nothing
is read from disk.  Images are uint8-valued: the reference's callers feed
uint8 camera frames converted to float32 in [0, 255]
(reference sample/image_matching.py:42-46).

image(seed)  = coarse 8x8 blocks with values 0..199  +  per-pixel texture 0..54
pair(seed)   = (image, image circularly shifted by (dy, dx) [+ optional +-noise])
"""
from __future__ import annotations

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z: np.ndarray) -> np.ndarray:
    """splitmix64 output function on a uint64 array (wrap-around arithmetic)."""
    z = z.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _hash3(seed: int, a: np.ndarray, b: np.ndarray, salt: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        k = (
            np.uint64(seed) * np.uint64(0xD1342543DE82EF95)
            + a.astype(np.uint64) * np.uint64(0x2545F4914F6CDD1D)
            + b.astype(np.uint64) * np.uint64(0x9FB21C651E98DF25)
            + np.uint64(salt)
        )
    return _mix64(_mix64(k))


def synth_image(seed: int, height: int = 480, width: int = 640) -> np.ndarray:
    """uint8 (H, W) image for `seed`."""
    y = np.arange(height, dtype=np.uint64)[:, None]
    x = np.arange(width, dtype=np.uint64)[None, :]
    yy, xx = np.broadcast_arrays(y, x)
    coarse = _hash3(seed, yy // np.uint64(8), xx // np.uint64(8), 1) % np.uint64(200)
    fine = _hash3(seed, yy, xx, 2) % np.uint64(55)
    return np.minimum(coarse + fine, np.uint64(255)).astype(np.uint8)


def synth_pair(
    seed: int,
    height: int = 480,
    width: int = 640,
    shift: tuple[int, int] = (3, 5),
    noise: int = 0,
) -> tuple[np.ndarray, np.ndarray]:
    """uint8 image pair: second image = first rolled by `shift` (+ optional noise)."""
    img1 = synth_image(seed, height, width)
    img2 = np.roll(img1, shift=shift, axis=(0, 1))
    if noise > 0:
        y = np.arange(height, dtype=np.uint64)[:, None]
        x = np.arange(width, dtype=np.uint64)[None, :]
        yy, xx = np.broadcast_arrays(y, x)
        n = (_hash3(seed + 1, yy, xx, 3) % np.uint64(2 * noise + 1)).astype(np.int64) - noise
        img2 = np.clip(img2.astype(np.int64) + n, 0, 255).astype(np.uint8)
    return img1, img2


def synth_batch(
    first_seed: int,
    num_pairs: int,
    height: int = 480,
    width: int = 640,
    shift: tuple[int, int] = (3, 5),
    noise: int = 0,
) -> tuple[np.ndarray, np.ndarray]:
    """float32 (B,1,H,W) x2 in [0,255]; pair i uses seed first_seed + i."""
    a = np.empty((num_pairs, 1, height, width), np.float32)
    b = np.empty((num_pairs, 1, height, width), np.float32)
    for i in range(num_pairs):
        p, q = synth_pair(first_seed + i, height, width, shift, noise)
        a[i, 0] = p
        b[i, 0] = q
    return a, b


def synth_batch_u8(
    first_seed: int,
    num_pairs: int,
    height: int = 480,
    width: int = 640,
    shift: tuple[int, int] = (3, 5),
    noise: int = 0,
) -> tuple[np.ndarray, np.ndarray]:
    """uint8 (B,1,H,W) x2: the same frames as synth_batch before the float32 conversion (what a camera delivers;
    the u8 ingest path takes them as they are)."""
    a = np.empty((num_pairs, 1, height, width), np.uint8)
    b = np.empty((num_pairs, 1, height, width), np.uint8)
    for i in range(num_pairs):
        a[i, 0], b[i, 0] = synth_pair(first_seed + i, height, width, shift, noise)
    return a, b


def _depth_image64(seed: int, height: int, width: int, depth_min: float, depth_max: float):
    """(yy, xx, z float64 (H, W)): the depth image behind synth_depth_cloud / synth_depth_frame."""
    y = np.arange(height, dtype=np.uint64)[:, None]
    x = np.arange(width, dtype=np.uint64)[None, :]
    yy, xx = np.broadcast_arrays(y, x)
    ramp = depth_min + (depth_max - depth_min) * (1.0 - yy.astype(np.float64) / max(1, height - 1)) * 0.75
    blocks = (_hash3(seed, yy // np.uint64(16), xx // np.uint64(16), 4) % np.uint64(1001)).astype(np.float64) / 1000.0
    jitter = (_hash3(seed, yy, xx, 5) % np.uint64(4001)).astype(np.float64) / 1e6 - 0.002
    z = np.clip(ramp + 0.25 * (depth_max - depth_min) * blocks + jitter, depth_min, depth_max)
    return yy, xx, z


def synth_depth_cloud(seed: int, height: int = 480, width: int = 640, fx: float = 525.0, fy: float = 525.0,
                      depth_min: float = 0.5, depth_max: float = 4.5) -> np.ndarray:
    """float32 (height * width, 3) point cloud: a synthetic depth frame back-projected through a pinhole camera
    (principal point at the image centre), row-major pixel order -- the input a VO / RGB-D host hands to
    VoxelDownsampling.  Depth = a floor-to-wall ramp + 16x16-pixel blocks of hashed offsets (objects) + per-pixel
    hashed jitter of +-2 mm; every pixel is valid, so there are exactly height * width points.  float64 arithmetic
    on hashed integers: the same points everywhere."""
    yy, xx, z = _depth_image64(seed, height, width, depth_min, depth_max)
    u = xx.astype(np.float64) - (width - 1) / 2.0
    v = yy.astype(np.float64) - (height - 1) / 2.0
    pts = np.stack([u * z / fx, v * z / fy, z], axis=-1)
    return pts.reshape(-1, 3).astype(np.float32)


def synth_depth_frame(seed: int, height: int = 480, width: int = 640, depth_min: float = 0.5, depth_max: float = 4.5,
                      hole_share: float = 0.0) -> np.ndarray:
    """float32 (height, width) depth image in metres: the frame synth_depth_cloud back-projects (its z column, row-major),
    what a depth camera hands to DepthToPointCloud / DepthAlignment.  hole_share > 0 sets that share of the pixels,
    chosen by a per-pixel hash, to 0 ("no measurement")."""
    yy, xx, z = _depth_image64(seed, height, width, depth_min, depth_max)
    d = z.astype(np.float32)
    if hole_share > 0.0:
        hole = (_hash3(seed, yy, xx, 6) % np.uint64(1 << 20)).astype(np.float64) < hole_share * (1 << 20)
        d[hole] = 0.0
    return d


THRESHOLD_FAMILIES = ("uniform", "bimodal", "sawtooth", "constant", "trimodal", "spikes")


def synth_threshold_frame(seed: int, height: int = 480, width: int = 640, family: str = "trimodal",
                          levels: int = 256) -> np.ndarray:
    """(height, width) frame with values in [0, levels) for the threshold kernels, uint8 for levels <= 256 and uint16
    above.  Families: "uniform" (every level equally likely), "bimodal" / "trimodal" (8x8-pixel regions assigned to two
    or three modes, triangular per-pixel spread of +-levels/10 around each), "sawtooth" (a diagonal ramp that wraps, plus
    +-levels/32 of noise), "constant" (one level, the worst case for histogram contention) and "spikes" (three exact
    levels, every other bin empty: exact ties between threshold candidates).  Pure integer hashes: the same frame
    everywhere."""
    if family not in THRESHOLD_FAMILIES:
        raise ValueError(f"family must be one of {THRESHOLD_FAMILIES}, got {family!r}")
    if not 2 <= levels <= 65536:
        raise ValueError(f"levels must be between 2 and 65536, got {levels}")
    y = np.arange(height, dtype=np.uint64)[:, None]
    x = np.arange(width, dtype=np.uint64)[None, :]
    yy, xx = np.broadcast_arrays(y, x)
    L = np.int64(levels)

    def h(a, b, salt, mod):
        return (_hash3(seed, a, b, salt) % np.uint64(mod)).astype(np.int64)

    if family == "uniform":
        v = h(yy, xx, 11, levels)
    elif family == "constant":
        v = np.full((height, width), int(h(np.uint64(0), np.uint64(0), 12, levels)), np.int64)
    elif family == "sawtooth":
        spread = max(1, levels // 32)
        v = (3 * xx.astype(np.int64) + 5 * yy.astype(np.int64)) * max(1, levels // 256) % L + h(yy, xx, 13, 2 * spread + 1) - spread
    elif family == "spikes":
        at = np.array([levels // 9, levels // 2 + 1, levels - 1 - levels // 7], np.int64)
        v = at[np.minimum(h(yy, xx, 14, 10) // 3, 2)]              # shares 3 : 3 : 4
    else:
        centres = np.array([levels // 4, (7 * levels) // 10] if family == "bimodal"
                           else [(3 * levels) // 20, levels // 2, (17 * levels) // 20], np.int64)
        spread = max(1, levels // 10)
        mode = h(yy // np.uint64(8), xx // np.uint64(8), 15, len(centres))
        v = centres[mode] + (h(yy, xx, 16, spread + 1) + h(yy, xx, 17, spread + 1) - spread)
    v = np.clip(v, 0, L - 1)
    return v.astype(np.uint8 if levels <= 256 else np.uint16)


TWO_VIEW_IMAGE = (480, 640)            # (height, width) of synth_two_view's camera; principal point at (320, 240)


def two_view_camera(f: float = 500.0) -> np.ndarray:
    """float64 (3, 3) camera matrix of synth_two_view: focal length f, principal point (320, 240)."""
    return np.array([[f, 0.0, TWO_VIEW_IMAGE[1] / 2.0], [0.0, f, TWO_VIEW_IMAGE[0] / 2.0], [0.0, 0.0, 1.0]])


def synth_two_view(seed: int, n: int, outlier_fraction: float, noise_px: float, f: float = 500.0):
    """A two-view scene for the relative-pose kernels: (keypoints1, keypoints2, R, t, inlier).  keypoints (n, 2) float32
    in pixel (y, x) order under two_view_camera(f); R (3, 3), t (3,) float64 with x2 ~ R x1 + t and |t| = 1; inlier (n,)
    bool, the planted inlier mask.  n points uniform in [-2, 2] x [-1.5, 1.5] x [3, 9] in the first camera's frame; R the
    Rodrigues rotation of a N(0, 0.08^2) vector; a baseline of 0.4 in a uniformly random direction; N(0, noise_px^2) added
    to both views' pixels; round(outlier_fraction * n) correspondences, chosen by a hashed ranking, have their second-view
    point replaced by a uniform draw over the image.  float64 arithmetic on hashed integers: the same scene everywhere."""
    idx = np.arange(n, dtype=np.uint64)

    def uni(salt, count=n):
        """uniform (0, 1) float64, `count` draws"""
        i = np.arange(count, dtype=np.uint64)
        return ((_hash3(seed, i, np.uint64(salt) + 0 * i, 21) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)

    def normal(salt, count=n):
        return np.sqrt(-2.0 * np.log(uni(salt, count))) * np.cos(2.0 * np.pi * uni(salt + 1, count))

    pts = np.stack([-2.0 + 4.0 * uni(0), -1.5 + 3.0 * uni(1), 3.0 + 6.0 * uni(2)], axis=1)
    w = 0.08 * normal(3, 3)
    th = float(np.linalg.norm(w))
    k = w / th if th > 0 else np.array([0.0, 0.0, 1.0])
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)
    d = normal(5, 3)
    t = d / np.linalg.norm(d)
    K = two_view_camera(f)
    x1 = pts
    x2 = pts @ R.T + 0.4 * t
    px1 = (x1 / x1[:, 2:]) @ K.T
    px2 = (x2 / x2[:, 2:]) @ K.T
    px1 = px1[:, :2] + noise_px * np.stack([normal(7), normal(9)], axis=1)
    px2 = px2[:, :2] + noise_px * np.stack([normal(11), normal(13)], axis=1)
    n_out = int(round(outlier_fraction * n))
    order = np.argsort(_hash3(seed, idx, np.uint64(15) + 0 * idx, 21), kind="stable")
    inlier = np.ones(n, dtype=bool)
    inlier[order[:n_out]] = False
    rand_px = np.stack([TWO_VIEW_IMAGE[1] * uni(16), TWO_VIEW_IMAGE[0] * uni(17)], axis=1)
    px2[~inlier] = rand_px[~inlier]
    return (px1[:, ::-1].astype(np.float32), px2[:, ::-1].astype(np.float32), R, t, inlier)


def synth_planar_two_view(seed: int, n: int, outlier_fraction: float, noise_px: float, baseline: float = 0.4, f: float = 500.0):
    """synth_two_view's scene with every point on ONE PLANE, for the homography kernels: (keypoints1, keypoints2, R, t,
    normal, distance, inlier).  The same hashed draws as synth_two_view (x and y of the points, the rotation, the
    translation's direction, the noise, the outliers); the depth of a point is not drawn but follows from the plane
    normal . X = distance through (0, 0, 5), whose unit normal is (0, 0, 1) tilted by a hashed angle of up to 20 degrees
    about a hashed axis in the image plane.  t (3,) float64 is the whole translation, `baseline` times the unit direction
    (synth_two_view returns the direction alone): x2 ~ (R + t normal^T / distance) x1 for the planted inliers.
    baseline = 0 gives the rotation-only scene (t = 0)."""
    idx = np.arange(n, dtype=np.uint64)

    def uni(salt, count=n):
        i = np.arange(count, dtype=np.uint64)
        return ((_hash3(seed, i, np.uint64(salt) + 0 * i, 21) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)

    def normal_draw(salt, count=n):
        return np.sqrt(-2.0 * np.log(uni(salt, count))) * np.cos(2.0 * np.pi * uni(salt + 1, count))

    tilt, phi = np.deg2rad(20.0) * uni(19, 1)[0], 2.0 * np.pi * uni(20, 1)[0]
    nrm = np.array([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)])
    dist = 5.0 * nrm[2]
    x, y = -2.0 + 4.0 * uni(0), -1.5 + 3.0 * uni(1)
    pts = np.stack([x, y, (dist - nrm[0] * x - nrm[1] * y) / nrm[2]], axis=1)
    w = 0.08 * normal_draw(3, 3)
    th = float(np.linalg.norm(w))
    k = w / th if th > 0 else np.array([0.0, 0.0, 1.0])
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)
    d = normal_draw(5, 3)
    t = float(baseline) * d / np.linalg.norm(d)
    K = two_view_camera(f)
    x2 = pts @ R.T + t
    px1 = (pts / pts[:, 2:]) @ K.T
    px2 = (x2 / x2[:, 2:]) @ K.T
    px1 = px1[:, :2] + noise_px * np.stack([normal_draw(7), normal_draw(9)], axis=1)
    px2 = px2[:, :2] + noise_px * np.stack([normal_draw(11), normal_draw(13)], axis=1)
    n_out = int(round(outlier_fraction * n))
    order = np.argsort(_hash3(seed, idx, np.uint64(15) + 0 * idx, 21), kind="stable")
    inlier = np.ones(n, dtype=bool)
    inlier[order[:n_out]] = False
    rand_px = np.stack([TWO_VIEW_IMAGE[1] * uni(16), TWO_VIEW_IMAGE[0] * uni(17)], axis=1)
    px2[~inlier] = rand_px[~inlier]
    return (px1[:, ::-1].astype(np.float32), px2[:, ::-1].astype(np.float32), R, t, nrm, dist, inlier)


RGBD_BASELINE = 0.4                   # metres between the two views of synth_rgbd_pair


def rgbd_camera(height: int = 480, width: int = 640) -> np.ndarray:
    """float64 (3, 3) camera matrix of synth_rgbd_pair: two_view_camera() at 480 x 640, scaled with the width otherwise."""
    f = 500.0 * width / TWO_VIEW_IMAGE[1]
    return np.array([[f, 0.0, width / 2.0], [0.0, f, height / 2.0], [0.0, 0.0, 1.0]])


def synth_rgbd_pair(seed: int, n: int, outlier_fraction: float, noise_px: float, depth_noise: float, height: int = 480,
                    width: int = 640):
    """An RGB-D pair for the metric pose kernels: (keypoints1, keypoints2, depth1, depth2, R, t, inlier).  keypoints (n, 2)
    float32 in pixel (y, x) order under rgbd_camera(height, width); depth (height, width) float32 in metres, ZERO except at
    the rounded keypoint pixels (floor(v + 0.5)), where it holds the point's Z in that view; R (3, 3), t (3,) float64 with
    X2 = R X1 + t and |t| = RGBD_BASELINE metres; inlier (n,) bool, the planted inlier mask.

    synth_two_view's geometry with a metric baseline: points uniform in [-2, 2] x [-1.5, 1.5] x [3, 9] m in the first
    camera's frame, R the Rodrigues rotation of a N(0, 0.08^2) vector, the baseline in a uniformly random direction;
    N(0, noise_px^2) on both views' pixels and N(0, (depth_noise z^2)^2) on both depths (a stereo sensor's error grows with
    z^2).  round(outlier_fraction * n) rows, chosen by a hashed ranking, are outliers: their second-view pixel is uniform over
    the image and both their depths are uniform in [3, 9] m.  A row whose pixel falls outside the frame in either view, or
    rounds to a pixel that an earlier row (or an earlier candidate of the same attempt) already holds in that view, is
    RE-DRAWN whole from a hashed attempt counter until it fits: within a view no two keypoints share a depth pixel.
    float64 arithmetic on hashed integers: the same scene everywhere."""
    K = rgbd_camera(height, width)

    def uni(rows, attempt, salt):
        """uniform (0, 1) float64 per row for this attempt"""
        r = np.asarray(rows, dtype=np.uint64)
        return ((_hash3(seed, r, np.uint64(attempt) * np.uint64(64) + np.uint64(salt) + 0 * r, 23) >> np.uint64(11)).astype(np.float64)
                + 0.5) / float(1 << 53)

    def normal(rows, attempt, salt):
        return np.sqrt(-2.0 * np.log(uni(rows, attempt, salt))) * np.cos(2.0 * np.pi * uni(rows, attempt, salt + 1))

    three = np.arange(3)
    w = 0.08 * normal(three, 0, 40)
    th = float(np.linalg.norm(w))
    k = w / th if th > 0 else np.array([0.0, 0.0, 1.0])
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)
    d = normal(three, 0, 42)
    t = RGBD_BASELINE * d / np.linalg.norm(d)
    idx = np.arange(n, dtype=np.uint64)
    n_out = int(round(outlier_fraction * n))
    order = np.argsort(_hash3(seed, idx, np.uint64(15) + 0 * idx, 23), kind="stable")
    inlier = np.ones(n, dtype=bool)
    inlier[order[:n_out]] = False

    kp1, kp2 = np.zeros((n, 2)), np.zeros((n, 2))              # pixel (x, y)
    z1, z2 = np.zeros(n), np.zeros(n)
    taken = [np.zeros(height * width, bool), np.zeros(height * width, bool)]
    pending, attempt = np.arange(n), 0
    while pending.size:
        if attempt >= 1024:
            raise ValueError(f"synth_rgbd_pair: {pending.size} of {n} keypoints found no free pixel in a {height} x {width} frame")
        rows = pending
        x1 = np.stack([-2.0 + 4.0 * uni(rows, attempt, 0), -1.5 + 3.0 * uni(rows, attempt, 1), 3.0 + 6.0 * uni(rows, attempt, 2)], axis=1)
        x2 = x1 @ R.T + t
        p1 = ((x1 / x1[:, 2:]) @ K.T)[:, :2] + noise_px * np.stack([normal(rows, attempt, 4), normal(rows, attempt, 6)], axis=1)
        p2 = ((x2 / x2[:, 2:]) @ K.T)[:, :2] + noise_px * np.stack([normal(rows, attempt, 8), normal(rows, attempt, 10)], axis=1)
        za = x1[:, 2] + depth_noise * x1[:, 2] ** 2 * normal(rows, attempt, 12)
        zb = x2[:, 2] + depth_noise * x2[:, 2] ** 2 * normal(rows, attempt, 14)
        out = ~inlier[rows]
        p2[out] = np.stack([width * uni(rows, attempt, 16), height * uni(rows, attempt, 17)], axis=1)[out]
        za[out] = (3.0 + 6.0 * uni(rows, attempt, 18))[out]
        zb[out] = (3.0 + 6.0 * uni(rows, attempt, 19))[out]
        p1, p2 = p1.astype(np.float32), p2.astype(np.float32)          # what the caller gets: round THESE
        ok = np.ones(rows.size, bool)
        pix = []
        for p in (p1, p2):
            q = np.floor(p + np.float32(0.5)).astype(np.int64)
            ok &= (q[:, 0] >= 0) & (q[:, 0] < width) & (q[:, 1] >= 0) & (q[:, 1] < height)
            pix.append(np.clip(q[:, 1], 0, height - 1) * width + np.clip(q[:, 0], 0, width - 1))
        for view in (0, 1):
            ok &= ~taken[view][pix[view]]
            cand = np.flatnonzero(ok)
            first = np.zeros(rows.size, bool)
            first[cand[np.unique(pix[view][cand], return_index=True)[1]]] = True      # the lowest row among equal pixels
            ok &= first
        acc = rows[ok]
        kp1[acc], kp2[acc], z1[acc], z2[acc] = p1[ok], p2[ok], za[ok], zb[ok]
        taken[0][pix[0][ok]] = True
        taken[1][pix[1][ok]] = True
        pending = rows[~ok]
        attempt += 1
    kp1, kp2 = kp1.astype(np.float32), kp2.astype(np.float32)
    depth1, depth2 = np.zeros((height, width), np.float32), np.zeros((height, width), np.float32)
    for kp, z, depth in ((kp1, z1, depth1), (kp2, z2, depth2)):
        q = np.floor(kp + np.float32(0.5)).astype(np.int64)
        depth[q[:, 1], q[:, 0]] = z.astype(np.float32)
    return (np.ascontiguousarray(kp1[:, ::-1]), np.ascontiguousarray(kp2[:, ::-1]), depth1, depth2, R, t, inlier)


def synth_colour_frame(seed: int, height: int, width: int, channels: int = 3) -> np.ndarray:
    """uint8 (height, width, channels) interleaved colour frame with structure, what a camera hands to the frame ingest:
    synth_image(seed) at half the size, upsampled 2x by pixel repetition (so that its corners survive an ingest to half
    the size), times a per-channel gain (0.9, 1.0, 0.8, then 1.0) plus +-6 of per-byte hashed noise.  A 4th channel is
    filled like the others (the ingest ignores it).  The same frame everywhere."""
    if channels not in (1, 3, 4):
        raise ValueError(f"channels must be 1, 3 or 4, got {channels}")
    small = synth_image(seed, (height + 1) // 2, (width + 1) // 2).astype(np.int64)
    base = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)[:height, :width]
    y = np.arange(height, dtype=np.uint64)[:, None]
    x = np.arange(width, dtype=np.uint64)[None, :]
    yy, xx = np.broadcast_arrays(y, x)
    gains = (9, 10, 8, 10)
    out = np.empty((height, width, channels), np.uint8)
    for c in range(channels):
        noise = (_hash3(seed, yy, xx, 40 + c) % np.uint64(13)).astype(np.int64) - 6
        out[:, :, c] = np.clip(base * gains[c if channels > 1 else 1] // 10 + noise, 0, 255)
    return out


def synth_depth_room(seed: int, height: int, width: int, rotation_deg: float = 2.0, translation: float = 0.05,
                     sphere: bool = True):
    """Two dense depth frames of one room for the dense refinement kernels: (depth1, depth2, R, t).  depth (height, width)
    float32 in metres, the Z of the nearest surface along the ray of every integer pixel under rgbd_camera(height, width),
    ray-cast analytically in float64; R (3, 3), t (3,) float64 with X2 = R X1 + t.

    The room, in the first camera's frame (y down): the floor y = 0.9, two walls n . X = c with n = (+-sqrt(.5), 0, sqrt(.5))
    and c = 3 sqrt(.5) + 0.3 and 3 sqrt(.5) - 0.1 (a corner ahead of the camera) and, with `sphere`, a sphere of radius 0.4
    at (0.3, 0.4, 2.2).  Without the sphere the scene is three planes, whose registration is ill-conditioned at coarse
    strides: use it only where degeneracy is the point.  The second view is rotated by rotation_deg about a seeded random
    axis and moved by `translation` metres in a seeded random direction.  Every pixel of both frames has a depth."""
    K = rgbd_camera(height, width)
    three = np.arange(3, dtype=np.uint64)

    def normal3(salt):
        u1 = ((_hash3(seed, three, np.uint64(salt) + 0 * three, 29) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)
        u2 = ((_hash3(seed, three, np.uint64(salt + 1) + 0 * three, 29) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)

    k = normal3(0)
    k = k / np.linalg.norm(k)
    th = np.deg2rad(rotation_deg)
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)
    d = normal3(2)
    t = translation * d / np.linalg.norm(d)
    s5 = np.sqrt(0.5)
    planes = [(np.array([0.0, 1.0, 0.0]), 0.9), (np.array([s5, 0.0, s5]), 3.0 * s5 + 0.3), (np.array([-s5, 0.0, s5]), 3.0 * s5 - 0.1)]
    centre, radius = np.array([0.3, 0.4, 2.2]), 0.4
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    rays = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)

    def cast(origin, rot):
        """depth along rays `rot @ ray` from `origin`, both in the first camera's frame; the ray's own z is 1, so the ray
        parameter is the depth in the casting camera"""
        dirs = rays @ rot.T
        best = np.full(xs.shape, np.inf)
        for n, c in planes:
            den = dirs @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                s = (c - origin @ n) / den
            best = np.where((den > 1e-12) & (s > 0) & (s < best), s, best)
        if sphere:
            oc = origin - centre
            a = (dirs * dirs).sum(-1)
            bq = dirs @ oc
            disc = bq * bq - a * (oc @ oc - radius * radius)
            with np.errstate(invalid="ignore"):
                s = (-bq - np.sqrt(disc)) / a
            best = np.where((disc > 0) & (s > 0) & (s < best), s, best)
        return np.where(np.isfinite(best), best, 0.0).astype(np.float32)

    return cast(np.zeros(3), np.eye(3)), cast(-R.T @ t, R.T), R, t


BA_FRAME_SPACING = 0.15               # metres between neighbouring cameras of synth_ba_window


def _rodrigues64(w: np.ndarray) -> np.ndarray:
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def synth_ba_window(seed: int, frames: int, landmarks: int, visibility: float = 1.0, noise_px: float = 0.5,
                    outlier_fraction: float = 0.0, pose_noise: float = 0.01, point_noise: float = 0.05, num_fixed: int = 1):
    """A window for the bundle-adjustment kernels (K25): (R0, t0, X0, keypoints, visible, R, t, X, outlier).

    The truth: X (landmarks, 3) float64 uniform in [-2, 2] x [-1.5, 1.5] x [3, 9] m, synth_rgbd_pair's volume, in the frame
    of camera 0 (R[0] = I, t[0] = 0); camera f has its centre at f * BA_FRAME_SPACING m along x plus N(0, 0.02^2) m per axis and
    the Rodrigues rotation of a N(0, 0.04^2) vector; R (frames, 3, 3), t (frames, 3) float64 with X_c = R X + t.
    keypoints (frames, landmarks, 2) float32 in pixel (y, x) order under rgbd_camera(): the projection plus N(0, noise_px^2)
    per axis.  visible (frames, landmarks) bool: a hashed uniform below `visibility`, the point in front of the camera and its
    pixel inside the 480 x 640 frame.  outlier (frames, landmarks) bool marks round(outlier_fraction * visible.sum()) visible
    observations, chosen by a hashed ranking, whose pixel is uniform over the image instead.
    The start: the first num_fixed frames at their TRUE poses (they are the gauge; a perturbed gauge moves the optimum away
    from the truth); every other pose left-multiplied by the rotation of a N(0, pose_noise^2) vector (radians) with
    N(0, pose_noise^2) metres added to t; N(0, point_noise^2) metres on every point coordinate.  R0, t0, X0 are float32.
    float64 arithmetic on hashed integers: the same window everywhere."""
    if not 1 <= num_fixed <= frames:
        raise ValueError(f"synth_ba_window: num_fixed must be in 1 .. {frames}, got {num_fixed}")
    height, width = TWO_VIEW_IMAGE
    K = rgbd_camera(height, width)

    def uni(shape, salt):
        idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
        return (((_hash3(seed, idx, np.uint64(salt) + 0 * idx, 29) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)).reshape(shape)

    def normal(shape, salt):
        return np.sqrt(-2.0 * np.log(uni(shape, salt))) * np.cos(2.0 * np.pi * uni(shape, salt + 1))

    X = np.stack([-2.0 + 4.0 * uni((landmarks,), 0), -1.5 + 3.0 * uni((landmarks,), 1), 3.0 + 6.0 * uni((landmarks,), 2)], axis=1)
    w_true, c_noise = 0.04 * normal((frames, 3), 4), 0.02 * normal((frames, 3), 6)
    R, t = np.zeros((frames, 3, 3)), np.zeros((frames, 3))
    for f in range(frames):
        R[f] = _rodrigues64(w_true[f]) if f else np.eye(3)
        c = np.array([f * BA_FRAME_SPACING, 0.0, 0.0]) + c_noise[f] if f else np.zeros(3)
        t[f] = -R[f] @ c
    xc = np.einsum("fij,lj->fli", R, X) + t[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        px = K[0, 0] * xc[..., 0] / xc[..., 2] + K[0, 2] + noise_px * normal((frames, landmarks), 8)
        py = K[1, 1] * xc[..., 1] / xc[..., 2] + K[1, 2] + noise_px * normal((frames, landmarks), 10)
    visible = (uni((frames, landmarks), 12) < visibility) & (xc[..., 2] > 0.1) & (px >= 0) & (px <= width - 1) & (py >= 0) & (py <= height - 1)
    n_out = int(round(outlier_fraction * int(visible.sum())))
    rank = _hash3(seed, np.arange(frames * landmarks, dtype=np.uint64), np.full(frames * landmarks, 13, np.uint64), 29).reshape(frames, landmarks)
    order = np.argsort(np.where(visible, rank, np.uint64(0xFFFFFFFFFFFFFFFF)).ravel(), kind="stable")
    outlier = np.zeros(frames * landmarks, bool)
    outlier[order[:n_out]] = True
    outlier = outlier.reshape(frames, landmarks) & visible
    px = np.where(outlier, (width - 1) * uni((frames, landmarks), 14), px)
    py = np.where(outlier, (height - 1) * uni((frames, landmarks), 15), py)
    keypoints = np.nan_to_num(np.stack([py, px], axis=-1)).astype(np.float32)
    w0, dt0 = pose_noise * normal((frames, 3), 16), pose_noise * normal((frames, 3), 18)
    R0, t0 = R.copy(), t.copy()
    for f in range(num_fixed, frames):
        E = _rodrigues64(w0[f])
        R0[f], t0[f] = E @ R[f], E @ t[f] + dt0[f]
    X0 = X + point_noise * normal((landmarks, 3), 20)
    return R0.astype(np.float32), t0.astype(np.float32), X0.astype(np.float32), keypoints, visible, R, t, X, outlier


def synth_place_descriptors(seed: int, n_frames: int, k: int, num_bits: int, flip: float = 0.1, keep: float = 0.5):
    """Packed descriptors for the retrieval kernels (K26): (db_bits, q_bits, target, source).

    db_bits (n_frames, k, num_bits / 32) int32: uniform random bits, bit b of a descriptor in bit b % 32 of word b // 32.
    q_bits (k, num_bits / 32) int32: a REVISIT of keyframe `target` (a hashed choice): round(keep * k) of its descriptors,
    chosen by a hashed ranking, are kept with every bit flipped with probability `flip`, the others are replaced by fresh
    random descriptors, and the rows are permuted by a hashed ranking.  source (k,) int64: the row of keyframe `target` a
    query row was made from, -1 for a replaced one.  Hashed integers only: the same arrays everywhere."""
    if num_bits % 32 != 0 or num_bits <= 0:
        raise ValueError(f"synth_place_descriptors: num_bits must be a positive multiple of 32, got {num_bits}")
    if not (0.0 <= flip <= 1.0 and 0.0 <= keep <= 1.0) or n_frames < 1 or k < 1:
        raise ValueError("synth_place_descriptors: flip and keep must lie in [0, 1], n_frames and k be positive")
    words = num_bits // 32

    def draw(rows, cols, salt):                      # (rows, cols) uint64 hashes
        r, c = np.broadcast_arrays(np.arange(rows, dtype=np.uint64)[:, None], np.arange(cols, dtype=np.uint64)[None, :])
        return _hash3(seed, r, c, salt)

    db = (draw(n_frames * k, words, 31) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(n_frames, k, words)
    target = int(_hash3(seed, np.zeros(1, np.uint64), np.zeros(1, np.uint64), 32)[0] % np.uint64(n_frames))
    n_keep = int(round(keep * k))
    kept = np.zeros(k, bool)
    kept[np.argsort(draw(k, 1, 33)[:, 0], kind="stable")[:n_keep]] = True
    uniform = ((draw(k, num_bits, 34) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)
    flips = (uniform < flip).reshape(k, words, 32)
    mask = (flips.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    fresh = (draw(k, words, 35) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rows = np.where(kept[:, None], db[target] ^ mask, fresh)
    order = np.argsort(draw(k, 1, 36)[:, 0], kind="stable")
    source = np.where(kept, np.arange(k), -1)[order].astype(np.int64)
    return db.view(np.int32), np.ascontiguousarray(rows[order]).view(np.int32), target, source


def synth_pose_graph(seed: int, nodes: int, loops: int, sigma_rot: float, sigma_trans: float, false_loops: int = 0):
    """A pose graph for the pose-graph kernels (K27): (R0, t0, edge_index, R_meas, t_meas, information, fixed, protected, R, t,
    false_edge).

    The truth: `nodes` cameras going TWICE round a closed ring in the x-z plane (0.15 m between neighbours, so a radius of
    0.15 * (nodes / 2) / (2 pi) m), looking along the tangent, with a wobble of N(0, 0.02^2) m per axis on the centre and the
    Rodrigues rotation of a N(0, 0.04^2) vector on the orientation; R (nodes, 3, 3), t (nodes, 3) float64 with X_c = R X + t.
    Edges (i, j) carry the motion X_j = R_z X_i + t_z: nodes - 1 odometry edges (k, k + 1), then `loops` loop edges
    (i, i + nodes // 2), i = l * ((nodes - nodes // 2) // loops) -- a place seen on the first lap and again on the second --,
    then `false_loops` edges between hashed pairs.  A measurement is the true motion perturbed in the residual's coordinates:
    R_z = Exp(w)^T R_p, t_z = Exp(w)^T (t_p - tau) with w ~ N(0, sigma_rot^2), tau ~ N(0, sigma_trans^2) per axis, so that the
    edge's residual at the truth is exactly (w, tau); a false loop's (w, tau) is N(0, 0.5^2) rad and N(0, 1) m instead.
    information (E, 6, 6) = diag(1 / sigma_rot^2 x 3, 1 / sigma_trans^2 x 3) (sigma = 0: the identity); fixed (nodes,) bool: node
    0; protected (E,) bool: the odometry edges; false_edge (E,) bool.  The start R0, t0 (float32): node 0 at the truth, the
    odometry chained from it.  edge_index int32, measurements and information float32.  float64 arithmetic on hashed integers:
    the same graph everywhere."""
    if nodes < 2 or loops < 0 or false_loops < 0 or 2 * loops > nodes:
        raise ValueError(f"synth_pose_graph: nodes >= 2 and 0 <= 2 loops <= nodes, got {nodes} nodes, {loops} loops, {false_loops} false loops")

    def uni(shape, salt):
        idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
        return (((_hash3(seed, idx, np.uint64(salt) + 0 * idx, 37) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)).reshape(shape)

    def normal(shape, salt):
        return np.sqrt(-2.0 * np.log(uni(shape, salt))) * np.cos(2.0 * np.pi * uni(shape, salt + 1))

    radius = BA_FRAME_SPACING * (nodes / 2.0) / (2.0 * np.pi)
    ang = 4.0 * np.pi * np.arange(nodes) / nodes
    centre = np.stack([radius * np.sin(ang), np.zeros(nodes), radius * (1.0 - np.cos(ang))], 1) + 0.02 * normal((nodes, 3), 0)
    wob = 0.04 * normal((nodes, 3), 2)
    R, t = np.zeros((nodes, 3, 3)), np.zeros((nodes, 3))
    for k in range(nodes):
        heading = _rodrigues64(np.array([0.0, ang[k], 0.0]))              # camera-to-world: the z axis along the tangent
        R[k] = (heading @ _rodrigues64(wob[k])).T
        t[k] = -R[k] @ centre[k]
    step = (nodes - nodes // 2) // loops if loops else 0
    pairs = [(k, k + 1) for k in range(nodes - 1)] + [(l * step, l * step + nodes // 2) for l in range(loops)]
    for f in range(false_loops):
        h = _hash3(seed, np.array([f, f], np.uint64), np.array([0, 1], np.uint64), 38)
        i = int(h[0] % np.uint64(nodes))
        j = (i + 2 + int(h[1] % np.uint64(max(nodes - 3, 1)))) % nodes
        pairs.append((i, j))
    E = len(pairs)
    ei = np.array(pairs, np.int32).reshape(E, 2)
    false_edge = np.arange(E) >= nodes - 1 + loops
    w = sigma_rot * normal((E, 3), 4)
    tau = sigma_trans * normal((E, 3), 6)
    w[false_edge] = 0.5 * normal((E, 3), 8)[false_edge]
    tau[false_edge] = 1.0 * normal((E, 3), 10)[false_edge]
    zr, zt = np.zeros((E, 3, 3)), np.zeros((E, 3))
    for e, (i, j) in enumerate(pairs):
        Rp = R[j] @ R[i].T
        tp = t[j] - Rp @ t[i]
        Ew = _rodrigues64(w[e])
        zr[e], zt[e] = Ew.T @ Rp, Ew.T @ (tp - tau[e])
    sr = 1.0 / sigma_rot ** 2 if sigma_rot > 0 else 1.0
    st = 1.0 / sigma_trans ** 2 if sigma_trans > 0 else 1.0
    information = np.tile(np.diag([sr, sr, sr, st, st, st]), (E, 1, 1))
    R0, t0 = R.copy(), t.copy()
    for k in range(nodes - 1):
        R0[k + 1], t0[k + 1] = zr[k] @ R0[k], zr[k] @ t0[k] + zt[k]
    fixed = np.arange(nodes) == 0
    protected = np.arange(E) < nodes - 1
    return (R0.astype(np.float32), t0.astype(np.float32), ei, zr.astype(np.float32), zt.astype(np.float32), information.astype(np.float32),
            fixed, protected, R, t, false_edge)


def synth_sim3_graph(seed: int, nodes: int, loops: int, sigma_rot: float, sigma_trans: float, sigma_scale: float, drift: float,
                     false_loops: int = 0):
    """A similarity pose graph for the Sim(3) pose-graph kernels (K31): (s0, R0, t0, edge_index, s_meas, R_meas, t_meas,
    information, fixed, protected, s, R, t, false_edge) -- a monocular trajectory whose unit drifts, and the loops that show it.

    The truth is synth_pose_graph(seed, nodes, loops, ...)'s ring with its edges (odometry, loops, false loops), metric:
    s = ones (nodes,), R, t float64 with X_c = s R X + t.  Edges (i, j) carry the similarity X_j = s_z R_z X_i + t_z, the true
    one perturbed in the residual's coordinates: s_z = exp(-sigma) s_p, R_z = Exp(w)^T R_p, t_z = exp(-sigma) Exp(w)^T (t_p - tau)
    with w ~ N(0, sigma_rot^2), tau ~ N(0, sigma_trans^2) per axis and sigma ~ N(0, sigma_scale^2), so that the edge's residual
    at the truth is exactly (w, tau, sigma).  ODOMETRY edges have sigma = 0: their scale is exactly 1, as relative poses taken
    from a metric trajectory have.  A false loop's (w, tau, sigma) is N(0, 0.5^2) rad, N(0, 1) m and N(0, 0.5^2) instead.
    information (E, 7, 7) = diag(1 / sigma_rot^2 x 3, 1 / sigma_trans^2 x 3, 1 / sigma_scale^2) (a sigma of 0: 1).  The start
    (float32): node 0 at the truth, then the odometry chained with a scale drift of exp(drift) per edge:
    s0[k + 1] = exp(drift) s0[k], R0[k + 1] = R_z R0[k], t0[k + 1] = exp(drift) R_z t0[k] + t_z -- the unit of node k is
    exp(k drift) world units, which no odometry edge agrees with and only the loops can measure.  fixed: node 0; protected: the
    odometry edges.  edge_index int32, measurements and information float32.  float64 arithmetic on hashed integers: the same
    graph everywhere."""
    if not (sigma_scale >= 0 and np.isfinite(drift)):
        raise ValueError(f"synth_sim3_graph: sigma_scale >= 0 and a finite drift, got {sigma_scale} and {drift}")
    _, _, ei, _, _, _, fixed, protected, R, t, false_edge = synth_pose_graph(seed, nodes, loops, 0.0, 0.0, false_loops)
    E = len(ei)

    def uni(shape, salt):
        idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
        return (((_hash3(seed, idx, np.uint64(salt) + 0 * idx, 51) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)).reshape(shape)

    def normal(shape, salt):
        return np.sqrt(-2.0 * np.log(uni(shape, salt))) * np.cos(2.0 * np.pi * uni(shape, salt + 1))

    w, tau, sig = sigma_rot * normal((E, 3), 0), sigma_trans * normal((E, 3), 2), sigma_scale * normal((E,), 4)
    sig[protected] = 0.0
    w[false_edge] = 0.5 * normal((E, 3), 6)[false_edge]
    tau[false_edge] = 1.0 * normal((E, 3), 8)[false_edge]
    sig[false_edge] = 0.5 * normal((E,), 10)[false_edge]
    zs, zr, zt = np.zeros(E), np.zeros((E, 3, 3)), np.zeros((E, 3))
    for e, (i, j) in enumerate(ei):
        Rp = R[j] @ R[i].T
        tp = t[j] - Rp @ t[i]
        Ew = _rodrigues64(w[e])
        zs[e] = np.exp(-sig[e])
        zr[e], zt[e] = Ew.T @ Rp, zs[e] * (Ew.T @ (tp - tau[e]))
    inv = lambda v: 1.0 / v ** 2 if v > 0 else 1.0
    information = np.tile(np.diag([inv(sigma_rot)] * 3 + [inv(sigma_trans)] * 3 + [inv(sigma_scale)]), (E, 1, 1))
    s0, R0, t0 = np.ones(nodes), R.copy(), t.copy()
    gain = np.exp(drift)
    for k in range(nodes - 1):
        s0[k + 1] = gain * s0[k]
        R0[k + 1], t0[k + 1] = zr[k] @ R0[k], gain * (zr[k] @ t0[k]) + zt[k]
    f32 = np.float32
    return (s0.astype(f32), R0.astype(f32), t0.astype(f32), ei, zs.astype(f32), zr.astype(f32), zt.astype(f32), information.astype(f32),
            fixed, protected, np.ones(nodes), R, t, false_edge)


def synth_track_window(seed: int, frames: int, keypoints: int, landmarks: int, pair_span: int = 2, miss: float = 0.1,
                       outlier_fraction: float = 0.1, noise_px: float = 0.5, pose_noise: float = 0.002):
    """A window for the landmark-track kernels (K28): (keypoints, kp_id, pair_frames, match_ij, match_valid, R0, t0, R, t, X).

    The scene is synth_ba_window(seed, frames, landmarks, visibility = 1 - miss, noise_px, pose_noise = pose_noise): its truth
    R, t, X (float64), its perturbed start R0, t0 (float32, frame 0 at the truth; 0.002 rad is one pixel at this camera: poses
    as a PnP on a few hundred matches leaves them) and its observations.  Every frame has `keypoints` keypoint slots:
    the landmarks the frame sees go to slots chosen by a hashed permutation, the other slots are clutter, uniform over the
    480 x 640 image.  keypoints (frames, keypoints, 2) float32 pixel (y, x); kp_id (frames, keypoints) int32: the planted
    landmark, -1 for clutter.  pair_frames (P, 2) int32: every (a, b) with 0 < b - a <= pair_span, a ascending.  Per pair the
    matcher is one-to-one: every landmark both frames see is matched; round(outlier_fraction * their number) of those matches,
    chosen by a hashed ranking, have their end in b moved to a keypoint of b that no match of the pair uses (clutter, or a
    landmark a does not see): wrong matches.  match_ij (P, M, 2) int32 with M = keypoints, match_valid (P, M) bool: the matches
    at hashed positions of the list; every other record is padding whose index fields hold garbage (-1, 0x7fffffff, -2^31 or
    a number that looks like an index).  float64 arithmetic on hashed integers: the same window everywhere."""
    if frames < 2 or not 1 <= landmarks <= keypoints or not 1 <= pair_span < frames or not 0 <= miss < 1 or not 0 <= outlier_fraction <= 1:
        raise ValueError(f"synth_track_window: frames >= 2, 1 <= landmarks <= keypoints, 1 <= pair_span < frames, 0 <= miss < 1, "
                         f"0 <= outlier_fraction <= 1, got {frames}, {landmarks}, {keypoints}, {pair_span}, {miss}, {outlier_fraction}")
    R0, t0, _, kp_l, visible, R, t, X, _ = synth_ba_window(seed, frames, landmarks, 1.0 - miss, noise_px, pose_noise=pose_noise)
    height, width = TWO_VIEW_IMAGE

    def uni(shape, salt):
        idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
        return (((_hash3(seed, idx, np.uint64(salt) + 0 * idx, 41) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)).reshape(shape)

    K = keypoints
    kp = np.stack([(height - 1) * uni((frames, K), 0), (width - 1) * uni((frames, K), 1)], axis=-1).astype(np.float32)
    kp_id = np.full((frames, K), -1, np.int32)
    slot_of = np.full((frames, landmarks), -1, np.int64)
    for f in range(frames):
        seen = np.flatnonzero(visible[f])
        slots = np.argsort(uni((K,), 10 + f), kind="stable")[:len(seen)]
        kp[f, slots] = kp_l[f, seen]
        kp_id[f, slots] = seen
        slot_of[f, seen] = slots
    pairs = [(a, b) for a in range(frames) for b in range(a + 1, min(a + pair_span, frames - 1) + 1)]
    P, M = len(pairs), K
    pick = np.floor(4.0 * uni((P, M, 2), 2)).astype(np.int64)
    looks = np.floor(K * uni((P, M, 2), 3)).astype(np.int64)
    match_ij = np.choose(pick, [np.full_like(looks, -1), np.full_like(looks, 0x7FFFFFFF), looks, np.full_like(looks, -(1 << 31))]).astype(np.int32)
    match_valid = np.zeros((P, M), bool)
    for p, (a, b) in enumerate(pairs):
        both = np.flatnonzero((slot_of[a] >= 0) & (slot_of[b] >= 0))
        i, j = slot_of[a, both].copy(), slot_of[b, both].copy()
        free = np.setdiff1d(np.arange(K), j)
        free = free[np.argsort(uni((K,), 100 + 3 * p)[free], kind="stable")]
        wrong = np.argsort(uni((landmarks,), 101 + 3 * p)[both], kind="stable")[:min(int(round(outlier_fraction * len(both))), len(free))]
        j[wrong] = free[:len(wrong)]
        at = np.argsort(uni((M,), 102 + 3 * p), kind="stable")[:len(both)]
        match_ij[p, at, 0], match_ij[p, at, 1] = i, j
        match_valid[p, at] = True
    return kp, kp_id, np.array(pairs, np.int32).reshape(P, 2), match_ij, match_valid, R0, t0, R, t, X


def synth_localmap_window(seed: int, frames: int, keypoints: int, landmarks: int, num_bits: int, flip: float = 0.1, twins: float = 0.25,
                          rotation_deg: float = 2.0, translation: float = 0.05, **window):
    """A window for the local-map kernels (K29): synth_track_window(seed, frames, keypoints, landmarks, **window)'s tuple
    (keypoints, kp_id, pair_frames, match_ij, match_valid, R0, t0, R, t, X) followed by (bits, R_pred, t_pred, twin_of).

    Descriptors.  Every landmark has a BASE descriptor of num_bits uniform random bits (bit b in bit b % 32 of word b // 32).
    round(twins * landmarks) landmarks, chosen among 1 .. landmarks - 1 by a hashed ranking, are TWINS: taken in ascending
    order, twin l copies the base of a hashed landmark below l (repeated texture: what the ratio test and the claims are for);
    twin_of (landmarks,) int32 is that landmark, -1 for the others.  bits (frames, keypoints, num_bits / 32) int32: a planted
    keypoint holds its landmark's base with every bit flipped with probability `flip`, independently per observation; clutter
    holds independent uniform bits.
    The predicted pose of the LAST frame (float32): the truth R[-1], t[-1] moved by E, the rotation of rotation_deg degrees
    about the axis (1, -1, 1) / sqrt 3, and by d = translation * (1, 1, 1) / sqrt 3 metres: R_pred = E R[-1], t_pred = E t[-1] + d.
    Hashed integers only: the same arrays everywhere."""
    if num_bits % 32 != 0 or num_bits <= 0:
        raise ValueError(f"synth_localmap_window: num_bits must be a positive multiple of 32, got {num_bits}")
    if not (0.0 <= flip <= 1.0 and 0.0 <= twins <= 1.0):
        raise ValueError(f"synth_localmap_window: flip and twins must lie in [0, 1], got {flip} and {twins}")
    base_window = synth_track_window(seed, frames, keypoints, landmarks, **window)
    kp_id, R, t = base_window[1], base_window[7], base_window[8]
    words = num_bits // 32

    def draw(rows, cols, salt):                      # (rows, cols) uint64 hashes
        r, c = np.broadcast_arrays(np.arange(rows, dtype=np.uint64)[:, None], np.arange(cols, dtype=np.uint64)[None, :])
        return _hash3(seed, r, c, salt)

    base = (draw(landmarks, words, 43) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    n_twins = min(int(round(twins * landmarks)), landmarks - 1)
    twin_of = np.full(landmarks, -1, np.int32)
    chosen = np.sort(1 + np.argsort(draw(landmarks - 1, 1, 44)[:, 0], kind="stable")[:n_twins]) if n_twins else np.zeros(0, np.int64)
    source = draw(landmarks, 1, 45)[:, 0]
    for l in chosen:
        twin_of[l] = int(source[l] % np.uint64(l))
        base[l] = base[twin_of[l]]
    n = frames * keypoints
    uniform = ((draw(n, num_bits, 46) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)
    flips = (uniform < flip).reshape(n, words, 32)
    mask = (flips.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    fresh = (draw(n, words, 47) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ids = kp_id.reshape(n)
    bits = np.where((ids >= 0)[:, None], base[np.maximum(ids, 0)] ^ mask, fresh).reshape(frames, keypoints, words)
    E = _rodrigues64(np.radians(rotation_deg) * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0))
    R_pred = (E @ R[-1]).astype(np.float32)
    t_pred = (E @ t[-1] + translation * np.ones(3) / np.sqrt(3.0)).astype(np.float32)
    return (*base_window, np.ascontiguousarray(bits).view(np.int32), R_pred, t_pred, twin_of)


def synth_sim3_maps(seed: int, n: int, outliers: float, ray_noise: float, scale: float):
    """Two camera-frame point sets of one scene for the similarity kernels (K30): (pts1, pts2, s, R, t, inlier).  pts1, pts2
    (n, 3) float32: the landmarks in keyframe 1's camera frame and map-1 units, and in keyframe 2's camera frame and map-2
    units; s = scale, R (3, 3), t (3,) float64 with X2 = s R X1 + t for the noise-free points; inlier (n,) bool, the planted
    inlier mask.

    synth_rgbd_pair's geometry: points uniform in [-2, 2] x [-1.5, 1.5] x [3, 9] in frame 1, R the Rodrigues rotation of a
    N(0, 0.08^2) vector, t = scale * RGBD_BASELINE in a uniformly random direction.  The noise is the depth error of a
    triangulated point, ALONG the rays: each point of either set is multiplied by max(1 + ray_noise * N(0, 1), 0.1), so its
    projection into its own camera does not move.  round(outliers * n) rows, chosen by a hashed ranking, are outliers: their
    point of frame 2 is scale times a fresh uniform point of the same box.  float64 arithmetic on hashed integers: the same
    scene everywhere."""
    if n < 1 or not 0 <= outliers <= 1 or not ray_noise >= 0 or not (scale > 0 and scale < float("inf")):
        raise ValueError(f"synth_sim3_maps: n >= 1, 0 <= outliers <= 1, ray_noise >= 0, 0 < scale < inf, got {n}, {outliers}, "
                         f"{ray_noise}, {scale}")
    idx = np.arange(n, dtype=np.uint64)

    def uni(rows, salt):
        r = np.asarray(rows, dtype=np.uint64)
        return ((_hash3(seed, r, np.uint64(salt) + 0 * r, 53) >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)

    def normal(rows, salt):
        return np.sqrt(-2.0 * np.log(uni(rows, salt))) * np.cos(2.0 * np.pi * uni(rows, salt + 1))

    def box(salt):
        return np.stack([-2.0 + 4.0 * uni(idx, salt), -1.5 + 3.0 * uni(idx, salt + 1), 3.0 + 6.0 * uni(idx, salt + 2)], axis=1)

    three = np.arange(3)
    R = _rodrigues64(0.08 * normal(three, 40))
    d = normal(three, 42)
    t = float(scale) * RGBD_BASELINE * d / np.linalg.norm(d)
    x1 = box(0)
    x2 = float(scale) * (x1 @ R.T) + t
    n_out = int(round(outliers * n))
    inlier = np.ones(n, dtype=bool)
    inlier[np.argsort(_hash3(seed, idx, np.uint64(15) + 0 * idx, 53), kind="stable")[:n_out]] = False
    x2[~inlier] = (float(scale) * box(4))[~inlier]
    x1 = x1 * np.maximum(1.0 + ray_noise * normal(idx, 8), 0.1)[:, None]
    x2 = x2 * np.maximum(1.0 + ray_noise * normal(idx, 10), 0.1)[:, None]
    return x1.astype(np.float32), x2.astype(np.float32), float(scale), R, t, inlier


def synth_flow_pair(seed: int, height: int, width: int, angle_deg: float = 0.0, scale: float = 1.0, shift=(0.0, 0.0),
                    lam=(6.0, 64.0), terms: int = 24, quantise: bool = False):
    """Two frames that a tracker can follow (the hash images above are per-pixel noise and cannot be): exact samples of ONE
    analytic function I(x, y) = 128 + sum_m a_m sin(2 pi (fx_m x + fy_m y) + phi_m) with `terms` waves of wavelengths
    log-uniform in `lam`, directions uniform, a_m proportional to sqrt(lambda_m) and scaled to sum to 110 (so I stays inside
    [18, 238]).  Frame 1 is I at the pixel centres q = (x, y); frame 2 is I(A^-1 (q - d)) with A = scale * rotation by
    angle_deg about the frame centre c (A p = scale R (p - c) + c) and d = shift = (dx, dy), so that the point p of frame 1
    is seen at A p + d in frame 2 with no interpolation involved.  Returns (frame1, frame2, A (2, 3) float64 acting on
    (x, y, 1), d (2,) float64); the frames are (height, width) float32, or rounded to uint8 with `quantise`."""
    if height < 1 or width < 1 or terms < 1 or not 0 < lam[0] <= lam[1] or not scale > 0:
        raise ValueError("synth_flow_pair: height, width, terms >= 1, 0 < lam[0] <= lam[1], scale > 0")
    rng = np.random.default_rng(seed)
    wavelength = np.exp(rng.uniform(np.log(lam[0]), np.log(lam[1]), terms))
    theta = rng.uniform(0.0, 2.0 * np.pi, terms)
    phi = rng.uniform(0.0, 2.0 * np.pi, terms)
    fx, fy = np.cos(theta) / wavelength, np.sin(theta) / wavelength
    amp = np.sqrt(wavelength)
    amp *= 110.0 / amp.sum()

    def image(x, y):
        out = np.full(x.shape, 128.0)
        for m in range(terms):
            out += amp[m] * np.sin(2.0 * np.pi * (fx[m] * x + fy[m] * y) + phi[m])
        return out

    ang = np.deg2rad(angle_deg)
    lin = scale * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    centre = np.array([(width - 1) / 2.0, (height - 1) / 2.0])
    A = np.concatenate([lin, (centre - lin @ centre)[:, None]], axis=1)
    d = np.array([float(shift[0]), float(shift[1])])
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    inv = np.linalg.inv(lin)
    qx, qy = x - d[0] - A[0, 2], y - d[1] - A[1, 2]
    f1, f2 = image(x, y), image(inv[0, 0] * qx + inv[0, 1] * qy, inv[1, 0] * qx + inv[1, 1] * qy)
    if quantise:
        return np.rint(f1).astype(np.uint8), np.rint(f2).astype(np.uint8), A, d
    return f1.astype(np.float32), f2.astype(np.float32), A, d


def synth_stereo_pair(seed: int, height: int, width: int, d_background: float = 4.0, d_box: float = 20.0, d_ramp=(6.0, 16.0),
                      noise: float = 2.0, quantise: bool = False):
    """A rectified stereo pair with a known disparity: the left view is per-pixel random texture, and its true disparity is a
    background plane at `d_background`, a foreground box at `d_box` (rows height/5 .. height/2, columns width/3 .. 2 width/3)
    and, in the lowest third of the rows, a ramp from d_ramp[0] at the left border to d_ramp[1] at the right one.  The right
    view is the left one splatted to x_right = rint(x - d) with a depth test (the larger disparity wins a contested pixel);
    pixels that nothing lands on are filled with fresh texture, and uniform noise of +-`noise` gray levels is added to the
    right view.  Returns (left, right, disparity (height, width) float32, visible (height, width) bool: the left pixel
    lands inside the right frame and wins its pixel there); the views are float32 clipped to [0, 255], or rounded to uint8
    with `quantise`.  Deterministic in `seed`."""
    if height < 1 or width < 1 or min(d_background, d_box, d_ramp[0], d_ramp[1]) < 0 or noise < 0:
        raise ValueError("synth_stereo_pair: height, width >= 1, disparities and noise >= 0")
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (height, width)).astype(np.float64)
    y, x = np.mgrid[0:height, 0:width]
    disp = np.full((height, width), float(d_background))
    ramp = y >= height - height // 3
    disp[ramp] = (d_ramp[0] + (d_ramp[1] - d_ramp[0]) * x / max(width - 1, 1))[ramp]
    box = (y >= height // 5) & (y < height // 2) & (x >= width // 3) & (x < 2 * width // 3)
    disp[box] = float(d_box)
    xr = np.rint(x - disp).astype(np.int64)
    inside = (xr >= 0) & (xr < width)
    order = np.argsort(disp[inside], kind="stable")                          # ascending: the nearest surface is written last
    ys, xs, xrs = y[inside][order], x[inside][order], xr[inside][order]
    right = np.full((height, width), np.nan)
    owner = np.full((height, width), -1, np.int64)
    for i in range(len(ys)):                                                 # in order: a repeated target keeps the last writer
        right[ys[i], xrs[i]] = left[ys[i], xs[i]]
        owner[ys[i], xrs[i]] = ys[i] * width + xs[i]
    visible = inside & (owner[y, np.clip(xr, 0, width - 1)] == y * width + x)
    holes = np.isnan(right)
    right[holes] = rng.integers(0, 256, int(holes.sum())).astype(np.float64)
    right = np.clip(right + rng.uniform(-noise, noise, (height, width)), 0.0, 255.0)
    if quantise:
        return left.astype(np.uint8), np.rint(right).astype(np.uint8), disp.astype(np.float32), visible
    return left.astype(np.float32), right.astype(np.float32), disp.astype(np.float32), visible


def synth_distorted_rig(seed: int, height: int, width: int, model: str = "pinhole", disparity: float = 12.0, terms: int = 48,
                        lam=(3.0, 24.0), quantise: bool = False):
    """The raw left and right views of a textured plane as a stereo rig with real lenses sees it: two cameras with lens
    distortion (`model` "pinhole": radial-tangential, or "fisheye": Kannala-Brandt; different coefficients per camera) and a
    small relative rotation.  The plane is fronto-parallel in the RECTIFIED frame of the rig (x along the baseline, z the mean
    optical axis made orthogonal to it), at the depth where the rectified disparity is `disparity` pixels everywhere; its
    texture is a smooth band-limited sum of `terms` sinusoids with wavelengths lam[0] .. lam[1] in rectified pixels.  Each raw
    pixel is rendered exactly, without resampling: its ray comes from the inverse lens model (iterated to convergence in
    float64), meets the plane, and the texture is evaluated there.  Returns (left, right, rig): the views (height, width)
    float32 in [0, 255], or rounded to uint8 with `quantise`, and rig = dict(k1, d1, k2, d2, R, T: X2 = R X1 + T; model;
    disparity; depth: the plane's depth in T's unit; focal: the rectified focal length (fy1 + fy2) / 2; baseline).
    Deterministic in `seed`."""
    if height < 1 or width < 1 or model not in ("pinhole", "fisheye") or not disparity > 0 or terms < 1 or not 0 < lam[0] <= lam[1]:
        raise ValueError("synth_distorted_rig: height, width, terms >= 1, model 'pinhole' or 'fisheye', disparity > 0, 0 < lam[0] <= lam[1]")
    rng = np.random.default_rng(seed)
    wavelength = np.exp(rng.uniform(np.log(lam[0]), np.log(lam[1]), terms))
    theta, phi = rng.uniform(0.0, 2.0 * np.pi, terms), rng.uniform(0.0, 2.0 * np.pi, terms)
    wx, wy = np.cos(theta) / wavelength, np.sin(theta) / wavelength
    amp = np.sqrt(wavelength)
    amp *= 110.0 / amp.sum()

    def texture(x, y):
        out = np.full(x.shape, 128.0)
        for m in range(terms):
            out += amp[m] * np.sin(2.0 * np.pi * (wx[m] * x + wy[m] * y) + phi[m])
        return out

    f1, f2 = 0.9 * width, 0.92 * width
    k1 = np.array([[f1, 0.0, (width - 1) / 2.0 + 1.5], [0.0, f1, (height - 1) / 2.0 - 1.0], [0.0, 0.0, 1.0]])
    k2 = np.array([[f2, 0.0, (width - 1) / 2.0 - 2.0], [0.0, f2, (height - 1) / 2.0 + 0.5], [0.0, 0.0, 1.0]])
    if model == "pinhole":
        d1 = np.array([-0.27, 0.08, 0.0012, -0.0015, -0.01, 0.0, 0.0, 0.0])
        d2 = np.array([-0.22, 0.05, -0.0010, 0.0008, 0.0, 0.0, 0.0, 0.0])
    else:
        d1 = np.array([-0.035, 0.006, -0.001, 0.0, 0.0, 0.0, 0.0, 0.0])
        d2 = np.array([-0.020, 0.003, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    ax, ay, az = 0.02, -0.03, 0.015
    rot = (np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]]) @
           np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]]) @
           np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]]))
    centre2 = np.array([0.1, 0.003, -0.002])                                 # camera 2 in camera 1's frame
    t = -rot @ centre2
    baseline = float(np.linalg.norm(t))
    # the rectified frame (include/mi355x_match_rectify.h, "Stereo rig")
    x_axis = centre2 / baseline
    y_axis = np.cross(np.array([0.0, 0.0, 1.0]) + rot.T @ np.array([0.0, 0.0, 1.0]), x_axis)
    y_axis /= np.linalg.norm(y_axis)
    r1 = np.stack([x_axis, y_axis, np.cross(x_axis, y_axis)])
    r2 = r1 @ rot.T
    focal = (k1[1, 1] + k2[1, 1]) / 2.0
    depth = focal * baseline / disparity

    def rays(k, d):
        """the normalised undistorted coordinates of every raw pixel"""
        v, u = np.mgrid[0:height, 0:width].astype(np.float64)
        xd, yd = (u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1]
        if model == "fisheye":
            thd = np.sqrt(xd * xd + yd * yd)
            th = thd.copy()
            for _ in range(30):
                t2 = th * th
                th = th - (th * (1 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3])))) - thd) / \
                    (1 + t2 * (3 * d[0] + t2 * (5 * d[1] + t2 * (7 * d[2] + t2 * 9 * d[3]))))
            s = np.where(thd > 0, np.tan(th) / np.where(thd > 0, thd, 1.0), 1.0)
            return xd * s, yd * s
        x, y = xd.copy(), yd.copy()
        for _ in range(60):
            r2_ = x * x + y * y
            icd = (1 + r2_ * (d[5] + r2_ * (d[6] + r2_ * d[7]))) / (1 + r2_ * (d[0] + r2_ * (d[1] + r2_ * d[4])))
            a = 2 * x * y
            x, y = (xd - (d[2] * a + d[3] * (r2_ + 2 * x * x))) * icd, (yd - (d[2] * (r2_ + 2 * y * y) + d[3] * a)) * icd
        return x, y

    def view(k, d, r_rect, origin_x):
        x, y = rays(k, d)
        dx, dy, dz = (r_rect[i, 0] * x + r_rect[i, 1] * y + r_rect[i, 2] for i in range(3))
        s = depth / dz
        px, py = origin_x + s * dx, s * dy                                    # the point of the plane, in the rectified frame
        return np.clip(texture(focal * px / depth, focal * py / depth), 0.0, 255.0)

    left, right = view(k1, d1, r1, 0.0), view(k2, d2, r2, baseline)
    rig = dict(k1=k1, d1=d1, k2=k2, d2=d2, R=rot, T=t, model=model, disparity=float(disparity), depth=float(depth), focal=float(focal),
               baseline=baseline)
    if quantise:
        return np.rint(left).astype(np.uint8), np.rint(right).astype(np.uint8), rig
    return left.astype(np.float32), right.astype(np.float32), rig


def synth_textureless_pair(seed: int, height: int = 40, width: int = 160):
    """synth_stereo_pair(seed, height, width) in float32 with a textureless patch painted over the first 8 rows: left[0:8, 70:150]
    and right[0:8, 66:146] (the same surface at the background's disparity 4) are 128 plus uniform noise of +-1 gray level, from
    two draws of numpy.random.default_rng(1000 + seed).  On such a surface the census bits are noise and the matcher accepts
    small blobs of wrong disparities: what the speckle filter (K35) is for.  Returns (left, right, disparity, visible, patch
    (height, width) bool: the patch in the left view).  Needs height >= 8 and width >= 150."""
    if height < 8 or width < 150:
        raise ValueError("synth_textureless_pair: height >= 8 and width >= 150")
    left, right, disp, visible = synth_stereo_pair(seed, height, width)
    rng = np.random.default_rng(1000 + seed)
    left[0:8, 70:150] = (128.0 + rng.uniform(-1.0, 1.0, (8, 80))).astype(np.float32)
    right[0:8, 66:146] = (128.0 + rng.uniform(-1.0, 1.0, (8, 80))).astype(np.float32)
    patch = np.zeros((height, width), bool)
    patch[0:8, 70:150] = True
    return left, right, disp, visible, patch
