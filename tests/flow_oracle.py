"""numpy oracle of K32 (include/mi355x_match_flow.h): the four entries stated in float64, and with dtype=np.float32 a twin
that follows the header's operation order (tap sums, the bilinear sample, the lanes' sums in index order, then the tree)."""
import numpy as np

OK, PADDING, FLAT, LEFT = 0, 1, 2, 3


def level_shapes(h, w, levels):
    out = []
    for _ in range(levels):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def level_offsets(batch, h, w, levels):
    """float offsets of the levels inside the pyramid block, and the block's bytes"""
    offs, b = [], 0
    for hl, wl in level_shapes(h, w, levels):
        offs.append(b // 4)
        b = (b + batch * hl * wl * 4 + 255) // 256 * 256
    return offs, b


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _tap(a, b, c, d, e, dtype):
    return ((a + e) + dtype(4) * (b + d)) + dtype(6) * c


def pyr_down(src, dtype):
    src = np.asarray(src, dtype)
    h, w = src.shape[-2:]
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    xs = [_reflect(2 * np.arange(w2) - 2 + j, w) for j in range(5)]
    ys = [_reflect(2 * np.arange(h2) - 2 + j, h) for j in range(5)]
    rows = _tap(*[src[..., :, x] for x in xs], dtype)
    return (_tap(*[rows[..., y, :] for y in ys], dtype) * dtype(1.0 / 256.0)).astype(dtype)


def pyramid(gray, levels, dtype=np.float64):
    """list of `levels` arrays of gray's leading shape x (h_l, w_l)"""
    out = [np.asarray(gray).astype(dtype)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1], dtype))
    return out


def sample(f, x, y, dtype):
    """the header's clamped bilinear sample of one (h, w) level at arrays x, y"""
    h, w = f.shape
    with np.errstate(invalid="ignore"):
        x = np.fmin(np.fmax(np.asarray(x, dtype), dtype(0)), dtype(w - 1))
        y = np.fmin(np.fmax(np.asarray(y, dtype), dtype(0)), dtype(h - 1))
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    i1, j1 = np.minimum(i0 + 1, w - 1), np.minimum(j0 + 1, h - 1)
    top = f[j0, i0] + fx * (f[j0, i1] - f[j0, i0])
    bot = f[j1, i0] + fx * (f[j1, i1] - f[j1, i0])
    return top + fy * (bot - top)


def wave_sum(terms, dtype):
    """the header's sum order: lane t adds the pixels t, t + 64, ... in that order, then the neighbour tree"""
    n = terms.shape[0]
    nj = (n + 63) // 64
    p = np.zeros(nj * 64, dtype)
    p[:n] = terms
    p = p.reshape(nj, 64)
    lane = np.zeros(64, dtype)
    for j in range(nj):
        lane = lane + p[j]
    while lane.shape[0] > 1:
        lane = lane[0::2] + lane[1::2]
    return lane[0]


def _inside(x, y, h, w):
    return bool(x >= 0 and x <= w - 1 and y >= 0 and y <= h - 1)


def track_point(pyr1, pyr2, p, guess, radius, max_iterations, epsilon, min_eigen, dtype=np.float64):
    """one keypoint p = (y, x) on the per-image pyramids (lists of (h_l, w_l) arrays of `dtype`) ->
    (kp2 (2,), status, code, residual, iterations, min_eig per level from the top (what was computed of it))"""
    f = dtype
    levels = len(pyr1)
    h0, w0 = pyr1[0].shape
    lost = (-1.0, -1.0), 0
    py, px = f(p[0]), f(p[1])
    eigs = []
    if not (np.isfinite(py) and np.isfinite(px) and _inside(px, py, h0, w0)):
        return np.array(lost[0], f), 0, PADDING, f(0), 0, eigs
    gy0, gx0 = (f(0), f(0)) if guess is None else (f(guess[0]), f(guess[1]))
    if not (np.isfinite(gy0) and np.isfinite(gx0)):
        return np.array(lost[0], f), 0, PADDING, f(0), 0, eigs
    r, side = radius, 2 * radius + 1
    n = side * side
    q = np.arange(n)
    qy, qx = (q // side - r).astype(f), (q % side - r).astype(f)
    top = f(1.0 / (1 << (levels - 1)))
    dx, dy = gx0 * top, gy0 * top
    its, mean_abs = 0, f(0)
    eps2 = f(epsilon) * f(epsilon)
    with np.errstate(all="ignore"):
        for l in range(levels - 1, -1, -1):
            f1, f2 = pyr1[l], pyr2[l]
            h, w = f1.shape
            scale = f(1.0 / (1 << l))
            cx, cy = px * scale, py * scale
            x, y = cx + qx, cy + qy
            t = sample(f1, x, y, f)
            gx = f(0.5) * (sample(f1, cx + (qx + f(1)), y, f) - sample(f1, cx + (qx - f(1)), y, f))
            gy = f(0.5) * (sample(f1, x, cy + (qy + f(1)), f) - sample(f1, x, cy + (qy - f(1)), f))
            gxx, gxy, gyy = wave_sum(gx * gx, f), wave_sum(gx * gy, f), wave_sum(gy * gy, f)
            dif = gxx - gyy
            min_eig = ((gyy + gxx) - np.sqrt(dif * dif + f(4) * (gxy * gxy))) / (f(2) * f(n))
            eigs.append(float(min_eig))
            if not min_eig >= f(min_eigen):
                return np.array(lost[0], f), 0, FLAT, f(0), 0, eigs
            det = gxx * gyy - gxy * gxy
            for _ in range(max_iterations):
                ox, oy = cx + dx, cy + dy
                e = t - sample(f2, ox + qx, oy + qy, f)
                bx, by = wave_sum(e * gx, f), wave_sum(e * gy, f)
                mean_abs = wave_sum(np.abs(e), f) / f(n)
                sx, sy = (gyy * bx - gxy * by) / det, (gxx * by - gxy * bx) / det
                dx, dy = dx + sx, dy + sy
                its += 1
                if sx * sx + sy * sy < eps2:
                    break
            ex, ey = cx + dx, cy + dy
            if not (np.isfinite(ex) and np.isfinite(ey) and _inside(ex, ey, h, w)):
                return np.array(lost[0], f), 0, LEFT, f(0), 0, eigs
            if l > 0:
                dx, dy = f(2) * dx, f(2) * dy
    return np.array([py + dy, px + dx], f), 1, OK, mean_abs, its, eigs


def track(pyr1, pyr2, keypoints1, guess, radius, max_iterations, epsilon, min_eigen, dtype=np.float64):
    """batched: pyr1 / pyr2 are lists of (B, h_l, w_l) arrays, keypoints1 (B, K, 2), guess (B, K, 2) or None ->
    dict(kp2 (B, K, 2), status, code (B, K) uint8, residual (B, K), iterations (B, K) int32, min_eig (B, K) list of lists)"""
    kp = np.asarray(keypoints1)
    B, K = kp.shape[:2]
    p1 = [np.asarray(lv, dtype) for lv in pyr1]
    p2 = [np.asarray(lv, dtype) for lv in pyr2]
    out = dict(kp2=np.zeros((B, K, 2), dtype), status=np.zeros((B, K), np.uint8), code=np.zeros((B, K), np.uint8),
               residual=np.zeros((B, K), dtype), iterations=np.zeros((B, K), np.int32), min_eig=[[None] * K for _ in range(B)])
    for b in range(B):
        l1, l2 = [lv[b] for lv in p1], [lv[b] for lv in p2]
        for i in range(K):
            g = None if guess is None else guess[b, i]
            r = track_point(l1, l2, kp[b, i], g, radius, max_iterations, epsilon, min_eigen, dtype)
            out["kp2"][b, i], out["status"][b, i], out["code"][b, i], out["residual"][b, i], out["iterations"][b, i] = r[:5]
            out["min_eig"][b][i] = r[5]
    return out


def check(keypoints1, keypoints_back, status_fwd, status_bwd, max_distance, dtype=np.float64):
    a, b = np.asarray(keypoints1, dtype), np.asarray(keypoints_back, dtype)
    both = (np.asarray(status_fwd) != 0) & (np.asarray(status_bwd) != 0)
    with np.errstate(all="ignore"):
        dyx = b - a
        dist = np.sqrt(dyx[..., 0] * dyx[..., 0] + dyx[..., 1] * dyx[..., 1])
        status = (both & (dist <= dtype(max_distance))).astype(np.uint8)
    return status, np.where(both, dist, dtype(np.inf)).astype(dtype)


def cell_of(y, x, h, w, cell):
    cells_x = (w + cell - 1) // cell
    with np.errstate(invalid="ignore"):
        x = np.fmin(np.fmax(np.float32(x), np.float32(0)), np.float32(w - 1))
        y = np.fmin(np.fmax(np.float32(y), np.float32(0)), np.float32(h - 1))
    return (int(y) // cell) * cells_x + int(x) // cell


def replenish(keypoints, status, candidates, cand_count, h, w, cell):
    """(B, K, 2), (B, K), (B, C, 2), (B,) -> keypoints_out (B, K, 2) float32, is_new (B, K) uint8, counts (B, 3) int32"""
    kp, st, cand = np.asarray(keypoints, np.float32), np.asarray(status), np.asarray(candidates, np.float32)
    B, K = st.shape
    out = np.full((B, K, 2), -1.0, np.float32)
    is_new = np.zeros((B, K), np.uint8)
    counts = np.zeros((B, 3), np.int32)
    for b in range(B):
        live = st[b] != 0
        out[b, live] = kp[b, live]
        taken = {cell_of(y, x, h, w, cell) for y, x in kp[b, live]}
        accepted = []
        for i in range(min(max(int(cand_count[b]), 0), cand.shape[1])):
            y, x = cand[b, i]
            if not (np.isfinite(y) and np.isfinite(x) and y >= 0 and x >= 0):
                continue
            c = cell_of(y, x, h, w, cell)
            if c not in taken:
                taken.add(c)
                accepted.append(i)
        slots = np.flatnonzero(~live)
        for s, i in zip(slots, accepted):
            out[b, s] = cand[b, i]
            is_new[b, s] = 1
        counts[b] = live.sum(), len(accepted), min(len(accepted), len(slots))
    return out, is_new, counts


# ---- the scenes of the tests (tests/test_flow_host.py, tests/test_gpu_flow.py) -----------------------------------------------------
EPSILON, MAX_ITERATIONS, MIN_EIGEN, POINTS = 0.01, 30, 1e-3, 40
# measured in tests/test_flow_host.py (its docstring): twice the float32 deviation from the float64 oracle; the share of a
# scene's points that may differ from it in status or iteration count
POS_TOL, RES_TOL, CAP = 2.8e-5, 1.5e-5, 0.05
# name: (h, w, levels, radius, shift (dx, dy), angle_deg, scale, lam, quantise)
SCENES = {
    "shift": (83, 97, 3, 7, (6.3, -4.7), 0.0, 1.0, (6.0, 64.0), False),
    "shift_u8": (83, 97, 3, 7, (6.3, -4.7), 0.0, 1.0, (6.0, 64.0), True),
    "rot2": (83, 97, 3, 7, (6.3, -4.7), 2.0, 1.02, (6.0, 64.0), False),
    "rot-3": (83, 97, 3, 7, (-9.6, 7.2), -3.0, 0.98, (6.0, 64.0), False),
    "l1": (83, 97, 1, 7, (2.3, 1.4), 1.0, 1.0, (6.0, 64.0), False),
    "l2r3": (83, 97, 2, 3, (3.4, -2.2), 0.0, 1.0, (6.0, 64.0), False),
    "l1r2": (83, 97, 1, 2, (0.37, -0.81), 0.0, 1.0, (6.0, 64.0), False),
    "big": (161, 193, 3, 10, (11.5, 9.5), 2.0, 1.01, (6.0, 64.0), False),
    "l4r5": (161, 193, 4, 5, (20.5, -13.25), 0.0, 1.0, (24.0, 160.0), False),
    "l4r7": (161, 193, 4, 7, (-17.75, 15.5), 0.0, 1.0, (24.0, 160.0), False),
}
# seed 1: the float64 oracle tracks all 40 points of every scene; under seed 0 three points (one of "shift", two of "l4r5")
# diverge on the top level and leave it (MI_FLOW_LEFT)
SEED = 1
_cache = {}


def scene(name, seed=SEED):
    """dict of a scene: frames f1, f2 (h, w), keypoints kp (POINTS, 2) float32 (y, x), their true positions `truth`
    (POINTS, 2) float64, the shift as a guess (2,) (dy, dx), levels, radius, and the float64 / float32 oracle results
    `o64` / `o32` on pyramids of the frames (computed once, cached, read-only)"""
    key = (name, seed)
    if key in _cache:
        return _cache[key]
    from onnx_image_processing_amd.synth import synth_flow_pair
    h, w, levels, radius, shift, angle, scale, lam, quantise = SCENES[name]
    idx = sorted(SCENES).index(name)
    f1, f2, A, d = synth_flow_pair(1000 + 17 * seed + idx, h, w, angle, scale, shift, lam, 24, quantise)
    rng = np.random.default_rng(77 + 1000 * seed + idx)
    margin = radius + 4 + max(abs(shift[0]), abs(shift[1]))
    kp = np.stack([rng.uniform(margin, h - 1 - margin, POINTS), rng.uniform(margin, w - 1 - margin, POINTS)], axis=1).astype(np.float32)
    xy = kp[:, ::-1].astype(np.float64)
    true_xy = xy @ A[:, :2].T + A[:, 2] + d
    s = dict(name=name, f1=f1, f2=f2, kp=kp, truth=true_xy[:, ::-1].copy(), guess=np.array([shift[1], shift[0]], np.float32),
             levels=levels, radius=radius, h=h, w=w)
    for tag, dt in (("o64", np.float64), ("o32", np.float32)):
        p1, p2 = pyramid(f1[None], levels, dt), pyramid(f2[None], levels, dt)
        s[tag] = track(p1, p2, kp[None], None, radius, MAX_ITERATIONS, EPSILON, MIN_EIGEN, dt)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = s
    return s


def comparable(got_status, got_iterations, o64, b=0):
    """points whose status and total iteration count agree with the float64 oracle's (and that it tracked)"""
    return (np.asarray(got_status) == o64["status"][b]) & (np.asarray(got_iterations) == o64["iterations"][b]) & (o64["status"][b] == 1)


def fb_oracle(f1, f2, kp, levels, radius, threshold, dtype=np.float64):
    """forward, backward and the check on one frame pair -> (forward result, status (K,), fb_distance (K,))"""
    p1, p2 = pyramid(f1[None], levels, dtype), pyramid(f2[None], levels, dtype)
    fw = track(p1, p2, kp[None], None, radius, MAX_ITERATIONS, EPSILON, MIN_EIGEN, dtype)
    bw = track(p2, p1, fw["kp2"].astype(np.float32), None, radius, MAX_ITERATIONS, EPSILON, MIN_EIGEN, dtype)
    st, fb = check(kp[None], bw["kp2"], fw["status"], bw["status"], threshold, dtype)
    return fw, st[0], fb[0]


BLOCK = (30, 52, 36, 62)                      # y0, y1, x0, x1 of the block of frame 2 that shows another scene


def block_scene():
    """the "l2r3" scene (two levels, radius 3: a window reaches 12 pixels) with BLOCK of frame 2 overwritten by a different
    scene -> (f1, f2, keypoints (K, 2) float32, inside (K,) bool): 9 keypoints whose true position lies at least 5 pixels
    inside the block, then the scene's keypoints whose true position is at least 13 pixels away from it"""
    if "block" in _cache:
        return _cache["block"]
    from onnx_image_processing_amd.synth import synth_flow_pair
    s = scene("l2r3")
    y0, y1, x0, x1 = BLOCK
    other = synth_flow_pair(4242, s["h"], s["w"])[0]
    f2 = s["f2"].copy()
    f2[y0:y1, x0:x1] = other[y0:y1, x0:x1]
    gy, gx = np.meshgrid(np.linspace(y0 + 5.5, y1 - 6.5, 3), np.linspace(x0 + 5.5, x1 - 6.5, 3), indexing="ij")
    inside = np.stack([gy.ravel(), gx.ravel()], axis=1) - s["guess"]
    t = s["truth"]
    far = (t[:, 0] < y0 - 14) | (t[:, 0] > y1 + 13) | (t[:, 1] < x0 - 14) | (t[:, 1] > x1 + 13)
    kp = np.concatenate([inside, s["kp"][far]]).astype(np.float32)
    _cache["block"] = s["f1"], f2, kp, np.arange(len(kp)) < 9
    return _cache["block"]


# keypoints and guesses that are not finite, huge, padding, on the four borders and the corners, and one ordinary point
HOSTILE = np.array([[np.nan, 10.0], [10.0, np.nan], [np.inf, 10.0], [10.0, -np.inf], [1e30, 10.0], [10.0, -1e30], [-1.0, -1.0],
                    [0.0, 40.0], [82.0, 40.0], [40.0, 0.0], [40.0, 96.0], [0.0, 0.0], [82.0, 96.0], [41.3, 47.9]], np.float32)
HOSTILE_GUESS = np.array([[0.0, 0.0]] * 7 + [[np.nan, 0.0], [0.0, np.inf], [-np.inf, 0.0], [1e30, 1e30], [-1e30, 0.0], [0.0, 1e30], [-4.7, 6.3]],
                         np.float32)

# the bit and shape cases: radius 1 (9 window pixels in a 64-lane wave, five levels down to the 6 x 7 the level rule admits) and
# the radii whose lane-pixel counts no scene reaches (6, 8, 9: 3, 5, 6 pixels per lane), 70 keypoints over two workgroups.
# Accuracy is not asked of them (at r = 1 the normal matrix of 9 pixels is often poor): only the float32 oracle's bits.
BIT_CASES = {1: 5, 6: 2, 8: 2, 9: 2}          # radius: levels


def bit_case(radius):
    """(f1, f2, keypoints (70, 2) float32, levels, the float32 oracle's result) on the "shift" frames"""
    key = ("bit", radius)
    if key not in _cache:
        s, levels = scene("shift"), BIT_CASES[radius]
        rng = np.random.default_rng(100 + radius)
        kp = np.stack([rng.uniform(6, s["h"] - 7, 70), rng.uniform(6, s["w"] - 7, 70)], axis=1).astype(np.float32)
        o32 = track(pyramid(s["f1"][None], levels, np.float32), pyramid(s["f2"][None], levels, np.float32), kp[None], None, radius,
                    MAX_ITERATIONS, EPSILON, MIN_EIGEN, np.float32)
        _cache[key] = s["f1"], s["f2"], kp, levels, o32
    return _cache[key]
