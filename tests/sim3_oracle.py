"""numpy restatement of the K30 similarity alignment (include/mi355x_match_sim3.h), written from the header's definitions:
K17's sampler and Horn rotation (rigid_oracle: the quaternion from numpy.linalg.eigh, where the kernels use Jacobi sweeps),
Umeyama's scale, the range test, the two metrics, the MSAC score, the refit, the RANSAC loop and the float64 `apply`.  Every
function takes `dtype`: float64 is the oracle, float32 the same arithmetic at the kernels' precision -- its deviation from
float64 is what the GPU tests take their tolerances from.  Host only; shared by tests/test_sim3_host.py and
tests/test_gpu_sim3*.py."""
import numpy as np

import rigid_oracle as RO

MIN_SCALE, MAX_SCALE = 1e-3, 1e3
POINT, REPROJ = 0, 1


def _scale_and_t(R, da, db, den, ca, cb, dtype):
    """s = num / den and t = cb - s R ca from the centred rows; None when not finite or out of range"""
    with np.errstate(all="ignore"):
        r = (da @ R.T).astype(dtype)
        num = ((db[:, 0] * r[:, 0] + db[:, 1] * r[:, 1]) + db[:, 2] * r[:, 2]).astype(dtype).sum(dtype=dtype)
        s = dtype(num) / dtype(den)
        t = (cb - s * (R @ ca)).astype(dtype)
    if not (np.isfinite(s) and np.isfinite(t).all() and np.isfinite(R).all()):
        return None
    if not (s >= dtype(np.float32(MIN_SCALE)) and s <= dtype(np.float32(MAX_SCALE))):
        return None
    return dtype(s), t


def solve_minimal(a, b, dtype=np.float64):
    """(s, R, t) from three rows a (3, 3) <-> b (3, 3); None for a refused sample"""
    a, b = a.astype(dtype), b.astype(dtype)
    if RO.degenerate3(a) or RO.degenerate3(b):
        return None
    ca, cb = ((a[0] + a[1]) + a[2]) / dtype(3), ((b[0] + b[1]) + b[2]) / dtype(3)
    da, db = a - ca, b - cb
    m = RO.horn((da.T @ db).astype(dtype), ca, cb, dtype)
    if m is None:
        return None
    R = m[0]
    den = ((da[:, 0] ** 2 + da[:, 1] ** 2) + da[:, 2] ** 2).astype(dtype).sum(dtype=dtype)
    st = _scale_and_t(R, da, db, den, ca, cb, dtype)
    return None if st is None else (st[0], R, st[1])


def dist2(s, R, t, x1, x2, metric):
    """d^2 of every row under the model, in the model's dtype"""
    dt = R.dtype.type
    x1, x2 = x1.astype(R.dtype), x2.astype(R.dtype)
    with np.errstate(all="ignore"):
        y = (dt(s) * (x1 @ R.T) + t).astype(R.dtype)
        if metric == POINT:
            u = y - x2
            return ((u[:, 0] ** 2 + u[:, 1] ** 2) + u[:, 2] ** 2).astype(R.dtype)
        inv_s = dt(1) / dt(s)
        w = (((x2 - t) @ R) * inv_s).astype(R.dtype)
        e2 = (y[:, 0] / y[:, 2] - x2[:, 0] / x2[:, 2]) ** 2 + (y[:, 1] / y[:, 2] - x2[:, 1] / x2[:, 2]) ** 2
        e1 = (w[:, 0] / w[:, 2] - x1[:, 0] / x1[:, 2]) ** 2 + (w[:, 1] / w[:, 2] - x1[:, 1] / x1[:, 2]) ** 2
        d2 = (e1 + e2).astype(R.dtype)
        behind = ~((x1[:, 2] > 0) & (x2[:, 2] > 0) & (y[:, 2] > 0) & (w[:, 2] > 0))
    d2[behind] = np.inf
    return d2


def score(s, R, t, x1, x2, thr, metric):
    """(MSAC cost, count, d2) in the model's dtype; a NaN d^2 counts as beyond the threshold"""
    d2 = dist2(s, R, t, x1, x2, metric)
    t2 = R.dtype.type(thr) * R.dtype.type(thr)
    with np.errstate(invalid="ignore"):
        inl = d2 <= t2
    return R.dtype.type(np.where(inl, d2, t2).sum(dtype=R.dtype)), int(inl.sum()), d2


def pack(s, R, t):
    return np.concatenate([R.ravel(), t, [s]])


def hypotheses(x1, x2, valid, num_hyp, thr, metric, seed, b=0, dtype=np.float64):
    """one pair: (srt_h (H, 13), cost (H,), count (H,), ranks (H, 3)); x1, x2 (n, 3), valid (n,) or None"""
    sel = np.arange(len(x1)) if valid is None else np.flatnonzero(valid)
    q1, q2 = x1[sel].astype(dtype), x2[sel].astype(dtype)
    nv = len(sel)
    srt_h = np.zeros((num_hyp, 13), dtype)
    cost = np.full(num_hyp, np.inf, dtype)
    count = np.zeros(num_hyp, np.int32)
    ranks = np.zeros((num_hyp, 3), np.int64)
    if nv < 3:
        return srt_h, cost, count, ranks
    for h in range(num_hyp):
        ranks[h] = RO.sample_ranks(seed, b, h, nv)
        m = solve_minimal(q1[ranks[h]], q2[ranks[h]], dtype)
        if m is None:
            continue
        c, k, _ = score(*m, q1, q2, thr, metric)
        if np.isfinite(c):
            srt_h[h], cost[h], count[h] = pack(*m), c, k
    return srt_h, cost, count, ranks


def refit(x1, x2, mask, dtype=np.float64):
    """(s, R, t, ok) from the masked rows; 1 / identity / zero / False for < 3 rows, a collinear set or a refused scale"""
    sel = np.flatnonzero(mask)
    ident = (dtype(1), np.eye(3, dtype=dtype), np.zeros(3, dtype), False)
    if len(sel) < 3:
        return ident
    a, b = x1[sel].astype(dtype), x2[sel].astype(dtype)
    ca, cb = a.sum(axis=0, dtype=dtype) / dtype(len(sel)), b.sum(axis=0, dtype=dtype) / dtype(len(sel))
    da, db = a - ca, b - cb
    if not (np.isfinite(da).all() and np.isfinite(db).all()):
        return ident
    Ca = (da.T @ da).astype(dtype)
    if RO.scatter_degenerate(Ca) or RO.scatter_degenerate((db.T @ db).astype(dtype)):
        return ident
    m = RO.horn((da.T @ db).astype(dtype), ca, cb, dtype)
    if m is None:
        return ident
    st = _scale_and_t(m[0], da, db, (Ca[0, 0] + Ca[1, 1]) + Ca[2, 2], ca, cb, dtype)
    return ident if st is None else (st[0], m[0], st[1], True)


def step_cost(s, R, t, q1, q2, thr, metric):
    """the header's cost inside the refinement step: (rows beyond the threshold) thr^2 + the inliers' sum of d^2 (summed in
    the model's dtype), combined in float64"""
    d2 = dist2(s, R, t, q1, q2, metric)
    t2 = R.dtype.type(thr) * R.dtype.type(thr)
    with np.errstate(invalid="ignore"):
        inl = d2 <= t2
    return float(int((~inl).sum())) * float(t2) + float(d2[inl].sum(dtype=R.dtype))


def ransac(x1, x2, valid, num_hyp, thr, metric, rounds, seed, b=0, dtype=np.float64):
    """one pair: (s, R, t, inlier (n,) bool, best_h, count, rmse, ok), the header's float64 step cost"""
    n = len(x1)
    vmask = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    srt_h, cost, _, _ = hypotheses(x1, x2, valid, num_hyp, thr, metric, seed, b, dtype)
    best_h = int(np.argmin(cost)) if np.isfinite(cost).any() else 0
    fail = (dtype(1), np.eye(3, dtype=dtype), np.zeros(3, dtype), np.zeros(n, bool), best_h, 0, dtype(0), False)
    if not np.isfinite(cost[best_h]):
        return fail
    q1, q2 = np.where(vmask[:, None], x1, 0).astype(dtype), np.where(vmask[:, None], x2, 0).astype(dtype)
    R, t, s = srt_h[best_h, :9].reshape(3, 3), srt_h[best_h, 9:12], srt_h[best_h, 12]
    cur = step_cost(s, R, t, q1[vmask], q2[vmask], thr, metric)
    for r in range(rounds):
        kr = 1.0 + 0.5 * (rounds - 1 - r)
        with np.errstate(invalid="ignore"):
            near = dist2(s, R, t, q1, q2, metric) <= dtype(kr * thr) ** 2
        s2, R2, t2, ok = refit(q1, q2, vmask & near, dtype)
        if not ok:
            continue
        c2 = step_cost(s2, R2, t2, q1[vmask], q2[vmask], thr, metric)
        if c2 < cur:
            s, R, t, cur = s2, R2, t2, c2
    d2 = dist2(s, R, t, q1, q2, metric)
    with np.errstate(invalid="ignore"):
        inlier = vmask & (d2 <= dtype(thr) ** 2)
    cnt = int(inlier.sum())
    if cnt < 3:
        return fail
    return s, R, t, inlier, best_h, cnt, dtype(np.sqrt(d2[inlier].mean(dtype=dtype))), True


def apply(s, R, t, Rk=None, tk=None, X=None):
    """mi_sim3_apply for one batch item, the header's float64 operations in its order, rounded to float32 once: (Rk', tk', X');
    float32 inputs"""
    s, R, t = np.float64(np.float32(s)), np.asarray(R, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    r_out = t_out = x_out = None
    if Rk is not None:
        Rk, tk = np.asarray(Rk, np.float32).astype(np.float64), np.asarray(tk, np.float32).astype(np.float64)
        rp = (Rk[:, :, None, 0] * R[None, None, :, 0] + Rk[:, :, None, 1] * R[None, None, :, 1]) + Rk[:, :, None, 2] * R[None, None, :, 2]
        t_out = (s * tk - ((rp[:, :, 0] * t[0] + rp[:, :, 1] * t[1]) + rp[:, :, 2] * t[2])).astype(np.float32)
        r_out = rp.astype(np.float32)
    if X is not None:
        X = np.asarray(X, np.float32).astype(np.float64)
        x_out = (s * ((X[:, None, 0] * R[None, :, 0] + X[:, None, 1] * R[None, :, 1]) + X[:, None, 2] * R[None, :, 2]) + t).astype(np.float32)
    return r_out, t_out, x_out


def rodrigues(w):
    """the rotation matrix of the rotation vector w, float64"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def scale_error(s, s0):
    return abs(float(s) / float(s0) - 1.0)


# ---- the scenes the host and GPU tests share --------------------------------------------------------------------------------
THR_REPROJ = 0.004               # normalised units: 2 px at the 500 px focal length of the synthetic cameras
THR_POINT = 0.05                 # map-2 units at scale 1 (K17's 5 cm)


def maps(seeds, n, outliers, ray_noise, scale):
    """a batch of synth_sim3_maps scenes: x1, x2 (B, n, 3) float32, lists of s, R, t, planted inlier masks (B, n)"""
    from onnx_image_processing_amd.synth import synth_sim3_maps
    sc = [synth_sim3_maps(seed, n, outliers, ray_noise, scale) for seed in seeds]
    return (np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc]), [x[2] for x in sc], [x[3] for x in sc], [x[4] for x in sc],
            np.stack([x[5] for x in sc]))


# ---- two windows that share a frame (the end-to-end scene of the host and GPU tests) --------------------------------------------
E2E_SIGMA = 3.0
E2E_TOL = 2e-3 * E2E_SIGMA        # map-B units: the point metric's threshold and the distance at which two landmarks "agree"


def shared_frame_windows():
    """Frames 0..3 (window A) and 3..5 (window B) of synth_track_window(31, 6, 64, 48, noise_px=0) as two windows of their own
    with the true poses in float32; window B lives in a map of its own, X_B = sigma Q X + c, its poses (R_k Q^T, sigma t_k -
    R_k Q^T c).  -> (A, B) with A = (keypoints, pair_frames, match_ij, match_valid, R, t); the shared frame is A's 3 and B's 0"""
    from onnx_image_processing_amd.synth import synth_track_window
    w = synth_track_window(31, 6, 64, 48, noise_px=0.0)
    kp, _, pf, ij, mv = w[:5]
    Rt, tt = w[7], w[8]
    Q, c = rodrigues(np.array([0.3, -0.5, 0.2])), np.array([1.0, -2.0, 0.5])

    def sub(lo, hi):
        keep = [p for p, (a, b) in enumerate(pf) if lo <= a and b < hi]
        return kp[lo:hi], (pf[keep] - lo).astype(np.int32), ij[keep], mv[keep]
    A = (*sub(0, 4), Rt[:4].astype(np.float32), tt[:4].astype(np.float32))
    RB = Rt[3:] @ Q.T
    B = (*sub(3, 6), RB.astype(np.float32), (E2E_SIGMA * tt[3:] - np.einsum("fij,j->fi", RB, c)).astype(np.float32))
    return A, B


def oracle_tracks(window, K, max_landmarks=64, min_views=2, max_reproj_px=3.0, min_parallax_deg=1.0):
    """LandmarkTracks.forward of one window by tests/tracks_oracle.py: (points (L, 3) float32, point_ok (L,), kp_track (F, K))"""
    import tracks_oracle as TO
    kp, pf, ij, mv, R, t = window
    o = TO.build(kp, pf, ij, mv, None, min_views, max_landmarks)
    focal = float((np.float32(K[0, 0]) + np.float32(K[1, 1])) / 2)
    tri = TO.triangulate(R, t, TO.normalise(o["track_keypoints"], K), o["vis"], min_views, (max_reproj_px / focal) ** 2,
                         np.cos(np.radians(min_parallax_deg)))
    return tri["points"].astype(np.float32), tri["point_ok"], o["kp_track"]


def compose_to_map(s, R, t, R1, t1, R2, t2):
    """(s, R, t) between two keyframes' camera frames (poses R1, t1 in map 1 and R2, t2 in map 2) as the similarity from map 1
    to map 2, float64: X_2 = R2^T (s R (R1 X_1 + t1) + t - t2)"""
    s, R, t, R1, t1, R2, t2 = (np.asarray(x, np.float64) for x in (s, R, t, R1, t1, R2, t2))
    return s, R2.T @ R @ R1, R2.T @ (s * (R @ t1) + t - t2)
