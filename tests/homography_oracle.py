"""numpy restatement of the K24 planar two-view algorithm (include/mi355x_match.h, "planar two-view pose"), written from the
header's definitions and textbook formulas: the 4-slot counter-based sampler, the 4-point homography through the projective
bases of the two quadruples, its refusals, the symmetric transfer error with the MSAC cost, selection, the DLT refit (by
numpy's eigh here) and the refit-and-rescore rounds, the decomposition of Ma, Soatto, Kosecka and Sastry with its depth test
and slot order, and the choice between E and H.  Every function takes `dtype`, as pose_oracle.py's do: float64 is the
oracle, float32 the same arithmetic at the kernels' precision -- its deviation from float64 is what the GPU tests take their
tolerances from.  Host only; shared by tests/test_homography_host.py and tests/test_gpu_homography*.py."""
import numpy as np

import pose_oracle as PO

COLLINEAR = 1e-6                 # K17's constant
ROTATION_TOL = 5.9e-6            # HG_ROTATION_TOL (csrc/homography_math.h)
MIN_POSE_ROWS = 4


def sample_ranks(seed, b, h, nv):
    """the 4 distinct ranks (among the valid rows, index order) of hypothesis h of pair b: K15's draws for slots 0 .. 3"""
    return PO.sample_ranks(seed, b, h, nv, 4)


def planted_h(R, t, normal, distance):
    """H = R + t n^T / d of a plane n . X1 = d, float64"""
    return np.asarray(R, np.float64) + np.outer(np.asarray(t, np.float64), np.asarray(normal, np.float64)) / float(distance)


def tri(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def collinear(a, b, c):
    e1, e2 = b - a, c - a
    cz = e1[0] * e2[1] - e1[1] * e2[0]
    return not (cz * cz > a.dtype.type(COLLINEAR) * (e1 * e1).sum() * (e2 * e2).sum())


def adjugate(h):
    """adj(H) negated when det H < 0, at unit Frobenius norm; None when det H = 0 or not finite"""
    g = np.stack([np.cross(h[:, 1], h[:, 2]), np.cross(h[:, 2], h[:, 0]), np.cross(h[:, 0], h[:, 1])]).astype(h.dtype)
    det = h[0] @ g[:, 0]
    nn = (g * g).sum()
    if not (det != 0 and np.isfinite(det) and nn > 0 and np.isfinite(nn)):
        return None
    return (g * (h.dtype.type(-1.0 if det < 0 else 1.0) / np.sqrt(nn))).astype(h.dtype)


def complete(h, sign):
    """(H at unit Frobenius norm times sign, G) as 18 floats; None for a zero, singular or non-finite H"""
    nn = (h * h).sum()
    if not (nn > 0 and np.isfinite(nn)):
        return None
    hn = (h * (h.dtype.type(sign) / np.sqrt(nn))).astype(h.dtype)
    g = adjugate(hn)
    if g is None or not np.isfinite(g).all():
        return None
    return np.concatenate([hn.ravel(), g.ravel()]).astype(h.dtype)


def hartley(p, dtype):
    c = p.sum(axis=0, dtype=dtype) / dtype(len(p))
    d = ((p - c) ** 2).sum(dtype=dtype)
    if not d > 0:
        return None
    return c, dtype(np.sqrt(dtype(2.0))) / np.sqrt(d / dtype(len(p)))


def denormalise(hh, c1, s1, c2, s2, dtype):
    t1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]], dtype)
    t2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]], dtype)
    return (t2i @ (hh @ t1)).astype(dtype)


def solve_minimal(p1, p2, dtype=np.float64):
    """the 18-float model of one 4-sample, or None when it is refused"""
    p1, p2 = np.asarray(p1, dtype), np.asarray(p2, dtype)
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        if collinear(p1[a], p1[b], p1[c]) or collinear(p2[a], p2[b], p2[c]):
            return None
    h1, h2 = hartley(p1, dtype), hartley(p2, dtype)
    if h1 is None or h2 is None:
        return None
    bases = []
    for p, (c, s) in ((p1, h1), (p2, h2)):
        q = ((p - c) * s).astype(dtype)
        lam = np.array([tri(q[3], q[1], q[2]), tri(q[0], q[3], q[2]), tri(q[0], q[1], q[3])], dtype)
        hom = np.concatenate([q[:3], np.ones((3, 1), dtype)], axis=1).T           # columns p0 p1 p2
        bases.append((hom * lam).astype(dtype))
    b1, b2 = bases
    adj = np.stack([np.cross(b1[:, 1], b1[:, 2]), np.cross(b1[:, 2], b1[:, 0]), np.cross(b1[:, 0], b1[:, 1])]).astype(dtype)
    h = denormalise((b2 @ adj).astype(dtype), *h1, *h2, dtype)
    w0 = (h[2, 0] * p1[0, 0] + h[2, 1] * p1[0, 1]) + h[2, 2]
    m = complete(h, -1.0 if w0 < 0 else 1.0)
    if m is None:
        return None
    w = (m[6] * p1[:, 0] + m[7] * p1[:, 1]) + m[8]
    return m if (w > 0).all() else None


def dist2(m, p1, p2):
    """squared symmetric transfer errors under the 18-float model, the header's operation order; +inf where a third
    coordinate is not positive"""
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hx, hy, hw = (m[0] * x1 + m[1] * y1) + m[2], (m[3] * x1 + m[4] * y1) + m[5], (m[6] * x1 + m[7] * y1) + m[8]
        gx, gy, gw = (m[9] * x2 + m[10] * y2) + m[11], (m[12] * x2 + m[13] * y2) + m[14], (m[15] * x2 + m[16] * y2) + m[17]
        ax, ay, bx, by = x2 - hx / hw, y2 - hy / hw, x1 - gx / gw, y1 - gy / gw
        d2 = ((ax * ax + ay * ay) + bx * bx) + by * by
    return np.where((hw > 0) & (gw > 0), d2, np.inf).astype(m.dtype)


def score(m, p1, p2, thr):
    d2 = dist2(m, p1, p2)
    t2 = m.dtype.type(thr) * m.dtype.type(thr)
    with np.errstate(invalid="ignore"):
        return m.dtype.type(np.where(d2 <= t2, d2, t2).sum(dtype=m.dtype)), int((d2 <= t2).sum()), d2


def hypotheses(p1, p2, valid, num_hyp, thr, seed, b=0, dtype=np.float64):
    """one pair: (m_h (H, 18), cost (H,), count (H,), ranks (H, 4)); a refused hypothesis has a zero model, cost +inf"""
    sel = np.arange(len(p1)) if valid is None else np.flatnonzero(valid)
    q1, q2 = p1[sel].astype(dtype), p2[sel].astype(dtype)
    nv = len(sel)
    m_h = np.zeros((num_hyp, 18), dtype)
    cost = np.full(num_hyp, np.inf, dtype)
    count = np.zeros(num_hyp, np.int32)
    ranks = np.zeros((num_hyp, 4), np.int64)
    if nv < 4:
        return m_h, cost, count, ranks
    for h in range(num_hyp):
        ranks[h] = sample_ranks(seed, b, h, nv)
        m = solve_minimal(q1[ranks[h]], q2[ranks[h]], dtype)
        if m is None:
            continue
        c, k, _ = score(m, q1, q2, thr)
        if np.isfinite(c):
            m_h[h], cost[h], count[h] = m, c, k
    return m_h, cost, count, ranks


def refit(p1, p2, mask, dtype=np.float64):
    """(18-float model, ok) from the masked rows: Hartley, two DLT lines per row, the eigenvector of the smallest eigenvalue
    of the normal equations, denormalisation, sign at the first image's centroid, completion"""
    sel = np.flatnonzero(mask)
    zero = np.zeros(18, dtype)
    if len(sel) < 4:
        return zero, False
    q1, q2 = p1[sel].astype(dtype), p2[sel].astype(dtype)
    h1, h2 = hartley(q1, dtype), hartley(q2, dtype)
    if h1 is None or h2 is None:
        return zero, False
    x1, y1 = ((q1 - h1[0]) * h1[1]).T
    x2, y2 = ((q2 - h2[0]) * h2[1]).T
    one, nil = np.ones_like(x1), np.zeros_like(x1)
    a = np.concatenate([np.stack([x1, y1, one, nil, nil, nil, -x2 * x1, -x2 * y1, -x2], axis=1),
                        np.stack([nil, nil, nil, x1, y1, one, -y2 * x1, -y2 * y1, -y2], axis=1)]).astype(dtype)
    _, vec = np.linalg.eigh((a.T @ a).astype(dtype))
    h = denormalise(vec[:, 0].reshape(3, 3).astype(dtype), *h1, *h2, dtype)
    c = h1[0]
    m = complete(h, -1.0 if (h[2, 0] * c[0] + h[2, 1] * c[1]) + h[2, 2] < 0 else 1.0)
    return (zero, False) if m is None else (m, True)


def _cost64(m, q1, q2, thr):
    """the round loop's cost: (rows beyond the threshold) thr^2 + the inliers' sum of d^2, compared in float64"""
    d2 = dist2(m, q1, q2)
    t2 = m.dtype.type(thr) * m.dtype.type(thr)
    inl = d2 <= t2
    return float(len(q1) - inl.sum()) * float(t2) + float(d2[inl].sum(dtype=m.dtype)), int(inl.sum())


def ransac(p1, p2, valid, num_hyp, thr, rounds, seed, b=0, dtype=np.float64):
    """one pair: (H (3, 3), inlier (n,) bool, best_h, count, cost)"""
    n = len(p1)
    vmask = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    m_h, cost, _, _ = hypotheses(p1, p2, valid, num_hyp, thr, seed, b, dtype)
    best_h = int(np.argmin(cost)) if np.isfinite(cost).any() else 0
    if not np.isfinite(cost[best_h]):
        return np.zeros((3, 3), dtype), np.zeros(n, bool), best_h, 0, np.inf
    q1, q2 = p1.astype(dtype), p2.astype(dtype)
    m = m_h[best_h]
    cur, _ = _cost64(m, q1[vmask], q2[vmask], thr)
    for r in range(rounds):
        kr = 1.0 + 0.5 * (rounds - 1 - r)
        m2, ok = refit(p1, p2, vmask & (dist2(m, q1, q2) <= dtype(kr * thr) ** 2), dtype)
        if not ok:
            continue
        c2, _ = _cost64(m2, q1[vmask], q2[vmask], thr)
        if c2 < cur:
            m, cur = m2, c2
    inlier = vmask & (dist2(m, q1, q2) <= dtype(thr) ** 2)
    return m[:9].reshape(3, 3), inlier, best_h, int(inlier.sum()), np.float32(cur)


def _newton(r0, dtype):
    return (0.5 * r0 @ (3 * np.eye(3, dtype=dtype) - r0.T @ r0)).astype(dtype)


def pose(h, p1, p2, mask, dtype=np.float64):
    """(R (4, 3, 3), t (4, 3), normal (4, 3), count (4,), pose_mask (n,), rotation_only, ok, spread = w1 - w3): the header's
    mi_homography_pose"""
    n = len(p1)
    sel = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    fail = (np.tile(np.eye(3, dtype=dtype), (4, 1, 1)), np.zeros((4, 3), dtype), np.zeros((4, 3), dtype), np.zeros(4, np.int32),
            np.zeros(n, bool), False, False, np.nan)
    h = np.asarray(h, dtype)
    fro = (h * h).sum()
    if not (np.isfinite(fro) and fro > 0):
        return fail
    h = (h / np.sqrt(fro)).astype(dtype)
    x1 = np.concatenate([p1.astype(dtype), np.ones((n, 1), dtype)], axis=1)
    x2 = np.concatenate([p2.astype(dtype), np.ones((n, 1), dtype)], axis=1)
    pos = int((((x1 @ h.T) * x2).sum(axis=1)[sel] > 0).sum())
    if 2 * pos < int(sel.sum()):
        h = -h
    w, v = np.linalg.eigh((h.T @ h).astype(dtype))
    w, v = w[::-1].astype(dtype), v[:, ::-1].astype(dtype)             # descending
    for k in range(3):
        if v[np.argmax(np.abs(v[:, k])), k] < 0:
            v[:, k] = -v[:, k]
    if not (w[1] > 0 and np.isfinite(w[0])):
        return fail
    hs = (h / np.sqrt(w[1])).astype(dtype)
    w1, w3 = w[0] / w[1], w[2] / w[1]
    spread = float(w1 - w3)
    v1, v2, v3 = v[:, 0], v[:, 1], v[:, 2]
    R, T, Nn = np.zeros((4, 3, 3), dtype), np.zeros((4, 3), dtype), np.zeros((4, 3), dtype)
    rotation_only = not spread > ROTATION_TOL
    if rotation_only:
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (np.outer(v1, v1) / np.sqrt(w1) + np.outer(v2, v2) + np.outer(v3, v3) / np.sqrt(w3)).astype(dtype)
        R[:] = _newton((hs @ s).astype(dtype), dtype)
        passing = [sel.copy() for _ in range(4)]
    else:
        ca, cb, den = np.sqrt(max(dtype(1) - w3, dtype(0))), np.sqrt(max(w1 - dtype(1), dtype(0))), np.sqrt(w1 - w3)
        for k, sg in enumerate((1.0, -1.0)):
            u = ((ca * v1 + dtype(sg) * cb * v3) / den).astype(dtype)
            nrm = np.cross(v2, u).astype(dtype)
            hv, hu = hs @ v2, hs @ u
            r0 = (np.outer(hv, v2) + np.outer(hu, u) + np.outer(np.cross(hv, hu), nrm)).astype(dtype)
            R[k] = R[k + 2] = _newton(r0, dtype)
            T[k] = (hs - R[k]) @ nrm
            Nn[k], T[k + 2], Nn[k + 2] = nrm, -T[k], -nrm
        passing = []
        for k in range(4):
            d1 = x1 @ Nn[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                z2 = (x1 @ R[k][2]) / d1 + T[k][2]
            passing.append(sel & (d1 > 0) & (z2 > 0))
    if not (np.isfinite(R).all() and np.isfinite(T).all() and np.isfinite(Nn).all()):
        return fail
    cnt = [int(p.sum()) for p in passing]
    order = sorted(range(4), key=lambda k: (-cnt[k], -float(np.trace(R[k])), k))
    if cnt[order[0]] < MIN_POSE_ROWS:
        return fail[:7] + (spread,)
    return (R[order], T[order], Nn[order], np.array([cnt[k] for k in order], np.int32), passing[order[0]], rotation_only, True,
            spread)


def select(e, h, p1, p2, valid, thr_e, thr_h, cut, dtype=np.float64):
    """(score_e, score_h, choice) of mi_two_view_select"""
    sel = np.arange(len(p1)) if valid is None else np.flatnonzero(valid)
    q1, q2 = p1[sel].astype(dtype), p2[sel].astype(dtype)
    e, h = np.asarray(e, dtype), np.asarray(h, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        se = np.maximum(0, 1 - PO.sampson(e, q1, q2) / (dtype(thr_e) * dtype(thr_e))).sum(dtype=dtype)
        g = adjugate(h) if np.isfinite(h).all() else None
        if g is None:
            sh = dtype(0)
        else:
            m = np.concatenate([h.ravel(), g.ravel()]).astype(dtype)
            sh = np.maximum(0, 1 - dist2(m, q1, q2) / (dtype(thr_h) * dtype(thr_h))).sum(dtype=dtype)
    return dtype(se), dtype(sh), bool(sh > dtype(cut) * (se + sh))


def h_distance(h, h0):
    """min(|H - H0|, |H + H0|) after scaling both to unit Frobenius norm, float64"""
    a, b = np.asarray(h, np.float64), np.asarray(h0, np.float64)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


def scenes(seeds, n, outlier_fraction, noise_px, baseline=0.4):
    """synth_planar_two_view scenes as the kernels see them: (p1, p2 (B, n, 2) float32 normalised (x, y), R, t, normal,
    distance (lists), inlier (B, n) bool)"""
    from onnx_image_processing_amd.synth import synth_planar_two_view, two_view_camera
    K = two_view_camera()
    p1, p2, Rs, ts, ns, ds, inl = [], [], [], [], [], [], []
    for s in seeds:
        k1, k2, R, t, nrm, d, m = synth_planar_two_view(s, n, outlier_fraction, noise_px, baseline)
        p1.append(PO.normalise(k1, K).astype(np.float32))
        p2.append(PO.normalise(k2, K).astype(np.float32))
        Rs.append(R), ts.append(t), ns.append(nrm), ds.append(d), inl.append(m)
    return np.stack(p1), np.stack(p2), Rs, ts, ns, ds, np.stack(inl)
