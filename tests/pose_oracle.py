"""numpy restatement of the K15 relative-pose algorithm (include/mi355x_match.h, "relative pose"), written from the header's
definitions and textbook formulas: the counter-based sampler, the Hartley-normalised 8-point solve by Gauss-Jordan
elimination with complete pivoting, the projection onto the essential manifold (by SVD here), Sampson scoring with the MSAC
cost, selection, refit-and-rescore rounds, pose recovery and two-view DLT.  Every function takes `dtype`: float64 is the
oracle, float32 the same arithmetic at the kernels' precision -- its deviation from float64 is what the GPU tests take their
tolerances from.  Host only; shared by tests/test_pose_host.py and tests/test_gpu_pose*.py."""
import numpy as np

RANK_TOL = 1e-5
M32 = 0xFFFFFFFF


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draw(seed, b, h, s):
    return mix((mix((mix((seed + 0x9E3779B9) & M32) + b) & M32) + (8 * h + s)) & M32)


def sample_ranks(seed, b, h, nv, k=8):
    """the k distinct ranks (among the valid rows, index order) of hypothesis h of pair b; draw index 8 * h + s for every k"""
    taken, out = [], []
    for s in range(k):
        r = draw(seed, b, h, s) % (nv - s)
        for q in sorted(taken):
            if r >= q:
                r += 1
        taken.append(r)
        out.append(r)
    return out


def sample_ranks_batch(seed, batch, num_hyp, nv, k=8):
    """sample_ranks for every (b, h) at once: (batch, num_hyp, k) int64"""
    def mixv(x):
        x = x & M32
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M32
        x ^= x >> 16
        return x
    b = np.arange(batch, dtype=np.uint64)[:, None]
    h = np.arange(num_hyp, dtype=np.uint64)[None, :]
    base = mixv(np.uint64(mix((seed + 0x9E3779B9) & M32)) + b)
    out = np.zeros((batch, num_hyp, k), np.int64)
    for s in range(k):
        r = (mixv(base + (np.uint64(8) * h + np.uint64(s))) % np.uint64(nv - s)).astype(np.int64)
        taken = np.sort(out[..., :s], axis=-1)
        for j in range(s):
            r = r + (r >= taken[..., j])
        out[..., s] = r
    return out


def normalise(kp_yx, K):
    """pixel (y, x) keypoints -> normalised (x, y), float64"""
    kp = np.asarray(kp_yx, np.float64)
    ki = np.linalg.inv(np.asarray(K, np.float64))
    hom = np.stack([kp[..., 1], kp[..., 0], np.ones(kp.shape[:-1])], axis=-1)
    return (hom @ ki.T)[..., :2]


def essential_from_pose(R, t):
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return tx @ np.asarray(R, np.float64)


def hartley(p, dtype):
    c = p.mean(axis=0, dtype=dtype)
    d = ((p - c) ** 2).sum(axis=1).mean(dtype=dtype)
    if not d > 0:
        return None
    return c, dtype(np.sqrt(dtype(2.0))) / np.sqrt(d)


def design_rows(p1, c1, s1, p2, c2, s2, dtype):
    x1, y1 = ((p1 - c1) * s1).T
    x2, y2 = ((p2 - c2) * s2).T
    return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=1).astype(dtype)


def null_vector_gj(a):
    """null vector of the 8x9 system by Gauss-Jordan with complete pivoting (first maximum in (row, column) order); None
    when a pivot is not above RANK_TOL times the first"""
    a = a.copy()
    cols = list(range(9))
    first = None
    for k in range(8):
        sub = np.abs(a[k:, cols[k:]])
        flat = int(np.argmax(sub))                    # first maximum in row-major order
        br, bc = k + flat // sub.shape[1], k + flat % sub.shape[1]
        best = sub.flat[flat]
        if k == 0:
            first = best
        if not best > a.dtype.type(RANK_TOL) * first:
            return None
        a[[k, br]] = a[[br, k]]
        cols[k], cols[bc] = cols[bc], cols[k]
        pk = cols[k]
        rest = cols[k + 1:]
        a[k, rest] = a[k, rest] / a[k, pk]
        for r in range(8):
            if r != k:
                a[r, rest] = a[r, rest] - a[r, pk] * a[k, rest]
    v = np.zeros(9, a.dtype)
    v[cols[8]] = 1
    for k in range(8):
        v[cols[k]] = -a[k, cols[8]]
    return v / np.sqrt((v * v).sum())


def project_manifold(e):
    u, s, vt = np.linalg.svd(e)
    m = (s[0] + s[1]) / 2
    return (u * np.array([m, m, 0], e.dtype)) @ vt


def finish(v, c1, s1, c2, s2, dtype):
    t1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]], dtype)
    t2 = np.array([[s2, 0, -s2 * c2[0]], [0, s2, -s2 * c2[1]], [0, 0, 1]], dtype)
    e = project_manifold((t2.T @ v.reshape(3, 3) @ t1).astype(dtype))
    return e if np.isfinite(e).all() and np.abs(e).sum() > 0 else None


def solve_minimal(p1, p2, dtype=np.float64):
    p1, p2 = p1.astype(dtype), p2.astype(dtype)
    h1, h2 = hartley(p1, dtype), hartley(p2, dtype)
    if h1 is None or h2 is None:
        return None
    v = null_vector_gj(design_rows(p1, *h1, p2, *h2, dtype))
    return None if v is None else finish(v, *h1, *h2, dtype)


def sampson(e, p1, p2):
    """squared Sampson distances, the header's operation order; +inf where the denominator is 0"""
    e = e.ravel()
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    ex0, ex1, ex2 = (e[0] * x1 + e[1] * y1) + e[2], (e[3] * x1 + e[4] * y1) + e[5], (e[6] * x1 + e[7] * y1) + e[8]
    et0, et1 = (e[0] * x2 + e[3] * y2) + e[6], (e[1] * x2 + e[4] * y2) + e[7]
    r = (x2 * ex0 + y2 * ex1) + ex2
    den = ((ex0 * ex0 + ex1 * ex1) + et0 * et0) + et1 * et1
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (r * r) / den, np.inf).astype(e.dtype)


def score(e, p1, p2, thr):
    d2 = sampson(e, p1, p2)
    t2 = e.dtype.type(thr) * e.dtype.type(thr)
    return e.dtype.type(np.minimum(d2, t2).sum(dtype=e.dtype)), int((d2 <= t2).sum()), d2


def hypotheses(p1, p2, valid, num_hyp, thr, seed, b=0, dtype=np.float64):
    """one pair: (e_h (H, 3, 3), cost (H,), count (H,), ranks (H, 8)); p1, p2 (n, 2) normalised (x, y), valid (n,) or None"""
    sel = np.arange(len(p1)) if valid is None else np.flatnonzero(valid)
    q1, q2 = p1[sel].astype(dtype), p2[sel].astype(dtype)
    nv = len(sel)
    e_h = np.zeros((num_hyp, 3, 3), dtype)
    cost = np.full(num_hyp, np.inf, dtype)
    count = np.zeros(num_hyp, np.int32)
    ranks = np.zeros((num_hyp, 8), np.int64)
    if nv < 8:
        return e_h, cost, count, ranks
    for h in range(num_hyp):
        ranks[h] = sample_ranks(seed, b, h, nv)
        e = solve_minimal(q1[ranks[h]], q2[ranks[h]], dtype)
        if e is None:
            continue
        c, k, _ = score(e, q1, q2, thr)
        if np.isfinite(c):
            e_h[h], cost[h], count[h] = e, c, k
    return e_h, cost, count, ranks


def refit(p1, p2, mask, dtype=np.float64):
    """(E, ok) from the masked rows: normal equations, eigenvector of the smallest eigenvalue, denormalise, project"""
    sel = np.flatnonzero(mask)
    if len(sel) < 8:
        return np.zeros((3, 3), dtype), False
    q1, q2 = p1[sel].astype(dtype), p2[sel].astype(dtype)
    h1, h2 = hartley(q1, dtype), hartley(q2, dtype)
    if h1 is None or h2 is None:
        return np.zeros((3, 3), dtype), False
    a = design_rows(q1, *h1, q2, *h2, dtype)
    w, vec = np.linalg.eigh((a.T @ a).astype(dtype))
    e = finish(vec[:, 0].astype(dtype), *h1, *h2, dtype)
    return (np.zeros((3, 3), dtype), False) if e is None else (e, True)


def ransac(p1, p2, valid, num_hyp, thr, rounds, seed, b=0, dtype=np.float64):
    """one pair: (E, inlier (n,) bool, best_h, count)"""
    n = len(p1)
    vmask = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    e_h, cost, _, _ = hypotheses(p1, p2, valid, num_hyp, thr, seed, b, dtype)
    best_h = int(np.argmin(cost)) if np.isfinite(cost).any() else 0
    inlier = np.zeros(n, bool)
    if not np.isfinite(cost[best_h]):
        return np.zeros((3, 3), dtype), inlier, best_h, 0
    q1, q2 = p1.astype(dtype), p2.astype(dtype)
    e, cur = e_h[best_h], cost[best_h]
    for r in range(rounds):
        kr = 1.0 + 0.5 * (rounds - 1 - r)
        d2 = sampson(e, q1, q2)
        e2, ok = refit(p1, p2, vmask & (d2 <= dtype(kr * thr) ** 2), dtype)
        if not ok:
            continue
        c2 = score(e2, q1[vmask], q2[vmask], thr)[0]
        if c2 < cur:
            e, cur = e2, c2
    inlier = vmask & (sampson(e, q1, q2) <= dtype(thr) ** 2)
    return e, inlier, best_h, int(inlier.sum())


def recover_pose(e, p1, p2, mask, dist=50.0, dtype=np.float64):
    """(R, t, pose_mask, count, ok, candidate): the header's construction -- t from the largest cross product of E's columns,
    Ra / Rb = cof(E) -/+ [t]x E (one Newton step towards a rotation each), candidates (Ra,t) (Rb,t) (Ra,-t) (Rb,-t)"""
    n = len(p1)
    sel = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    e = np.asarray(e, dtype)
    fro = (e * e).sum()
    ident = (np.eye(3, dtype=dtype), np.zeros(3, dtype), np.zeros(n, bool), 0, False, 0)
    if not (np.isfinite(fro) and fro > 0):
        return ident
    e = e * (np.sqrt(dtype(2.0)) / np.sqrt(fro))
    cr = [np.cross(e[:, 0], e[:, 1]), np.cross(e[:, 0], e[:, 2]), np.cross(e[:, 1], e[:, 2])]
    k = int(np.argmax([(c * c).sum() for c in cr]))
    t = cr[k] / np.sqrt((cr[k] * cr[k]).sum())
    cof = np.stack([np.cross(e[1], e[2]), np.cross(e[2], e[0]), np.cross(e[0], e[1])])
    te = np.cross(t, e.T).T                                       # [t]x E, column by column
    rots = []
    for r0 in (cof - te, cof + te):
        rots.append((0.5 * r0 @ (3 * np.eye(3, dtype=dtype) - r0.T @ r0)).astype(dtype))
    x1 = np.concatenate([p1.astype(dtype), np.ones((n, 1), dtype)], axis=1)
    x2 = np.concatenate([p2.astype(dtype), np.ones((n, 1), dtype)], axis=1)
    best = (-1, 0, None)
    for cand in range(4):
        rm, tk = rots[cand & 1], (t if cand < 2 else -t)
        rx = x1 @ rm.T
        a, c = np.cross(x2, rx), np.cross(x2, tk)
        den = (a * a).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            z1 = -(a * c).sum(axis=1) / den
        z2 = z1 * rx[:, 2] + tk[2]
        passing = sel & (den > 0) & (z1 > 0) & (z2 > 0) & (z1 < dist) & (z2 < dist)
        if int(passing.sum()) > best[0]:
            best = (int(passing.sum()), cand, passing)
    cnt, cand, passing = best
    if cnt < 5:
        return np.eye(3, dtype=dtype), np.zeros(3, dtype), passing, cnt, False, cand
    return rots[cand & 1], (t if cand < 2 else -t), passing, cnt, True, cand


def triangulate(proj1, proj2, x1, x2, dtype=np.float64):
    """(points (n, 3), finite (n,)): per point the unit right singular vector of the smallest singular value of the four
    unit-norm DLT rows; X[:3] / X[3] where |X[3]| > 1e-9 and the system has rank 3, else zeros"""
    p1, p2 = np.asarray(proj1, dtype), np.asarray(proj2, dtype)
    out = np.zeros((len(x1), 3), dtype)
    fin = np.zeros(len(x1), bool)
    for i, (a, b) in enumerate(zip(np.asarray(x1, dtype), np.asarray(x2, dtype))):
        m = np.stack([a[0] * p1[2] - p1[0], a[1] * p1[2] - p1[1], b[0] * p2[2] - p2[0], b[1] * p2[2] - p2[1]])
        m = m / np.sqrt((m * m).sum(axis=1, keepdims=True))
        _, sv, vt = np.linalg.svd(m)
        x = vt[-1]
        if sv[2] > 1e-5 * sv[0] and abs(x[3]) > 1e-9:                      # rank < 3: no unique solution
            out[i], fin[i] = x[:3] / x[3], True
    return out, fin


def rotation_angle_deg(ra, rb):
    """angle of ra^T rb in degrees, from the chord |ra - rb|_F = 2 sqrt(2) sin(angle / 2) (accurate near zero)"""
    d = np.linalg.norm(np.asarray(ra, np.float64) - np.asarray(rb, np.float64))
    return float(np.degrees(2 * np.arcsin(min(1.0, d / (2 * np.sqrt(2))))))


def direction_angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def e_distance(e, e0):
    """min(|E - E0|, |E + E0|) after scaling both to Frobenius norm sqrt(2)"""
    a = np.asarray(e, np.float64)
    b = np.asarray(e0, np.float64)
    a, b = a * np.sqrt(2) / np.linalg.norm(a), b * np.sqrt(2) / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))
