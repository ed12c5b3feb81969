"""numpy oracle of K28 (include/mi355x_match.h) for ONE window: a serial union-find over the active matches, then the
header's definitions word for word (label = smallest node, conflict, eligibility, the order by (length descending, label
ascending), the cut at L), and the N-view triangulation in float64 in the header's stated operation order."""
import numpy as np

F32, F64 = np.float32, np.float64
PIVOT_RATIO = 1e-6


def active_edges(pair_frames, match_ij, match_valid, kp_valid, F, K):
    """[(u, v)] node pairs of the ACTIVE matches, in list order"""
    out = []
    P, M = match_valid.shape
    for p in range(P):
        a, b = int(pair_frames[p, 0]), int(pair_frames[p, 1])
        for m in range(M):
            if not match_valid[p, m]:
                continue
            if not (0 <= a < F and 0 <= b < F and a != b):
                continue
            i, j = int(match_ij[p, m, 0]), int(match_ij[p, m, 1])
            if not (0 <= i < K and 0 <= j < K):
                continue
            if kp_valid is not None and not (kp_valid[a, i] and kp_valid[b, j]):
                continue
            out.append((a * K + i, b * K + j))
    return out


def components(n, edges):
    """label (n,): the smallest node of every node's component; serial union-find with path halving"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in edges:
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(x) for x in range(n)], np.int64)


def build(keypoints, pair_frames, match_ij, match_valid, kp_valid, min_views, L):
    """dict(track_kp (F, L) int32, vis (F, L) bool, track_keypoints (F, L, 2) float32, track_len (L,) int32, kp_track (F, K) int32,
    counts (4,) int32) and, for the tests, `eligible`: [(label, [nodes])] in slot order before the cut"""
    F, K = keypoints.shape[:2]
    N = F * K
    label = components(N, active_edges(pair_frames, match_ij, match_valid, kp_valid, F, K))
    members = {}
    for n in range(N):
        members.setdefault(int(label[n]), []).append(n)
    kp_track = np.full(N, -1, np.int32)
    big = conflicting = 0
    eligible = []
    for lab, nodes in members.items():
        if len(nodes) < 2:
            continue
        big += 1
        frames = [n // K for n in nodes]
        if len(set(frames)) < len(frames):
            conflicting += 1
            kp_track[nodes] = -2
        elif len(nodes) >= min_views:
            eligible.append((lab, nodes))
    eligible.sort(key=lambda e: (-len(e[1]), e[0]))
    track_kp = np.full((F, L), -1, np.int32)
    vis = np.zeros((F, L), bool)
    track_keypoints = np.zeros((F, L, 2), F32)
    track_len = np.zeros(L, np.int32)
    for slot, (lab, nodes) in enumerate(eligible[:L]):
        track_len[slot] = len(nodes)
        for n in nodes:
            f, k = divmod(n, K)
            track_kp[f, slot] = k
            vis[f, slot] = True
            track_keypoints[f, slot] = keypoints[f, k]
            kp_track[n] = slot
    counts = np.array([big, conflicting, len(eligible), min(len(eligible), L)], np.int32)
    return dict(track_kp=track_kp, vis=vis, track_keypoints=track_keypoints, track_len=track_len, kp_track=kp_track.reshape(F, K),
                counts=counts, eligible=eligible)


def _ray(R, x, y):
    n = np.sqrt((x * x + y * y) + 1.0)
    return np.stack([((R[0, k] * x + R[1, k] * y) + R[2, k]) / n for k in range(3)], -1)


def triangulate(R, t, obs, vis, min_views, max_e2, max_cos):
    """R (F, 3, 3), t (F, 3), obs (F, L, 2) normalised (x, y), vis (F, L) -> dict(points (L, 3) float64, usable, front, point_ok
    (L,) bool, vis_out (F, L) bool, e2max, cos_par (L,) float64, seen (L,) int).  Vectorised over the landmarks, every
    landmark's operations in the header's order; the float32 inputs are widened exactly and the thresholds are the float32
    values the entry receives."""
    R, t, obs = (np.asarray(a, F32).astype(F64) for a in (R, t, obs))
    vis = np.asarray(vis) != 0
    F, L = vis.shape
    max_e2, max_cos = F64(F32(max_e2)), F64(F32(max_cos))
    A = np.zeros((L, 6))
    b = np.zeros((L, 3))
    rays = np.zeros((F, L, 3))
    with np.errstate(all="ignore"):
        for f in range(F):
            x, y = np.where(vis[f], obs[f, :, 0], 0.0), np.where(vis[f], obs[f, :, 1], 0.0)
            d = _ray(R[f], x, y)
            rays[f] = d
            c = [-((R[f, 0, k] * t[f, 0] + R[f, 1, k] * t[f, 1]) + R[f, 2, k] * t[f, 2]) for k in range(3)]
            Pm = np.stack([1.0 - d[:, 0] * d[:, 0], 0.0 - d[:, 0] * d[:, 1], 0.0 - d[:, 0] * d[:, 2], 1.0 - d[:, 1] * d[:, 1],
                           0.0 - d[:, 1] * d[:, 2], 1.0 - d[:, 2] * d[:, 2]], -1)
            s = vis[f]
            A[s] = A[s] + Pm[s]
            add = np.stack([(Pm[:, 0] * c[0] + Pm[:, 1] * c[1]) + Pm[:, 2] * c[2], (Pm[:, 1] * c[0] + Pm[:, 3] * c[1]) + Pm[:, 4] * c[2],
                            (Pm[:, 2] * c[0] + Pm[:, 4] * c[1]) + Pm[:, 5] * c[2]], -1)
            b[s] = b[s] + add[s]
        a00, a01, a02, a11, a12, a22 = (A[:, k] for k in range(6))
        C = [a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11, a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01]
        det = (a00 * C[0] + a01 * C[1]) + a02 * C[2]
        p1, p2 = C[5] / a00, det / C[5]
        dmax = np.maximum(np.maximum(a00, a11), a22)
        thr = PIVOT_RATIO * dmax
        usable = (dmax > 0) & (a00 > thr) & (p1 > thr) & (p2 > thr)
        X = np.stack([((C[0] * b[:, 0] + C[1] * b[:, 1]) + C[2] * b[:, 2]) / det, ((C[1] * b[:, 0] + C[3] * b[:, 1]) + C[4] * b[:, 2]) / det,
                      ((C[2] * b[:, 0] + C[4] * b[:, 1]) + C[5] * b[:, 2]) / det], -1)
        usable &= (np.abs(X) < np.inf).all(-1)
        X = np.where(usable[:, None], X, 0.0)
        front = np.ones(L, bool)
        e2max = np.where(usable, 0.0, np.inf)
        for f in range(F):
            q = [((R[f, i, 0] * X[:, 0] + R[f, i, 1] * X[:, 1]) + R[f, i, 2] * X[:, 2]) + t[f, i] for i in range(3)]
            s = vis[f] & usable
            ahead = q[2] > 0
            u, v = q[0] / q[2] - obs[f, :, 0], q[1] / q[2] - obs[f, :, 1]
            e2 = u * u + v * v
            e2 = np.where(e2 < np.inf, e2, np.inf)
            e2max = np.where(s & ahead, np.maximum(e2max, e2), e2max)
            e2max = np.where(s & ~ahead, np.inf, e2max)
            front &= ~(s & ~ahead)
        cos_par = np.ones(L)
        for fa in range(F):
            for fb in range(fa + 1, F):
                cs = (rays[fa, :, 0] * rays[fb, :, 0] + rays[fa, :, 1] * rays[fb, :, 1]) + rays[fa, :, 2] * rays[fb, :, 2]
                both = vis[fa] & vis[fb]
                cos_par = np.where(both & (cs < cos_par), cs, cos_par)
    seen = vis.sum(0)
    ok = (seen >= min_views) & usable & front & (e2max <= max_e2) & (cos_par <= max_cos)
    return dict(points=X, usable=usable, front=front, point_ok=ok, vis_out=vis & ok[None, :], e2max=e2max, cos_par=cos_par, seen=seen)


def normalise(keypoints_yx, K):
    """pixel (y, x) -> normalised (x, y) in float32, mi_normalise_keypoints' arithmetic"""
    ki = np.linalg.inv(K).astype(F32)
    x, y = keypoints_yx[..., 1].astype(F32), keypoints_yx[..., 0].astype(F32)
    return np.stack([(x * ki[0, 0] + y * ki[0, 1]) + ki[0, 2], (x * ki[1, 0] + y * ki[1, 1]) + ki[1, 2]], -1).astype(F32)
