"""The numpy oracle of K29 (include/mi355x_match.h), written from the header's words: `descriptors` and `match` are
loops over landmarks and keypoints in Python floats (IEEE float64, the header's operation order); `match_vectorised` is the same
definition as whole-array numpy operations.  tests/test_localmap_host.py holds the two against each other, `descriptors` against
a brute force over sorted lists, and the host-compiled csrc/localmap_math.h against both.

`match` also marks a landmark as EXCUSED when one of its gates is decided by less than 1e-9 relative: z against the depth limits,
u and v against the image border, radius^2 against a valid keypoint's squared distance.  No generated scene of any test may hold
one (asserted on the CPU); the hand-made boundary cases use exactly representable numbers and are exempt."""
import numpy as np

F32, F64 = np.float32, np.float64
NEAR = 1e-9


def absent(num_bits):
    return num_bits + 1


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def hamming(a, b):
    """popcount(a xor b) over the last axis of two uint32 word arrays"""
    x = np.bitwise_xor(np.asarray(a, np.uint32), np.asarray(b, np.uint32))
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).sum(-1).astype(np.int64)


def hamming_matrix(a, b):
    """(L, W) against (K, W) -> (L, K) distances, by one matrix product on the unpacked bits"""
    ua, ub = (np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).astype(np.float32) for x in (a, b))
    return (ua.sum(1)[:, None] + ub.sum(1)[None] - 2.0 * (ua @ ub.T)).astype(np.int64)


def _near(a, b):
    return abs(a - b) <= NEAR * max(abs(a), abs(b), 1.0)


def _near_v(a, b):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) <= NEAR * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)


# ---- mi_localmap_descriptors --------------------------------------------------------------------------------------------------------
def descriptors(bits, track_kp, num_bits):
    """bits (F, K, W), track_kp (F, L) -> dict(rep_bits (L, W) uint32, rep_frame (L,), rep_median (L,) int32)"""
    bits = words(bits)
    F, K, W = bits.shape
    L = track_kp.shape[1]
    rep_bits = np.zeros((L, W), np.uint32)
    rep_frame = np.full(L, -1, np.int32)
    rep_median = np.full(L, absent(num_bits), np.int32)
    for l in range(L):
        views = [f for f in range(F) if 0 <= track_kp[f, l] < K]
        best = None
        for a in views:
            da = bits[a, track_kp[a, l]]
            dist = sorted(int(hamming(da, bits[b, track_kp[b, l]])) for b in views)
            key = dist[(len(views) - 1) // 2] << 8 | a
            if best is None or key < best:
                best = key
        if best is not None:
            rep_frame[l], rep_median[l] = best & 0xFF, best >> 8
            rep_bits[l] = bits[best & 0xFF, track_kp[best & 0xFF, l]]
    return dict(rep_bits=rep_bits, rep_frame=rep_frame, rep_median=rep_median)


# ---- mi_localmap_match --------------------------------------------------------------------------------------------------------------
def project(X, R, t, cam):
    """one landmark, Python floats: (q, u, v) in the header's order"""
    X, R, t, cam = ([float(v) for v in np.asarray(a, F32).ravel()] for a in (X, R, t, cam))
    q = [((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i] for i in range(3)]
    with np.errstate(all="ignore"):
        z = F64(q[2])
        u = float(F64(cam[0]) * (F64(q[0]) / z) + F64(cam[2]))
        v = float(F64(cam[1]) * (F64(q[1]) / z) + F64(cam[3]))
    return q, u, v


def match(points, point_valid, rep_bits, R, t, cam, kp, kp_valid, kp_bits, num_bits, height, width, min_depth, max_depth, radius,
          max_distance, ratio):
    """one batch item -> dict of the seven outputs, plus d2 (L,), in_window (L,) counts and excused (L,) bool"""
    points, kp = np.asarray(points, F32), np.asarray(kp, F32)
    rep_bits, kp_bits = words(rep_bits), words(kp_bits)
    L, K = len(points), len(kp)
    A = absent(num_bits)
    lo, hi, rad, rat = float(F32(min_depth)), float(F32(max_depth)), float(F32(radius)), F32(ratio)
    r2 = rad * rad
    proj = np.full((L, 2), -1, F32)
    state = np.zeros(L, np.uint8)
    d1s, d2s, j1s = np.full(L, A, np.int32), np.full(L, A, np.int32), np.full(L, -1, np.int32)
    in_window = np.zeros(L, np.int32)
    excused = np.zeros(L, bool)
    claim = {}
    for l in range(L):
        q, u, v = project(points[l], R, t, cam)
        ok = bool(point_valid is None or point_valid[l]) and all(np.isfinite(q))
        if ok:
            excused[l] = _near(q[2], lo) or _near(q[2], hi)
        if not (ok and lo <= q[2] <= hi):
            continue
        excused[l] |= _near(u, 0.0) or _near(u, width - 1.0) or _near(v, 0.0) or _near(v, height - 1.0)
        if not (0.0 <= u <= width - 1 and 0.0 <= v <= height - 1):
            continue
        proj[l] = (v, u)
        keys = []
        for j in range(K):
            if kp_valid is not None and not kp_valid[j]:
                continue
            du, dv = float(kp[j, 1]) - u, float(kp[j, 0]) - v
            dd = du * du + dv * dv
            excused[l] |= _near(dd, r2)
            if dd <= r2:
                keys.append(int(hamming(rep_bits[l], kp_bits[j])) << 16 | j)
        keys.sort()
        in_window[l] = len(keys)
        if not keys:
            state[l] = 1
            continue
        d1s[l], j1s[l] = keys[0] >> 16, keys[0] & 0xFFFF
        if len(keys) > 1:
            d2s[l] = keys[1] >> 16
        if d1s[l] <= max_distance and F32(d1s[l]) < rat * F32(d2s[l]):
            state[l] = 4
            ck = int(d1s[l]) << 16 | l
            claim[int(j1s[l])] = min(claim.get(int(j1s[l]), ck), ck)
        else:
            state[l] = 2
    kp_lm = np.full(K, -1, np.int32)
    for j, ck in claim.items():
        kp_lm[j] = ck & 0xFFFF
    for l in range(L):
        if state[l] == 4 and kp_lm[j1s[l]] != l:
            state[l] = 3
    return _outputs(proj, state, d1s, d2s, j1s, kp_lm, kp, A, in_window, excused)


def _outputs(proj, state, d1s, d2s, j1s, kp_lm, kp, A, in_window, excused):
    kept = state == 4
    mk = np.full((len(state), 2), -1, F32)
    mk[kept] = kp[j1s[kept]]
    return dict(proj=proj, lm_state=state, lm_kp=np.where(kept, j1s, -1).astype(np.int32),
                lm_distance=np.where(state >= 2, d1s, A).astype(np.int32), match_keypoints=mk, kp_lm=kp_lm,
                counts=np.bincount(state, minlength=5).astype(np.int32), d2=d2s, in_window=in_window, excused=excused)


def match_vectorised(points, point_valid, rep_bits, R, t, cam, kp, kp_valid, kp_bits, num_bits, height, width, min_depth, max_depth,
                     radius, max_distance, ratio):
    """`match` once more as whole-array operations"""
    X, kp = np.asarray(points, F32).astype(F64), np.asarray(kp, F32)
    R, t, cam = np.asarray(R, F32).astype(F64).reshape(3, 3), np.asarray(t, F32).astype(F64), np.asarray(cam, F32).astype(F64)
    rep_bits, kp_bits = words(rep_bits), words(kp_bits)
    L, K = len(X), len(kp)
    A = absent(num_bits)
    lo, hi, rad = F64(F32(min_depth)), F64(F32(max_depth)), F64(F32(radius))
    with np.errstate(all="ignore"):
        q = [((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)]
        z = q[2]
        u, v = cam[0] * (q[0] / z) + cam[2], cam[1] * (q[1] / z) + cam[3]
        pv = np.ones(L, bool) if point_valid is None else np.asarray(point_valid) != 0
        view = pv & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2]) & (z >= lo) & (z <= hi) & (u >= 0) & (u <= width - 1) & (v >= 0) & (v <= height - 1)
        du, dv = kp[None, :, 1].astype(F64) - u[:, None], kp[None, :, 0].astype(F64) - v[:, None]
        dd = du * du + dv * dv
        kv = np.ones(K, bool) if kp_valid is None else np.asarray(kp_valid) != 0
        inside = (dd <= rad * rad) & view[:, None] & kv[None]
        fin = pv & np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2])
        depth = fin & (z >= lo) & (z <= hi)
        excused = (fin & (_near_v(z, lo) | _near_v(z, hi))) | (depth & (_near_v(u, 0.0) | _near_v(u, width - 1.0) | _near_v(v, 0.0) | _near_v(v, height - 1.0))) \
            | (view & (_near_v(dd, rad * rad) & kv[None]).any(1))
    proj = np.where(view[:, None], np.stack([v, u], 1), -1.0).astype(F32)
    ham = hamming_matrix(rep_bits, kp_bits)
    BIG = np.int64(1) << 40
    keys = np.sort(np.where(inside, ham << 16 | np.arange(K)[None], BIG), axis=1)
    k1 = keys[:, 0]
    k2 = keys[:, 1] if K > 1 else np.full(L, BIG)
    d1 = np.where(k1 < BIG, k1 >> 16, A).astype(np.int32)
    j1 = np.where(k1 < BIG, k1 & 0xFFFF, -1).astype(np.int32)
    d2 = np.where(k2 < BIG, k2 >> 16, A).astype(np.int32)
    cand = view & (k1 < BIG) & (d1 <= max_distance) & (d1.astype(F32) < F32(ratio) * d2.astype(F32))
    claim = np.full(K, BIG)
    np.minimum.at(claim, j1[cand], (d1[cand].astype(np.int64) << 16) | np.flatnonzero(cand))
    kp_lm = np.where(claim < BIG, claim & 0xFFFF, -1).astype(np.int32)
    kept = cand & (kp_lm[np.maximum(j1, 0)] == np.arange(L))
    state = np.where(~view, 0, np.where(k1 >= BIG, 1, np.where(~cand, 2, np.where(kept, 4, 3)))).astype(np.uint8)
    return _outputs(proj, state, d1, d2, j1, kp_lm, kp, A, inside.sum(1).astype(np.int32), excused)


OUTPUTS = ("proj", "lm_state", "lm_kp", "lm_distance", "match_keypoints", "kp_lm", "counts")


def same(a, b, names=OUTPUTS + ("d2", "in_window", "excused")):
    """two result dicts equal: integers equal, floats bit for bit"""
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                                                                           np.ascontiguousarray(b[k]).view(np.uint8)) for k in names)
