"""fp64 reference of the essential-matrix head (K10, csrc/essential.hip) in stages, the inputs both K10 test files run
on, a per-case error bound that comes from the reference alone, and a numpy fp32 restatement with hooks for planted
errors.  Plain numpy, no GPU.  Nothing here is fitted to a GPU result.

Stages (on top of oracle/numpy_oracle.py: essential_weights, essential_from_weights, essential_from_sums, which cite the
reference by file and line).  With core = P[:n, :m] * valid1 * valid2 in fp32 and B = {core > fp32(0.01)}:
    thr_row[i]        the top_k-th largest of row i's B entries when the row has more than top_k of them, else -inf
    candidates of i   {(j, core_ij) : core_ij in B, core_ij >= thr_row[i]}, a SET (the kernel's slot order follows its
                      column mapping and is no part of the contract); cand_cnt[i] their number, 255 past EM_CAND = 8
    col_part[band, j] the top_k largest B entries of column j inside the 32-row band, descending, padded with -inf
    thr_col[j]        the top_k-th largest B entry of column j, -inf when it has fewer
    weights           core_ij where (i, j) is a candidate and core_ij >= thr_col[j], else 0: identical to
                      O.essential_weights (the entries <= 0.01 that its thresholds may name carry no weight either way)
    col_cnt[j]        the number of weights in column j
    dense             any cand_cnt above 8 or any col_cnt above 8: the pair must take em_dense_front
    E                 O.essential_from_weights(weights, pts1, pts2, dtype=float64)
Every one of these but E is exact: the candidate values are P's own bits.

The bound on E.  E is a function F(h, M(h) + dM) of the six Hartley parameters h = (c1x, c1y, s1, c2x, c2y, s2) and of
the 81 normal-equation sums M[3p+r][3q+s] = sum_ij w_ij f1_ip f1_ir f2_jq f2_js with f = ((x - cx) s, (y - cy) s, 1).
The kernels form both in fp32; with u = 2^-24 and L the number of weights, counting em_dense_front / em_sparse_kernel:
  * a term of M: (x - c) s is 2 roundings per factor, a product of two factors 2 + 2 + 1 = 5, times w (exact) 1: the
    inner factor w (f2 f2) carries 6, the outer f1 f1 carries 5, their product 1: c = 12.  The L terms are added in some
    order (a row's candidates, a wave's lanes, a wave's rows, 16 waves): at most L - 1 roundings each.
        |dM| <= u (L + 12) sum_ij w_ij |f1_ip f1_ir f2_jq f2_js|
  * a centroid, A / (W + 1e-8) with A = sum w x (one product per term, a sum of the L weights row by row or column by
    column and then over rows: L + 1) and W likewise (L), the addition of 1e-8 and the division (2):
        |dc| <= u (2 L + 4) sum w |x| / W
  * a scale sqrt(2) / (sqrt(D / W + 1e-8) + 1e-8), D = sum w ((x - cx)^2 + (y - cy)^2): a difference 1, its square
    2 + 1, the sum of the two 1, times w 1, the sum over L terms L: D carries L + 5, W carries L, the division and the
    addition 2, the square root halves all that and adds 1, then the addition, the constant sqrtf(2) and the division 3:
        |ds| <= u (L + 10) s
    (the centroid's own error enters D only in second order: dD / dc = -2 sum w (x - c) = 0).
  * the solve: lam I - M (the trace: 8 sums and one difference) and a row of the 9 x 9 product (9 products, a sum) round
    like a perturbation of every entry of the shifted matrix by 18 u lam at the most, lam = trace(M) >= |M_ab|:
        |dM| += 18 u trace(M)                                      on all 81 sums
  * what follows the eigenvector is not amplified by the 9 x 9 problem and is charged on E itself: the denormalisation
    (two products with three-term rows, 10), the Gram matrices (5), ten manifold iterations of a 3 x 3 product and a
    normalisation (13 each, none assumed to contract: 130), E v (5), the norms and divisions (8), the cross products (3)
    and U diag(s, s, 0) V^T (9): OUT_ROUNDINGS = 170,
        floor = 170 u max |E|.
The bound of a case is  MARGIN * S + floor,  S = max over DIRECTIONS seeded sign patterns d in {-1, +1}^87 of
max |F(h + d_h dh, M(h + d_h dh) + d_M dM) - F(h, M(h))|, evaluated in fp64 at the perturbations' own size (they are 1e9
times fp64's rounding, so the difference is the first-order term).  It is an absolute bound on the entries of E.
  MARGIN is chosen on the CPU, never against the GPU: the smallest power of two for which every one of eleven correct fp32
evaluations of every case lies inside the bound (fp32_evaluations: O.essential_from_weights in fp32 on the input as it
stands, with its rows permuted, its columns permuted, both permuted, its rows reversed, its columns reversed and both
reversed; and four evaluations whose every sum is ONE fp32 chain over the weights, row-major and column-major, plain and
permuted -- chains of L - 1 roundings, longer than any the kernels form).  The sign patterns charge every sum its full
worst-case rounding at once, where a real evaluation's roundings mostly cancel (sqrt(L), not L), so the margin is far
below 1.  Over the 254 pairs of p_cases() (calibrate() prints the figures, test_essential_host.py asserts them):
        worst (fp32 error - floor) / S = 0.0041 (2, 257, 301, top_k 3, "row9"):  MARGIN = 2^-7 = 0.0078
        worst fp32 error / bound = 0.71 (3, 33, 65, top_k 6, masked); the median pair is below its floor alone.

The condition.  A bound is only worth its name where it can tell a lost weight: for every case, removing the single
smallest weight must move the fp64 E by at least CONDITION = 4 bounds (one_weight_shift).  A case that missed it got
another input until the reference alone satisfied it: (1, 1024, 1024) at top_k 6 another seed (RESEED; 3.6 bounds with
the first); the dots inputs every point of the smaller set matched (unmatched rows spread their mass into weights
near 0.01, which move nothing) and their weak matches made wrong in the scene (below).  Least shift / bound over all
P cases: 4.45, (1, 1024, 1024) at top_k 7.  test_essential_host.py asserts the condition for every P case and for the
dots inputs on a numpy Sinkhorn; test_gpu_essential.py asserts it again on the P the solver wrote.

Inputs.  p_case: a background of rng ** 8 * 0.3 and true matches of two_view geometry (synth_two_view, 0.5 px noise)
with values in [0.3, 0.9] on a seeded pairing that is not the identity, among them (0, 0), (n-1, m-1), rows 31 and 32
and columns 63, 64, 127, 128, 511, 512 where they exist.  Where n >= 31 and m >= 20, planted on rows of their own: a row
whose top_k-th place is shared by top_k + 1 equal values (below top_k - 1 larger ones); a row with exactly 8 candidates
(variant "row9": 9) and a column with exactly 8 row winners (variant "col9": 9); fp32(0.01) and its two neighbours in
an otherwise empty row; an all-zero row and column; a masked row holding its column's largest entry and a masked column
holding its row's largest.  The dustbin row n and column m are NaN.  dots_case: packed descriptors, min(n, m)
correspondences i <-> i with one flipped bit, every seventh a duplicate of its predecessor in both sets (exact ties in
P), every fifth weaker (bits / 64 more flipped bits) and wrong in the scene: the smallest weights are outliers with
leverage.  The P the GPU test feeds the oracle is the one mi_sinkhorn_dots wrote (anchored by
tests/test_gpu_sinkhorn.py); test_essential_host.py uses O.sinkhorn_match in its place.
"""
import functools

import numpy as np

from onnx_image_processing_amd.synth import synth_two_view, two_view_camera
from oracle import numpy_oracle as O

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EM_CAND, BAND_ROWS = 8, 32
THR = F32(0.01)
MARGIN = 2.0 ** -7
DIRECTIONS = 16
CONDITION = 4.0
OUT_ROUNDINGS = 170
RESEED = {(1024, 1024, 6): 1}          # cases whose first input missed the one-weight condition: another seed
N_ITER, N_ITER_MANIFOLD = 30, 10

# (batch, n, m): what each reaches is listed in test_gpu_essential.py
SHAPES = ((1, 3, 3), (2, 31, 20), (1, 32, 64), (3, 33, 65), (2, 257, 301), (1, 100, 512), (1, 100, 513), (1, 40, 1023),
          (1, 1024, 1024))
ITER_SHAPES = ((3, 33, 65), (1, 100, 513))          # these also run at n_iter 1 and 2
VARIANT_SHAPES = ((2, 31, 20), (3, 33, 65), (2, 257, 301), (1, 100, 513))     # the 9-candidate / 9-winner variants


# ------------------------------------------------------------------ the stages
def stages(p, valid1, valid2, top_k):
    """The exact quantities of one pair (see the module docstring) as a dict."""
    p = np.asarray(p, F32)
    n, m = p.shape[0] - 1, p.shape[1] - 1
    core = p[:n, :m].copy()
    if valid1 is not None:
        core = (core * np.asarray(valid1, F32)[:, None]) * np.asarray(valid2, F32)[None, :]
    big = core > THR
    xb = np.where(big, core, F32(-np.inf))
    rows_desc = -np.sort(-xb, axis=1)
    thr_row = np.where(big.sum(1) > top_k, rows_desc[:, top_k - 1], F32(-np.inf)).astype(F32)
    cand = big & (core >= thr_row[:, None])
    cnt = cand.sum(1)
    nb = -(-n // BAND_ROWS)
    col_part = np.full((nb, m, top_k), -np.inf, F32)
    for band in range(nb):
        part = -np.sort(-xb[band * BAND_ROWS:(band + 1) * BAND_ROWS], axis=0)[:top_k]
        col_part[band, :, :part.shape[0]] = part.T
    cols_desc = -np.sort(-xb, axis=0)
    thr_col = cols_desc[top_k - 1].astype(F32)
    weights = np.where(cand & (core >= thr_col[None, :]), core, F32(0.0)).astype(F32)
    col_cnt = (weights != 0).sum(0)
    return dict(n=n, m=m, core=core, thr_row=thr_row, cand=cand, cnt=cnt,
                cand_cnt=np.where(cnt > EM_CAND, 255, cnt).astype(np.uint8), col_part=col_part, thr_col=thr_col,
                weights=weights, col_cnt=col_cnt, dense=bool((cnt > EM_CAND).any() or (col_cnt > EM_CAND).any()))


def workspace_layout(batch, n, m, top_k):
    """Offsets of (thr_row, cand_cnt, cand_j, cand_x, col_part) and the total, in bytes: em_carve's five slices, each
    rounded up to 256 bytes."""
    nb = -(-n // BAND_ROWS)
    sizes = (batch * n * 4, batch * n, batch * n * EM_CAND * 4, batch * n * EM_CAND * 4, batch * nb * m * top_k * 4)
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off += (s + 255) // 256 * 256
    return offs, off


# ------------------------------------------------------------------ E in fp64 from (h, M), and its sensitivity
def _sparse(weights):
    i, j = np.nonzero(weights)
    return i, j, np.asarray(weights)[i, j].astype(F64)


def _hartley6(i, j, x, p1, p2):
    out = []
    for pts in (p1[i], p2[j]):
        w_sum = x.sum() + 1e-8
        c = (x[:, None] * pts).sum(0) / w_sum
        mean_dist = np.sqrt((x * ((pts - c) ** 2).sum(1)).sum() / w_sum + 1e-8)
        out += [c[0], c[1], np.sqrt(2.0) / (mean_dist + 1e-8)]
    return np.array(out)


def _transform(c0, c1, s):
    return np.array([[s, 0.0, -s * c0], [0.0, s, -s * c1], [0.0, 0.0, 1.0]])


def _sums(i, j, x, p1, p2, h):
    f1 = np.concatenate([(p1[i] - h[0:2]) * h[2], np.ones((len(i), 1))], axis=1)
    f2 = np.concatenate([(p2[j] - h[3:5]) * h[5], np.ones((len(j), 1))], axis=1)
    a = (f1[:, :, None] * f1[:, None, :]).reshape(-1, 9)
    b = (f2[:, :, None] * f2[:, None, :]).reshape(-1, 9)
    return (a * x[:, None]).T @ b, (np.abs(a) * x[:, None]).T @ np.abs(b)


def e_bound(weights, pts1, pts2, n_iter=N_ITER, n_iter_manifold=N_ITER_MANIFOLD):
    """(E in fp64 through the (h, M) stages, the bound on |dE|) of one pair."""
    i, j, x = _sparse(weights)
    p1, p2 = np.asarray(pts1, F64), np.asarray(pts2, F64)
    h = _hartley6(i, j, x, p1, p2)
    length = len(x)

    def solve(hh, dm):
        return O.essential_from_sums(_sums(i, j, x, p1, p2, hh)[0] + dm, _transform(*hh[0:3]), _transform(*hh[3:6]),
                                     n_iter, n_iter_manifold, F64)

    e0 = solve(h, 0.0)
    m0, m_abs = _sums(i, j, x, p1, p2, h)
    d_m = U * (length + 12) * m_abs + U * 18 * np.trace(m0.reshape(3, 3, 3, 3).transpose(0, 2, 1, 3).reshape(9, 9))
    w_sum = x.sum()
    d_h = np.empty(6)
    d_h[0:2] = U * (2 * length + 4) * (x[:, None] * np.abs(p1[i])).sum(0) / w_sum
    d_h[3:5] = U * (2 * length + 4) * (x[:, None] * np.abs(p2[j])).sum(0) / w_sum
    d_h[2], d_h[5] = U * (length + 10) * h[2], U * (length + 10) * h[5]
    rng = np.random.default_rng(87)
    worst = 0.0
    for _ in range(DIRECTIONS):
        sh = rng.integers(0, 2, 6) * 2.0 - 1.0
        sm = rng.integers(0, 2, (9, 9)) * 2.0 - 1.0
        worst = max(worst, np.abs(solve(h + sh * d_h, sm * d_m) - e0).max())
    return e0, MARGIN * worst + U * OUT_ROUNDINGS * np.abs(e0).max()


def one_weight_shift(weights, pts1, pts2, n_iter=N_ITER, n_iter_manifold=N_ITER_MANIFOLD):
    """max |dE| in fp64 when the single smallest weight is removed."""
    w = np.asarray(weights, F32).copy()
    e0 = O.essential_from_weights(w, pts1, pts2, n_iter, n_iter_manifold, dtype=F64)
    pos = np.where(w > 0, w, np.inf)
    w[np.unravel_index(np.argmin(pos), w.shape)] = 0.0
    return np.abs(O.essential_from_weights(w, pts1, pts2, n_iter, n_iter_manifold, dtype=F64) - e0).max()


def fp32_evaluations(weights, pts1, pts2, n_iter=N_ITER, n_iter_manifold=N_ITER_MANIFOLD):
    """Seven correct fp32 evaluations of E: the input as it stands, rows / columns / both permuted, rows / columns / both
    reversed (the order of every sum changes, the value of none)."""
    w, p1, p2 = np.asarray(weights, F32), np.asarray(pts1, F32), np.asarray(pts2, F32)
    n, m = w.shape
    rng = np.random.default_rng(n * 4099 + m)
    pr, pc = rng.permutation(n), rng.permutation(m)
    ir, ic = np.arange(n), np.arange(m)
    out = []
    for r, c in ((ir, ic), (pr, ic), (ir, pc), (pr, pc), (ir[::-1], ic), (ir, ic[::-1]), (ir[::-1], ic[::-1])):
        out.append(O.essential_from_weights(w[r][:, c], p1[r], p2[c], n_iter, n_iter_manifold))
    for r, c, by_column in ((ir, ic, False), (ir, ic, True), (pr, pc, False), (ir[::-1], ic[::-1], True)):
        out.append(_sequential_f32(w[r][:, c], p1[r], p2[c], by_column, n_iter, n_iter_manifold))
    return out


def _chain(terms):
    """The sum of fp32 terms along axis 0, one after the other in fp32: a chain of len - 1 roundings, longer than any
    the kernels form (a lane's 16 entries, a wave's 64 rows, 16 waves)."""
    terms = np.asarray(terms, F32)
    return np.add.accumulate(terms, axis=0, dtype=F32)[-1] if len(terms) else np.zeros(terms.shape[1:], F32)


def _sequential_f32(w, p1, p2, by_column, n_iter, n_iter_manifold):
    """A correct fp32 evaluation whose every sum is ONE chain over the weights in row-major (or column-major) order."""
    i, j = np.nonzero(w.T)[::-1] if by_column else np.nonzero(w)
    x = w[i, j]
    hs = []
    for pts in (p1[i], p2[j]):
        w_sum = _chain(x) + F32(1e-8)
        c = _chain(x[:, None] * pts) / w_sum
        d = pts - c
        mean_dist = np.sqrt(_chain(x * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])) / w_sum + F32(1e-8))
        hs.append((c, F32(np.sqrt(F32(2.0)) / (mean_dist + F32(1e-8)))))
    (c1, s1), (c2, s2) = hs
    f1 = np.concatenate([(p1[i] - c1) * s1, np.ones((len(i), 1), F32)], axis=1)
    f2 = np.concatenate([(p2[j] - c2) * s2, np.ones((len(j), 1), F32)], axis=1)
    a = (f1[:, :, None] * f1[:, None, :]).reshape(-1, 9)
    b = (f2[:, :, None] * f2[:, None, :]).reshape(-1, 9) * x[:, None]
    m_flat = _chain(a[:, :, None] * b[:, None, :])
    return O.essential_from_sums(m_flat, _transform(c1[0], c1[1], s1).astype(F32), _transform(c2[0], c2[1], s2).astype(F32),
                                 n_iter, n_iter_manifold, F32)


# ------------------------------------------------------------------ a Python restatement of the head with planted errors
PLANTS = ("row_gt", "col_k_plus_1", "valid_after", "ge_001", "hartley_2", "no_shift", "one_iteration_less")


def head_f32(p, valid1, valid2, pts1, pts2, top_k, n_iter=N_ITER, n_iter_manifold=N_ITER_MANIFOLD, plant=None):
    """The head in numpy fp32.  plant=None is the head; each name in PLANTS changes one line of it."""
    assert plant is None or plant in PLANTS
    core = np.asarray(p, F32)[:-1, :-1].copy()
    n, m = core.shape
    mask = None if valid1 is None else np.asarray(valid1, F32)[:, None] * np.asarray(valid2, F32)[None, :]
    if mask is not None and plant != "valid_after":
        core = core * mask
    tr = np.sort(core, axis=1)[:, -top_k][:, None]
    tc = np.sort(core, axis=0)[-min(top_k + 1, n) if plant == "col_k_plus_1" else -top_k][None, :]
    in_row = core > tr if plant == "row_gt" else core >= tr
    confident = core >= THR if plant == "ge_001" else core > THR
    w = core * (in_row & (core >= tc) & confident).astype(F32)
    if mask is not None and plant == "valid_after":
        w = w * mask
    p1, p2 = np.asarray(pts1, F32), np.asarray(pts2, F32)
    t1, s1, c1 = O._hartley(p1, w.sum(axis=1, dtype=F32))
    t2, s2, c2 = O._hartley(p2, w.sum(axis=0, dtype=F32))
    if plant == "hartley_2":
        s1, s2 = F32(s1 * np.sqrt(F32(2.0))), F32(s2 * np.sqrt(F32(2.0)))
        t1, t2 = _transform(c1[0], c1[1], s1).astype(F32), _transform(c2[0], c2[1], s2).astype(F32)
    f1 = np.concatenate([(p1 - c1) * s1, np.ones((n, 1), F32)], axis=-1)
    f2 = np.concatenate([(p2 - c2) * s2, np.ones((m, 1), F32)], axis=-1)
    big1 = (f1[:, :, None] * f1[:, None, :]).reshape(n, 9)
    big2 = (f2[:, :, None] * f2[:, None, :]).reshape(m, 9)
    return O.essential_from_sums(big1.T @ (w @ big2), t1, t2, n_iter - (plant == "one_iteration_less"), n_iter_manifold,
                                 F32, shift=plant != "no_shift")


# ------------------------------------------------------------------ inputs
def _normalised(kp, f=500.0):
    """(y, x) pixels of synth_two_view -> normalised (x, y), fp32 (the head's input: exact from here on)."""
    k = two_view_camera(f)
    return np.stack([(kp[:, 1].astype(F64) - k[0, 2]) / k[0, 0], (kp[:, 0].astype(F64) - k[1, 2]) / k[1, 1]], axis=1).astype(F32)


def _geometry(n, m, pairs, seed, noise_px):
    """Points for an (n, m) problem whose listed (row, column) pairs are true correspondences of one two-view scene; every
    other row and column shows a scene point of its own."""
    kp1, kp2 = synth_two_view(seed, n + m, 0.0, noise_px)[:2]
    q1, q2 = _normalised(kp1), _normalised(kp2)
    pts1, pts2 = np.zeros((n, 2), F32), np.zeros((m, 2), F32)
    rows_left, cols_left = set(range(n)), set(range(m))
    t = 0
    for i, j in pairs:
        pts1[i], pts2[j] = q1[t], q2[t]
        rows_left.discard(i), cols_left.discard(j)
        t += 1
    for i in sorted(rows_left):
        pts1[i] = q1[t]
        t += 1
    for j in sorted(cols_left):
        pts2[j] = q2[t]
        t += 1
    return pts1, pts2


def _p_pair(n, m, top_k, seed, variant, noise_px):
    rng = np.random.default_rng([seed, n, m])
    core = (rng.random((n, m)) ** 8 * 0.3).astype(F32)
    free_r, free_c, pairs = list(range(n)), list(range(m)), []

    def take(i, j):
        pairs.append((i, j))
        free_r.remove(i), free_c.remove(j)

    take(0, 0)
    if n > 1 and m > 1:
        take(n - 1, m - 1)
    for c in (63, 64, 127, 128, 511, 512):
        if c in free_c and free_r:
            take(free_r[(7 * c) % len(free_r)], c)
    for r in (31, 32):
        if r in free_r and free_c:
            take(r, free_c[(5 * r) % len(free_c)])
    special = n >= 31 and m >= 20
    meta = dict(special=special)
    if special:
        rs = [free_r.pop(int(rng.integers(len(free_r)))) for _ in range(14)]
        zc, c8 = (free_c.pop(int(rng.integers(len(free_c)))) for _ in range(2))
    rr, cc = rng.permutation(free_r), rng.permutation(free_c)
    for i, j in zip(rr, cc):
        pairs.append((int(i), int(j)))
    ii, jj = np.array(pairs).T
    core[ii, jj] = rng.uniform(0.3, 0.9, len(pairs)).astype(F32)
    valid1, valid2 = rng.random(n) > 0.1, rng.random(m) > 0.1
    if special:
        zr, tie, r8, hr, mr, c8_rows = rs[0], rs[1], rs[2], rs[3], rs[4], rs[5:14]
        plain = np.array([j for j in range(m) if j not in (zc, c8)])
        kept = {c8, 0, m - 1}
        if len(plain) >= 2 * top_k:
            cols = rng.choice(plain, 2 * top_k, replace=False)
            core[tie, cols[:top_k - 1]] = 0.93
            core[tie, cols[top_k - 1:]] = 0.6
            valid2[cols] = True
            kept |= set(cols)
        q = 9 if variant == "row9" else 8
        cols = rng.choice(plain, q, replace=False)
        core[r8, cols] = 0.95
        valid2[cols] = True
        kept |= set(cols)
        q = 9 if variant == "col9" else 8
        core[c8_rows[:q], c8] = 0.97
        cols = rng.choice(plain, 3, replace=False)
        core[hr, :] = 0.0
        core[hr, cols] = [THR, np.nextafter(THR, F32(1.0)), np.nextafter(THR, F32(0.0))]
        valid2[cols] = True
        kept |= set(cols)
        i_m, j_m = pairs[len(pairs) // 2]
        core[mr, j_m] = 0.99                                     # its column's largest, in a row the masks switch off
        i_c, j_c = next(((i, j) for i, j in pairs[len(pairs) // 3:] + pairs if j not in kept and j != j_m), (None, None))
        if j_c is not None:                                      # (m = 20 at top_k = 8: every column is taken)
            core[i_c, j_c] = 0.98                                # its row's largest, in a column the masks switch off
        core[zr, :] = 0.0
        core[:, zc] = 0.0
        valid1[[zr, tie, r8, hr] + list(c8_rows)] = True
        valid2[[c8, j_m]] = True
        valid1[mr] = False
        if j_c is not None:
            valid2[j_c] = False
        valid1[i_m] = True
        meta.update(zero_row=zr, zero_col=zc, tie_row=tie, row8=r8, col8=c8, thr_row=hr, masked_row=mr, masked_col=j_c)
    p = np.full((n + 1, m + 1), np.nan, F32)
    p[:n, :m] = core
    pts1, pts2 = _geometry(n, m, pairs, seed, noise_px)
    return p, valid1, valid2, pts1, pts2, meta


@functools.lru_cache(maxsize=None)
def p_case(batch, n, m, top_k, variant="base", noise_px=0.5):
    """(P (b, n+1, m+1), valid1 (b, n), valid2 (b, m), pts1 (b, n, 2), pts2 (b, m, 2), meta of pair 0...) as a dict."""
    parts = [_p_pair(n, m, top_k, 1000 + 17 * b + RESEED.get((n, m, top_k), 0), variant, noise_px) for b in range(batch)]
    out = dict(p=np.stack([x[0] for x in parts]), valid1=np.stack([x[1] for x in parts]),
               valid2=np.stack([x[2] for x in parts]), pts1=np.stack([x[3] for x in parts]),
               pts2=np.stack([x[4] for x in parts]), meta=[x[5] for x in parts])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dots_case(batch, n, m, bits):
    """Packed descriptors (b, n, bits / 32), (b, m, bits / 32) uint32 -- min(n, m) correspondences i <-> i with one flipped
    bit (rows or columns without one spread their mass into entries near 0.01, weights without leverage), every seventh of those a duplicate of its predecessor in both sets;
    every fifth is weaker (bits / 64 more flipped bits) and wrong in the scene, so the smallest weights are outliers with
    leverage -- with points of one two-view scene per pair and validity masks."""
    rng = np.random.default_rng([bits, n, m])
    words = bits // 32
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, words), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, words), dtype=np.uint64).astype(np.uint32)
    k = min(n, m)
    b2[:, :k] = b1[:, :k]
    wrong = np.arange(k) % 5 == 2                                # descriptor matches that are wrong in the scene
    for b in range(batch):
        b2[b, np.arange(k), rng.integers(0, words, k)] ^= np.uint32(1) << rng.integers(0, 32, k).astype(np.uint32)
        for t in np.flatnonzero(wrong):                          # ... and weaker: bits / 64 more flipped bits
            flips = rng.choice(bits, bits // 64, replace=False)
            np.bitwise_xor.at(b2[b, t], flips // 32, np.uint32(1) << (flips % 32).astype(np.uint32))
        for t in range(7, k, 7):
            b1[b, t], b2[b, t] = b1[b, t - 1], b2[b, t - 1]
            wrong[t] = wrong[t - 1]
    pts = [_geometry(n, m, [(t, t) for t in range(k) if not wrong[t]], 2000 + 13 * b + n, 0.5) for b in range(batch)]
    out = dict(b1=b1, b2=b2, pts1=np.stack([x[0] for x in pts]), pts2=np.stack([x[1] for x in pts]),
               valid1=rng.random((batch, n)) > 0.1, valid2=rng.random((batch, m)) > 0.1)
    for v in out.values():
        v.setflags(write=False)
    return out


def sinkhorn_p(case, b, epsilon=0.05):
    """The CPU stand-in for the P of dots_case's pair b (unit-normalised bit descriptors, squared distance / eps)."""
    unpack = lambda w: np.unpackbits(w.view(np.uint8), bitorder="little").reshape(w.shape[0], -1).astype(F32)  # noqa: E731
    d1, d2 = unpack(case["b1"][b]), unpack(case["b2"][b])
    d1 /= np.maximum(np.linalg.norm(d1, axis=1, keepdims=True), 1e-12)
    d2 /= np.maximum(np.linalg.norm(d2, axis=1, keepdims=True), 1e-12)
    return O.sinkhorn_match(d1[None], d2[None], 20, epsilon, 1.0)[0].astype(F32)


# ------------------------------------------------------------------ references (cached)
def reference_pair(p, valid1, valid2, pts1, pts2, top_k, n_iter=N_ITER, n_iter_manifold=N_ITER_MANIFOLD):
    """The stages of one pair plus E (fp64) and its bound."""
    st = stages(p, valid1, valid2, top_k)
    st["E"], st["bound"] = e_bound(st["weights"], pts1, pts2, n_iter, n_iter_manifold)
    return st


@functools.lru_cache(maxsize=None)
def reference(batch, n, m, top_k, masked, variant="base", n_iter=N_ITER):
    """reference_pair of every pair of p_case(batch, n, m, top_k, variant)."""
    c = p_case(batch, n, m, top_k, variant)
    return [reference_pair(c["p"][b], c["valid1"][b] if masked else None, c["valid2"][b] if masked else None,
                           c["pts1"][b], c["pts2"][b], top_k, n_iter) for b in range(batch)]


def p_cases():
    """Every (batch, n, m, top_k, masked, variant, n_iter) the GPU test runs on the P source (a dense call and a banded
    call of the same key share one reference)."""
    out = []
    for shape in SHAPES:
        for masked in (False, True):
            for top_k in range(1, min(8, shape[1], shape[2]) + 1):
                out.append(shape + (top_k, masked, "base", N_ITER))
    for shape in ITER_SHAPES:
        for n_iter in (1, 2):
            out.append(shape + (3, False, "base", n_iter))
    for shape in VARIANT_SHAPES:
        for variant in ("row9", "col9"):
            for top_k in (1, 3, 4):
                out.append(shape + (top_k, False, variant, N_ITER))
    return out


DOTS_CASES = (((1, 3, 3), 256), ((2, 31, 20), 256), ((1, 32, 64), 512), ((3, 33, 65), 256), ((2, 257, 301), 512),
              ((1, 100, 512), 256), ((1, 100, 513), 512), ((1, 40, 1023), 256), ((1, 1024, 1024), 512))
DOTS_TOP_K = (1, 2, 3, 4, 5, 8)         # 1..4 banded and dense, 5 the refused workspace, 8 dense only


def case_report(ref, pts1, pts2, n_iter=N_ITER):
    """What the margin was chosen from, for one pair: (worst fp32 evaluation error, the bound's counted floor, its
    sensitivity part before the margin, the one-weight shift)."""
    evals = fp32_evaluations(ref["weights"], pts1, pts2, n_iter)
    err = max(np.abs(e.astype(F64) - ref["E"]).max() for e in evals)
    floor = U * OUT_ROUNDINGS * np.abs(ref["E"]).max()
    return err, floor, (ref["bound"] - floor) / MARGIN, one_weight_shift(ref["weights"], pts1, pts2, n_iter)


def calibrate():
    """Prints the figures MARGIN was chosen from.  From tests/: python -c 'import essential_oracle as E; E.calibrate()'"""
    worst_raw = worst = 0.0
    least = np.inf
    for key in p_cases():
        batch, n, m, top_k, masked, variant, n_iter = key
        c = p_case(batch, n, m, top_k, variant)
        for b, ref in enumerate(reference(*key)):
            err, floor, raw, shift = case_report(ref, c["pts1"][b], c["pts2"][b], n_iter)
            worst_raw, worst, least = max(worst_raw, (err - floor) / raw), max(worst, err / ref["bound"]), min(least, shift / ref["bound"])
            print(key, b, f"L {int((ref['weights'] != 0).sum())} err/raw {(err - floor) / raw:.3g} err/bound {err / ref['bound']:.3g} "
                  f"shift/bound {shift / ref['bound']:.3g} dense {ref['dense']}")
    print(f"worst (fp32 error - floor) / sensitivity {worst_raw:.3g}: MARGIN is the next power of two; worst error / bound "
          f"{worst:.3g}; least one-weight shift / bound {least:.3g}")
