"""fp64 reference of the Sinkhorn stage (K6, csrc/sinkhorn_dots.hip and csrc/sinkhorn.hip), one half-step at a time,
with a-priori fp32 error bounds, the inputs both Sinkhorn test files run on, and a numpy fp32 evaluation with hooks for
planted errors.  Plain numpy, no GPU.  Nothing here is fitted to a measurement.

The iteration (reference matching/sinkhorn.py:112-147,187-206).  Z is the (n+1) x (m+1) log-score matrix, its last row
and column the dustbin constant; log mu = (0, .., 0, log m), log nu = (0, .., 0, log n), the logarithms taken of fp32(m)
and fp32(n) as the kernels' logf((float)m) do.  From u = v = 0, T times
        u_i = log mu_i - LSE_j(z_ij + v_j)          row_step(Z, v)
        v_j = log nu_j - LSE_i(z_ij + u_i)          col_step(Z, u)
and P = exp(Z + u + v).  The half-steps here are exact (fp64) functions of GIVEN inputs: fed the kernel's own v(T-1)
they say what u(T) has to be whatever happened before, which is what separates one wrong half-step from the drift of T
right ones.

Z and its error dz.  fp32-Z form (mi_sinkhorn): Z is the input, dz = 0.  Dots form (mi_sinkhorn_dots): Z is
cost_oracle.bit_reference in fp64 and dz its bound, BITS_K u (|a|^2 + |b|^2 + 2 a.b) / eps.  The kernels rebuild z as
fma(dot * s_b, -2 nie s_a, |b|^2 nie) + |a|^2 nie with nie = fp32(-1 / eps): the scales carry 2 u each, the squared
norms 5 u (test_gpu_cost.py), nie two roundings (the division, and eps against fp32(eps)), the products and the sums
one each: 9 on the cross term, 9 on the norm terms, inside BITS_K = 10.  The dustbin constant is fp32(-unused / eps),
the number both entry points document and use: exact, dz = 0.

The one-step bound.  A half-step over L terms evaluates, in some frame (the dots kernels take the row constant
c_i = nie |a_i|^2 out of the row, the others have c = 0), exponents a_j = (z_ij - c_i) + w_j, a shift S, and
        r = (log mu) - (S + ln2 * log2(sum_j exp2((a_j - S) * log2 e))) - c_i.
With M = max_j |a_j| and u = 2^-24, in the log domain:
    1. forming a_j (one add or one fma)                                  u M
    2. subtracting the shift             u |a_j - S|                  <= u (M + |S|)
    3. the product with log2 e: its rounding and the constant's own error, 1.5 u |a_j - S|   <= 1.5 u (M + |S|)
    4. v_exp_f32, 1 ulp                                                  2 u
    5. a sum of L positive terms in ANY order                            (L - 1) u
    6. v_log_f32, 1 ulp of log2 s, and the product with ln 2 (rounding and constant): 3.5 u |ln s|, where
       |ln s| = |LSE - S| <= M + |S| + ln L                           <= 3.5 u (M + |S| + ln L)
    7. adding the shift back (and the rounding of -S log2 e itself)      u (M + |S| + ln L)
    8. the final subtractions (log mu <= ln L, and c_i in the dots form) u (M + 2 ln L) + u |c_i|
That is 9 on M, 7 on |S|, 6.5 on ln L, 1 on |c_i|, if a kernel pays every step in full.  None does:
  * the dots kernels (csrc/sinkhorn_dots.hip) form (a_j - S) log2 e in ONE fma, so steps 2 and 3 together cost 1.5, not
    2.5: 8 on M, 6 on |S|;
  * the fp32-Z kernels (csrc/sinkhorn.hip) subtract and multiply separately (sk_exp(x - mx): the full 2.5), but every one
    of them shifts by the maximum itself: |a_j - S| <= 2 M, so steps 2 and 3 cost at most 5 u M and nothing on |S|; and
    s lies in [1, L], so step 6 is 3.5 u ln L, not 3.5 u (M + |S| + ln L): 1 + 5 + 1 + 1 = 8 on M, 1 on |S|, 6.5 on
    ln L.  Their dustbin terms go through libm's expf / logf, which are no worse than the 1 ulp of v_exp_f32 /
    v_log_f32.  Where they merge (maximum, sum) pairs, a partial sum is rescaled by expf(m_old - m_new), 3 u +
    u |m_old - m_new| per merge; that is not in the count and rides on step 5, which charges (L - 1) u for a summation
    order no kernel has (a lane's chain plus a tree: tens of roundings, not L).
With A = M + |S| + |c_i| + ln L every form is therefore inside
        h = dz + u (C_A A + C_L L + 8),         C_A = 8, C_L = 1,
C_L = 1 being step 5 and the constant step 4 with six to spare.  C_A = 8 is the largest value these tests allow
themselves; the count supports no less for every form.  A is wider than max |a_j| + |S|: the row constant and ln L are
magnitudes that steps 6 to 8 really round at, and leaving them out would make the bound wrong for nearly constant rows
(M and S near 0, ln L = 7).
  The column half of the probability-form kernels (every dots kernel, the fused fp32 kernels of key 4 = 0 and 2) is
        v_j <- v_old_j + log nu_j - log(sum_i P_ij),        P_ij = exp2((a_ij - S) log2 e) / s_i
with the a_ij, S and s_i of the ROW half before it; u_i was written from the same s_i, so against col_step(Z, u_gpu) the
sum's own error cancels and what remains is u_i's last three roundings (steps 6 to 8 of its row: covered by that row's
A), the exponent's (steps 1 to 3 of that row), the reciprocal and the product (2 u + u), the sum over L = n + 1 rows
and the outer v_old + ... whose terms are as large as |v_old_j|.  So its A is
        A_j = max_i |z_ij + u_i + v_old_j| + |v_old_j| + ln L + max_i A_i(row half),
the maximum over ALL rows because a column's mass may sit in any of them, the row with the largest A included (a
planted match on an all-ones or empty descriptor's row is such a column); weighting the rows by the column's P would be
tighter and is not needed: every planted error and mutant is outside the bound as it is.
The log-domain column kernels (two-pass form, key 4 = 1) are the row count with rows and columns exchanged.
  Shifts.  S is the row (column) maximum of the a_j, except for the bounded-shift row kernels (sqnorm_bound > 0 and
2 sqnorm_bound / eps * log2 e < 90), whose S is one number per pair,
        S = max(max_j wp_j + G, dust + v_m + D),   wp_j = nie |b_j|^2 + v_j,   G = 2 sqnorm_bound / eps,
        D = sqnorm_bound / eps                     (the comment above SKD_AUX in csrc/sinkhorn_dots.hip),
evaluated here in fp64 from the same inputs.  The dustbin row always shifts by its own maximum.

End to end.  LSE is 1-Lipschitz in the sup norm, so an error e in v becomes at most e + h in u and at most e + 2 h in
the next v: after T iterations |u - u_ref|, |v - v_ref| <= 2 T max h.  Loose; it catches a wrong iteration count and
a stale first iteration, not rounding.

P.  P_ij = exp2(((z + u) + v) log2 e) from the fp32 duals: one rounding on z + u, one on the sum, 1.5 on the product,
2 u for v_exp_f32: relative error dz + u (C_P t + 4) with C_P = 4 >= 3.5 and t = max(|z + u|, |z + v|, |z + u + v|) --
the largest intermediate in either order of the two additions (|z + u + v| alone misses the rounding of z + u, which
at eps = 0.005 is two hundred times larger than the exponent of a matched pair).  Relative, so it holds every entry
to account however small; where the fp64 value is below the smallest normal fp32 (2^-126) the kernel's may be
anything up to 2^-126 (v_exp_f32 flushes denormals).

Inputs.  cost_oracle.bit_inputs (duplicates, thinned, all-ones, empty and complement descriptors) with matches of
fresh random descriptors planted on the structural edges: row 0 with column 0, row n-1 with column m-1, rows 31 and
32 with columns 511 and 512 where they exist, and one inside the last partial band; the all-ones pair, which the
first plant overwrites, moves to index 3.  The fp32-Z form runs on a seeded cost in [0.25, 2] with zeros planted at
the same places.  Regimes: "flat" (eps = 1: every element carries about 1 / L of its row's sum, so a lost element is
seen), "hamming" (raw bit vectors, eps = bits / 8, as flat), "standard" (eps = 0.05), "edge35" / "edge30" (the last
bounded-shift value and the first that falls back to row maxima), "floor" (MI_DOTS_MIN_EPSILON)."""
from __future__ import annotations

import numpy as np

import cost_oracle as C

U = C.U
C_A, C_L, C_P = 8.0, 1.0, 4.0
TINY = 2.0 ** -126
F = np.float32
L2E, LN2 = 1.4426950408889634, 0.6931471805599453
FAST_LIMIT = 90.0                  # SKD_FAST_LIMIT
MIN_EPSILON = 0.005                # MI_DOTS_MIN_EPSILON
BITS = 256

# regime -> (epsilon, unused_score, normalized)
REGIMES = {"flat": (1.0, 1.0, True), "hamming": (BITS / 8.0, BITS / 4.0, False), "standard": (0.05, 1.0, True),
           "edge35": (0.035, 1.0, True), "edge30": (0.03, 1.0, True), "floor": (MIN_EPSILON, 1.0, True)}

# The iteration counts whose duals are held against the reference's end to end: a stale first iteration or a wrong
# marginal shows at every one of them.  E2E_DISTINCT: those at which the check also tells T from T - 1 and T + 1, because
# one iteration moves the duals by ten bounds or more (asserted in test_sinkhorn_host.py).  In the flat regimes the
# iteration contracts so fast that its second pass already moves them by less than 2 T max h, and at the floor T = 20
# is all that runs.
E2E_ITERATIONS = {"flat": (1, 2, 3), "hamming": (1, 2, 3), "standard": (1, 2, 3), "edge35": (1, 2, 3), "edge30": (1, 2, 3),
                  "floor": (20,)}
E2E_DISTINCT = {"flat": (1,), "hamming": (1,), "standard": (1, 2, 3), "edge35": (1, 2, 3), "edge30": (1, 2, 3), "floor": ()}

# (batch, n, m) of tests/test_gpu_sinkhorn.py, per group of forms
PERSIST_SHAPES = [(1, 1, 1), (3, 33, 65), (8, 97, 130), (1, 512, 512)]
BAND_SHAPES = [(2, 97, 130), (1, 31, 512), (2, 512, 33), (9, 40, 56)]
BATCH64_SHAPES = [(64, 40, 56), (65, 33, 65)]
THREE_PARTS_SHAPE = (97, 33, 65)                # 32 pairs per part at least: parts of 32, 32 and 33 pairs
WIDE_SHAPES = [(2, 70, 513), (1, 33, 1000), (2, 130, 1024)]
FUSED_SHAPES = [(2, 70, 200), (2, 70, 257), (2, 70, 512), (2, 70, 513), (2, 70, 1000), (2, 70, 1024), (2, 130, 512)]
TWO_PASS_SHAPES = [(2, 40, 255), (2, 40, 258), (2, 40, 600), (2, 40, 1027), (2, 40, 1500), (3, 5, 3)]
DOTS_SHAPES = PERSIST_SHAPES + BAND_SHAPES + BATCH64_SHAPES + [THREE_PARTS_SHAPE] + WIDE_SHAPES
F32_SHAPES = FUSED_SHAPES + TWO_PASS_SHAPES


def bounded_shift(epsilon: float, sqnorm_bound: float) -> bool:
    """Whether mi_sinkhorn_dots takes the bounded-shift row kernels (the test of mi_sinkhorn_dots_impl)."""
    return sqnorm_bound > 0.0 and float(F(2.0 / epsilon * sqnorm_bound)) * L2E < FAST_LIMIT


# ------------------------------------------------------------------ exact half-steps
def lse(x: np.ndarray, axis: int) -> np.ndarray:
    mx = x.max(axis=axis, keepdims=True)
    return (np.log(np.exp(x - mx).sum(axis=axis, keepdims=True)) + mx).squeeze(axis)


def log_marginals(batch: int, n: int, m: int):
    log_mu, log_nu = np.zeros((batch, n + 1)), np.zeros((batch, m + 1))
    log_mu[:, n] = np.log(np.float64(F(m)))
    log_nu[:, m] = np.log(np.float64(F(n)))
    return log_mu, log_nu


def pad(z: np.ndarray, dust: float) -> np.ndarray:
    """(batch, n, m) -> (batch, n + 1, m + 1) with the dustbin row and column, in z's type."""
    b, n, m = z.shape
    out = np.full((b, n + 1, m + 1), dust, z.dtype)
    out[:, :n, :m] = z
    return out


def row_step(Z: np.ndarray, v_prev: np.ndarray) -> np.ndarray:
    b, n1, m1 = Z.shape
    return log_marginals(b, n1 - 1, m1 - 1)[0] - lse(Z + np.asarray(v_prev, np.float64)[:, None, :], 2)


def col_step(Z: np.ndarray, u: np.ndarray) -> np.ndarray:
    b, n1, m1 = Z.shape
    return log_marginals(b, n1 - 1, m1 - 1)[1] - lse(Z + np.asarray(u, np.float64)[:, :, None], 1)


def reference_duals(Z: np.ndarray, iterations: int):
    """[(u(1), v(1)), ..., (u(T), v(T))] in fp64."""
    b, n1, m1 = Z.shape
    v, out = np.zeros((b, m1)), []
    for _ in range(iterations):
        u = row_step(Z, v)
        v = col_step(Z, u)
        out.append((u, v))
    return out


# ------------------------------------------------------------------ inputs
def dust_of(epsilon: float, unused: float) -> float:
    return float(F(-unused / epsilon))


def band_plant(n: int, m: int):
    """(row, column) of the match planted inside the last partial band, away from its last row; None where that band
    has one row only (n - 1 a multiple of 16) or the shape is too small."""
    if n < 8 or m < 8 or (n - 1) % 16 == 0:
        return None
    i = (n - 1) // 16 * 16 + ((n - 1) % 16) // 2             # inside the last (partial) band of 16 or 32 rows
    j = (m - 1) // 8 * 8 - 3                                   # and in the last full 8-column group
    return (i, j) if 0 < i < n - 1 and 0 < j < m - 1 else None


def plants(n: int, m: int):
    """[(row, column)] of the planted matches; empty for shapes too small to hold them apart."""
    if n < 8 or m < 8:
        return []
    out = [(0, 0), (n - 1, m - 1)]
    for i, j in ((31, 511), (32, 512)):
        if i < n - 1 and j < m - 1:
            out.append((i, j))
    i, j = band_plant(n, m) or (0, 0)
    if all(i != a and j != c for a, c in out) and i > 0 and j > 0:
        out.append((i, j))
    return out


def bit_inputs(batch: int, n: int, m: int, words: int = BITS // 32):
    """cost_oracle.bit_inputs plus the planted edge matches (fresh random descriptors, so that each is unique)."""
    b1, b2 = C.bit_inputs(batch, n, m, words)
    rng = np.random.default_rng([n, m, words, 11])
    if n >= 8 and m >= 8:
        b1[0, 3], b2[0, 3] = np.uint32(0xFFFFFFFF), np.uint32(0xFFFFFFFF)
    for i, j in plants(n, m):
        fresh = rng.integers(0, 2 ** 32, size=(batch, words), dtype=np.uint64).astype(np.uint32)
        b1[:, i] = fresh
        b2[:, j] = fresh
    return b1, b2


def dots_problem(batch: int, n: int, m: int, regime: str):
    """The dots form's problem: dict with the packed descriptors, Z and dz (batch, n + 1, m + 1) fp64, the row and
    column constants of the kernels' frame (c_row = nie |a_i|^2 with 0 for the dustbin row; c_col likewise) and the
    scalars."""
    epsilon, unused, normalized = REGIMES[regime]
    b1, b2 = bit_inputs(batch, n, m)
    z, dz = C.bit_reference(b1, b2, normalized, epsilon)
    dust = dust_of(epsilon, unused)
    pop1, pop2 = C.unpack(b1).sum(-1), C.unpack(b2).sum(-1)
    na, nb = ((pop1 > 0).astype(np.float64), (pop2 > 0).astype(np.float64)) if normalized else (pop1, pop2)
    e = C.eps32(epsilon)
    c_row = np.concatenate([-na / e, np.zeros((batch, 1))], 1)
    c_col = np.concatenate([-nb / e, np.zeros((batch, 1))], 1)
    return dict(b1=b1, b2=b2, Z=pad(z, dust), dz=pad(dz, 0.0), dust=dust, c_row=c_row, c_col=c_col, epsilon=epsilon,
                unused=unused, normalized=normalized, sqnorm_bound=1.0 if normalized else float(BITS), shape=(batch, n, m))


def f32_problem(batch: int, n: int, m: int, regime: str):
    """The fp32-Z form's problem: z32 (batch, n, pitch) float32 with NaN in the row padding, Z = its fp64 copy padded,
    dz = 0."""
    epsilon, unused, _ = REGIMES[regime]
    rng = np.random.default_rng([n, m, 13])
    cost = 0.25 + 1.75 * rng.random((batch, n, m))
    for i, j in plants(n, m) or [(0, 0), (n - 1, m - 1)]:
        cost[:, i, :] = np.maximum(cost[:, i, :], 0.5)
        cost[:, :, j] = np.maximum(cost[:, :, j], 0.5)
        cost[:, i, j] = 0.0
    z = (-cost.astype(F) / F(epsilon)).astype(F)
    pitch = (m + 3) // 4 * 4
    z32 = np.full((batch, n, pitch), np.nan, F)
    z32[:, :, :m] = z
    dust = dust_of(epsilon, unused)
    Z = pad(z.astype(np.float64), dust)
    zero = np.zeros((batch, n + 1))
    return dict(z32=z32, pitch=pitch, Z=Z, dz=np.zeros_like(Z), dust=dust, c_row=zero, c_col=np.zeros((batch, m + 1)),
                epsilon=epsilon, unused=unused, shape=(batch, n, m))


# ------------------------------------------------------------------ bounds
def pair_shift(prob: dict, v_prev: np.ndarray) -> np.ndarray:
    """S of the bounded-shift row kernels, (batch,) fp64."""
    e = C.eps32(prob["epsilon"])
    G, D = 2.0 * prob["sqnorm_bound"] / e, prob["sqnorm_bound"] / e
    v_prev = np.asarray(v_prev, np.float64)
    wp = prob["c_col"][:, :-1] + v_prev[:, :-1]
    return np.maximum(wp.max(1) + G, prob["dust"] + v_prev[:, -1] + D)


def row_bound(prob: dict, v_prev: np.ndarray, bounded: bool = False, with_A: bool = False):
    """h of the row half-step from v_prev, (batch, n + 1).  bounded: the pair-wide shift for the rows below the dustbin
    row."""
    Z, c = prob["Z"], prob["c_row"]
    a = Z + np.asarray(v_prev, np.float64)[:, None, :] - c[:, :, None]
    M, S = np.abs(a).max(2), a.max(2)
    if bounded:
        S = S.copy()
        S[:, :-1] = pair_shift(prob, v_prev)[:, None]
    A = M + np.abs(S) + np.abs(c) + np.log(Z.shape[2])
    h = prob["dz"].max(2) + U * (C_A * A + C_L * Z.shape[2] + 8.0)
    return (h, A) if with_A else h


def col_bound(prob: dict, u: np.ndarray, v_old: np.ndarray | None = None, row_A: np.ndarray | None = None) -> np.ndarray:
    """h of the column half-step from u, (batch, m + 1).  v_old and row_A given: the probability form, whose exponents
    are the row half's; otherwise the log-domain form with the column maximum as shift."""
    Z = prob["Z"]
    a = Z + np.asarray(u, np.float64)[:, :, None]
    if v_old is None:
        A = np.abs(a).max(1) + np.abs(a.max(1)) + np.log(Z.shape[1])
    else:
        v_old = np.asarray(v_old, np.float64)
        A = np.abs(a + v_old[:, None, :]).max(1) + np.abs(v_old) + np.log(Z.shape[1]) + row_A.max(1)[:, None]
    return prob["dz"].max(1) + U * (C_A * A + C_L * Z.shape[1] + 8.0)


def step_bounds(prob: dict, v_prev, u, bounded: bool = False, prob_form: bool = True):
    """(row bound, column bound) of one iteration: u from v_prev, then v from u."""
    hr, A = row_bound(prob, v_prev, bounded, with_A=True)
    hc = col_bound(prob, u, v_prev, A) if prob_form else col_bound(prob, u)
    return hr, hc


def end_to_end_bound(prob: dict, iterations: int, bounded: bool = False, prob_form: bool = True, ref=None) -> float:
    """2 T max h, with h evaluated along the reference's own trajectory."""
    ref = ref or reference_duals(prob["Z"], iterations)
    v_prev, worst = np.zeros_like(ref[0][1]), 0.0
    for u, v in ref[:iterations]:
        hr, hc = step_bounds(prob, v_prev, u, bounded, prob_form)
        worst = max(worst, float(hr.max()), float(hc.max()))
        v_prev = v
    return 2.0 * iterations * worst


def p_ratio(prob: dict, p, u, v) -> float:
    """Worst (relative error of P against exp(Z + u + v) from the SAME fp32 duals) / bound; entries whose fp64 value is
    below 2^-126 must be at most 2^-126.  inf for a violation of the latter or a non-finite P."""
    Z = prob["Z"]
    p, u, v = np.asarray(p, np.float64), np.asarray(u, np.float64)[:, :, None], np.asarray(v, np.float64)[:, None, :]
    if not np.isfinite(p).all():
        return float("inf")
    t = Z + u + v
    want = np.exp(t)
    small = want < TINY
    if (p[small] > TINY).any():
        return float("inf")
    mag = np.maximum(np.maximum(np.abs(Z + u), np.abs(Z + v)), np.abs(t))
    bound = prob["dz"] + U * (C_P * mag + 4.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(small, 0.0, np.abs(p / want - 1.0) / bound)
    return float(r.max())


def worst(got, want, bound) -> float:
    """max |got - want| / bound (inf for a non-finite value)."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - want) / bound).max())


# ------------------------------------------------------------------ an fp32 evaluation, with planted errors
VARIANTS = ("rowmax", "bounded", "sequential", "prob_col")
ERRORS = ("drop_last_column", "exp12", "no_dustbin_row", "swap_logs", "stale_v", "extra_iteration", "column512_twice")


def sinkhorn_fp32(prob: dict, iterations: int, variant: str = "rowmax", error: str | None = None):
    """Sinkhorn on fp32(Z) in numpy float32.  Returns (history, p): history[k] = (u, v) after iteration k + 1, p from
    the last duals.  variant: "rowmax" (shift by the row / column maximum), "bounded" (rows shifted by pair_shift),
    "sequential" (every sum strictly left to right: np.cumsum, the worst order), "prob_col" (the column update in the
    probability domain: v_old + log nu - log sum_i exp(z + u + v_old)).  error: one of ERRORS, planted."""
    Z = prob["Z"].astype(F)
    b, n1, m1 = Z.shape
    n, m = n1 - 1, m1 - 1
    lmu, lnu = [x.astype(F) for x in log_marginals(b, n, m)]
    if error == "swap_logs":
        lmu[:, n], lnu[:, m] = lnu[:, m].copy(), lmu[:, n].copy()
    if error == "extra_iteration":
        iterations += 1

    def total(e, axis):
        if variant == "sequential":
            return np.take(np.cumsum(e, axis=axis, dtype=F), -1, axis=axis)
        return e.sum(axis=axis, dtype=F)

    def exp32(x, final=False):
        e = np.exp2((x * F(L2E)).astype(F)).astype(F)
        if error == "exp12" and not final:                           # the iteration's exponentials, not P's
            e = (e.view(np.uint32) & np.uint32(0xFFFFF000)).view(F)
        return e

    def lse32(x, axis, shift, kind):
        e = exp32((x - shift).astype(F))
        if error == "drop_last_column" and kind == "row":
            e[:, max(n - 3, 0):n, m - 1] = 0                       # the last real column, in the last band's rows
        if error == "no_dustbin_row" and kind == "col":
            e[:, n, :] = 0
        if error == "column512_twice" and kind == "row" and m > 512:
            e[:, :n, 512] *= F(2)
        return ((np.log2(total(e, axis)).astype(F) * F(LN2)).astype(F) + np.squeeze(shift, axis)).astype(F)

    u, v = np.zeros_like(lmu), np.zeros_like(lnu)
    if error == "stale_v":
        v = np.linspace(-0.5, 0.5, m1, dtype=F)[None, :].repeat(b, 0)      # what an earlier call left behind
    history = []
    for _ in range(iterations):
        a = (Z + v[:, None, :]).astype(F)
        shift = a.max(2, keepdims=True)
        if variant == "bounded":
            shift = shift.copy()
            shift[:, :n, 0] = pair_shift(prob, v).astype(F)[:, None]
        u = (lmu - lse32(a, 2, shift, "row")).astype(F)
        if variant == "prob_col":
            pr = exp32(((Z + u[:, :, None]).astype(F) + v[:, None, :]).astype(F))
            if error == "no_dustbin_row":
                pr[:, n, :] = 0
            v = ((v + lnu).astype(F) - (np.log2(total(pr, 1)).astype(F) * F(LN2)).astype(F)).astype(F)
        else:
            c = (Z + u[:, :, None]).astype(F)
            v = (lnu - lse32(c, 1, c.max(1, keepdims=True), "col")).astype(F)
        history.append((u.copy(), v.copy()))
    p = exp32(((Z + u[:, :, None]).astype(F) + v[:, None, :]).astype(F), final=True)
    return history, p
