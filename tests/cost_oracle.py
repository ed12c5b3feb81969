"""fp64 reference of the cost stage (K5, csrc/cost.hip) with a-priori fp32 error bounds, and the inputs both cost test
files run on.  Plain numpy, no GPU.

Nothing here repeats the kernels' arithmetic: the reference is the exact quantity in fp64, and a bound counts the fp32
roundings that the DEFINITION of the result allows, in any summation order, fused or not.  u = 2^-24 is the unit
roundoff of fp32; the kernels divide by fp32(epsilon), so the reference divides by that number too.

L2 (float descriptors).  cost = |a|^2 + |b|^2 - 2 a.b.  A sum of d products computed in fp32 in any order carries at
    most gamma_d = d u / (1 - d u) times the sum of the products' magnitudes, so the three sums carry
    gamma_d (|a|^2 + |b|^2 + 2 sum_k |a_k b_k|).  The add, the subtraction and the division add one rounding each on
    a quantity no larger than S = |a|^2 + |b|^2 + 2 sum_k |a_k b_k| (the product with 2 is exact), and one unit is
    spare.  First order: (d + 4) u S, and the factor 1.01 covers the higher-order terms of gamma (d u < 1e-4 for
    every d <= 1024).  The clamp at 0 moves a negative computed cost towards the exact one, which is >= 0: it can
    only reduce the error.
L1.  cost = sum_k |a_k - b_k|: one rounding per difference, d - 1 additions, one division: (d + 3) u sum_k |a_k - b_k|
    with a unit to spare, times 1.01.
bits, normalised.  dot = popcount(a & b) is an integer, exact.  With p = popcount:
        inv = 1 / sqrt(p)           2 roundings (sqrt, divide)                         relative 2 u
        nrm = p * (inv * inv)       2 * 2 u from inv, the product, the product by p    relative 6 u worst case; the
                                    tests hold it to 5 u, which test_cost_host.py checks for EVERY p in 1..4096 with
                                    correctly rounded fp32 sqrt / divide / multiply
        cross = dot * (inv_a * inv_b)       2 u + 2 u, two products                     relative 6 u
        cost = max((nrm_a + nrm_b) - 2 * cross, 0)      one add (norm terms only), one subtraction
        z = -cost / eps                                 one division
    so the norm terms carry at most 6 + 1 + 1 + 1 = 9 roundings and the cross term 6 + 1 + 1 = 8 (the product with 2
    is exact).  BITS_K = 10 leaves a unit for the second-order terms: bound = 10 u (nrm_a + nrm_b + 2 cross) / eps.
bits, Hamming.  Every intermediate is an integer below 2^24, the cost is exact and z carries the division's rounding
    alone: 2 u |z|."""
from __future__ import annotations

import numpy as np

from oracle import numpy_oracle as O

U = 2.0 ** -24
BITS_K = 10
DIST_NAME = {0: "l2", 1: "l1"}          # MI_DIST_L2, MI_DIST_L1


def eps32(epsilon: float) -> float:
    return float(np.float32(epsilon))


# ------------------------------------------------------------------ float descriptors
def float_inputs(kind: str, batch: int, n: int, m: int, d: int, distance: int):
    """desc1 (batch, n, d), desc2 (batch, m, d) float32, seeded by the shape.  kind "unit": Gaussian rows of norm 1;
    "sigmoid": raw sigmoid rows in (0, 1) (norms ~ sqrt(d / 3), cost a small difference of large numbers).  Planted:
    a block of rows of desc2 equal to rows of desc1 (exact cost 0: the clamp), an all-zero descriptor on each side and,
    for L2, one descriptor on each side scaled by 100.  Shapes too small for that (n or m below 4) carry one plant per
    batch member instead: use batch 3 there."""
    rng = np.random.default_rng([n, m, d, distance, 0 if kind == "unit" else 1])
    a = rng.standard_normal((batch, n, d))
    b = rng.standard_normal((batch, m, d))
    if kind == "unit":
        a /= np.linalg.norm(a, axis=-1, keepdims=True)
        b /= np.linalg.norm(b, axis=-1, keepdims=True)
    elif kind == "sigmoid":
        a = 1.0 / (1.0 + np.exp(-2.0 * a))
        b = 1.0 / (1.0 + np.exp(-2.0 * b))
    else:
        raise ValueError(kind)
    a, b = a.astype(np.float32), b.astype(np.float32)
    if n >= 4 and m >= 4:
        k = max(1, min(n, m) // 4)
        b[:, :k] = a[:, :k]
        a[0, n - 1] = 0.0
        b[-1, m - 1] = 0.0
        if distance == 0:
            a[-1, n - 2] *= np.float32(100.0)
            b[0, m - 2] *= np.float32(100.0)
    else:
        b[0, 0] = a[0, 0]
        if batch > 1:
            a[1, 0] = 0.0
        if batch > 2 and distance == 0:
            b[2, 0] *= np.float32(100.0)
    return a, b


def float_reference(a: np.ndarray, b: np.ndarray, distance: int, epsilon: float):
    """(z_ref, bound), both (batch, n, m) fp64, for float32 descriptors a, b."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    d = a.shape[-1]
    e = eps32(epsilon)
    cost = O.cost_matrix(a64, b64, DIST_NAME[distance], np.float64)
    z_ref = -cost / e
    if distance == 0:
        na = (a64 * a64).sum(-1)[:, :, None]
        nb = (b64 * b64).sum(-1)[:, None, :]
        cross = np.abs(a64) @ np.swapaxes(np.abs(b64), -1, -2)
        bound = 1.01 * (d + 4) * U * (na + nb + 2.0 * cross) / e
    else:
        bound = 1.01 * (d + 3) * U * cost / e          # the exact cost IS sum_k |a_k - b_k|
    return z_ref, bound


# ------------------------------------------------------------------ packed hard bits
def bit_inputs(batch: int, n: int, m: int, words: int):
    """bits1 (batch, n, words), bits2 (batch, m, words) uint32, seeded by the shape: random words, every seventh
    descriptor thinned to a quarter of the bits (populations differ), and planted an all-ones descriptor on each side, an
    empty one on each side, a complement pair (dot 0) and a block of duplicates.  n or m below 8: one plant per batch
    member (use batch 3)."""
    rng = np.random.default_rng([n, m, words, 7])
    draw = lambda *s: rng.integers(0, 2 ** 32, size=s, dtype=np.uint64).astype(np.uint32)
    b1, b2 = draw(batch, n, words), draw(batch, m, words)
    b1[:, 5::7] &= draw(*b1[:, 5::7].shape)
    b2[:, 6::7] &= draw(*b2[:, 6::7].shape)
    ones = np.uint32(0xFFFFFFFF)
    if n >= 8 and m >= 8:
        k = max(1, min(n, m) // 4)
        b2[:, 4:4 + k] = b1[:, 4:4 + k]
        b1[0, 0], b2[0, 0] = ones, ones
        b1[0, 1], b2[-1, 1] = 0, 0
        b2[:, 2] = ~b1[:, 2]
        b1[-1, n - 1], b2[0, m - 1] = ones, 0
    else:
        b1[0, 0], b2[0, 0] = ones, ones
        if batch > 1:
            b1[1, 0] = 0
        if batch > 2:
            b2[2, 0] = ~b1[2, 0]
    return b1, b2


def unpack(bits: np.ndarray) -> np.ndarray:
    """(..., words) uint32 -> (..., 32 * words) fp64 of 0 / 1."""
    w = np.ascontiguousarray(bits, np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(*w.shape[:-1], -1).astype(np.float64)


def bit_dots(b1: np.ndarray, b2: np.ndarray) -> np.ndarray:
    """popcount(a_i & b_j), (batch, n, m) int64: sums of at most 4096 products of 0 / 1, exact in fp64."""
    return np.rint(unpack(b1) @ np.swapaxes(unpack(b2), -1, -2)).astype(np.int64)


def bit_reference(b1: np.ndarray, b2: np.ndarray, normalized: bool, epsilon: float):
    """(z_ref, bound) for packed descriptors, both (batch, n, m) fp64."""
    e = eps32(epsilon)
    f1, f2 = unpack(b1), unpack(b2)
    if not normalized:
        z_ref = -O.cost_matrix(f1, f2, "l2", np.float64) / e
        return z_ref, 2.0 * U * np.abs(z_ref)
    p1, p2 = f1.sum(-1, keepdims=True), f2.sum(-1, keepdims=True)
    d1, d2 = f1 / np.maximum(np.sqrt(p1), 1e-12), f2 / np.maximum(np.sqrt(p2), 1e-12)
    z_ref = -O.cost_matrix(d1, d2, "l2", np.float64) / e
    nrm1, nrm2 = (p1 > 0).astype(np.float64), (p2 > 0).astype(np.float64)
    cross = d1 @ np.swapaxes(d2, -1, -2)
    bound = BITS_K * U * (nrm1 + np.swapaxes(nrm2, -1, -2) + 2.0 * cross) / e
    return z_ref, bound


def info_errors(info: np.ndarray, bits: np.ndarray, normalized: bool):
    """The per-descriptor (scale, squared norm) pairs `info` (batch, k, 2) float32 against fp64.  Asserts what must hold
    exactly -- (0, 0) for an empty descriptor, (1, pop) for Hamming -- and returns the worst relative errors
    (inv, nrm) in units of u over the non-empty descriptors, for the caller to hold against 2 and 5."""
    pop = unpack(bits).sum(-1)
    assert info.shape == pop.shape + (2,) and info.dtype == np.float32, (info.shape, info.dtype)
    if not normalized:
        assert np.array_equal(info[..., 0], np.ones_like(pop, np.float32)), "Hamming scale is not exactly 1"
        assert np.array_equal(info[..., 1].astype(np.float64), pop), "Hamming squared norm is not exactly the popcount"
        return 0.0, 0.0
    empty = pop == 0
    assert np.array_equal(info[empty], np.zeros((int(empty.sum()), 2), np.float32)), "empty descriptor is not (0, 0)"
    if empty.all():
        return 0.0, 0.0
    inv_ref = 1.0 / np.sqrt(pop[~empty])
    got = info[~empty].astype(np.float64)
    inv_err = float((np.abs(got[:, 0] - inv_ref) / inv_ref).max() / U)
    nrm_err = float(np.abs(got[:, 1] - 1.0).max() / U)
    return inv_err, nrm_err


def worst_ratio(z: np.ndarray, z_ref: np.ndarray, bound: np.ndarray) -> float:
    """max |z - z_ref| / bound over the entries (0 where both are 0; inf where an error meets a zero bound or z is not
    finite)."""
    z = np.asarray(z, np.float64)
    if not np.isfinite(z).all():
        return float("inf")
    err = np.abs(z - z_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max())
