"""The test of the cost tests (no GPU): the fp64 reference and the derived bounds of cost_oracle.py, on the inputs
test_gpu_cost.py uses.  A correct fp32 evaluation stays inside the bounds; three wrong ones do not -- a lost k term,
inputs cut to a 10-bit mantissa (a reduced-precision matrix core), one descriptor's squared norm off by 1e-3 -- and
the last of them still passes p_close after Sinkhorn, which is why the cost stage needs a test of its own."""
import os

import numpy as np
import pytest

import cost_oracle as C
from helpers import p_close
from oracle import numpy_oracle as O

F32 = np.float32
FLOAT_SHAPES = [(37, 130, 7), (65, 63, 33), (130, 67, 256), (64, 300, 512)]
BIT_SHAPES = [(127, 129, 3), (130, 67, 16), (64, 40, 33), (33, 70, 128)]          # (n, m, words)
EPSILONS = (1.0, 0.05)


def _report(what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[cost_host] {what}: worst error / bound {ratio:.3g}")


def _z32(cost32, epsilon):
    return -cost32 / F32(epsilon)


def _cut_mantissa(x, bits=10):
    """float32 with the mantissa truncated to `bits` bits."""
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFFFFFF << (23 - bits) & 0xFFFFFFFF)).view(F32)


def _bits_epilogue_f32(b1, b2, normalized, epsilon):
    """The bits form evaluated in fp32 the way its definition reads: (z, row_info, col_info)."""
    dot = C.bit_dots(b1, b2).astype(F32)
    p1, p2 = C.unpack(b1).sum(-1).astype(F32), C.unpack(b2).sum(-1).astype(F32)
    if normalized:
        with np.errstate(divide="ignore"):
            i1 = np.where(p1 > 0, F32(1) / np.sqrt(p1), F32(0)).astype(F32)
            i2 = np.where(p2 > 0, F32(1) / np.sqrt(p2), F32(0)).astype(F32)
        n1, n2 = p1 * (i1 * i1), p2 * (i2 * i2)
    else:
        i1, i2, n1, n2 = np.ones_like(p1), np.ones_like(p2), p1, p2
    cross = dot * (i1[:, :, None] * i2[:, None, :])
    cost = np.maximum((n1[:, :, None] + n2[:, None, :]) - F32(2) * cross, F32(0))
    assert cost.dtype == F32
    return _z32(cost, epsilon), np.stack([i1, n1], -1), np.stack([i2, n2], -1)


@pytest.mark.parametrize("kind", ["unit", "sigmoid"])
@pytest.mark.parametrize("n,m,d", FLOAT_SHAPES)
@pytest.mark.parametrize("distance", [0, 1])
def test_fp32_reference_formula_is_inside_the_bound(n, m, d, distance, kind):
    a, b = C.float_inputs(kind, 2, n, m, d, distance)
    cost32 = O.cost_matrix(a, b, C.DIST_NAME[distance], F32)
    assert cost32.dtype == F32
    for epsilon in EPSILONS:
        z_ref, bound = C.float_reference(a, b, distance, epsilon)
        ratio = C.worst_ratio(_z32(cost32, epsilon), z_ref, bound)
        _report(f"{C.DIST_NAME[distance]} {kind} {(n, m, d)} eps {epsilon}", ratio)
        assert ratio <= 1.0
    k = max(1, min(n, m) // 4)
    z_ref, _ = C.float_reference(a, b, distance, 1.0)
    assert (np.abs(z_ref[:, np.arange(k), np.arange(k)]) < 1e-9).all(), "the planted duplicates do not have cost 0"


@pytest.mark.parametrize("kind", ["unit", "sigmoid"])
@pytest.mark.parametrize("n,m,d", FLOAT_SHAPES)
@pytest.mark.parametrize("distance", [0, 1])
def test_lost_term_and_short_mantissa_exceed_the_bound(n, m, d, distance, kind):
    a, b = C.float_inputs(kind, 2, n, m, d, distance)
    name = C.DIST_NAME[distance]
    for epsilon in EPSILONS:
        z_ref, bound = C.float_reference(a, b, distance, epsilon)
        lost = C.worst_ratio(_z32(O.cost_matrix(a[..., :-1], b[..., :-1], name, F32), epsilon), z_ref, bound)
        short = C.worst_ratio(_z32(O.cost_matrix(_cut_mantissa(a), _cut_mantissa(b), name, F32), epsilon), z_ref, bound)
        _report(f"mutants {name} {kind} {(n, m, d)} eps {epsilon}: lost term {lost:.3g}, 10-bit mantissa", short)
        assert lost > 1.0, "a dropped k term passes the bound"
        assert short > 1.0, "inputs cut to a 10-bit mantissa pass the bound"


@pytest.mark.parametrize("kind", ["unit", "sigmoid"])
@pytest.mark.parametrize("n,m,d", FLOAT_SHAPES[:3])
def test_wrong_norm_exceeds_the_bound_but_passes_sinkhorn(n, m, d, kind):
    """One descriptor's squared norm off by 1e-3 relative: an error of Z that is constant along a row.  The bound sees
    it; P after Sinkhorn (20 iterations, epsilon 0.05) does not -- the row normalisation absorbs it.  The descriptor is a
    matched one (row 0 has its duplicate in the other image), the case a matcher is run for: the row's mass sits in the
    core, and the only entry the shift moves relative to the others is a dustbin entry of ~exp(-1 / epsilon).  (On an
    unmatched row, whose mass sits in the dustbin, Sinkhorn does notice: p_close ratio 34 at (65, 63, 33).)"""
    epsilon = 0.05
    a, b = C.float_inputs(kind, 2, n, m, d, 0)
    i = 0
    n1 = (a * a).sum(-1, keepdims=True)
    n2 = (b * b).sum(-1, keepdims=True)
    n1[:, i] *= F32(1.0 + 1e-3)
    cost = np.maximum(n1 + np.swapaxes(n2, -1, -2) - F32(2) * (a @ np.swapaxes(b, -1, -2)), F32(0))
    assert cost.dtype == F32
    z_ref, bound = C.float_reference(a, b, 0, epsilon)
    ratio = C.worst_ratio(_z32(cost, epsilon), z_ref, bound)
    _report(f"wrong norm {kind} {(n, m, d)}", ratio)
    assert ratio > 1.0, "a wrong squared norm passes the bound"
    good = C.worst_ratio(_z32(O.cost_matrix(a, b, "l2", F32), epsilon), z_ref, bound)
    assert good <= 1.0
    exact = O.cost_matrix(a.astype(np.float64), b.astype(np.float64), "l2", np.float64)
    p_ref = O.sinkhorn_from_cost(exact, 20, epsilon, 1.0, dtype=np.float64)
    p_mut = O.sinkhorn_from_cost(cost.astype(np.float64), 20, epsilon, 1.0, dtype=np.float64)
    ok, worst = p_close(p_mut[:, :n, :m], p_ref[:, :n, :m])
    _report(f"wrong norm {kind} {(n, m, d)}: p_close ratio of the core P", worst)
    assert ok, f"Sinkhorn was expected to hide the wrong norm (p_close ratio {worst:.3g})"


@pytest.mark.parametrize("n,m,words", BIT_SHAPES)
@pytest.mark.parametrize("normalized", [True, False])
def test_fp32_bits_epilogue_is_inside_the_bound(n, m, words, normalized):
    b1, b2 = C.bit_inputs(2, n, m, words)
    for epsilon in EPSILONS:
        z, ri, ci = _bits_epilogue_f32(b1, b2, normalized, epsilon)
        z_ref, bound = C.bit_reference(b1, b2, normalized, epsilon)
        ratio = C.worst_ratio(z, z_ref, bound)
        _report(f"bits {32 * words} {(n, m)} normalized {normalized} eps {epsilon}", ratio)
        assert ratio <= 1.0
    for info, bits in ((ri, b1), (ci, b2)):
        inv_err, nrm_err = C.info_errors(info, bits, normalized)
        assert inv_err <= 2.0 and nrm_err <= 5.0, (inv_err, nrm_err)
    # what the planted descriptors are there for
    dots = C.bit_dots(b1, b2)
    assert dots[0, 0, 0] == 32 * words and (dots[:, 2, 2] == 0).all() and (dots[0, 1] == 0).all()
    z_ref, _ = C.bit_reference(b1, b2, normalized, 1.0)
    assert (np.abs(z_ref[:, 4, 4]) < 1e-9).all(), "the planted duplicates do not have cost 0"


@pytest.mark.parametrize("normalized", [True, False])
def test_bits_lost_term_exceeds_the_bound(normalized):
    """The last word of the dot product dropped."""
    n, m, words = 130, 67, 16
    b1, b2 = C.bit_inputs(2, n, m, words)
    cut = b1.copy()
    cut[..., -1] = 0
    dot_lost = C.bit_dots(cut, b2)
    assert (dot_lost != C.bit_dots(b1, b2)).any()
    p1, p2 = C.unpack(b1).sum(-1), C.unpack(b2).sum(-1)
    s1 = np.where(p1 > 0, 1 / np.sqrt(np.maximum(p1, 1)), 0.0) if normalized else np.ones_like(p1)
    s2 = np.where(p2 > 0, 1 / np.sqrt(np.maximum(p2, 1)), 0.0) if normalized else np.ones_like(p2)
    cost = (p1 * s1 * s1)[:, :, None] + (p2 * s2 * s2)[:, None, :] - 2 * dot_lost * s1[:, :, None] * s2[:, None, :]
    z_ref, bound = C.bit_reference(b1, b2, normalized, 0.05)
    assert C.worst_ratio((-np.maximum(cost, 0) / C.eps32(0.05)).astype(F32), z_ref, bound) > 1.0


def test_scale_and_norm_of_every_population_count():
    """(1 / sqrt(p), p / sqrt(p)^2) in correctly rounded fp32 for every p in 1..4096: within 2 u and 5 u."""
    p = np.arange(1, 4097).astype(F32)
    inv = F32(1) / np.sqrt(p)
    nrm = p * (inv * inv)
    assert inv.dtype == F32 and nrm.dtype == F32
    ref = 1.0 / np.sqrt(np.arange(1, 4097, dtype=np.float64))
    assert (np.abs(inv.astype(np.float64) - ref) <= 2 * C.U * ref).all()
    assert (np.abs(nrm.astype(np.float64) - 1.0) <= 5 * C.U).all()
