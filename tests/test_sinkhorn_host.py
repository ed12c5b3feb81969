"""tests/sinkhorn_oracle.py against itself, without a GPU: four correct fp32 evaluations of Sinkhorn stay inside the
one-step, end-to-end and P bounds at the shapes and regimes tests/test_gpu_sinkhorn.py runs; seven planted errors fall
outside one; and the conditions on the reference alone without which the GPU tests could pass vacuously.

What helpers.p_close (|dP| <= 1e-4) makes of the planted errors, at the case each is shown on below (worst error /
bound, below 1 passes), against the log-domain check that catches it:
    drop_last_column   40 x 1500 flat      p_close passes    one-step rows fail
    exp12              40 x 1500 flat      p_close passes    one-step rows fail
    no_dustbin_row     40 x 56 flat        p_close fails     one-step columns fail
    swap_logs          40 x 1500 flat      p_close fails     one-step rows (the dustbin row) fail
    stale_v            97 x 130 flat, T=1  p_close fails     end to end fails
    extra_iteration    97 x 130 standard, T=2 p_close fails     end to end fails
    column512_twice    33 x 1000 flat      p_close passes    one-step rows fail
test_planted_errors_fall_outside_a_bound asserts the column "p_close" too (for the row-maximum evaluation; with the
probability-domain column update the truncated exponentials bias v as well, and p_close does see exp12 there), so the
table cannot go stale."""
import numpy as np
import pytest

import sinkhorn_oracle as S
from helpers import p_close


def _problem(form, batch, n, m, regime):
    return S.dots_problem(batch, n, m, regime) if form == "dots" else S.f32_problem(batch, n, m, regime)


def _small(batch, n, m):
    return min(batch, 2 if min(n, m) >= 8 else 3)          # the host tests need the shape, not the batch


def _ratios(prob, history, p, iterations, bounded, prob_form):
    """Worst error / bound of the last iteration's two half-steps, of the duals end to end, of P; and p_close.
    history: of a run asked for `iterations`; its last entry is what the run returns."""
    Z = prob["Z"]
    u, v = history[-1]
    v_prev = history[-2][1] if len(history) > 1 else np.zeros_like(v)
    hr, hc = S.step_bounds(prob, v_prev, u, bounded, prob_form)
    ref = S.reference_duals(Z, iterations)
    e2e = S.end_to_end_bound(prob, iterations, bounded, prob_form, ref)
    ur, vr = ref[-1]
    p_ref = np.exp(Z + ur[:, :, None] + vr[:, None, :])
    return dict(row=S.worst(u, S.row_step(Z, v_prev), hr), col=S.worst(v, S.col_step(Z, u), hc),
                e2e=max(S.worst(u, ur, e2e), S.worst(v, vr, e2e)), p=S.p_ratio(prob, p, u, v), p_close=p_close(p, p_ref)[1])


def _cases():
    out = []
    for form, shapes, regimes in (("dots", S.DOTS_SHAPES, ("flat", "hamming", "standard", "edge35", "edge30")),
                                  ("f32", S.F32_SHAPES, ("flat", "standard"))):
        for batch, n, m in dict.fromkeys((_small(*s), s[1], s[2]) for s in shapes):
            for regime in regimes if n * m <= 64 * 1024 else regimes[:1]:
                out.append((form, batch, n, m, regime, 3))
    out.append(("dots", 2, 97, 130, "floor", 20))
    return out


@pytest.mark.parametrize("form,batch,n,m,regime,iterations", _cases())
def test_correct_fp32_evaluations_stay_inside_the_bounds(form, batch, n, m, regime, iterations):
    prob = _problem(form, batch, n, m, regime)
    can_bound = form == "dots" and S.bounded_shift(prob["epsilon"], prob["sqnorm_bound"])
    for variant in S.VARIANTS:
        if variant == "bounded" and not can_bound:
            continue
        history, p = S.sinkhorn_fp32(prob, iterations, variant)
        r = _ratios(prob, history, p, iterations, variant == "bounded", variant == "prob_col")
        for name in ("row", "col", "e2e", "p"):
            assert r[name] <= 1.0, f"{variant}: {name} error {r[name]:.3g} times its bound"
        assert r["p_close"] <= 1.0


PLANTED = [  # error, form, (batch, n, m), regime, T, the check that must fail, whether p_close passes
    ("drop_last_column", "f32", (2, 40, 1500), "flat", 3, "row", True),
    ("exp12", "f32", (2, 40, 1500), "flat", 3, "row", True),
    ("no_dustbin_row", "dots", (2, 40, 56), "flat", 3, "col", False),
    ("swap_logs", "f32", (2, 40, 1500), "flat", 3, "row", False),
    ("stale_v", "dots", (2, 97, 130), "flat", 1, "e2e", False),
    ("extra_iteration", "dots", (2, 97, 130), "standard", 2, "e2e", False),
    ("column512_twice", "dots", (1, 33, 1000), "flat", 3, "row", True),
]


@pytest.mark.parametrize("error,form,shape,regime,iterations,check,p_close_passes", PLANTED)
def test_planted_errors_fall_outside_a_bound(error, form, shape, regime, iterations, check, p_close_passes):
    prob = _problem(form, *shape, regime)
    for variant in ("rowmax", "prob_col"):
        history, p = S.sinkhorn_fp32(prob, iterations, variant, error)
        r = _ratios(prob, history, p, iterations, False, variant == "prob_col")
        assert r[check] > 1.0, f"{error} ({variant}) passes the {check} check: {r}"
        if variant == "rowmax":
            assert (r["p_close"] <= 1.0) == p_close_passes, f"{error}: p_close ratio {r['p_close']:.3g}"


def test_every_planted_error_is_covered():
    assert sorted(e[0] for e in PLANTED) == sorted(S.ERRORS)


# ------------------------------------------------------------------ preconditions on the reference alone
def _e2e_cases():
    for form, shapes, regimes in (("dots", S.DOTS_SHAPES, ("flat", "hamming", "standard", "edge35", "edge30")),
                                  ("f32", S.F32_SHAPES, ("flat", "standard"))):
        for shape in shapes:
            for regime in regimes:
                yield form, shape, regime


@pytest.mark.parametrize("form,shape,regime", list(_e2e_cases()))
def test_one_iteration_moves_the_duals_ten_end_to_end_bounds(form, shape, regime):
    """At the counts of E2E_DISTINCT; otherwise T - 1 or T + 1 iterations would pass the end-to-end check of T."""
    batch, n, m = shape
    prob = _problem(form, _small(*shape), n, m, regime)
    ref = S.reference_duals(prob["Z"], 3)
    can_bound = form == "dots" and S.bounded_shift(prob["epsilon"], prob["sqnorm_bound"])
    for t in S.E2E_DISTINCT[regime]:
        bound = max(S.end_to_end_bound(prob, t, bounded, True, ref) for bounded in ({False, can_bound}))
        before = ref[t - 2][0] if t > 1 else np.zeros_like(ref[0][0])
        moved = float(np.abs(ref[t - 1][0] - before).max())
        assert moved >= 10.0 * bound, f"T = {t}: u moves {moved:.3g}, the bound is {bound:.3g}"


# 1 / L >= 10 u (C_A A + C_L L + 8) needs L (L + 8) <= 2^24 / 10 even with A = 0: L <= 1290.  The row half of m = 1500
# (L = 1501) cannot have it with C_L = 1, whatever the inputs: there an element's share is required to be 6 bounds.
FLAT_MARGIN = lambda L: 10.0 if L <= 1290 else 6.0


@pytest.mark.parametrize("form,shape", [("dots", s) for s in S.DOTS_SHAPES] + [("f32", s) for s in S.F32_SHAPES])
def test_flat_regime_an_element_outweighs_the_one_step_bound(form, shape):
    """In the flat regime a term left out of a sum of L moves the result by about 1 / L: ten one-step bounds (six at
    L = 1501, see FLAT_MARGIN), so a lost element cannot hide in the rounding allowance."""
    batch, n, m = shape
    for regime in ("flat", "hamming") if form == "dots" else ("flat",):
        prob = _problem(form, _small(*shape), n, m, regime)
        ref = S.reference_duals(prob["Z"], 3)
        v_prev = np.zeros_like(ref[0][1])
        for u, v in ref:
            for bounded in {False, form == "dots"}:
                hr, hc = S.step_bounds(prob, v_prev, u, bounded, True)
                assert 1.0 / (m + 1) >= FLAT_MARGIN(m + 1) * hr.max(), (regime, 1.0 / (m + 1) / hr.max())
                assert 1.0 / (n + 1) >= FLAT_MARGIN(n + 1) * hc.max(), (regime, 1.0 / (n + 1) / hc.max())
            v_prev = v


@pytest.mark.parametrize("form,shape", [("dots", s) for s in S.DOTS_SHAPES] + [("f32", s) for s in S.F32_SHAPES])
def test_planted_matches_are_the_largest_of_their_row_and_column(form, shape):
    batch, n, m = shape
    planted = S.plants(n, m)
    for regime in ("flat", "hamming", "standard", "edge35", "edge30") if form == "dots" else ("flat", "standard"):
        prob = _problem(form, _small(*shape), n, m, regime)
        u, v = S.reference_duals(prob["Z"], 7)[-1]
        p = np.exp(prob["Z"] + u[:, :, None] + v[:, None, :])[:, :n, :m]
        for i, j in planted:
            others_r, others_c = np.delete(p[:, i, :], j, axis=1), np.delete(p[:, :, j], i, axis=1)
            assert (p[:, i, j] > others_r.max(1)).all() and (p[:, i, j] > others_c.max(1)).all(), (regime, i, j)
    if min(n, m) >= 8:
        assert (0, 0) in planted and (n - 1, m - 1) in planted            # the latter sits in the last band
        assert S.band_plant(n, m) is None or S.band_plant(n, m) in planted
        assert ((31, 511) in planted) == (n > 32 and m > 512) and ((32, 512) in planted) == (n > 33 and m > 513)


@pytest.mark.parametrize("group", ["PERSIST_SHAPES", "BAND_SHAPES", "BATCH64_SHAPES", "WIDE_SHAPES", "FUSED_SHAPES",
                                   "TWO_PASS_SHAPES"])
def test_every_group_of_forms_has_a_match_inside_the_last_partial_band(group):
    """The plant away from the band's last row exists only where n - 1 is no multiple of 16: every group of forms must
    have a shape that carries it."""
    carrying = [(n, m) for _, n, m in getattr(S, group) if S.band_plant(n, m) in S.plants(n, m) and S.band_plant(n, m)]
    assert carrying, group
    for n, m in carrying:
        i, j = S.band_plant(n, m)
        assert (n - 1) // 16 * 16 <= i < n - 1 and j < m - 1


def test_end_to_end_counts():
    for regime in S.REGIMES:
        assert set(S.E2E_DISTINCT[regime]) <= set(S.E2E_ITERATIONS[regime])
        assert regime == "floor" or S.E2E_ITERATIONS[regime] == (1, 2, 3)
