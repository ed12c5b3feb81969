"""The Sinkhorn stage (K6, csrc/sinkhorn_dots.hip and csrc/sinkhorn.hip) against fp64 at every dispatch of its two entry
points, in the log domain and one half-step at a time: mi_sinkhorn_dots in its single-launch form, its batched row
kernels (bounded shift or row maxima, fp16-denormal read or conversion, one or two chunks per wave, the paired-wave
form), every stream schedule of 64 pairs and more, and mi_sinkhorn in its three fused forms and its two-pass kernels;
and the kernels that write P.

For every form and T in {1, 2, 7}: u(T) against the exact row half-step from the kernel's own v(T - 1) (a second call
with T - 1 iterations), v(T) against the exact column half-step from the kernel's own u(T), both to the a-priori bounds
of sinkhorn_oracle.py (nothing here is fitted to a measurement); the duals against the fp64 oracle end to end for the
iteration counts sinkhorn_oracle.E2E_ITERATIONS lists (1, 2, 3; 20 at the smallest epsilon); P relative to exp(Z + u + v) from the kernel's own duals, entry
by entry; helpers.p_close as everywhere else.

u, v, P and the workspace are filled with 0xFF bytes (NaN) before every call; u, v and P sit between guard rows, and the
workspace, handed over at exactly the size its query asks for, between guard bands, all of which must come back
untouched; the dots' row pitch is one granule wider than needed and columns m..pitch hold 0xFFFF.  Every call runs twice
and must repeat bit for bit; every dots call must leave the status word 0.  MI_REPORT=1 prints the worst error / bound
of each case.  Run with `-m gpu` on an MI355X."""
import functools
import os

import numpy as np
import pytest
import torch

import sinkhorn_oracle as S
from gpu_common import DEV, mods, twice, up  # noqa: F401  (mods: the module fixture)
from helpers import p_close

pytestmark = pytest.mark.gpu

MI_E_NULL, MI_E_SHAPE, MI_E_PARAM, MI_E_CAPACITY, MI_E_ALIGN = -1, -2, -3, -4, -5
MULTI_LAUNCH, NO_FORK, BELOW_1024 = 1, 2, 4
ITERATIONS = (1, 2, 7)


def _report(group, what, **ratios):
    if os.environ.get("MI_REPORT"):
        print(f"[sinkhorn {group}] {what}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


# ------------------------------------------------------------------ guarded, poisoned outputs
class _Out:
    """`rows` rows of `pitch` floats between two guard rows, every byte 0xFF (a NaN)."""

    def __init__(self, rows, pitch):
        self.full = torch.full(((rows + 2) * pitch,), -1, dtype=torch.int32, device=DEV).view(rows + 2, pitch)
        self.ptr = self.full[1].data_ptr()

    def read(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[0] == -1).all()), f"{what}: the row in front of the output was written"
        assert bool((self.full[-1] == -1).all()), f"{what}: the row behind the output was written"
        return self.full[1:-1].cpu().numpy().view(np.float32)


class _Work:
    """A workspace of exactly `nbytes` bytes (16-byte aligned) between two guard bands, every byte 0xFF."""
    GUARD = 4096

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.full = torch.full((nbytes + 2 * self.GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.body = self.full[self.GUARD: self.GUARD + nbytes]
        self.ptr = self.full.data_ptr() + self.GUARD
        assert self.ptr % 16 == 0

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[:self.GUARD] == 0xFF).all()), f"{what}: bytes in front of the workspace were written"
        assert bool((self.full[self.GUARD + self.nbytes:] == 0xFF).all()), f"{what}: bytes behind the workspace were written"


# ------------------------------------------------------------------ problems, references and device inputs (cached)
@functools.lru_cache(maxsize=None)
def _problem(form, batch, n, m, regime):
    prob = S.dots_problem(batch, n, m, regime) if form == "dots" else S.f32_problem(batch, n, m, regime)
    prob["ref"] = S.reference_duals(prob["Z"], 20 if regime == "floor" else max(ITERATIONS))
    return prob


@functools.lru_cache(maxsize=None)
def _dots_on_device(batch, n, m, normalized):
    """mi_cost_dots_bits of the problem's descriptors at a pitch one granule wider than needed, then 0xFFFF into the
    columns m..pitch: (dots, row_info, col_info, pitch), all read-only from here on."""
    from onnx_image_processing_amd import _native as N
    b1, b2 = S.bit_inputs(batch, n, m)
    words = b1.shape[-1]
    t1, t2 = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(DEV) for x in (b1, b2)]
    pitch = up(m, 8) + 8
    dots = torch.zeros((batch * n, pitch), dtype=torch.int16, device=DEV)
    ri, ci = torch.zeros((batch * n, 2), device=DEV), torch.zeros((batch * m, 2), device=DEV)
    N.call("mi_cost_dots_bits", t1.data_ptr(), t2.data_ptr(), batch, n, m, 32 * words, int(normalized), dots.data_ptr(), pitch,
           ri.data_ptr(), ci.data_ptr(), N.stream_ptr())
    torch.cuda.synchronize()
    dots[:, m:] = -1
    return dots, ri, ci, pitch


def _run_dots(N, prob, iterations, sqnorm_bound, flags, want_p):
    """One poisoned call of mi_sinkhorn_dots: (u, v[, p]) as numpy."""
    batch, n, m = prob["shape"]
    dots, ri, ci, pitch = _dots_on_device(batch, n, m, prob["normalized"])
    lib = N.load()
    wbytes = int(lib.mi_sinkhorn_dots_workspace_bytes(batch, n, m))
    assert wbytes > 0
    work = _Work(wbytes)
    u, v = _Out(batch, n + 1), _Out(batch, m + 1)
    p = _Out(batch * (n + 1), m + 1) if want_p else None
    N.call("mi_sinkhorn_dots", dots.data_ptr(), ri.data_ptr(), ci.data_ptr(), batch, n, m, pitch, float(prob["epsilon"]),
           float(prob["unused"]), float(sqnorm_bound), iterations, u.ptr, v.ptr, p.ptr if want_p else None, work.ptr,
           wbytes, flags, N.stream_ptr())
    out = (u.read("u"), v.read("v")) + ((p.read("p").reshape(batch, n + 1, m + 1),) if want_p else ())
    work.check("mi_sinkhorn_dots")
    status = lib.mi_sinkhorn_dots_status_word(work.ptr, batch, n, m)
    assert status is not None and work.ptr <= status <= work.ptr + wbytes - 4
    word = work.body[status - work.ptr:][:4].cpu().numpy().view(np.uint32)[0]
    assert word == 0, f"status word {word:#x}"
    if batch <= 8 and n <= 512 and m <= 512:
        # The form that ran.  For these extents the workspace holds, right in front of the status word, the granules the
        # bands of the single-launch kernel exchange (at least 8320 bytes; csrc/sinkhorn_dots.hip, dots_status_offset):
        # that form zeroes and then tags them, the multi-launch form never touches them.
        before = work.body[status - work.ptr - 4096: status - work.ptr]
        untouched = bool((before == 0xFF).all())
        assert untouched == bool(flags & MULTI_LAUNCH), \
            "the multi-launch form ran where the single-launch form was due" if untouched else "the single-launch form ran under MI_SOLVER_MULTI_LAUNCH"
    return out


def _run_f32(N, prob, iterations, workspace, want_p):
    """One poisoned call of mi_sinkhorn: (u, v[, p]) as numpy."""
    batch, n, m = prob["shape"]
    z = torch.from_numpy(prob["z32"]).to(DEV)
    wbytes = int(N.load().mi_sinkhorn_workspace_bytes(batch, n, m)) if workspace else 0
    assert (wbytes > 0) == (workspace and m <= 1024)
    work = _Work(wbytes) if wbytes else None
    u, v = _Out(batch, n + 1), _Out(batch, m + 1)
    p = _Out(batch * (n + 1), m + 1) if want_p else None
    N.call("mi_sinkhorn", z.data_ptr(), batch, n, m, prob["pitch"], prob["dust"], iterations, u.ptr, v.ptr,
           p.ptr if want_p else None, work.ptr if wbytes else None, wbytes, N.stream_ptr())
    out = (u.read("u"), v.read("v")) + ((p.read("p").reshape(batch, n + 1, m + 1),) if want_p else ())
    if wbytes:
        work.check("mi_sinkhorn")
    return out


# ------------------------------------------------------------------ the checks of one form on one problem
def _check_p(group, what, prob, u, v, p, iterations):
    r4 = S.p_ratio(prob, p, u, v)
    ur, vr = prob["ref"][iterations - 1]
    r5 = p_close(p, np.exp(prob["Z"] + ur[:, :, None] + vr[:, None, :]))[1]
    _report(group, f"{what} T {iterations}", P=r4, p_close=r5)
    assert r4 <= 1.0, f"{what}: P is off exp(Z + u + v) by {r4:.3g} times the bound"
    assert r5 <= 1.0, f"{what}: p_close, {r5:.3g} times 1e-4"


def _check_form(group, what, prob, run, bounded, prob_form, regime, iterations=ITERATIONS):
    """run(T, want_p) -> (u, v[, p]).  Checks 1 to 5 of the module docstring."""
    e2e = [t for t in S.E2E_ITERATIONS[regime]]
    need = sorted(set(iterations) | {t - 1 for t in iterations if t > 1} | set(e2e))
    last = max(iterations)
    got = {t: twice(f"{what} T {t}", lambda: run(t, t == last)) for t in need}
    Z = prob["Z"]
    for t in iterations:
        u, v = got[t][:2]
        v_prev = got[t - 1][1] if t > 1 else np.zeros_like(v)
        hr, hc = S.step_bounds(prob, v_prev, u, bounded, prob_form)
        rows, cols = S.worst(u, S.row_step(Z, v_prev), hr), S.worst(v, S.col_step(Z, u), hc)
        _report(group, f"{what} T {t}", rows=rows, columns=cols)
        assert rows <= 1.0, f"{what} T {t}: u is off its row half-step by {rows:.3g} times the bound"
        assert cols <= 1.0, f"{what} T {t}: v is off its column half-step by {cols:.3g} times the bound"
    for t in e2e:
        bound = S.end_to_end_bound(prob, t, bounded, prob_form, prob["ref"])
        ur, vr = prob["ref"][t - 1]
        r = max(S.worst(got[t][0], ur, bound), S.worst(got[t][1], vr, bound))
        _report(group, f"{what} T {t}", end_to_end=r)
        assert r <= 1.0, f"{what} T {t}: the duals are off the oracle's by {r:.3g} times 2 T max h"
    _check_p(group, what, prob, *got[last], last)


def _dots_forms(N, group, shape, variants, regimes):
    """variants: [(name, sqnorm bound given?, flags)]; every variant in every regime it applies to."""
    for regime in regimes:
        prob = _problem("dots", *shape, regime)
        for name, with_bound, flags in variants:
            sq = prob["sqnorm_bound"] if with_bound else 0.0
            bounded = S.bounded_shift(prob["epsilon"], sq)
            if regime in ("edge35", "edge30") and not with_bound:
                continue                                   # the edge is the bounded-shift dispatch's
            if regime == "edge35":
                assert bounded
            if regime == "edge30":
                assert not bounded
            what = f"{name} {shape} {regime}" + (" bounded shift" if bounded else " row maxima")
            _check_form(group, what, prob, lambda t, want_p: _run_dots(N, prob, t, sq, flags, want_p), bounded, True, regime)


DOTS_REGIMES = ("flat", "hamming", "standard", "edge35", "edge30")
FOUR_FORMS = [("fp16 read", True, MULTI_LAUNCH | BELOW_1024), ("converted", True, MULTI_LAUNCH),
              ("fp16 read", False, MULTI_LAUNCH | BELOW_1024), ("converted", False, MULTI_LAUNCH)]


# ------------------------------------------------------------------ A. the single-launch form
@pytest.mark.parametrize("shape", S.PERSIST_SHAPES)
def test_single_launch_form_vs_fp64(mods, shape):
    """sk_persist_kernel<true, 4> (sqnorm_bound given) and <false, 4> (0); _run_dots asserts that this form ran."""
    from onnx_image_processing_amd import _native as N
    _dots_forms(N, "A", shape, [("single launch", True, 0), ("single launch", False, 0)], DOTS_REGIMES)


# ------------------------------------------------------------------ B. the batched row kernel, m <= 512
@pytest.mark.parametrize("shape", S.BAND_SHAPES)
def test_band_kernel_four_forms_vs_fp64(mods, shape):
    """sk_band_dots_kernel<1, 4, 8, FAST, MIX, false>: bounded shift or row maxima, the dots read as fp16 denormals
    (MI_SOLVER_DOTS_BELOW_1024) or converted; and the flag with debug key 15 = 0, which converts after all."""
    from onnx_image_processing_amd import _native as N
    _dots_forms(N, "B", shape, FOUR_FORMS, DOTS_REGIMES)
    with N.debug_library() as lib:
        assert lib.mi_debug_set(15, 0) == 0
        _dots_forms(N, "B", shape, [("flag, key 15 = 0", True, MULTI_LAUNCH | BELOW_1024)], ("flat", "standard"))


@pytest.mark.parametrize("shape,key,value", [(s, k, x) for s in S.BATCH64_SHAPES
                                             for k, x in [(11, 0), (11, 1), (11, 2), (6, 1), (6, 2), (0, 0)]]
                         + [(S.THREE_PARTS_SHAPE, 6, 3), (S.THREE_PARTS_SHAPE, 6, 2)])
def test_band_kernel_batch_of_64_and_more_vs_fp64(mods, shape, key, value):
    """Every fixed stream schedule (key 11), one and two batch parts (key 6, on the two-helper schedule) and
    MI_SOLVER_NO_FORK (key 0: nothing set) at 64 and 65 pairs; three parts at 97 pairs -- launch_dots gives a part no
    fewer than 32 pairs, so 96 is the least that splits in three, and 97 makes the parts uneven (32, 32, 33: the offsets
    of u, v, the partials and the per-column arrays at b0 = 0, 32, 64).  Schedule 0 runs every regime, the others the
    flat and the standard one: the row kernels are those of the four-form test, what differs is where the parts run."""
    from onnx_image_processing_amd import _native as N
    with N.debug_library() as lib:
        if key:
            assert lib.mi_debug_set(key, value) == 0
        if key == 6:
            assert lib.mi_debug_set(11, 1) == 0
        flags = MULTI_LAUNCH | BELOW_1024 | (0 if key else NO_FORK)
        name = f"key {key} = {value}" if key else "no fork"
        regimes = DOTS_REGIMES if (key, value) in ((11, 0), (6, 3)) else ("flat", "standard")
        _dots_forms(N, "C", shape, [(name, True, flags), (name, False, flags)], regimes)


# ------------------------------------------------------------------ D, E. 512 < m <= 1024
@pytest.mark.parametrize("shape", S.WIDE_SHAPES)
def test_paired_wave_kernel_vs_fp64(mods, shape):
    """sk_band_dots_kernel<1, 4, 16, true, MIX, true> (bounded shift, debug key 16 = 1, the default); at eps = 0.03 the
    dispatch falls back to <2, 2, 8, false, MIX, false>."""
    from onnx_image_processing_amd import _native as N
    _dots_forms(N, "D", shape, FOUR_FORMS[:2], ("flat", "standard", "edge35", "edge30"))


@pytest.mark.parametrize("shape", S.WIDE_SHAPES)
def test_two_chunk_kernel_four_forms_vs_fp64(mods, shape):
    """sk_band_dots_kernel<2, 2, 8, FAST, MIX, false>: debug key 16 = 0 for the bounded shift, sqnorm_bound = 0 for row
    maxima."""
    from onnx_image_processing_amd import _native as N
    with N.debug_library() as lib:
        assert lib.mi_debug_set(16, 0) == 0
        _dots_forms(N, "E", shape, FOUR_FORMS, DOTS_REGIMES)


def test_row_maximum_kernel_at_the_smallest_epsilon_vs_fp64(mods):
    """MI_DOTS_MIN_EPSILON with 20 iterations: exponents of several hundred, duplicates whose unclamped cost is rounding
    noise divided by eps."""
    from onnx_image_processing_amd import _native as N
    shape = (2, 97, 130)
    prob = _problem("dots", *shape, "floor")
    assert not S.bounded_shift(prob["epsilon"], prob["sqnorm_bound"])
    for name, flags in (("fp16 read", MULTI_LAUNCH | BELOW_1024), ("single launch", 0)):
        _check_form("B", f"{name} {shape} floor", prob,
                    lambda t, want_p: _run_dots(N, prob, t, prob["sqnorm_bound"], flags, want_p), False, True, "floor", (20,))


# ------------------------------------------------------------------ F, G. mi_sinkhorn
@pytest.mark.parametrize("shape", S.FUSED_SHAPES)
@pytest.mark.parametrize("key4", [0, 1, 2])
def test_fused_forms_vs_fp64(mods, shape, key4):
    """launch_fused<1, 4, 8> (m <= 256), <2, 4, 8> (<= 512), <4, 2, 8> (<= 1024) in the lean probability form (debug
    key 4 = 0), the log-domain partials (1) and the first probability form (2)."""
    from onnx_image_processing_amd import _native as N
    with N.debug_library() as lib:
        assert lib.mi_debug_set(4, key4) == 0
        for regime in ("flat", "standard"):
            prob = _problem("f32", *shape, regime)
            _check_form("F", f"fused key 4 = {key4} {shape} {regime}", prob,
                        lambda t, want_p: _run_f32(N, prob, t, True, want_p), False, key4 != 1, regime)


@pytest.mark.parametrize("shape", S.TWO_PASS_SHAPES)
def test_two_pass_kernels_vs_fp64(mods, shape):
    """No workspace (or m > 1024, for which there is none): sk_row_kernel<1>, <2>, <4> and sk_row_generic_kernel with
    sk_col_kernel<1> (m odd), <2>, <4>."""
    from onnx_image_processing_amd import _native as N
    for regime in ("flat", "standard"):
        prob = _problem("f32", *shape, regime)
        _check_form("G", f"two-pass {shape} {regime}", prob, lambda t, want_p: _run_f32(N, prob, t, False, want_p), False, False,
                    regime)


# ------------------------------------------------------------------ H. the kernels that write P
@pytest.mark.parametrize("form,shape,key18", [("dots", (2, 97, 130), 0), ("dots", (2, 97, 130), 1), ("dots", (2, 70, 513), 1),
                                              ("f32", (2, 70, 200), 0), ("f32", (2, 70, 257), 1), ("f32", (2, 70, 513), 1),
                                              ("f32", (2, 40, 1027), 1)])
def test_p_writers_vs_fp64(mods, form, shape, key18):
    """sk_exp_dots_kernel (debug key 18 = 0), sk_exp_rows_kernel<1> (m <= 512), <2>; sk_exp_kernel (key 18 = 0, or
    m > 1024), sk_exp_rows_kernel<8> (m <= 512), <16>."""
    from onnx_image_processing_amd import _native as N
    with N.debug_library() as lib:
        assert lib.mi_debug_set(18, key18) == 0
        for regime in ("flat", "standard"):
            prob = _problem(form, *shape, regime)
            what = f"P {form} {shape} key 18 = {key18} {regime}"
            if form == "dots":
                run = lambda: _run_dots(N, prob, 7, prob["sqnorm_bound"], MULTI_LAUNCH, True)
            else:
                run = lambda: _run_f32(N, prob, 7, True, True)
            _check_p("H", what, prob, *twice(what, run), 7)


# ------------------------------------------------------------------ I. argument checks
def test_argument_checks(mods):
    """What no other test holds: epsilon below MI_DOTS_MIN_EPSILON, m > 1024 on the dots entry, unknown flag bits, a
    misaligned and a short workspace; nothing is written by a refused call."""
    from onnx_image_processing_amd import _native as N
    lib = N.load()
    batch, n, m = 2, 40, 56
    prob = _problem("dots", batch, n, m, "standard")
    dots, ri, ci, pitch = _dots_on_device(batch, n, m, True)
    wbytes = int(lib.mi_sinkhorn_dots_workspace_bytes(batch, n, m))
    assert int(lib.mi_sinkhorn_dots_workspace_bytes(batch, n, 1025)) == 0
    assert lib.mi_sinkhorn_dots_status_word(None, batch, n, m) is None
    work, u, v = _Work(wbytes + 16), _Out(batch, n + 1), _Out(batch, m + 1)
    base = dict(dots=dots.data_ptr(), ri=ri.data_ptr(), ci=ci.data_ptr(), batch=batch, n=n, m=m, pitch=pitch, epsilon=0.05,
                unused=1.0, sqnorm=1.0, iterations=3, u=u.ptr, v=v.ptr, p=None, work=work.ptr, wbytes=wbytes, flags=0,
                stream=N.stream_ptr())
    cases = [({"epsilon": 0.004999}, MI_E_PARAM), ({"epsilon": float("nan")}, MI_E_PARAM), ({"epsilon": 0.0}, MI_E_PARAM),
             ({"m": 1025, "pitch": 1032}, MI_E_PARAM), ({"flags": 8}, MI_E_PARAM), ({"flags": -1}, MI_E_PARAM),
             ({"flags": MULTI_LAUNCH | 16}, MI_E_PARAM), ({"work": work.ptr + 8}, MI_E_ALIGN),
             ({"work": work.ptr + 4}, MI_E_ALIGN), ({"wbytes": wbytes - 1}, MI_E_CAPACITY), ({"wbytes": 0}, MI_E_CAPACITY),
             ({"work": None}, MI_E_NULL), ({"iterations": 0}, MI_E_PARAM)]
    for change, code in cases:
        rc = lib.mi_sinkhorn_dots(*{**base, **change}.values())
        assert rc == code, f"mi_sinkhorn_dots with {change}: returned {rc}, expected {code}"
    torch.cuda.synchronize()
    assert bool((u.full == -1).all()) and bool((v.full == -1).all()), "a refused mi_sinkhorn_dots call wrote to an output"
    assert bool((work.full == 0xFF).all()), "a refused mi_sinkhorn_dots call wrote to the workspace"
    assert lib.mi_sinkhorn_dots(*{**base, "epsilon": S.MIN_EPSILON}.values()) == 0          # the floor itself is accepted
    assert np.isfinite(u.read("u")).all() and np.isfinite(v.read("v")).all()

    fp = _problem("f32", 2, 70, 200, "standard")
    fb, fn, fm = fp["shape"]
    z = torch.from_numpy(fp["z32"]).to(DEV)
    need = int(lib.mi_sinkhorn_workspace_bytes(fb, fn, fm))
    assert need > 0 and int(lib.mi_sinkhorn_workspace_bytes(fb, fn, 1025)) == 0
    # 512 < m <= 768 runs the four-chunk instance: band partials of 16-row bands, then 1024 + 4 floats of padded v per pair
    assert int(lib.mi_sinkhorn_workspace_bytes(2, 70, 513)) == 2 * 6 * 514 * 8 + 2 * (1024 + 4) * 4
    fwork, fu, fv = _Work(need + 16), _Out(fb, fn + 1), _Out(fb, fm + 1)
    fbase = dict(z=z.data_ptr(), batch=fb, n=fn, m=fm, pitch=fp["pitch"], dust=fp["dust"], iterations=3, u=fu.ptr, v=fv.ptr,
                 p=None, work=fwork.ptr, wbytes=need, stream=N.stream_ptr())
    for change, code in [({"wbytes": need - 1}, MI_E_CAPACITY), ({"wbytes": 0}, MI_E_CAPACITY), ({"iterations": 0}, MI_E_PARAM),
                         ({"pitch": fm - 4}, MI_E_ALIGN), ({"pitch": fp["pitch"] + 2}, MI_E_ALIGN), ({"z": z.data_ptr() + 4}, MI_E_ALIGN)]:
        rc = lib.mi_sinkhorn(*{**fbase, **change}.values())
        assert rc == code, f"mi_sinkhorn with {change}: returned {rc}, expected {code}"
    torch.cuda.synchronize()
    for out in (fu, fv):
        assert bool((out.full == -1).all()), "a refused mi_sinkhorn call wrote to an output"
    assert bool((fwork.full == 0xFF).all()), "a refused mi_sinkhorn call wrote to the workspace"
    # a workspace that is not 16-byte aligned is not an error for mi_sinkhorn: the two-pass form runs and never touches it
    want = _run_f32(N, fp, 3, False, False)
    assert lib.mi_sinkhorn(*{**fbase, "work": fwork.ptr + 8}.values()) == 0
    got = (fu.read("u"), fv.read("v"))
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "misaligned workspace: not the two-pass form's duals"
    assert bool((fwork.full == 0xFF).all()), "mi_sinkhorn wrote to a workspace it had to ignore"
