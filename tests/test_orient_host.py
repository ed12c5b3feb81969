"""The test of the orientation tests (no GPU): the fp64 reference and the bounds of orient_oracle.py on the inputs
test_gpu_orient.py uses.  The reference agrees with numpy_oracle.angle_map; an fp32 evaluation of each kernel's
arithmetic, in two summation orders, is exact on the integer cases and inside the bound on the Gaussian ones, so the
bars can be met; no textured case has more than 1 % ill-conditioned entries; a kernel with a short halo, a lost tap, a
missing attain mask or one image set read twice is outside them; and the entry points refuse bad arguments before any
launch."""
import ctypes
import os

import numpy as np
import pytest

import orient_oracle as R
from oracle import numpy_oracle as O

F32 = np.float32
MI_E_NULL, MI_E_SHAPE, MI_E_PARAM = -1, -2, -3
KP_GAUSS = {15: 2.5, 13: 2.0, 17: 3.0, 31: 5.0}             # test_gpu_orient.py's keypoint cases
KP_HW = (17, 65)


def _report(what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[orient_host] {what}: worst error / bound {ratio:.3g}")


# ------------------------------------------------------------------ fp32 emulations
def _moments_f32(img, wk, ps, order, shift=0, drop=None):
    """The two moments in fp32.  order "rows": one accumulator per pixel, taps row by row (angle_map_kernel); "lanes": 64
    partial sums over taps lane, lane + 64, ... and a butterfly over the lanes (patch_angle).  shift / drop build the
    wrong kernels of the mutant tests: a tile filled one pixel off, a tap left out."""
    n, h, w = img.shape
    half = ps // 2
    e = np.pad(img.astype(F32), ((0, 0), (half + 1, half + 1), (half + 1, half + 1)))
    taps = [(dy, dx) for dy in range(ps) for dx in range(ps)]
    flat = wk.reshape(2, -1).astype(F32)
    lanes = 64 if order == "lanes" else 1
    acc = np.zeros((2, lanes, n, h, w), F32)
    for i, (dy, dx) in enumerate(taps):
        if i == drop:
            continue
        win = e[:, 1 + shift + dy:1 + shift + dy + h, 1 + shift + dx:1 + shift + dx + w]
        acc[0, i % lanes] += flat[0, i] * win
        acc[1, i % lanes] += flat[1, i] * win
    o = lanes // 2
    while o:
        acc = acc + acc[:, np.arange(lanes) ^ o]
        o //= 2
    assert acc.dtype == F32
    return acc[0, 0], acc[1, 0]


def _atan2_f32(m01, m10):
    """a correctly rounded atan2f: what the bound's ATAN2F_A term allows for, and more"""
    return np.arctan2(m01.astype(np.float64), m10.astype(np.float64)).astype(F32)


def _dense_cases():
    for ps in R.INT_PATCHES:
        for shape in R.INT_SHAPES:
            yield f"int {shape} ps {ps}", R.int_case(*shape, ps), ps, False
        yield f"isolated pixels ps {ps}", R.seam_case(ps), ps, False
    for ps, sigma in R.GAUSS:
        for shape in R.GAUSS_SHAPES:
            yield f"gauss {shape} ps {ps}", R.gauss_case(*shape, ps, sigma), ps, True
    for ps, sigma in KP_GAUSS.items():
        yield f"gauss keypoint image ps {ps}", R.gauss_case(3, *KP_HW, ps, sigma), ps, True


# ------------------------------------------------------------------ the reference is the reference
@pytest.mark.parametrize("ps,sigma", R.GAUSS)
def test_moments_agree_with_numpy_oracle(ps, sigma):
    img = R.textured(2, 17, 65)
    wk = O.moment_kernels(ps, sigma)
    m10, m01, s10, s01 = R.moments(img, wk, ps)
    ang, o10, o01 = O.angle_map(img[:, None], ps, sigma, return_moments=True)
    np.testing.assert_allclose(m10, o10, rtol=1e-13, atol=1e-9)
    np.testing.assert_allclose(m01, o01, rtol=1e-13, atol=1e-9)
    assert np.array_equal(np.arctan2(m01, m10).astype(F32), ang[:, 0])
    assert (s10 >= np.abs(m10)).all() and (s01 >= np.abs(m01)).all()
    # the module's buffer (torch) and the oracle's (numpy) are the same weights up to exp's last bits
    np.testing.assert_allclose(R.gauss_weights(ps, sigma), wk, rtol=4 * R.U * 2, atol=0)


def test_nearest_pixel_is_the_oracles_chain():
    h, w = 17, 65
    kp = R.keypoints(3, 13, h, w, 7)
    cy, cx = R.nearest_pixel(kp, h, w)
    assert cy.min() == 0 and cy.max() == h - 1 and cx.min() == 0 and cx.max() == w - 1
    field = np.arange(3 * h * w, dtype=F32).reshape(3, 1, h, w)
    assert np.array_equal(O.sample_nearest(field, kp), field[np.arange(3)[:, None], 0, cy, cx])
    ints = np.stack(np.meshgrid(np.arange(h), np.arange(w), indexing="ij"), -1).reshape(1, -1, 2).astype(F32)
    cy, cx = R.nearest_pixel(ints, h, w)
    assert np.array_equal(cy[0], ints[0, :, 0]) and np.array_equal(cx[0], ints[0, :, 1])
    assert R.nearest_pixel(np.array([[[0.3, -5.0]]], F32), 1, 1) == (0, 0)


def test_keypoint_lists_hold_the_awkward_points():
    h, w = KP_HW
    kp = R.keypoints(3, 13, h, w, 7).reshape(-1, 2)
    have = {tuple(p) for p in kp.tolist()}
    assert {(-1.0, -1.0), (0.0, 0.0), (2.5, 4.5), (3.5, 5.5), (0.0, w - 1.0), (h - 1.0, 0.0), (h - 1.0, w - 1.0)} <= have
    assert np.signbit(kp).any() and (kp[:, 0] > h - 1).any() and (kp[:, 1] > w - 1).any()
    assert any(abs(p[0] - 4.4999) < 1e-6 for p in have)
    assert sorted(n * k for n, k, _ in [(1, 1, 0), (1, 7, 1), (2, 4, 8), (3, 3, 16), (3, 13, 0)]) == [1, 7, 8, 9, 39]


# ------------------------------------------------------------------ the bars can be met
def test_fp32_emulations_meet_every_bar():
    worst = {}
    for what, (img, wk, ref), ps, textured in _dense_cases():
        for order in ("rows", "lanes"):
            m10, m01 = _moments_f32(img, wk, ps, order)
            if not textured:
                assert np.array_equal(m10, ref.m10) and np.array_equal(m01, ref.m01), f"{what} {order}: moments not exact"
            ratio, ill = R.check(_atan2_f32(m01, m10), ref, what)
            _report(f"{what} {order} (ill-conditioned share {ill:.3g})", ratio)
            assert ratio <= 1.0, f"{what} {order}: a correct fp32 evaluation is {ratio:.3g} times the bound"
            assert ill <= (R.ILL_CAP if textured else 0.0), f"{what}: ill-conditioned share {ill:.3g}"
            worst[textured] = max(worst.get(textured, 0.0), ratio)
    assert worst[False] <= 0.5 / (R.ATAN2F_MEASURED_UNITS + 1.0) + 1e-9      # exact moments: half a unit of rounding


@pytest.mark.parametrize("ps,sigma", [(15, 2.5), (9, 1.5), (31, 5.0), (3, 1.0), (15, 5.0)])
@pytest.mark.parametrize("n,h,w", [(2, 37, 131), (2, 17, 65), (2, 33, 70)])
def test_ill_conditioned_share_of_textured_images(n, h, w, ps, sigma):
    """At most 1 % of the pixels of a synth_batch image have r >= 0.25 (measured: none)."""
    ref = R.gauss_case(n, h, w, ps, sigma)[2]
    _report(f"{(n, h, w)} ps {ps} sigma {sigma}: ill share {ref.ill.mean():.3g}, median bound {np.median(ref.bound):.3g} rad, worst r", ref.r.max())
    assert ref.ill.mean() <= R.ILL_CAP
    assert 1e-6 < np.median(ref.bound) < 1e-3


def _akaze_inputs(family, scales, ps):
    n, (h, w), k = 2, KP_HW, 13
    sigma = 2.5 if ps == 15 else 1.5
    cases = [R.int_case(n, h, w, ps, s) if family == "int" else R.gauss_case(n, h, w, ps, sigma, R.SEED + 10 * s)
             for s in range(scales)]
    kp = R.keypoints(n, k, h, w, ps // 2)
    attain = R.attain_bytes(n, h, w, scales, kp)
    return cases, kp, attain


def _akaze_f32(cases, attain, kp, ps, scales, descending=False, mask=True):
    """akaze_angle_kp_kernel's arithmetic in fp32: acc += t (1 / cnt) over the attained scales"""
    n, h, w = attain.shape
    cy, cx = R.nearest_pixel(kp, h, w)
    rows = np.arange(n)[:, None]
    raw = attain[rows, cy, cx].astype(np.int64)
    a = raw & ((1 << scales) - 1) if mask else raw
    cnt = np.maximum(sum((a >> b) & 1 for b in range(8)), 1).astype(F32)
    acc = np.zeros(a.shape, F32)
    for s in (range(scales - 1, -1, -1) if descending else range(scales)):
        img, wk, _ = cases[s]
        m10, m01 = _moments_f32(img, wk, ps, "lanes")
        t = _atan2_f32(m01, m10)[rows, cy, cx]
        acc = np.where((a >> s) & 1, acc + t * (F32(1) / cnt), acc).astype(F32)
    return acc


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("ps", [15, 9])
@pytest.mark.parametrize("scales", [1, 3, 8])
def test_akaze_select_reference_and_emulation(scales, ps, family):
    cases, kp, attain = _akaze_inputs(family, scales, ps)
    ref = R.akaze_select([c[2] for c in cases], attain, kp)
    assert ref.zero.any() and (ref.cnt == scales).any()
    if scales < 8:
        assert ((ref.bits == 0) & (ref.raw != 0)).any()                 # only bits >= S set: must give 0
    for descending in (False, True):
        ratio, ill = R.check(_akaze_f32(cases, attain, kp, ps, scales, descending), ref, "akaze")
        _report(f"akaze {family} S {scales} ps {ps} descending {descending} (ill share {ill:.3g})", ratio)
        assert ratio <= 1.0 and ill <= (R.ILL_CAP if family == "gauss" else 0.0)
    if scales < 8:                                                      # without the mask the planted bytes give it away
        with pytest.raises(AssertionError):
            ratio, _ = R.check(_akaze_f32(cases, attain, kp, ps, scales, mask=False), ref, "akaze without the mask")
            assert ratio <= 1.0


# ------------------------------------------------------------------ wrong kernels are outside the bars
@pytest.mark.parametrize("ps", R.INT_PATCHES)
def test_short_halo_and_lost_tap_exceed_the_bound(ps):
    """A tile filled one pixel off (what a halo of half - 1 amounts to at the tile's edge) and the last tap left out
    (ic clamped to ps^2 - 2)."""
    for what, (img, wk, ref) in (("int", R.int_case(2, 17, 65, ps)), ("isolated", R.seam_case(ps))):
        for mutant in (dict(shift=1), dict(drop=ps * ps - 1), dict(drop=0)):
            m10, m01 = _moments_f32(img, wk, ps, "rows", **mutant)
            try:
                ratio, _ = R.check(_atan2_f32(m01, m10), ref, what)
            except AssertionError:
                continue                                                # a zero patch that no longer gives 0.0
            _report(f"mutant {what} ps {ps} {mutant}", ratio)
            assert ratio > 1.0, f"{what} ps {ps} {mutant} passes"


def test_pair_reference_tells_the_sets_apart():
    """The pair test's reference at set b differs from set a's: reading set a twice cannot pass."""
    for family, ps in (("int", 15), ("gauss", 13)):
        for per_set in (1, 3):
            n = 2 * per_set
            _, _, dense = R.int_case(n, *KP_HW, ps) if family == "int" else R.gauss_case(n, *KP_HW, ps, KP_GAUSS[ps])
            kp = R.keypoints(n, 5, *KP_HW, ps // 2, first=3 * per_set)
            ref = R.at_keypoints(dense, kp)
            cy, cx = R.nearest_pixel(kp, *KP_HW)
            twice_a = dense.angle[(np.arange(n) % per_set)[:, None], cy, cx]
            assert (R.ang_diff(twice_a, ref.angle)[per_set:] > 100 * ref.bound[per_set:]).any()


# ------------------------------------------------------------------ argument checks
def test_argument_checks_return_before_any_launch():
    """Every call below is refused on the host (no kernel is launched: safe without a GPU)."""
    from onnx_image_processing_amd import _native as N
    lib = N.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def refused(name, base, cases):
        fn = getattr(lib, name)
        for change, code in cases:
            args = {**base, **change}
            assert fn(*args.values()) == code, f"{name} with {change}: expected {code}"

    bad_ps = [({"ps": v}, MI_E_PARAM) for v in (0, -3, 2, 14, 32, 33)]
    m = dict(image=p, n=1, h=8, w=8, ps=15, weights=p, angle=p, stream=None)
    refused("mi_angle_map", m, bad_ps + [({"image": None}, MI_E_NULL), ({"weights": None}, MI_E_NULL), ({"angle": None}, MI_E_NULL),
                                         ({"n": 0}, MI_E_SHAPE), ({"h": 0}, MI_E_SHAPE), ({"w": -1}, MI_E_SHAPE)])
    kp = dict(image=p, n=1, h=8, w=8, kpts=p, k=4, ps=15, weights=p, theta=p, stream=None)
    kp_cases = bad_ps + [({"kpts": None}, MI_E_NULL), ({"weights": None}, MI_E_NULL), ({"theta": None}, MI_E_NULL),
                         ({"h": 0}, MI_E_SHAPE), ({"w": 0}, MI_E_SHAPE), ({"k": 0}, MI_E_SHAPE), ({"k": -2}, MI_E_SHAPE)]
    refused("mi_angle_at_keypoints", kp, kp_cases + [({"image": None}, MI_E_NULL), ({"n": 0}, MI_E_SHAPE)])
    pair = dict(image_a=p, image_b=p, per_set=1, h=8, w=8, kpts=p, k=4, ps=15, weights=p, theta=p, stream=None)
    refused("mi_angle_at_keypoints_pair", pair, kp_cases + [({"image_a": None}, MI_E_NULL), ({"image_b": None}, MI_E_NULL),
                                                            ({"per_set": 0}, MI_E_SHAPE), ({"per_set": -1}, MI_E_SHAPE),
                                                            ({"image_b": None, "per_set": 0}, MI_E_NULL)])
    ak = dict(scale_images=p, stride=64, scales=3, attain=p, n=1, h=8, w=8, kpts=p, k=4, ps=15, weights=p, theta=p, stream=None)
    refused("mi_akaze_orientation_select", ak, kp_cases + [
        ({"scale_images": None}, MI_E_NULL), ({"attain": None}, MI_E_NULL), ({"n": 0}, MI_E_SHAPE),
        ({"scales": 0}, MI_E_SHAPE), ({"scales": 9}, MI_E_SHAPE), ({"stride": 63}, MI_E_SHAPE), ({"stride": 0}, MI_E_SHAPE),
        ({"scales": 1, "stride": 0, "ps": 14}, MI_E_PARAM)])            # one scale: any stride goes; the call ends at ps
