"""The orientation stage (K8, csrc/orient.hip) against fp64 at every dispatch of its four entry points: the dense map
kernel, the keypoint kernel in its <15> and its generic instance, the two-set (pair) form and AKAZE's select-by-attain
kernel.  Two families of case (orient_oracle.py): integer images and integer weight planes, whose fp32 moments are exact
in any order, so that the angle is held to atan2f's own error and every tap shows; and the module's Gaussian planes on
textured images, held to the a-priori fp32 summation bound.  Nothing here is fitted to what the kernels return; the one
measured number, atan2f's error, is measured on torch.atan2 and re-measured below.

Every output is allocated with a sentinel-filled guard row at both ends, which must come back untouched.  Every call runs
twice and must repeat bit for bit.  MI_REPORT=1 prints the worst error / bound of each case.  Run with `-m gpu` on an
MI355X."""
import os

import numpy as np
import pytest
import torch

import orient_oracle as R
from gpu_common import DEV, GPU, gpu, mods, twice  # noqa: F401  (mods: the module fixture)

pytestmark = GPU


def _report(group, what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[orient {group}] {what}: worst error / bound {ratio:.3g}")


class _Out:
    """`rows` rows of `cols` float32 between two guard rows, all NaN until written"""

    def __init__(self, rows, cols):
        self.full = torch.full((rows + 2, cols), float("nan"), dtype=torch.float32, device=DEV)
        self.ptr = self.full[1].data_ptr()

    def read(self, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.full[0]).all()), f"{what}: the row in front of the output was written"
        assert bool(torch.isnan(self.full[-1]).all()), f"{what}: the row behind the output was written"
        return self.full[1:-1].cpu().numpy()


def _judge(group, what, got, ref, textured):
    ratio, ill = R.check(got, ref, what)
    _report(group, what + (f" (ill-conditioned share {ill:.3g})" if textured else ""), ratio)
    assert not np.isnan(got).any(), f"{what}: an output element was not written"
    assert ill <= (R.ILL_CAP if textured else 0.0), f"{what}: {ill:.3g} of the entries are ill-conditioned"
    assert ratio <= 1.0, f"{what}: error {ratio:.3g} times the bound"


# ------------------------------------------------------------------ the atan2f constant
def test_atan2f_constant_still_covers_torch(mods):
    y, x = R.atan2f_probe_pairs()
    got = torch.atan2(gpu(y), gpu(x)).cpu().numpy()
    err = np.abs(got.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64))) / R.ATAN2F_UNIT
    _report("atan2f", f"{len(y)} pairs, worst error {err.max():.4f} units of 2^-22, constant", err.max() / R.ATAN2F_MEASURED_UNITS)
    assert err.max() <= R.ATAN2F_MEASURED_UNITS


# ------------------------------------------------------------------ A, B. mi_angle_map
def _angle_map(N, what, img, wk, ps):
    n, h, w = img.shape
    d_img, d_wk = gpu(img, wk)

    def run():
        out = _Out(n * h, w)
        N.call("mi_angle_map", d_img.data_ptr(), n, h, w, ps, d_wk.data_ptr(), out.ptr, N.stream_ptr())
        return (out.read(what),)
    return twice(what, run)[0].reshape(n, h, w)


@pytest.mark.parametrize("ps", R.INT_PATCHES)
@pytest.mark.parametrize("n,h,w", R.INT_SHAPES)
def test_angle_map_integer_weights_vs_fp64(mods, n, h, w, ps):
    from onnx_image_processing_amd import _native as N
    img, wk, ref = R.int_case(n, h, w, ps)
    what = f"map int {(n, h, w)} ps {ps}"
    _judge("A", what, _angle_map(N, what, img, wk, ps), ref, textured=False)


@pytest.mark.parametrize("ps", R.INT_PATCHES)
def test_angle_map_isolated_pixels_show_every_tap(mods, ps):
    """One pixel of value 8 per window: the map around it is atan2 of the flipped weight planes, tap by tap, cut off by the
    zero padding at the corners and continued across the tile seams."""
    from onnx_image_processing_amd import _native as N
    img, wk, ref = R.seam_case(ps)
    assert (~ref.zero).sum() >= len(R.SEAM_PIXELS) * (ps // 2 + 1) ** 2 * 0.8      # the taps are seen
    what = f"map isolated pixels ps {ps}"
    _judge("A", what, _angle_map(N, what, img, wk, ps), ref, textured=False)


@pytest.mark.parametrize("ps,sigma", R.GAUSS)
@pytest.mark.parametrize("n,h,w", R.GAUSS_SHAPES)
def test_angle_map_gaussian_weights_vs_fp64(mods, n, h, w, ps, sigma):
    from onnx_image_processing_amd import _native as N
    img, wk, ref = R.gauss_case(n, h, w, ps, sigma)
    what = f"map gauss {(n, h, w)} ps {ps} sigma {sigma}"
    _judge("B", what, _angle_map(N, what, img, wk, ps), ref, textured=True)


# ------------------------------------------------------------------ C. mi_angle_at_keypoints
KP_PATCHES = [15, 13, 17, 31]                                  # 15: the <15> instance; the others: the generic one
KP_GAUSS = {15: 2.5, 13: 2.0, 17: 3.0, 31: 5.0}
KP_COUNTS = [(1, 1, 0), (1, 7, 1), (2, 4, 8), (3, 3, 16), (3, 13, 0)]      # (n, k, first special keypoint): n k = 1, 7, 8, 9, 39
KP_HW = (17, 65)


def _case(family, n, h, w, ps):
    return R.int_case(n, h, w, ps) if family == "int" else R.gauss_case(n, h, w, ps, KP_GAUSS.get(ps, 1.5))


def _at_keypoints(N, what, img, wk, ps, kp):
    n, h, w = img.shape
    k = kp.shape[1]
    d_img, d_wk, d_kp = gpu(img, wk, kp)

    def run():
        out = _Out(n, k)
        N.call("mi_angle_at_keypoints", d_img.data_ptr(), n, h, w, d_kp.data_ptr(), k, ps, d_wk.data_ptr(), out.ptr,
               N.stream_ptr())
        return (out.read(what),)
    return twice(what, run)[0]


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("ps", KP_PATCHES)
@pytest.mark.parametrize("n,k,first", KP_COUNTS)
def test_angle_at_keypoints_vs_fp64(mods, n, k, first, ps, family):
    """The same images and keypoints for every patch size: the <15> instance and the generic one side by side."""
    from onnx_image_processing_amd import _native as N
    h, w = KP_HW
    img, wk, dense = _case(family, n, h, w, ps)
    kp = R.keypoints(n, k, h, w, 15 // 2, first)
    what = f"keypoints {family} n {n} k {k} ps {ps}"
    _judge("C", what, _at_keypoints(N, what, img, wk, ps, kp), R.at_keypoints(dense, kp), textured=family == "gauss")


@pytest.mark.parametrize("ps", KP_PATCHES)
@pytest.mark.parametrize("n,h,w,k", [(1, 3, 5, 9), (1, 1, 1, 3)])
def test_angle_at_keypoints_image_smaller_than_the_patch(mods, n, h, w, k, ps):
    from onnx_image_processing_amd import _native as N
    img, wk, dense = R.int_case(n, h, w, ps)
    kp = R.keypoints(n, k, h, w, 1)
    what = f"keypoints int small image {(n, h, w)} k {k} ps {ps}"
    _judge("C", what, _at_keypoints(N, what, img, wk, ps, kp), R.at_keypoints(dense, kp), textured=False)


# ------------------------------------------------------------------ D. mi_angle_at_keypoints_pair
@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("ps", [15, 13])
@pytest.mark.parametrize("per_set", [1, 3])
def test_angle_at_keypoints_pair_vs_fp64(mods, per_set, ps, family):
    """Two sets in separate allocations holding different images: a kernel that read set a twice fails."""
    from onnx_image_processing_amd import _native as N
    h, w = KP_HW
    n, k = 2 * per_set, 5
    img, wk, dense = _case(family, n, h, w, ps)
    assert not np.array_equal(img[:per_set], img[per_set:])
    kp = R.keypoints(n, k, h, w, ps // 2, first=3 * per_set)
    d_a, d_b, d_wk, d_kp = gpu(img[:per_set], img[per_set:], wk, kp)
    what = f"pair {family} per_set {per_set} ps {ps}"

    def run():
        out = _Out(n, k)
        N.call("mi_angle_at_keypoints_pair", d_a.data_ptr(), d_b.data_ptr(), per_set, h, w, d_kp.data_ptr(), k, ps,
               d_wk.data_ptr(), out.ptr, N.stream_ptr())
        return (out.read(what),)
    _judge("D", what, twice(what, run)[0], R.at_keypoints(dense, kp), textured=family == "gauss")


# ------------------------------------------------------------------ E. mi_akaze_orientation_select
@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("gap", [0, 37])
@pytest.mark.parametrize("ps", [15, 9])
@pytest.mark.parametrize("scales", [1, 3, 8])
def test_akaze_orientation_select_vs_fp64(mods, scales, ps, gap, family):
    """scale_stride = n h w and n h w + 37 with NaN between the scales; attain bytes with no bit, every bit and only bits
    >= S set at planted keypoints."""
    from onnx_image_processing_amd import _native as N
    n, h, w, k = 2, 17, 65, 13
    sigma = 2.5 if ps == 15 else 1.5
    cases = [R.int_case(n, h, w, ps, s) if family == "int" else R.gauss_case(n, h, w, ps, sigma, R.SEED + 10 * s)
             for s in range(scales)]
    wk = cases[0][1]
    kp = R.keypoints(n, k, h, w, ps // 2)
    attain = R.attain_bytes(n, h, w, scales, kp)
    ref = R.akaze_select([c[2] for c in cases], attain, kp)
    assert ref.zero.any() and (ref.cnt == scales).any() and (scales == 8 or ((ref.bits == 0) & (ref.raw != 0)).any())
    stride = n * h * w + gap
    stack = np.full((scales, stride), np.nan, np.float32)
    for s, c in enumerate(cases):
        stack[s, :n * h * w] = c[0].ravel()
    d_stack, d_wk, d_kp, d_attain = gpu(stack, wk, kp, attain)
    what = f"akaze {family} S {scales} ps {ps} stride +{gap}"

    def run():
        out = _Out(n, k)
        N.call("mi_akaze_orientation_select", d_stack.data_ptr(), stride, scales, d_attain.data_ptr(), n, h, w,
               d_kp.data_ptr(), k, ps, d_wk.data_ptr(), out.ptr, N.stream_ptr())
        return (out.read(what),)
    _judge("E", what, twice(what, run)[0], ref, textured=family == "gauss")
