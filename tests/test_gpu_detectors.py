"""The FAST / DoG stage (K11, csrc/detectors.hip) against its references at every dispatch: the FAST kernel on all 65536
ring masks and at the awkward shapes and thresholds, bit for bit; the register-blocked DoG kernel (kernel size 39) and the
generic one, crossed with the three output forms, bit for bit on integer images with integer weights and within the
a-priori fp32 bound on textured images with the module's Gaussian weights (detector_oracle.py); the uint8 conversion on
its word path, its tail and its misaligned-base fallback.  Nothing here is fitted to what the kernels return.

Every output is allocated with a sentinel-filled guard row at both ends, which must come back untouched.  Every call runs
twice and must repeat bit for bit.  MI_REPORT=1 prints the worst error / bound of each case.  Run with `-m gpu` on an
MI355X."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import detector_oracle as D
from gpu_common import DEV, GPU, gpu, mods, twice  # noqa: F401  (mods: the module fixture)
from oracle import numpy_oracle as O

pytestmark = GPU


def _report(group, what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[detectors {group}] {what}: worst error / bound {ratio:.3g}")


class _Out:
    """`rows` rows of `cols` float32 between two guard rows, all NaN until written"""

    def __init__(self, rows, cols):
        self.full = torch.full((rows + 2, cols), float("nan"), dtype=torch.float32, device=DEV)
        self.ptr = self.full[1].data_ptr()

    def read(self, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.full[0]).all()), f"{what}: the row in front of the output was written"
        assert bool(torch.isnan(self.full[-1]).all()), f"{what}: the row behind the output was written"
        body = self.full[1:-1].cpu().numpy()
        assert not np.isnan(body).any(), f"{what}: an output element was not written"
        return body


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------ F, G. mi_fast_score
def _fast(N, what, img, thr):
    n, _, h, w = img.shape
    d_img = gpu(img)

    def run():
        out = _Out(n * h, w)
        N.call("mi_fast_score", d_img.data_ptr(), n, h, w, float(thr), out.ptr, N.stream_ptr())
        return (out.read(what),)
    return twice(what, run)[0].reshape(n, 1, h, w)


@lru_cache(maxsize=None)
def _ring_reference(centre, delta):
    img = D.ring_image(centre, delta)
    return img, O.fast_score(img, 20)


@pytest.mark.parametrize("centre,delta", D.RING_FORMS)
def test_fast_every_ring_mask(mods, centre, delta):
    """All 65536 masks: dark (delta +20) and bright (-20) at threshold 20; at +-19 nothing may fire."""
    from onnx_image_processing_amd import _native as N
    img, want = _ring_reference(centre, delta)
    got = _fast(N, f"fast rings delta {delta}", img, 20)
    assert _same(got, want), f"{int((got != want).sum())} pixels differ from the oracle"
    masks = np.arange(65536).reshape(256, 256)
    fires = D.fast_bruteforce(masks) if abs(delta) >= 20 else np.zeros((256, 256), bool)
    bad = np.flatnonzero((D.ring_centres(got) != 0) != fires)
    assert bad.size == 0, f"{bad.size} ring masks decided wrongly, the first {int(bad[0]):#06x}"


@pytest.mark.parametrize("kind", ["textured", "signed"])
@pytest.mark.parametrize("n,h,w", D.FAST_SHAPES)
def test_fast_shapes_and_thresholds(mods, n, h, w, kind):
    """Threshold 300 fires nowhere.  Threshold 0 fires everywhere on a constant image (every difference is both >= 0 and
    <= -0) but not on a textured one, whose ring may alternate between brighter and darker without a run of 9: there the
    oracle decides, as at every other threshold."""
    from onnx_image_processing_amd import _native as N
    img = D.fast_image(n, h, w, kind)
    assert kind == "textured" or img.min() < 0
    for thr in D.FAST_THRESHOLDS:
        got = _fast(N, f"fast {kind} {(n, h, w)} threshold {thr}", img, thr)
        assert _same(got, O.fast_score(img, thr)), (kind, (n, h, w), thr)
        if thr == 300:
            assert (got == 0).all()
    flat = np.full_like(img, img[0, 0, 0, 0])
    assert (_fast(N, f"fast constant {(n, h, w)} threshold 0", flat, 0) == 1).all()


# ------------------------------------------------------------------ H, I. mi_dog_responses
def _dog(N, what, d_img, d_wk, shape, scales, ks, want_maps, want_score):
    n, h, w = shape

    def run():
        maps = _Out(n * (scales - 1) * h, w) if want_maps else None
        score = _Out(n * h, w) if want_score else None
        N.call("mi_dog_responses", d_img.data_ptr(), n, h, w, d_wk.data_ptr(), scales, ks, maps.ptr if maps else None,
               score.ptr if score else None, N.stream_ptr())
        return (maps.read(what + " maps") if maps else None, score.read(what + " score") if score else None)
    maps, score = twice(what, run)
    return (maps.reshape(n, scales - 1, h, w) if want_maps else None, score.reshape(n, h, w) if want_score else None)


def _dog_three_forms(N, what, img, wk):
    """maps only, score only, both: the forms must give identical bits, the score must be max |maps| exactly"""
    scales, ks = wk.shape
    d_img, d_wk = gpu(img, wk)
    maps, score = _dog(N, what + " both", d_img, d_wk, img.shape, scales, ks, True, True)
    only_maps, _ = _dog(N, what + " maps only", d_img, d_wk, img.shape, scales, ks, True, False)
    _, only_score = _dog(N, what + " score only", d_img, d_wk, img.shape, scales, ks, False, True)
    assert _same(maps, only_maps), f"{what}: the maps differ between the maps-only form and the form with both"
    assert _same(score, only_score), f"{what}: the score differs between the score-only form and the form with both"
    assert _same(score, np.abs(maps).max(axis=1)), f"{what}: the score is not max |maps|"
    return maps, score


def _dog_int(N, n, h, w, ks, scales):
    img, wk, want_maps, want_score = D.dog_int_case(n, h, w, ks, scales)
    what = f"dog int {(n, h, w)} ks {ks} scales {scales}"
    maps, score = _dog_three_forms(N, what, img, wk)
    bad = np.argwhere(maps != want_maps)
    assert bad.size == 0, f"{what}: {len(bad)} map values differ, the first at {bad[0].tolist()}: {maps[tuple(bad[0])]} vs {want_maps[tuple(bad[0])]}"
    assert _same(maps, want_maps) and _same(score, want_score), what


@pytest.mark.parametrize("n,h,w", D.DOG_SHAPES)
@pytest.mark.parametrize("ks,scales", D.DOG_BLOCKED)
def test_dog_blocked_kernel_integer_weights_bit_exact(mods, ks, scales, n, h, w):
    from onnx_image_processing_amd import _native as N
    _dog_int(N, n, h, w, ks, scales)


@pytest.mark.parametrize("n,h,w", D.DOG_SHAPES)
@pytest.mark.parametrize("ks,scales", D.DOG_GENERIC)
def test_dog_generic_kernel_integer_weights_bit_exact(mods, ks, scales, n, h, w):
    from onnx_image_processing_amd import _native as N
    _dog_int(N, n, h, w, ks, scales)


@pytest.mark.parametrize("kind", ["textured", "unit"])
@pytest.mark.parametrize("config", range(len(D.DOG_GAUSS)))
def test_dog_gaussian_weights_vs_fp64(mods, config, kind):
    """No pixel is left out."""
    from onnx_image_processing_amd import _native as N
    kw = D.DOG_GAUSS[config]
    img, wk = D.gauss_image(kind), D.gauss_weights_1d(**kw)
    what = f"dog gauss {kw or 'default'} {kind}"
    maps, score = _dog_three_forms(N, what, img, wk)
    ref_maps, ref_score, map_bound, score_bound = D.dog_reference(img, wk)
    r_maps, r_score = D.worst_ratio(maps, ref_maps, map_bound), D.worst_ratio(score, ref_score, score_bound)
    _report("I", what + " maps", r_maps)
    _report("I", what + " score", r_score)
    assert r_maps <= 1.0, f"{what}: map error {r_maps:.3g} times the fp32 bound"
    assert r_score <= 1.0, f"{what}: score error {r_score:.3g} times the fp32 bound"


# ------------------------------------------------------------------ J. mi_convert_u8_f32
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("count", D.U8_COUNTS)
def test_convert_u8_f32(mods, count, offset):
    """The source base `offset` bytes into an allocation: 0 takes the 4-byte word path (and its scalar tail), the others
    the misaligned-base fallback."""
    from onnx_image_processing_amd import _native as N
    src = D.u8_bytes(count)
    buf = torch.zeros(count + offset, dtype=torch.uint8, device=DEV)
    buf[offset:].copy_(torch.from_numpy(src))
    assert buf.data_ptr() % 4 == 0
    what = f"convert {count} bytes, base + {offset}"

    def run():
        out = _Out(1, count)
        N.call("mi_convert_u8_f32", buf.data_ptr() + offset, count, out.ptr, N.stream_ptr())
        return (out.read(what),)
    got = twice(what, run)[0].reshape(-1)
    assert _same(got, src.astype(np.float32)), what
