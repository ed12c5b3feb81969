"""The test of the detector tests (no GPU): the references and the bounds of detector_oracle.py on the inputs
test_gpu_detectors.py uses.  numpy_oracle.fast_score decides all 65536 ring masks as the brute-force count does; the
separable fp64 DoG agrees with numpy_oracle.dog_responses; an fp32 evaluation of the DoG kernels' arithmetic, in two
summation orders, is bit-exact on the integer cases and inside the bound on the Gaussian ones, so the bars can be met; a
short halo, a lost end tap and a wrong run test are outside them; and the entry points refuse bad arguments before any
launch."""
import ctypes
import os

import numpy as np
import pytest

import detector_oracle as D
from oracle import numpy_oracle as O

F32 = np.float32
MI_E_NULL, MI_E_SHAPE, MI_E_PARAM = -1, -2, -3


def _report(what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[detectors_host] {what}: worst error / bound {ratio:.3g}")


# ------------------------------------------------------------------ FAST
def test_fast_bruteforce_counts():
    masks = np.arange(65536)
    fires = D.fast_bruteforce(masks)
    assert int(fires.sum()) == 1025
    assert fires[0x01FF] and fires[0xFF80] and fires[0xF01F] and fires[0xFFFF]          # 9 in a row, the last one wrapping
    assert not fires[0x00FF] and not fires[0xF00F] and not fires[0xFEFE] and not fires[0]
    for r in range(16):                                                                  # every rotation of 8 and of 9
        rot = lambda m: ((m << r) | (m >> (16 - r))) & 0xFFFF
        assert fires[rot(0x01FF)] and not fires[rot(0x00FF)]


@pytest.mark.parametrize("centre,delta", D.RING_FORMS)
def test_fast_oracle_decides_every_ring_mask_as_the_bruteforce(centre, delta):
    img = D.ring_image(centre, delta)
    assert img.shape == (1, 1, 1792, 1792) and img.dtype == F32
    score = O.fast_score(img, 20)
    masks = np.arange(65536).reshape(256, 256)
    if abs(delta) >= 20:
        assert np.array_equal(D.ring_centres(score) != 0, D.fast_bruteforce(masks))
        assert int(D.ring_centres(score).sum()) == 1025
    else:
        assert not score.any()                                                           # |difference| 19 < 20: nothing fires


def test_wrong_run_test_is_seen_by_the_ring_masks():
    """run9 with x >> 3 in place of x >> 4 (a run of 8 passes) differs from the brute force."""
    def run9(bits, third):
        x = bits | ((bits & 0xFF) << 16)
        x &= x >> 1
        x &= x >> 2
        x &= x >> third
        x &= x >> 1
        return (x & 0xFFFF) != 0
    masks = np.arange(65536)
    assert np.array_equal(run9(masks, 4), D.fast_bruteforce(masks))
    assert not np.array_equal(run9(masks, 3), D.fast_bruteforce(masks))


@pytest.mark.parametrize("n,h,w", D.FAST_SHAPES)
def test_fast_inputs(n, h, w):
    """Threshold 300 fires nowhere and threshold 0 everywhere on a constant image (every difference is both >= 0 and
    <= -0); on a textured image threshold 0 need not fire: the ring may alternate."""
    for kind in ("textured", "signed"):
        img = D.fast_image(n, h, w, kind)
        assert img.shape == (n, 1, h, w) and img.dtype == F32
        assert not O.fast_score(img, 300).any()
    assert (O.fast_score(np.full((n, 1, h, w), 7.25, F32), 0) == 1).all()


# ------------------------------------------------------------------ DoG
def _dog_f32(img, wk, descending=False, halo_short=False, lost_tap=False):
    """Both passes in fp32, taps ascending or descending, unfused.  halo_short: the padded tile filled one pixel off;
    lost_tap: the last tap of the rows left out."""
    s_count, ks = wk.shape
    half = ks // 2
    n, h, w = img.shape
    e = np.pad(img.astype(F32), ((0, 0), (half, half), (half, half)), mode="edge")
    if halo_short:
        e = np.pad(e, ((0, 0), (0, 1), (0, 1)), mode="edge")[:, 1:, 1:]
    order = range(ks - 1, -1, -1) if descending else range(ks)
    blur = np.zeros((n, s_count, h, w), F32)
    for s in range(s_count):
        tmp = np.zeros((n, h + 2 * half, w), F32)
        for k in order:
            if not (lost_tap and k == ks - 1):
                tmp += wk[s, k] * e[:, :, k:k + w]
        for k in order:
            blur[:, s] += wk[s, k] * tmp[:, k:k + h, :]
    maps = blur[:, 1:] - blur[:, :-1]
    assert maps.dtype == F32
    return maps, np.abs(maps).max(axis=1)


@pytest.mark.parametrize("ks,scales", D.DOG_BLOCKED + D.DOG_GENERIC)
def test_dog_integer_cases_are_exact_in_fp32(ks, scales):
    for n, h, w in D.DOG_SHAPES:
        img, wk, want_maps, want_score = D.dog_int_case(n, h, w, ks, scales)
        assert img.max() <= 15 and wk.min() >= 1 and wk.max() <= (3 if ks == 49 else 4)
        for descending in (False, True):
            maps, score = _dog_f32(img, wk, descending)
            assert np.array_equal(maps, want_maps) and np.array_equal(score, want_score), (n, h, w, descending)
    img, wk, want_maps, _ = D.dog_int_case(2, 33, 65, ks, scales)
    assert not np.array_equal(_dog_f32(img, wk, halo_short=True)[0], want_maps), "a tile filled one pixel off passes"
    assert not np.array_equal(_dog_f32(img, wk, lost_tap=True)[0], want_maps), "a lost end tap passes"


@pytest.mark.parametrize("kind", ["textured", "unit"])
@pytest.mark.parametrize("config", range(len(D.DOG_GAUSS)))
def test_dog_gaussian_cases_in_fp32_are_inside_the_bound(config, kind):
    img, wk = D.gauss_image(kind), D.gauss_weights_1d(**D.DOG_GAUSS[config])
    ref_maps, ref_score, map_bound, score_bound = D.dog_reference(img, wk)
    for descending in (False, True):
        maps, score = _dog_f32(img, wk, descending)
        r_maps, r_score = D.worst_ratio(maps, ref_maps, map_bound), D.worst_ratio(score, ref_score, score_bound)
        _report(f"{D.DOG_GAUSS[config] or 'default'} {kind} descending {descending}: maps {r_maps:.3g}, score", r_score)
        assert r_maps <= 1.0 and r_score <= 1.0
    if config == 2:                     # wide sigmas: the end taps weigh enough for the bound to see them go
        assert D.worst_ratio(_dog_f32(img, wk, lost_tap=True)[0], ref_maps, map_bound) > 1.0
        assert D.worst_ratio(_dog_f32(img, wk, halo_short=True)[0], ref_maps, map_bound) > 1.0


@pytest.mark.parametrize("config", range(len(D.DOG_GAUSS)))
def test_dog_separable_agrees_with_numpy_oracle(config):
    """numpy_oracle.dog_responses blurs with the fp64 row sums of the fp32 2-D kernels, the module's _weights_1d are those
    row sums rounded to (and summed in) fp32: ks u relative per weight, two weights per product -- the two references
    agree to (2 gamma_ks + gamma_ks^2) (B_s + B_{s-1}), plus the oracle's own rounding of its result to fp32."""
    kw = D.DOG_GAUSS[config]
    img, wk = D.gauss_image("textured"), D.gauss_weights_1d(**kw)
    s_count, ks = wk.shape
    k2 = O.gaussian_kernels_2d(**{**dict(num_scales=5, sigma_base=1.6, sigma_ratio=2 ** 0.5, kernel_size=None), **kw})
    assert k2.shape == (s_count, ks, ks)
    g = D.gamma(ks)
    assert (np.abs(wk - k2.astype(np.float64).sum(-1)) <= g * k2.astype(np.float64).sum(-1) + 1e-30).all()
    maps, _, _, _ = D.dog_reference(img, wk)
    _, b = D.dog_separable(img, wk)
    want = O.dog_responses(img[:, None], **kw).astype(np.float64)
    tol = (2 * g + g * g) * (b[:, 1:] + b[:, :-1]) * (1 + g) ** 2 + D.U * np.abs(want)
    assert (np.abs(maps - want) <= tol).all()
    assert np.abs(maps - want).max() < 1e-3 * np.abs(want).max()


# ------------------------------------------------------------------ u8 conversion
def test_u8_bytes_hold_the_extremes():
    for count in D.U8_COUNTS:
        a = D.u8_bytes(count)
        assert a.dtype == np.uint8 and a.shape == (count,)
        assert count < 3 or (a.min() == 0 and a.max() == 255)
    assert {c % 4 for c in D.U8_COUNTS} == {0, 1, 3} and max(D.U8_COUNTS) > 4096         # whole words, tails, several blocks


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

    dog = dict(image=p, n=1, h=8, w=8, weights=p, scales=3, ks=9, out=p, score=p, stream=None)
    refused("mi_dog_responses", dog, [({"scales": 9}, MI_E_PARAM), ({"ks": 51}, MI_E_PARAM), ({"scales": 1}, MI_E_PARAM),
                                      ({"ks": 8}, MI_E_PARAM), ({"ks": 0}, MI_E_PARAM), ({"image": None}, MI_E_NULL),
                                      ({"weights": None}, MI_E_NULL), ({"out": None, "score": None}, MI_E_NULL),
                                      ({"n": 0}, MI_E_SHAPE), ({"h": 0}, MI_E_SHAPE), ({"w": 0}, MI_E_SHAPE)])
    fast = dict(image=p, n=1, h=8, w=8, threshold=20.0, score=p, stream=None)
    refused("mi_fast_score", fast, [({"image": None}, MI_E_NULL), ({"score": None}, MI_E_NULL), ({"n": 0}, MI_E_SHAPE),
                                    ({"h": -1}, MI_E_SHAPE), ({"w": 0}, MI_E_SHAPE)])
    conv = dict(src=p, count=16, dst=p, stream=None)
    refused("mi_convert_u8_f32", conv, [({"src": None}, MI_E_NULL), ({"dst": None}, MI_E_NULL), ({"count": 0}, MI_E_SHAPE),
                                        ({"count": -4}, MI_E_SHAPE)])
