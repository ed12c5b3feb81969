"""K2 candidates from block maxima (nms_block_kernel, dispatched by mi_nms_candidates at radius 3 and 5 when
w % 4 == 0) against the dense tile kernel (debug key 20 = 1), in the debug and the product library, and against the
oracle where it defines the result.  Keypoints and scores are compared bit for bit with k >= the candidate count
(k <= 4096, the top-k kernel's limit), so the comparison is one of whole candidate sets; where a map has more
candidates than that, the candidate buffers of mi_nms_candidates themselves are compared segment by segment."""
import numpy as np
import pytest
import torch

from gpu_common import gpu, mods  # noqa: F401  (mods: the module fixture)
from onnx_image_processing_amd.synth import synth_batch
from oracle import numpy_oracle as O

pytestmark = pytest.mark.gpu

RADII = (3, 5, 4)                       # 3 and 5 run the block form, 4 stays on the dense kernel
THR_MARGIN = ((0.0, 0), (0.25, 3), (0.0, 7))


def _three_ways(scores, radius, k, thr, margin):
    """(block form, dense kernel, product library) results of ops.nms_topk as numpy (keypoints, scores) pairs."""
    from onnx_image_processing_amd import _native as N, ops
    out = []
    with N.debug_library() as lib:
        for impl in (0, 1):
            assert lib.mi_debug_set(20, impl) == 0
            out.append(ops.nms_topk(scores, radius, k, thr, margin))
        assert lib.mi_debug_set(20, 2) != 0
    out.append(ops.nms_topk(scores, radius, k, thr, margin))
    torch.cuda.synchronize()
    return [(kp.cpu().numpy(), sc.cpu().numpy()) for kp, sc in out]


def _candidate_sets(scores, radius, thr, margin):
    """(block form, dense kernel, product library): per image and segment the sorted keys mi_nms_candidates wrote."""
    from onnx_image_processing_amd import _native as N, ops
    b, h, w = scores.shape

    def run():
        cand, count, seg, cap = ops._candidate_buffers(b, h, w, scores.device)
        N.call("mi_nms_candidates", scores.data_ptr(), b, h, w, radius, thr, margin, cand.data_ptr(), count.data_ptr(),
               N.stream_ptr())
        torch.cuda.synchronize()
        cand, count = cand.cpu().numpy(), count.cpu().numpy()
        return [[np.sort(cand[i, j, :count[i, j]]) for j in range(seg)] for i in range(b)]
    out = []
    with N.debug_library() as lib:
        for impl in (0, 1):
            assert lib.mi_debug_set(20, impl) == 0
            out.append(run())
    out.append(run())
    return out


def _oracle_keys(sc, radius, thr, margin):
    """Per image the sorted keys (score bits high, inverted linear index low) of the oracle's survivors."""
    b, h, w = sc.shape
    keep = (O.nms_mask(sc, radius) > 0) & (sc > np.float32(max(thr, 0.0)))
    if margin > 0:
        inner = np.zeros((h, w), bool)
        inner[margin:h - margin, margin:w - margin] = True
        keep &= inner[None]
    out = []
    for i in range(b):
        lin = np.flatnonzero(keep[i].ravel()).astype(np.uint64)
        bits = sc[i].ravel()[lin.astype(np.int64)].view(np.uint32).astype(np.uint64)
        out.append(np.sort((bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - lin)))
    return out


def _check_candidate_sets(sc, radius, thr, margin, oracle=True):
    """The candidate buffers themselves: block form and product library equal to the dense kernel segment by segment
    (same keys, so same score bits), and their union per image equal to the oracle's survivors."""
    block, dense, product = _candidate_sets(gpu(sc), radius, thr, margin)
    for name, got in (("block", block), ("product", product)):
        for i in range(len(dense)):
            for j, (x, y) in enumerate(zip(got[i], dense[i])):
                assert np.array_equal(x, y), (name, sc.shape, radius, thr, margin, i, j)
    if oracle:
        want = _oracle_keys(sc, radius, thr, margin)
        for i in range(len(block)):
            got = np.sort(np.concatenate(block[i]).view(np.uint64))
            assert np.array_equal(got, want[i]), (sc.shape, radius, thr, margin, i)
    return block


def _same(results, what):
    block, dense, product = results
    for name, got in (("block", block), ("product", product)):
        assert np.array_equal(got[0], dense[0]), (what, name, "keypoints")
        assert np.array_equal(got[1].view(np.uint32), dense[1].view(np.uint32)), (what, name, "scores")


def _family(rng, n, h, w):
    sc = rng.standard_normal((n, h, w)).astype(np.float32)
    sc[:, : h // 2] = np.round(sc[:, : h // 2] * 2) / 2                     # exact ties in the upper half
    sc[:, h // 2:, : w // 2] *= np.float32(1e-6)                             # the 1e-7 slack bites: several candidates per block
    return sc


@pytest.mark.parametrize("radius", RADII)
def test_block_form_on_the_radius_tests_maps(mods, radius):
    """Negative values, plateaus of exact ties, ragged tile and block edges, several images: all three ways equal and
    equal to the oracle's selection."""
    rng = np.random.default_rng(100 + radius)
    for (n, h, w) in ((2, 75, 132), (1, 32, 128), (3, 97, 260), (1, 5, 8), (1, 38, 260)):
        sc = _family(rng, n, h, w)
        ref_mask = O.nms_mask(sc, radius)
        for thr, margin in THR_MARGIN:
            ncand = int(((ref_mask > 0) & (sc > thr)).sum(axis=(1, 2)).max())
            k = min(h * w, 4096, max(ncand, 1))
            _check_candidate_sets(sc, radius, thr, margin)
            res = _three_ways(gpu(sc), radius, k, thr, margin)
            _same(res, (radius, n, h, w, thr, margin))
            kp_ref, sc_ref, _ = O.select_topk_keypoints(sc, ref_mask, k, thr, margin)
            assert np.array_equal(res[0][0], kp_ref) and np.array_equal(res[0][1], sc_ref), (radius, h, w, thr, margin)


@pytest.mark.parametrize("radius", RADII)
def test_block_form_ties_and_near_ties(mods, radius):
    """Two equal maxima inside one 4x4 block, both window maxima; scores in (0, 1) with pairs closer than 1e-7 inside
    one block -- the larger first and the larger last in raster order, since the verification loop takes a block's
    candidates in that order and each needs its OWN score in the key and in the test -- and across a block edge in either
    axis; three distinct values within 1e-7 in one block; a low-contrast map whose every block has several candidates of
    different scores; a constant positive 64x256 map (every pixel a candidate, every segment full); an all-negative map
    (no candidate).  Candidate buffers (keys = score bits and index) against the dense kernel and the oracle, then top-k."""
    rng = np.random.default_rng(7)
    base = (rng.random((1, 64, 256), dtype=np.float32) * 0.25 + 0.01).astype(np.float32)
    ties = base.copy()
    ties[0, 20, 40] = ties[0, 21, 43] = 0.75                                 # one block: rows 20-23, columns 40-43
    ties[0, 40, 100:104] = 0.5                                               # a whole block row tied
    near = base.copy()
    lo, hi = np.float32(0.6), np.nextafter(np.float32(0.6), np.float32(1))  # 6e-8 apart
    near[0, 10, 16], near[0, 11, 18] = hi, lo                                # inside one block, the larger FIRST in raster order
    near[0, 14, 24], near[0, 15, 26] = lo, hi                                # inside one block, the larger last
    near[0, 30, 63], near[0, 30, 64] = hi, lo                                # across a vertical block edge
    near[0, 45, 130], near[0, 46, 130] = lo, hi                              # across a horizontal block edge
    near[0, 50:54, 200:208] = lo                                             # a plateau with one pixel just above it, last ...
    near[0, 51, 203] = hi
    near[0, 4:8, 100:104] = lo                                               # ... and first in its block
    near[0, 4, 100] = hi
    t0 = np.float32(0.3)                                                     # three distinct values 3e-8 apart in one block,
    t1 = np.nextafter(t0, np.float32(1))                                     # largest first
    t2 = np.nextafter(t1, np.float32(1))
    near[0, 24, 160], near[0, 25, 161], near[0, 26, 163] = t2, t1, t0
    near[0, 36, 220], near[0, 36, 222], near[0, 39, 221] = t1, t0, t2        # ... and in another order
    # low contrast everywhere: four distinct values 6e-8 apart, so every block holds several candidates of different
    # scores and far more than 4096 pixels survive
    lowc = (np.float32(0.5) + rng.integers(0, 4, (1, 64, 256)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    assert len(np.unique(lowc)) == 4
    const = np.full((1, 64, 256), 0.5, np.float32)
    neg = -base - 1.0
    for name, sc in (("ties", ties), ("near", near), ("lowc", lowc), ("const", const), ("neg", neg)):
        ref_mask = O.nms_mask(sc, radius)
        for thr, margin in THR_MARGIN:
            _check_candidate_sets(sc, radius, thr, margin)
            res = _three_ways(gpu(sc), radius, 4096, thr, margin)
            _same(res, (name, radius, thr, margin))
            kp_ref, sc_ref, _ = O.select_topk_keypoints(sc, ref_mask, 4096, thr, margin)
            assert np.array_equal(res[0][0], kp_ref) and np.array_equal(res[0][1], sc_ref), (name, radius, thr, margin)
    got = {(int(x), int(y)) for y, x in _three_ways(gpu(ties), radius, 4096, 0.0, 0)[0][0][0] if x >= 0}
    assert {(40, 20), (43, 21), (100, 40), (103, 40)} <= got
    got = {(int(x), int(y)) for y, x in _three_ways(gpu(near), radius, 4096, 0.0, 0)[0][0][0] if x >= 0}
    assert {(16, 10), (18, 11), (24, 14), (26, 15), (63, 30), (64, 30), (130, 45), (130, 46), (203, 51), (200, 50), (100, 4),
            (103, 7), (160, 24), (161, 25), (163, 26), (220, 36), (222, 36), (221, 39)} <= got
    assert sum(len(x) for x in _candidate_sets(gpu(lowc), radius, 0.0, 0)[0][0]) > 4096
    for thr, margin in THR_MARGIN:                                           # the constant map's 16 384 candidates, key by key
        block = _check_candidate_sets(const, radius, thr, margin)
        assert sum(len(seg) for seg in block[0]) == (64 - 2 * margin) * (256 - 2 * margin)
        if margin == 0:
            assert all(len(seg) == 4096 for seg in block[0])                 # every segment filled to its capacity
    assert int((_three_ways(gpu(neg), radius, 64, 0.0, 0)[0][1] > 0).sum()) == 0


@pytest.mark.parametrize("radius", RADII)
def test_block_form_ignores_nan_like_the_dense_kernel(mods, radius):
    """A few NaN pixels (alone, as a whole block, next to a maximum): never candidates, ignored by the maxima; compared
    with the dense kernel only."""
    rng = np.random.default_rng(11)
    sc = rng.random((2, 70, 132), dtype=np.float32)
    sc[0, 10, 10] = sc[0, 33, 64] = sc[1, 69, 131] = np.nan
    sc[1, 20:22, 40:44] = np.nan                                             # a whole block
    sc[0, 50, 50], sc[0, 50, 51] = 2.0, np.nan                               # beside a maximum
    for thr, margin in THR_MARGIN:
        _check_candidate_sets(sc, radius, thr, margin, oracle=False)
        res = _three_ways(gpu(sc), radius, 4096, thr, margin)
        _same(res, (radius, thr, margin))
        assert np.isfinite(res[0][1]).all()
    assert (50, 50) in {(int(x), int(y)) for y, x in res[0][0][0] if x >= 0}


def test_block_form_on_a_corner_map(mods):
    """One seeded 480x640 corner map at R = 5, k = 512, margin 7 (the bench's configuration), and its whole candidate set."""
    from onnx_image_processing_amd import ops
    a, _ = synth_batch(1000, 1, 480, 640)
    sc = ops.corner_response(gpu(a), 3).squeeze(1)
    host = sc.cpu().numpy()
    ref_mask = O.nms_mask(host, 5)
    _check_candidate_sets(host, 5, 0.0, 7)
    for k in (512, 4096):
        res = _three_ways(sc, 5, k, 0.0, 7)
        _same(res, k)
        kp_ref, sc_ref, _ = O.select_topk_keypoints(host, ref_mask, k, 0.0, 7)
        assert np.array_equal(res[0][0], kp_ref) and np.array_equal(res[0][1], sc_ref)
    assert int((res[0][1] > 0).sum()) > 2000
