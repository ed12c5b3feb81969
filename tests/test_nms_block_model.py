"""The argument behind K2's block form (csrc/nms.hip, nms_block_kernel) as a numpy model, against the window form.

Partition the pixels into blocks of at most (R+1) x (R+1).  A pixel's (2R+1)^2 window contains its whole block, so the
window maximum M is at least the block maximum B, and x -> fl(x - 1e-7f) is monotone: a pixel can pass
s >= fl(M - 1e-7f) only if s >= fl(B - 1e-7f).  Those pixels -- the block's candidates -- are the only ones that need an
exact window maximum.  The model does exactly that and must give the mask of O.nms_mask(...) & (s > thr) for every
block size up to R + 1 in both axes, ragged blocks at the image edges included."""
import numpy as np
import pytest

from oracle import numpy_oracle as O

F32 = np.float32
SHAPES = ((1, 5, 8), (1, 32, 128), (2, 75, 132), (3, 97, 260))


def _maps():
    """The radius test's family (normal scores: negatives; exact half-integer ties in the upper half) plus a region
    scaled by 1e-6, where neighbouring scores differ by less than the 1e-7 slack of the test."""
    rng = np.random.default_rng(2024)
    out = []
    for n, h, w in SHAPES:
        sc = rng.standard_normal((n, h, w)).astype(F32)
        sc[:, : h // 2] = np.round(sc[:, : h // 2] * 2) / 2
        sc[:, h // 2:, : w // 2] *= F32(1e-6)
        out.append(sc)
    return out


MAPS = _maps()
REFERENCE = {}                  # (map index, radius) -> the window form's mask, computed once


def _reference(i, radius):
    if (i, radius) not in REFERENCE:
        REFERENCE[(i, radius)] = O.nms_mask(MAPS[i], radius) > 0
    return REFERENCE[(i, radius)]


def block_form(s, radius, bh, bw, thr):
    """keep-mask by the block procedure with bh x bw blocks (ragged at the bottom and right edges)."""
    b, h, w = s.shape
    ys, xs = np.arange(0, h, bh), np.arange(0, w, bw)
    bmax = np.maximum.reduceat(np.maximum.reduceat(s, ys, axis=1), xs, axis=2)        # 1. one maximum per block
    bexp = np.repeat(np.repeat(bmax, bh, axis=1)[:, :h], bw, axis=2)[:, :, :w]
    cand = (s >= (bexp - F32(1e-7))) & (s > F32(thr))                                 # 2. the blocks' candidates
    r = radius
    e = np.pad(s, ((0, 0), (r, r), (r, r)), mode="constant", constant_values=-np.inf)
    win = np.lib.stride_tricks.sliding_window_view(e, (2 * r + 1, 2 * r + 1), axis=(1, 2))
    ii, yy, xx = np.nonzero(cand)
    m = win[ii, yy, xx].max(axis=(1, 2))                                              # 3. exact maximum, candidates only
    keep = np.zeros_like(cand)
    keep[ii, yy, xx] = s[ii, yy, xx] >= (m - F32(1e-7))
    return keep, cand


@pytest.mark.parametrize("radius", range(1, 9))
def test_block_form_equals_window_form(radius):
    for i, s in enumerate(MAPS):
        ref_mask = _reference(i, radius)
        for thr in (0.0, 0.25, -np.inf):                      # -inf: no threshold at all
            ref = ref_mask & (s > F32(thr))
            for bh in range(1, radius + 2):
                for bw in range(1, radius + 2):
                    keep, cand = block_form(s, radius, bh, bw, thr)
                    assert np.array_equal(keep, ref), (s.shape, radius, bh, bw, thr)
                    assert not (ref & ~cand).any()            # no survivor outside the candidates


def test_blocks_larger_than_the_window_allows_lose_maxima():
    """The bound is sharp: with blocks of R + 2 a block's maximum can lie outside a pixel's window, and a window maximum
    that is not its block's maximum is lost."""
    s = np.zeros((1, 8, 8), F32)
    s[0, 0, 0], s[0, 0, 3] = 2.0, 1.0                         # R = 1: (0, 3) is a window maximum; a 4-wide block hides it
    ref = (O.nms_mask(s, 1) > 0) & (s > 0)
    assert ref[0, 0, 3]
    keep, _ = block_form(s, 1, 1, 4, 0.0)
    assert not keep[0, 0, 3]
    keep, _ = block_form(s, 1, 2, 2, 0.0)
    assert np.array_equal(keep, ref)
