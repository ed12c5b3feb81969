"""numpy oracle of K33 (include/mi355x_match_stereo.h): census, matching cost, semi-global path sums, selection with its tests,
the sub-pixel step and depth, restated from the header's definitions: integers up to the aggregated volume, float32 for the
sub-pixel step and the division.  Also the scenes the stereo tests share, and a raw winner-take-all on the matching cost for
comparison.  No test module: importing it computes nothing."""
import functools

import numpy as np

from onnx_image_processing_amd.synth import synth_stereo_pair

OK, NOT_UNIQUE, LR = 0, 1, 2
COST_OUTSIDE = 64
BORDER = 8
ABSENT = 1 << 20
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))
P1, P2, UNIQUENESS, LR_MAX_DIFF = 10, 120, 10, 1


def census(gray):
    """(..., h, w) uint8 or float32 -> uint64: bit k for the k-th offset of the 9 x 7 window, the centre skipped"""
    g = np.asarray(gray)
    h, w = g.shape[-2:]
    pad = np.pad(g, [(0, 0)] * (g.ndim - 2) + [(3, 3), (4, 4)], mode="edge")
    out = np.zeros(g.shape, np.uint64)
    k = 0
    with np.errstate(invalid="ignore"):
        for dy in range(-3, 4):
            for dx in range(-4, 5):
                if dy == 0 and dx == 0:
                    continue
                out |= (pad[..., 3 + dy:3 + dy + h, 4 + dx:4 + dx + w] < g).astype(np.uint64) << np.uint64(k)
                k += 1
    assert k == 62
    return out


def popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(*x.shape, 8), axis=-1).sum(-1).astype(np.int32)


def cost(cl, cr, D):
    """(h, w) census words of both views -> C (h, w, D) int32"""
    h, w = cl.shape
    c = np.full((h, w, D), COST_OUTSIDE, np.int32)
    for d in range(min(D, w)):
        c[:, d:, d] = popcount(cl[:, d:] ^ cr[:, :w - d])
    return c


def _step(c, prev, p1, p2):
    m = prev.min(-1, keepdims=True)
    lo, hi = np.full_like(prev, ABSENT), np.full_like(prev, ABSENT)
    lo[..., 1:], hi[..., :-1] = prev[..., :-1], prev[..., 1:]
    return c + np.minimum(np.minimum(prev, m + p2), np.minimum(lo, hi) + p1) - m


def path(c, dy, dx, p1, p2):
    """L_r (h, w, D) int32 of one direction"""
    h, w, _ = c.shape
    out = c.copy()
    if dy == 0:
        xs = range(1, w) if dx > 0 else range(w - 2, -1, -1)
        for x in xs:
            out[:, x] = _step(c[:, x], out[:, x - dx], p1, p2)
        return out
    ys = range(1, h) if dy > 0 else range(h - 2, -1, -1)
    x = np.arange(w)
    has = (x - dx >= 0) & (x - dx < w)
    for y in ys:
        out[y, has] = _step(c[y, has], out[y - dy, x[has] - dx], p1, p2)
    return out


def aggregate(cl, cr, D, paths, p1=P1, p2=P2):
    """S (h, w, D) uint16: the sum of L_r over the first `paths` directions"""
    c = cost(cl, cr, D)
    s = np.zeros(c.shape, np.int32)
    for dy, dx in DIRS[:paths]:
        l = path(c, dy, dx, p1, p2)
        assert l.max() <= c.max() + p2 and l.min() >= 0
        s += l
    assert s.max() <= 8 * 319
    return s.astype(np.uint16)


def right_disparity(volume):
    """dR (h, w) int16 from S (h, w, D)"""
    h, w, D = volume.shape
    t = np.full((h, w, D), 1 << 30, np.int64)
    for d in range(min(D, w)):
        t[:, :w - d, d] = volume[:, d:, d]
    return t.argmin(-1).astype(np.int16)


def select(volume, uniqueness=UNIQUENESS, lr_max_diff=LR_MAX_DIFF):
    """S (h, w, D) -> disparity (h, w) float32, disparity_right (h, w) int16, code (h, w) uint8"""
    s = volume.astype(np.int64)
    h, w, D = s.shape
    best = s.argmin(-1)
    s_best = np.take_along_axis(s, best[..., None], -1)[..., 0]
    d = np.arange(D)
    rival = (np.abs(d - best[..., None]) > 1) & (s * (100 - uniqueness) < s_best[..., None] * 100)
    code = np.where(rival.any(-1), NOT_UNIQUE, OK).astype(np.uint8)
    right = right_disparity(volume)
    if lr_max_diff >= 0:
        xr = np.arange(w)[None, :] - best
        fails = (xr < BORDER) | (np.abs(np.take_along_axis(right.astype(np.int64), np.clip(xr, 0, w - 1), 1) - best) > lr_max_diff)
        code[(code == OK) & fails] = LR
    inner = (best > 0) & (best < D - 1)
    s_lo = np.take_along_axis(s, np.clip(best - 1, 0, D - 1)[..., None], -1)[..., 0]
    s_hi = np.take_along_axis(s, np.clip(best + 1, 0, D - 1)[..., None], -1)[..., 0]
    den = s_lo + s_hi - 2 * s_best
    assert (den[inner] >= 0).all()
    use = inner & (den > 0)
    offset = np.zeros((h, w), np.float32)
    offset[use] = (s_lo - s_hi)[use].astype(np.float32) / (2 * den)[use].astype(np.float32)
    assert (np.abs(offset) <= 0.5).all()
    disparity = best.astype(np.float32) + offset
    disparity[code != OK] = np.float32(-1.0)
    return disparity, right, code


def depth(disparity, fb, min_disparity):
    d = np.asarray(disparity, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d >= np.float32(min_disparity), np.float32(fb) / d, np.float32(0.0)).astype(np.float32)


def wta(cl, cr, D):
    """the raw winner-take-all on the matching cost, the lowest d on ties: (h, w) int"""
    return cost(cl, cr, D).argmin(-1)


def run(left, right, D, paths, p1=P1, p2=P2, uniqueness=UNIQUENESS, lr_max_diff=LR_MAX_DIFF, fb=100.0, min_disparity=0.5):
    """one pair (h, w) through every stage -> dict of census_left, census_right, volume, disparity, disparity_right, code, depth"""
    cl, cr = census(left), census(right)
    volume = aggregate(cl, cr, D, paths, p1, p2)
    disparity, dr, code = select(volume, uniqueness, lr_max_diff)
    return dict(census_left=cl, census_right=cr, volume=volume, disparity=disparity, disparity_right=dr, code=code,
                depth=depth(disparity, fb, min_disparity))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def plane_pair(seed, h, w, d0):
    """random uint8 texture at the constant disparity d0: right[y, x - d0] = left[y, x]; the columns of the right view that no
    left pixel reaches are fresh texture"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (h, w)).astype(np.uint8)
    right = rng.integers(0, 256, (h, w)).astype(np.uint8)
    if d0 < w:
        right[:, :w - d0] = left[:, d0:]
    return left, right


def plane_interior(h, w, d0):
    """rows 3 .. h - 4, columns d0 + 8 .. w - 5 as a boolean mask"""
    m = np.zeros((h, w), bool)
    m[3:h - 3, d0 + 8:w - 4] = True
    return m


@functools.lru_cache(maxsize=None)
def pair(seed, h, w, u8):
    """the pair of a GPU case: synth_stereo_pair, (left, right) read-only"""
    l, r = synth_stereo_pair(seed, h, w, quantise=u8)[:2]
    l.setflags(write=False)
    r.setflags(write=False)
    return l, r


def hostile_pair(seed, h, w):
    """float32 views with NaN, both infinities and +-1e30 sprinkled over a tenth of the pixels of each"""
    l, r = (a.copy() for a in pair(seed, h, w, False))
    rng = np.random.default_rng(seed + 99)
    values = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    for a in (l, r):
        hit = rng.uniform(size=a.shape) < 0.1
        a[hit] = values[rng.integers(0, len(values), int(hit.sum()))]
    return l, r


@functools.lru_cache(maxsize=None)
def _cached_run(seed, h, w, u8, D, paths, p1, p2, uniqueness, lr_max_diff):
    out = run(*pair(seed, h, w, u8), D, paths, p1, p2, uniqueness, lr_max_diff)
    for v in out.values():
        v.setflags(write=False)
    return out


def case(seed, h, w, u8, D, paths, p1=P1, p2=P2, uniqueness=UNIQUENESS, lr_max_diff=LR_MAX_DIFF):
    """the oracle's result for pair(seed, h, w, u8), computed once"""
    return _cached_run(seed, h, w, u8, D, paths, p1, p2, uniqueness, lr_max_diff)
