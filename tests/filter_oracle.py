"""numpy / plain-Python oracle of K35 (include/mi355x_match_filter.h): validity and adjacency, connected components by flood fill,
the speckle filter and the median, restated from the header's definitions and nothing cleverer.  Also the frames the filter tests
share.  No test module: importing it computes nothing."""
import functools

import numpy as np

NO_LABEL = -1
SPECKLE = 3
TILE_H, TILE_W = 16, 64
F32 = np.float32


def valid(values, min_valid):
    v = np.asarray(values)
    if v.dtype == np.uint8:
        return v.astype(np.int64) >= int(min_valid)
    with np.errstate(invalid="ignore"):
        return v >= F32(min_valid)


def _near(a, b, max_diff):
    if a.dtype == np.uint8:
        return np.abs(a.astype(np.int64) - b.astype(np.int64)) <= int(max_diff)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((a - b).astype(F32)) <= F32(max_diff)


def joins(values, min_valid, max_diff):
    """(h, w) -> right (h, w - 1), down (h - 1, w) booleans: the pixel is joined to its right / lower neighbour"""
    v, ok = np.asarray(values), valid(values, min_valid)
    return ok[:, :-1] & ok[:, 1:] & _near(v[:, :-1], v[:, 1:], max_diff), ok[:-1] & ok[1:] & _near(v[:-1], v[1:], max_diff)


def components(values, min_valid, max_diff):
    """one frame (h, w) uint8 or float32 -> labels (h, w) int32 (the smallest y * w + x of the component, -1 on an invalid pixel),
    sizes (h, w) int32 (0 on an invalid pixel): a flood fill in raster order, so that a component's first pixel is its label"""
    v = np.asarray(values)
    h, w = v.shape
    ok = valid(v, min_valid)
    right, down = joins(v, min_valid, max_diff)
    right, down, okl = right.tolist(), down.tolist(), ok.tolist()
    labels = [[NO_LABEL] * w for _ in range(h)]
    sizes = np.zeros((h, w), np.int32)
    for y0 in range(h):
        for x0 in range(w):
            if not okl[y0][x0] or labels[y0][x0] != NO_LABEL:
                continue
            label = y0 * w + x0
            labels[y0][x0] = label
            stack, members = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                members.append((y, x))
                for ny, nx, joined in ((y, x + 1, x + 1 < w and right[y][x]), (y, x - 1, x > 0 and right[y][x - 1]),
                                       (y + 1, x, y + 1 < h and down[y][x]), (y - 1, x, y > 0 and down[y - 1][x])):
                    if joined and labels[ny][nx] == NO_LABEL:
                        labels[ny][nx] = label
                        stack.append((ny, nx))
            ys, xs = zip(*members)
            sizes[list(ys), list(xs)] = len(members)
    return np.array(labels, np.int32).reshape(h, w), sizes


def speckle(x, max_size, max_diff, min_valid=0.0, invalid_value=-1.0, sizes=None):
    """one float32 frame -> (out float32, removed uint8)"""
    x = np.asarray(x, F32)
    ok = valid(x, min_valid)
    if sizes is None:
        sizes = components(x, min_valid, max_diff)[1]
    keep = ok & (sizes > max_size)
    out = np.where(keep, x, F32(invalid_value)).astype(F32)
    return out, (ok & ~keep).astype(np.uint8)


def key(x):
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def median(x, k=3, min_valid=0.0, invalid_value=-1.0):
    """one float32 frame -> float32: rank (n - 1) // 2 among the n valid taps of the k x k window (replicate border)"""
    x = np.asarray(x, F32)
    h, w = x.shape
    r = k // 2
    pad = np.pad(x, r, mode="edge")
    taps = np.stack([pad[r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    ok = valid(taps, min_valid)
    keys = np.sort(np.where(ok, key(taps).reshape(taps.shape), np.uint32(0xFFFFFFFF)), axis=0)
    n = ok.sum(0)
    picked = np.take_along_axis(keys, np.maximum((n - 1) // 2, 0)[None], 0)[0]
    return np.where(valid(x, min_valid), unkey(picked).reshape(h, w), F32(invalid_value)).astype(F32)


def disparity_filter(disparity, code, speckle_size=0, speckle_range=1.0, median_k=0):
    """pytorch_model.stereo.DisparityFilter on one frame: the median first, then the speckle filter; the code of a dropped pixel"""
    d, c = np.asarray(disparity, F32), np.array(code, np.uint8)
    if median_k:
        d = median(d, median_k, 0.0, -1.0)
    if speckle_size > 0:
        d, removed = speckle(d, speckle_size, speckle_range, 0.0, -1.0)
        c[removed != 0] = SPECKLE
    return d, c


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def constant(h, w):
    return np.full((h, w), 5.0, F32)


def alternating(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((y + x) % 2 == 0, 0.0, 10.0).astype(F32)


def spiral(h, w):
    """a one-pixel-wide spiral of 5.0 from the corner inwards over a background of -1, the arms one pixel apart"""
    on = np.zeros((h, w), bool)

    def free(y, x, dy, dx):
        ny, nx = y + dy, x + dx
        if not (0 <= ny < h and 0 <= nx < w) or on[ny, nx]:
            return False
        ay, ax = ny + dy, nx + dx
        return not (0 <= ay < h and 0 <= ax < w and on[ay, ax])
    y, x, dy, dx = 0, 0, 0, 1
    on[0, 0] = True
    for _ in range(h * w):
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        on[y, x] = True
    return np.where(on, 5.0, -1.0).astype(F32)


def comb(h, w):
    """a serpentine: every second row whole, joined to the next whole row by one pixel at alternating ends"""
    on = np.zeros((h, w), bool)
    on[0::2] = True
    on[1::4, w - 1] = True
    on[3::4, 0] = True
    return np.where(on, 5.0, -1.0).astype(F32)


def percolation(h, w, seed):
    return np.where(np.random.default_rng(seed).uniform(size=(h, w)) < 0.6, 7.0, -1.0).astype(F32)


def ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (0.25 * x + 0.5 * y).astype(F32)


def steps(h, w):
    return (0.25 * np.random.default_rng(5).integers(0, 6, (h, w))).astype(F32)


def hostile(h, w):
    """steps with NaN, both infinities, -0.0 and 1e30 in a tenth of the pixels"""
    a = steps(h, w)
    rng = np.random.default_rng(99)
    hit = rng.uniform(size=a.shape) < 0.1
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30], F32)
    a[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    return a


def classes(h, w):
    """a uint8 map of three classes in blobs of 3 x 3"""
    coarse = np.random.default_rng(3).integers(0, 3, ((h + 2) // 3, (w + 2) // 3))
    return np.repeat(np.repeat(coarse, 3, 0), 3, 1)[:h, :w].astype(np.uint8)


def stereo_disparity(h, w, seed=11):
    import stereo_oracle as SO
    return np.array(SO.case(seed, h, w, False, 64, 8)["disparity"])


# name -> (frame maker, min_valid, max_diff); float32 but for "classes*"
PATTERNS = {
    "constant": (constant, 0.0, 1.0), "alternating": (alternating, 0.0, 1.0), "spiral": (spiral, 0.0, 1.0), "comb": (comb, 0.0, 1.0),
    "percolation0": (lambda h, w: percolation(h, w, 0), 0.0, 1.0), "percolation1": (lambda h, w: percolation(h, w, 1), 0.0, 1.0),
    "percolation2": (lambda h, w: percolation(h, w, 2), 0.0, 1.0),
    "ramp025": (ramp, 0.0, 0.25), "ramp05": (ramp, 0.0, 0.5), "steps025": (steps, 0.0, 0.25), "steps05": (steps, 0.25, 0.5),
    "hostile": (hostile, 0.0, 0.5), "hostile_all": (hostile, -np.inf, 0.25),
    "classes": (classes, 0, 0), "classes1": (classes, 1, 1),
}
FLOAT_PATTERNS = [n for n in PATTERNS if not n.startswith("classes")]


@functools.lru_cache(maxsize=None)
def case(name, h, w):
    """(values, min_valid, max_diff, labels, sizes) of a pattern, computed once, read-only"""
    make, min_valid, max_diff = PATTERNS[name]
    values = make(h, w)
    labels, sizes = components(values, min_valid, max_diff)
    for a in (values, labels, sizes):
        a.setflags(write=False)
    return values, min_valid, max_diff, labels, sizes


def invalid_for(min_valid):
    """an invalid_value the entries accept next to min_valid"""
    return F32(np.nan) if np.isneginf(min_valid) else F32(min_valid - 1.0)
