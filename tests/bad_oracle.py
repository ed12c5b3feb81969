"""fp64 reference of the sparse BAD descriptors (K4: csrc/bad.hip, K4o: csrc/bad_oriented.hip) with a-priori error
bounds, and the inputs that test_bad_host.py and test_gpu_bad.py both run on.  Plain numpy, no GPU.

A second, plainer statement of SparseBAD.forward (reference descriptor/bad.py:436-576) than oracle/numpy_oracle.py,
which it does not import: a box sum here is the direct sum of the (2r+1)^2 pixels of the replicate-extended image, in
float64 -- no summed-area table, so it shares no structure with the kernels or with that oracle.  Direct sums of
pixels that are multiples of 0.5 are exact; so are the kernels' tables on such images.

What IS reproduced op by op, in float32, is the arithmetic that decides WHERE a box sits, because a centre is a rounded
quantity and one ulp moves it by a pixel:
    valid = y >= 0 ; y, x clamped into the image                                        bad.py:461-466
    rot_dy = ox*sin + oy*cos ; rot_dx = ox*cos - oy*sin    two products, one sum, unfused bad.py:505-509
    pos = keypoint + offset ; g = pos * fp32(2 / (size - 1 + 1e-8)) - 1                 bad.py:469-470,518-535
    ATen grid_sampler, align_corners, border padding: x = ((g + 1) / 2) * (size - 1) ; clip to [0, size - 1] ;
    nearest: nearbyint (half to even); bilinear: floor, weights x - x0 and (x0 + 1) - x
    response = mean1 - mean2 - thr ; raw / sigmoid(-T * response) / (response <= 0) ; x valid ; L2-normalised.

Firm and fragile pairs.  The only legitimate difference between the device and this file is sinf / cosf.  The device
library's worst error for them is taken as TRIG_ULP = 2 ulp: a fall-back, chosen without the ROCm math library's
documented figure at hand (DESIGN.md K4 records it; put the documented figure here once it is).  sin and cos are
evaluated in float64 and rounded once, so they lie within 0.5 ulp of the true value and the device within TRIG_ULP ulp
of it: an integer number of ulps <= TRIG_ULP from ours.  Every pair is therefore evaluated (2 TRIG_ULP + 1)^2 times,
with the sine and the cosine each moved by -TRIG_ULP .. +TRIG_ULP ulp; the results are the pair's CANDIDATES.  A pair
with one distinct candidate is firm: the GPU must give that bit, and that value to the bound below.  Any other pair is
fragile: the GPU's result must be one of the candidates.  Where the image is not made of multiples of 0.5, sums are not
exact in fp64 either, and a pair whose |s1 - s2 - t * area| is within (OW + 1)^2 * 2^-53 * 255 * area (OW: the kernel's
window edge) is fragile on its bit too.

Bounds (u = 2^-24; nothing is fitted to a measurement).
raw, nearest.  The kernels form (s1 - s2) / area - t in fp64 and round it once: half an ulp of the value, plus the
    fp64 roundings of any way to write that (mean1 - mean2 - t included): 2^-52 (2 M + |t|), M = max |pixel|.
    Inexact images add the worst case of a summed-area table in fp64: every entry is the result of at most 2 OW
    additions of partial sums below OW^2 M, eight entries per pair: 8 * 2 OW * 2^-53 * OW^2 * M, over the area.
raw, bilinear.  fp32 throughout: a sample is four products fl(fl(mean) * fl(wx * wy)) (3 roundings each, weights exact
    and summing to 1) and three additions: 6 u M; two samples, their difference (|.| <= 2 M) and the threshold:
    (12 + 2 + 2) u M + u |t|.  A fused multiply-add only removes roundings.
soft.  s = 1 / (1 + expf(c * T)): ds/dz = -s (1 - s) <= 1/4, so the raw bound enters times T s (1 - s) <= T / 4; then
    the product's rounding u |z|, expf's EXP_ULP ulp (2 u relative each) -- all times s (1 - s) --, and on s itself the
    addition's u and the division's DIV_ULP ulp.  2^-126 absolute covers a flushed denormal.
normalised.  v_i / max(sqrt(sum v^2), 1e-12): the sum of P squares in fp32 in ANY order carries (P + 1) u of itself (P
    squares, P - 1 additions, first order) plus 2 sum |v_i| d_i from the terms' own errors d_i; the square root halves
    the relative error and adds SQRT_ULP ulp, the division DIV_ULP ulp.  In the hard mode the sum is a popcount, exact.
Second-order terms: a factor 1.01 (P u < 1e-4)."""
from __future__ import annotations

import functools
import os

import numpy as np

F32 = np.float32
U = 2.0 ** -24
TRIG_ULP = 2            # sinf / cosf of the device library, see above
EXP_ULP = 2             # expf: the same fall-back
SQRT_ULP = 1            # sqrtf and the fp32 division are correctly rounded by default (-fhip-fp32-correctly-rounded-
DIV_ULP = 1             # divide-sqrt); one whole ulp each leaves room
RAW, SOFT, HARD = 0, 1, 2          # MI_BAD_RAW, MI_BAD_SOFT, MI_BAD_HARD
TEMPERATURE = 4.0
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "onnx_image_processing_amd", "data", "bad_tables.npz")


# ------------------------------------------------------------------ pair tables
def pack_geom(box: np.ndarray) -> np.ndarray:
    """(P, 5) x1, x2, y1, y2 (patch frame, offset + 16), r -> the uint32 words mi_sparse_bad takes."""
    b = np.asarray(box).astype(np.uint32)
    return (b[:, 0] | (b[:, 1] << 5) | (b[:, 2] << 10) | (b[:, 3] << 15) | (b[:, 4] << 20)).astype(np.uint32)


def reach(box: np.ndarray) -> float:
    """Largest |offset| + radius of a table in pixels, a hair up: the max_reach that sizes the oriented window."""
    off = np.asarray(box)[:, :4].astype(np.float64) - 16.0
    r = np.maximum(np.hypot(off[:, 0], off[:, 2]), np.hypot(off[:, 1], off[:, 3])) + np.asarray(box)[:, 4]
    return float(r.max()) + 1e-3


def _synthetic(pairs: int, wide: bool):
    """Random boxes of the 32x32 patch frame.  narrow: |offset| + r <= 15 on both axes (the fast plan's geometry check
    passes; reach <= 15 sqrt 2 = 21.3 < 22.5: the 48-pixel window).  wide: |offset| <= 15, any r <= 7, two planted pairs
    on the diagonal with r = 7 (reach 28.2: the 60-pixel window)."""
    rng = np.random.default_rng([pairs, int(wide), 4])
    r = rng.integers(0, 8, pairs)
    lim = np.full(pairs, 15) if wide else 15 - r
    off = rng.integers(-lim[:, None], lim[:, None] + 1, (pairs, 4))
    if wide:
        off[0], r[0] = (15, -15, 15, -15), 7
        off[1], r[1] = (-15, 15, 15, -15), 7
    thr = (rng.standard_normal(pairs) * 8.0).astype(F32)
    return np.concatenate([off + 16, r[:, None]], 1).astype(np.int64), thr


TABLES = ("learned256", "learned512", "syn64", "syn128", "syn320", "syn576", "syn1024", "wide256", "wide512", "tie256",
          "tie256o", "const512")
TIE_INPUTS = ("u8", 2, 64, 80, 95, "int")      # image kind, b, h, w, k, keypoint kind of the two tie cases


def _tie_thresholds(box: np.ndarray, oriented: bool) -> np.ndarray:
    """Thresholds that the tie case's OWN box differences meet exactly.  area is odd, so t = d0 / area is a float only
    for d0 a multiple of area, i.e. integer t: per pair, the non-zero integer t for which most keypoints of the case
    (TIE_INPUTS; oriented: at the case's angles) have s1 - s2 == t * area; a pair no keypoint serves gets the integer
    nearest to its median mean difference.  Image and keypoints do not depend on the table: nothing is circular."""
    kind, b, h, w, k, kps = TIE_INPUTS
    theta = angles("kp", b, k, h, w) if oriented else None
    ref = reference(image(kind, b, h, w), keypoints(kps, b, k, h, w), box, np.zeros(len(box), F32), theta,
                    window=48 if oriented else 34)
    area = (2 * box[:, 4] + 1) ** 2
    d = np.rint(ref["cands"][ref["nominal"]] * area).astype(np.int64)[ref["valid"]]          # (keypoints, P), exact integers
    thr = np.rint(np.median(d, 0) / area)
    for p in range(len(box)):
        m = d[:, p][(d[:, p] % area[p] == 0) & (d[:, p] != 0)] // area[p]
        if m.size:
            values, counts = np.unique(m, return_counts=True)
            thr[p] = values[counts.argmax()]
    return thr.astype(F32)


@functools.lru_cache(maxsize=None)
def table(name: str):
    """box (P, 5) int64, thr (P,) float32."""
    assert name in TABLES, name
    if name.startswith("learned") or name in ("tie256", "tie256o", "const512"):
        t = np.load(_DATA)
        pairs = int(name.rstrip("o")[-3:])
        box, thr = t[f"box_{pairs}"].astype(np.int64), t[f"thr_{pairs}"].astype(F32)
        if name.startswith("tie"):    # exact ties s1 - s2 == t * area with a non-zero product, by the hundred
            thr = _tie_thresholds(box, name.endswith("o"))
        if name == "const512":        # with a constant image every bit is (0 <= t * area)
            thr = np.tile(np.array([0.0, -0.0, 1e-9, -1e-9], F32), pairs // 4)
        return box, thr
    return _synthetic(int(name[3:] if name.startswith("syn") else name[4:]), name.startswith("wide"))


# ------------------------------------------------------------------ images
IMAGE_KINDS = ("u8", "mixed", "unit", "const")


@functools.lru_cache(maxsize=None)
def image(kind: str, b: int, h: int, w: int) -> np.ndarray:
    """(b, h, w) float32.  "u8": uint8-valued texture.  "mixed": member 0 has a +0.5 region (exact in fp64), the last
    member a region scaled by 1.001, one -0.0 pixel, one pixel 256 and one -1 (integers that are not uint8).  "unit":
    the texture / 255.  "const": 77 everywhere."""
    assert kind in IMAGE_KINDS, kind
    rng = np.random.default_rng([b, h, w, 11])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((b, h, w), np.float64)
    for i in range(b):
        ph = rng.random(3) * 6.28
        img[i] = (128 + 70 * np.sin(0.21 * xx + 0.13 * (i + 1) * yy + ph[0]) * np.cos(0.09 * yy - 0.05 * xx + ph[1])
                  + 25 * np.sin(0.9 * xx + ph[2]) * np.sin(0.7 * yy) + 20 * rng.standard_normal((h, w)))
    img = (np.clip(np.rint(img), 0, 255) + 0.0).astype(F32)            # + 0.0: rint(-0.3) is -0.0, which is no uint8 value
    if kind == "const":
        img[:] = 77
    elif kind == "unit":
        img = (img / F32(255)).astype(F32)
    elif kind == "mixed":
        img[0, h // 4:h // 2, w // 4:3 * w // 4] += F32(0.5)
        img[-1, h // 2:, :] *= F32(1.001)
        img[-1, 2, 3] = F32(-0.0)
        img[-1, min(5, h - 1), w - 4] = F32(256)
        img[-1, h // 4, 1] = F32(-1)
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------ keypoints and angles
def _specials(h: int, w: int):
    below, above = np.nextafter(F32(20.5), F32(0)), np.nextafter(F32(20.5), F32(100))
    edges_y, edges_x = (14, 15, 16, h - 16, h - 15, h - 14), (14, 15, 16, w - 16, w - 15, w - 14)
    s = [(10, -3), (0, -0.5), (h + 5, w + 5), (h - 1 + 0.25, 3), (-1, -1), (-0.0, -0.0), (-0.0, 7),
         (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (20.5, 30.5), (below, above), (above, below), (7.25, 9.75)]
    s += list(zip(edges_y, edges_x)) + list(zip(edges_y, reversed(edges_x)))
    return np.array(s, F32)


KEYPOINT_KINDS = ("int", "frac", "chunks", "pixels")


@functools.lru_cache(maxsize=None)
def keypoints(kind: str, b: int, k: int, h: int, w: int) -> np.ndarray:
    """(b, k, 2) float32 (y, x).  Random pixels ("frac": half of them moved off the grid) with the special points
    scattered among them: (-1, -1); valid points left of, below and right of the image, which are clamped; -0.0; the
    corners; the fast path's eligibility edges 14, 15, 16, size - 16, size - 15, size - 14; exact .5 positions and the
    floats either side.  "chunks" (k = 48, b = 2: six 16-keypoint chunks of the chunked general kernel): chunk 0 all
    interior pixels, chunk 1 all fractional, the rest as "frac".  "pixels": random pixels and nothing else."""
    assert kind in KEYPOINT_KINDS, kind
    rng = np.random.default_rng([b, k, h, w, KEYPOINT_KINDS.index(kind)])
    n = b * k
    kp = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], -1).astype(F32)
    if kind in ("frac", "chunks"):
        move = rng.random(n) < 0.5
        kp[move] += rng.choice(np.array([0.25, 0.5, 0.75, 0.3, 0.9999], F32), (int(move.sum()), 2))
    sp = _specials(h, w)
    if kind == "pixels":
        pass
    elif n == 3:
        kp[:] = [(min(15, h - 1), min(15, w - 1)), (10, -3), (h + 5, w + 5)]
    else:
        slots = rng.permutation(n)[:len(sp)]
        kp[slots] = sp[:len(slots)]
    if kind == "chunks":
        assert h >= 32 and w >= 32 and n >= 32
        kp[:16] = np.stack([rng.integers(15, h - 14, 16), rng.integers(15, w - 14, 16)], -1)
        kp[16:32] = kp[:16] + F32(0.5)
    kp = kp.reshape(b, k, 2)
    kp.setflags(write=False)
    return kp


SPECIAL_ANGLES = np.array([j * np.pi / 6 for j in range(-11, 12, 2)] + [j * np.pi / 4 for j in range(-7, 8, 2)]
                          + [0.0, np.pi / 2, -np.pi / 2, np.pi], F32)          # 24 angles


@functools.lru_cache(maxsize=None)
def angles(kind: str, b: int, k: int, h: int, w: int):
    """kind "kp": (b, k) random angles in (-pi, pi), one of them 1e6.  "map": a dense (b, h, w) map of random angles.
    "special": every odd multiple of pi/6 and of pi/4, 0, +-pi/2, pi, in turn.  "zero": 0 (the non-oriented bilinear
    descriptor)."""
    rng = np.random.default_rng([b, k, h, w, 23])
    if kind == "map":
        a = ((rng.random((b, h, w)) * 2 - 1) * np.pi).astype(F32)
    elif kind == "special":
        a = np.resize(SPECIAL_ANGLES, b * k).reshape(b, k).astype(F32)
    elif kind == "zero":
        a = np.zeros((b, k), F32)
    else:
        assert kind == "kp", kind
        a = ((rng.random((b, k)) * 2 - 1) * np.pi).astype(F32)
        a[0, 0] = F32(1e6)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ the reference
def _unnormalised(pos: np.ndarray, size: int) -> np.ndarray:
    """float32, op by op: the normalisation of bad.py and ATen's un-normalisation with align_corners."""
    assert pos.dtype == F32
    scale = F32(2.0 / ((size - 1) + 1e-8))
    g = pos * scale - F32(1)
    x = ((g + F32(1)) / F32(2)) * F32(size - 1)
    assert x.dtype == F32
    return x


def _clip(x: np.ndarray, size: int) -> np.ndarray:
    return np.minimum(np.maximum(x, F32(0)), F32(size - 1))


def nearest_centre(pos: np.ndarray, size: int) -> np.ndarray:
    return np.rint(_clip(_unnormalised(pos, size), size)).astype(np.int64)


def box_sums(plane: np.ndarray, radii) -> dict:
    """{r: (h, w) float64}: at every pixel the direct sum of the (2r+1)^2 box of the replicate-extended plane."""
    h, w = plane.shape
    rmax = max(radii)
    e = np.pad(plane.astype(np.float64), rmax, mode="edge")
    out = {}
    for r in radii:
        acc = np.zeros((h, w), np.float64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                acc += e[rmax + dy:rmax + dy + h, rmax + dx:rmax + dx + w]
        out[int(r)] = acc
    return out


def _ulp_steps(x: np.ndarray, u: int):
    """x moved by -u .. +u float32 ulps: a list of 2u + 1 arrays, x itself in the middle."""
    down, up = [x], [x]
    for _ in range(u):
        down.append(np.nextafter(down[-1], F32(-np.inf)))
        up.append(np.nextafter(up[-1], F32(np.inf)))
    return down[:0:-1] + up


def sample_map(amap: np.ndarray, kp: np.ndarray) -> np.ndarray:
    """bad.py:490-500: the dense angle map (b, h, w) at the clamped keypoints, nearest: (b, k)."""
    b, h, w = amap.shape
    cy = nearest_centre(_clip(kp[:, :, 0], h), h)
    cx = nearest_centre(_clip(kp[:, :, 1], w), w)
    return np.stack([amap[i, cy[i], cx[i]] for i in range(b)]).astype(F32)


def reference(img, kp, box, thr, theta=None, bilinear=False, window=34, trig_ulp=TRIG_ULP) -> dict:
    """img (B, H, W) float32, kp (B, K, 2), box (P, 5), thr (P,) float32, theta (B, K) float32 or None (not oriented).
    `window`: the edge OW of the kernel's window (34: K4; 48 or 60: K4o), for the summation bounds.  Returns
      valid (B, K) bool; cands (C, B, K, P) float64, the centred response of every candidate, cands[nominal] the one
      with our own sine and cosine; raw_bound (C, B, K, P); firm (B, K, P): one distinct candidate; may1 / may0
      (B, K, P): a candidate (or the summation band) allows the bit to be 1 / 0; bits = the nominal bit;
      fragile (B, K, P): not firm, or within the summation band (bilinear: the bit may be either)."""
    img = np.asarray(img)
    kp = np.asarray(kp)
    assert img.dtype == F32 and kp.dtype == F32
    bsz, h, w = img.shape
    box = np.asarray(box).astype(np.int64)
    t32 = np.asarray(thr, F32)
    t = t32.astype(np.float64)
    rad = box[:, 4]
    area = ((2 * rad + 1) ** 2).astype(np.float64)
    radii = sorted(set(int(r) for r in rad))
    ridx = np.searchsorted(radii, rad)
    ox1, ox2, oy1, oy2 = [(box[:, i] - 16).astype(F32) for i in range(4)]
    valid = kp[:, :, 0] >= F32(0)
    ky, kx = _clip(kp[:, :, 0], h)[:, :, None], _clip(kp[:, :, 1], w)[:, :, None]
    sums = [np.stack([s[r] for r in radii]) for s in (box_sums(img[i], radii) for i in range(bsz))]   # per image (nr, h, w)
    exact = np.array([bool(np.all(img[i] * 2 == np.rint(img[i] * 2))) for i in range(bsz)])
    big = float(np.abs(img).max())
    sat_err = 8 * 2 * window * 2.0 ** -53 * window * window * big          # on s1 - s2, inexact images only
    band = (window + 1) ** 2 * 2.0 ** -53 * 255 * area                     # the bit's summation band, on s1 - s2 - t * area

    if theta is None:
        trig = [(None, None)]
    else:
        th = np.asarray(theta, F32).astype(np.float64)
        sins = _ulp_steps(np.sin(th).astype(F32)[:, :, None], trig_ulp)
        coss = _ulp_steps(np.cos(th).astype(F32)[:, :, None], trig_ulp)
        trig = [(s, c) for s in sins for c in coss]
    nominal = len(trig) // 2

    def positions(oxv, oyv, s, c):
        if s is None:
            return ky + oyv[None, None, :], kx + oxv[None, None, :]
        dy = oxv[None, None, :] * s + oyv[None, None, :] * c               # two rounded products, one rounded sum
        dx = oxv[None, None, :] * c - oyv[None, None, :] * s
        assert dy.dtype == F32 and dx.dtype == F32
        return ky + dy, kx + dx

    def gather(cy, cx):                                                    # box sums at integer centres (B, K, P)
        return np.stack([sums[i][ridx[None, :], cy[i], cx[i]] for i in range(bsz)])

    def mean_bilinear(py, px):
        iy, ix = _clip(_unnormalised(py, h), h), _clip(_unnormalised(px, w), w)
        y0f, x0f = np.floor(iy), np.floor(ix)
        wy1, wx1, wy0, wx0 = iy - y0f, ix - x0f, (y0f + F32(1)) - iy, (x0f + F32(1)) - ix     # exact in float32
        y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)     # out of range: its weight is 0
        f = np.float64
        return (gather(y0, x0) * (wx0.astype(f) * wy0) + gather(y0, x1) * (wx1.astype(f) * wy0)
                + gather(y1, x0) * (wx0.astype(f) * wy1) + gather(y1, x1) * (wx1.astype(f) * wy1)) / area

    cands, diffs = [], []
    for s, c in trig:
        p1y, p1x = positions(ox1, oy1, s, c)
        p2y, p2x = positions(ox2, oy2, s, c)
        if bilinear:
            cands.append((mean_bilinear(p1y, p1x) - mean_bilinear(p2y, p2x)) - t)
        else:
            d = gather(nearest_centre(p1y, h), nearest_centre(p1x, w)) - gather(nearest_centre(p2y, h), nearest_centre(p2x, w))
            diffs.append(d)
            cands.append(d / area - t)
    cands = np.stack(cands)
    inexact = (~exact)[None, :, None, None]
    if bilinear:
        raw_bound = np.broadcast_to(1.01 * U * (16 * big + np.abs(t)), cands.shape).copy()
        ones, zeros = (cands <= raw_bound).any(0), (cands >= -raw_bound).any(0)
        firm = np.ones(cands.shape[1:], bool)                              # floats: nearest candidate, see module text
        fragile = ones & zeros
    else:
        diffs = np.stack(diffs)
        half_ulp = 0.5 * np.spacing(np.abs(cands).astype(F32)).astype(np.float64)
        raw_bound = half_ulp + 2.0 ** -52 * (2 * big + np.abs(t)) + inexact * (sat_err / area)
        near = inexact & (np.abs(diffs - t * area) <= band)                # t * area is exact in fp64
        ones, zeros = ((diffs <= t * area) | near).any(0), ((diffs > t * area) | near).any(0)
        firm = (cands == cands[nominal]).all(0)
        fragile = ~firm | near.any(0)
    v3 = valid[:, :, None]
    return dict(valid=valid, cands=cands, nominal=nominal, raw_bound=raw_bound, firm=firm | ~v3,
                may1=ones & v3, may0=zeros | ~v3, bits=(cands[nominal] <= 0 if bilinear else diffs[nominal] <= t * area) & v3,
                fragile=fragile & v3, pairs=len(t32))


# ------------------------------------------------------------------ the five forms and their bounds
def sigmoid(c: np.ndarray, c_bound: np.ndarray, temperature: float):
    """s = sigmoid(-T c) in fp64 and the bound of the module text."""
    tt = float(F32(temperature))
    z = c * tt
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(z))
    bound = 1.01 * (s * (1 - s) * (tt * c_bound + U * np.abs(z) + 2 * U * EXP_ULP) + s * (U + 2 * U * DIV_ULP)) + 2.0 ** -126
    return s, bound


def normalised(v: np.ndarray, v_bound, exact_sum: bool = False):
    """v (..., P) float64 -> v / max(|v|, 1e-12) and the bound of the module text; v_bound: the terms' own errors."""
    v = np.asarray(v, np.float64)
    d = np.broadcast_to(np.asarray(v_bound, np.float64), v.shape)
    p = v.shape[-1]
    ss = (v * v).sum(-1, keepdims=True)
    nrm = np.maximum(np.sqrt(ss), 1e-12)
    safe = np.maximum(ss, 1e-300)
    rel_ss = (0.0 if exact_sum else (p + 1) * U) + 2 * (np.abs(v) * d).sum(-1, keepdims=True) / safe
    rel = 0.5 * rel_ss + 2 * U * (SQRT_ULP + DIV_ULP)
    return v / nrm, 1.01 * (d / nrm + np.abs(v) / nrm * rel)


def worst_ratio(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    """max over the entries of min over the candidates (leading axis of want / bound, if any) of |got - want| / bound;
    an entry whose bound is 0 must be equal."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if ratio.ndim > got.ndim:
        ratio = ratio.min(0)
    return float(ratio.max()) if ratio.size else 0.0


def forms(ref: dict, temperature: float = TEMPERATURE) -> dict:
    """The descriptor in its five forms from the NOMINAL candidate, each (value, bound), float64 (B, K, P): raw, raw_n,
    soft, soft_n (normalised), hard; hard_n comes with an exact sum.  Rows of invalid keypoints are 0."""
    v3 = ref["valid"][:, :, None]
    c, cb = ref["cands"][ref["nominal"]] * v3, ref["raw_bound"][ref["nominal"]] * v3
    s, sb = sigmoid(ref["cands"][ref["nominal"]], ref["raw_bound"][ref["nominal"]], temperature)
    s, sb = s * v3, sb * v3
    hard = ref["bits"].astype(np.float64)
    return dict(raw=(c, cb), raw_n=normalised(c, cb), soft=(s, sb), soft_n=normalised(s, sb), hard=(hard, np.zeros_like(hard)),
                hard_n=normalised(hard, 0.0, exact_sum=True))


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """bool (..., P) -> uint32 (..., P / 32): bit p in word p // 32 at position p % 32."""
    b = np.asarray(bits, bool)
    w = b.reshape(*b.shape[:-1], b.shape[-1] // 32, 32).astype(np.uint64)
    return (w << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words: np.ndarray, pairs: int) -> np.ndarray:
    w = np.asarray(words).view(np.uint32)
    return (((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(*w.shape[:-1], -1)[..., :pairs]).astype(bool)


# ------------------------------------------------------------------ checks shared by the host and the GPU tests
def check_bits(ref: dict, bits: np.ndarray, what: str) -> None:
    """bits (B, K, P) bool: every firm pair has the reference's bit, every fragile pair a candidate's."""
    bits = np.asarray(bits, bool)
    wrong = (bits & ~ref["may1"]) | (~bits & ~ref["may0"])
    at = np.argwhere(wrong)
    assert at.size == 0, (f"{what}: {len(at)} bits are no candidate's, first at (image, keypoint, pair) {at[0].tolist()}: "
                          f"got {int(bits[tuple(at[0])])}, response {ref['cands'][(ref['nominal'], *at[0])]!r}")


def float_ratio(ref: dict, got: np.ndarray, form: str, temperature: float = TEMPERATURE) -> float:
    """Worst error / bound of an UN-normalised float descriptor (B, K, P) in form "raw", "soft" or "hard" against the
    candidates."""
    v3 = ref["valid"][None, :, :, None]
    if form == "raw":
        want, bound = ref["cands"] * v3, ref["raw_bound"] * v3
    elif form == "soft":
        want, bound = sigmoid(ref["cands"], ref["raw_bound"], temperature)
        want, bound = want * v3, bound * v3
    else:
        assert form == "hard"
        got = np.asarray(got)
        assert np.isin(got, (0.0, 1.0)).all(), "a hard descriptor holds something other than 0 and 1"
        check_bits(ref, got != 0, "hard descriptor")
        return 0.0
    return worst_ratio(got, want, bound)


def normalised_ratio(got_n: np.ndarray, got_plain: np.ndarray, hard: bool) -> float:
    """Worst error / bound of a normalised descriptor against the fp64 normalisation of the same call's un-normalised
    output (which float_ratio has tied to the candidates): rows with fragile pairs need no special case."""
    want, bound = normalised(np.asarray(got_plain, np.float64), 0.0, exact_sum=hard)
    return worst_ratio(got_n, want, bound)


# ------------------------------------------------------------------ the cases of both test files
def _case(name, tab, img, b, h, w, k, kps, ang=None, bilinear=False, wide_window=False):
    return dict(name=name, table=tab, image=img, b=b, h=h, w=w, k=k, kps=kps, angles=ang, bilinear=bilinear,
                window=(60 if wide_window else 48) if ang else 34, wide_window=wide_window)


# K4.  Every table size on an image with windows of every kind; the edge shapes (31x64 and 8x8 lie below the fast
# path's 32-pixel line, 8x8 below the window); ragged last workgroups (k = 37, 1); chunks with nothing / everything flagged
PLAIN_CASES = [_case(f"{t}-mixed-64x80", t, "mixed", 2, 64, 80, 37, "frac")
               for t in ("learned256", "learned512", "syn64", "syn128", "syn320", "syn576", "syn1024")]
PLAIN_CASES += [
    _case("learned512-u8-64x80-chunks", "learned512", "u8", 2, 64, 80, 48, "chunks"),
    _case("syn320-u8-64x80-chunks", "syn320", "u8", 2, 64, 80, 48, "chunks"),
    _case("tie256-u8-64x80", "tie256", *TIE_INPUTS),
    _case("const512-const-33x45", "const512", "const", 2, 33, 45, 37, "frac"),
    _case("learned256-unit-33x45", "learned256", "unit", 2, 33, 45, 37, "frac"),
    _case("learned256-mixed-32x32", "learned256", "mixed", 3, 32, 32, 37, "frac"),
    _case("learned512-mixed-32x40-k1", "learned512", "mixed", 3, 32, 40, 1, "int"),
    _case("syn128-u8-31x64", "syn128", "u8", 2, 31, 64, 37, "frac"),
    _case("learned256-u8-31x64", "learned256", "u8", 2, 31, 64, 37, "int"),
    _case("learned256-mixed-33x45", "learned256", "mixed", 3, 33, 45, 37, "frac"),
    _case("learned512-u8-8x8", "learned512", "u8", 3, 8, 8, 37, "frac"),
    _case("syn1024-u8-96x128", "syn1024", "u8", 2, 96, 128, 37, "int"),
]
# K4o.  wide_window: the call states no reach (max_reach = 0) or the table's own, above 22.5: the 60-pixel window
ORIENTED_CASES = [
    _case("learned512-mixed-48", "learned512", "mixed", 2, 64, 80, 37, "frac", "kp"),
    _case("learned256-mixed-48", "learned256", "mixed", 2, 64, 80, 37, "frac", "kp"),
    _case("learned512-mixed-60", "learned512", "mixed", 2, 64, 80, 37, "frac", "kp", wide_window=True),
    _case("learned256-mixed-60", "learned256", "mixed", 2, 64, 80, 37, "frac", "kp", wide_window=True),
    _case("wide256-mixed-60", "wide256", "mixed", 2, 64, 80, 37, "frac", "kp", wide_window=True),
    _case("wide512-u8-60", "wide512", "u8", 2, 96, 128, 37, "int", "kp", wide_window=True),
    _case("learned512-u8-48", "learned512", "u8", 2, 64, 80, 37, "frac", "kp"),
    _case("learned512-mixed-48-map", "learned512", "mixed", 2, 64, 80, 37, "frac", "map"),
    _case("learned256-u8-60-map", "learned256", "u8", 3, 33, 45, 37, "int", "map", wide_window=True),
    _case("learned512-u8-48-special", "learned512", "u8", 2, 64, 80, 24, "pixels", "special"),
    _case("learned256-u8-60-special", "learned256", "u8", 2, 64, 80, 24, "pixels", "special", wide_window=True),
    _case("syn128-mixed-48", "syn128", "mixed", 2, 64, 80, 37, "frac", "kp"),
    _case("syn1024-mixed-48", "syn1024", "mixed", 2, 64, 80, 37, "frac", "kp"),
    _case("syn64-u8-60-k1", "syn64", "u8", 3, 32, 40, 1, "int", "kp", wide_window=True),
    _case("learned256-unit-48", "learned256", "unit", 2, 33, 45, 37, "frac", "kp"),
    _case("learned512-u8-48-31x64", "learned512", "u8", 2, 31, 64, 37, "frac", "kp"),
    _case("learned256-mixed-60-8x8", "learned256", "mixed", 3, 8, 8, 37, "frac", "kp", wide_window=True),
    _case("tie256o-u8-48", "tie256o", *TIE_INPUTS, "kp"),
    _case("const512-const-48", "const512", "const", 2, 33, 45, 37, "frac", "kp"),
    _case("learned256-mixed-bilinear-zero", "learned256", "mixed", 2, 64, 80, 37, "frac", "zero", bilinear=True, wide_window=True),
    _case("learned512-mixed-bilinear", "learned512", "mixed", 2, 64, 80, 37, "frac", "kp", bilinear=True, wide_window=True),
    _case("syn128-u8-bilinear", "syn128", "u8", 2, 33, 45, 37, "frac", "kp", bilinear=True, wide_window=True),
]
FRAGILE_CAP, FRAGILE_CAP_SPECIAL = 0.005, 0.25


def inputs(case: dict) -> dict:
    """image (b, h, w), kp (b, k, 2), box, thr, geom, and for an oriented case theta (b, k) -- the angle every keypoint
    gets -- with amap, the dense map it came from, when the case passes a map."""
    box, thr = table(case["table"])
    b, h, w, k = case["b"], case["h"], case["w"], case["k"]
    out = dict(image=image(case["image"], b, h, w), kp=keypoints(case["kps"], b, k, h, w), box=box, thr=thr,
               geom=pack_geom(box), theta=None, amap=None)
    if case["angles"] == "map":
        out["amap"] = angles("map", b, k, h, w)
        out["theta"] = sample_map(out["amap"], out["kp"])
    elif case["angles"]:
        out["theta"] = angles(case["angles"], b, k, h, w)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name: str) -> dict:
    case = CASE[name]
    x = inputs(case)
    return reference(x["image"], x["kp"], x["box"], x["thr"], x["theta"], case["bilinear"], case["window"])


def expected(case: dict) -> dict:
    """reference() of a case, computed once per process and shared: treat it as read-only."""
    return _expected(case["name"])


def fragile_share(ref: dict) -> float:
    n = int(ref["valid"].sum()) * ref["pairs"]
    return float(ref["fragile"].sum()) / max(n, 1)


CASE = {c["name"]: c for c in PLAIN_CASES + ORIENTED_CASES}
assert len(CASE) == len(PLAIN_CASES) + len(ORIENTED_CASES)
