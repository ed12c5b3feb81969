"""The K33 rate workload and its torch-on-GPU yardstick, shared by tests/test_gpu_stereo_perf.py and tools/stereo_bench.py (no
test module: importing it builds nothing): 16 rectified pairs of 640 x 480 at D = 128 over 8 paths, and census plus semi-global
matching written from stock ops -- a replicate pad and 62 shifted compares for the census, xor and a 16-bit popcount table for
the matching cost (which the yardstick has to materialise, (B, h, w, D) bytes), and for every direction a loop over the path
steps with vectorised torch.minimum over all lines at once; argmin for the winner.  It does less than the timed HIP calls: no
right view, no uniqueness or left-right test, no sub-pixel step."""
import numpy as np
import torch
import torch.nn.functional as F

from gpu_common import DEV
from onnx_image_processing_amd.synth import synth_stereo_pair

PAIRS, H, W, D, PATHS, P1, P2 = 16, 480, 640, 128, 8, 10, 120
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))
BIG = 1 << 14


def workload(pairs=PAIRS, h=H, w=W, distinct=4, u8=True):
    """both views (pairs, h, w) on the GPU: `distinct` synth_stereo_pair scenes (background 8, box 40, ramp 12 .. 90 pixels of
    disparity), repeated"""
    s = [synth_stereo_pair(900 + i, h, w, 8.0, 40.0, (12.0, 90.0), quantise=u8)[:2] for i in range(min(distinct, pairs))]
    pick = [i % len(s) for i in range(pairs)]
    return tuple(torch.from_numpy(np.stack([s[i][j] for i in pick])).to(DEV) for j in range(2))


def torch_census(gray):
    """(B, h, w) -> int64 census words, the header's bit order"""
    g = gray.float()
    h, w = g.shape[-2:]
    pad = F.pad(g[:, None], (4, 4, 3, 3), mode="replicate")[:, 0]
    out = torch.zeros(g.shape, dtype=torch.int64, device=g.device)
    k = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            out |= (pad[:, 3 + dy:3 + dy + h, 4 + dx:4 + dx + w] < g).to(torch.int64) << k
            k += 1
    return out


_table = {}


def _popcount(x):
    if x.device not in _table:
        t = torch.arange(1 << 16, device=x.device)
        _table[x.device] = sum((t >> i) & 1 for i in range(16)).to(torch.int16)
    t = _table[x.device]
    return t[x & 0xffff] + t[(x >> 16) & 0xffff] + t[(x >> 32) & 0xffff] + t[(x >> 48) & 0xffff]


def torch_cost(cl, cr, disparities):
    """C (B, h, w, D) int16"""
    b, h, w = cl.shape
    c = torch.full((b, h, w, disparities), 64, dtype=torch.int16, device=cl.device)
    for d in range(min(disparities, w)):
        c[:, :, d:, d] = _popcount(cl[:, :, d:] ^ cr[:, :, :w - d])
    return c


def _step(c, prev, p1, p2):
    m = prev.amin(-1, keepdim=True)
    lo = F.pad(prev[..., :-1], (1, 0), value=BIG)
    hi = F.pad(prev[..., 1:], (0, 1), value=BIG)
    return c + torch.minimum(torch.minimum(prev, m + p2), torch.minimum(lo, hi) + p1) - m


def torch_aggregate(c, paths=PATHS, p1=P1, p2=P2):
    """S (B, h, w, D) int16: every direction as a loop over its steps, all lines of a step at once"""
    b, h, w, _ = c.shape
    s = torch.zeros_like(c)
    for dy, dx in DIRS[:paths]:
        l = c.clone()
        if dy == 0:
            for x in (range(1, w) if dx > 0 else range(w - 2, -1, -1)):
                l[:, :, x] = _step(c[:, :, x], l[:, :, x - dx], p1, p2)
        else:
            lo, hi = max(dx, 0), w + min(dx, 0)                              # the columns whose predecessor is inside the frame
            for y in (range(1, h) if dy > 0 else range(h - 2, -1, -1)):
                l[:, y, lo:hi] = _step(c[:, y, lo:hi], l[:, y - dy, lo - dx:hi - dx], p1, p2)
        s += l
    return s


def torch_disparity(left, right, disparities=D, paths=PATHS, p1=P1, p2=P2):
    """d* (B, h, w) int64 and S"""
    s = torch_aggregate(torch_cost(torch_census(left), torch_census(right), disparities), paths, p1, p2)
    return s.to(torch.int32).argmin(-1), s
