"""The K34 rate workload and its torch-on-GPU yardstick, shared by tests/test_gpu_rectify_perf.py and tools/rectify_bench.py (no
test module: importing it builds nothing): 256 frames of 640 x 480 uint8 through one map, bilinear, and the same picture from
torch.nn.functional.grid_sample -- the map turned once, outside the timed region, into grid_sample's normalised float32
coordinates (align_corners=True, zeros padding, which is the constant border 0), the frames converted to float32, sampled, rounded
and converted back to uint8 inside it, since that is what a host without the kernel has to run per batch."""
import numpy as np
import torch
import torch.nn.functional as F

import rectify_oracle as RO
from gpu_common import DEV

FRAMES, H, W = 256, 480, 640
# a wide-angle lens of moderate strength: the corners of the ideal camera see past the frame
DIST = np.array([-0.21, 0.05, 0.0008, -0.0011, -0.004, 0.0, 0.0, 0.0])


def cameras(h=H, w=W):
    """(k, dist, k_new): a (h, w) camera and the ideal camera of the same size with a shorter focal length, so that its border
    looks past the source frame"""
    k = np.array([[0.8 * w, 0.0, w / 2.0 - 3.25], [0.0, 0.8 * w, h / 2.0 + 1.5], [0.0, 0.0, 1.0]])
    k_new = np.array([[0.7 * w, 0.0, (w - 1) / 2.0], [0.0, 0.7 * w, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    return k, DIST, k_new


def workload(frames=FRAMES, h=H, w=W, distinct=4, dtype=np.uint8):
    """(frames, h, w) on the GPU: `distinct` smooth textured frames, repeated"""
    rng = np.random.default_rng(910)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(min(distinct, frames)):
        g = np.full((h, w), 128.0)
        for _ in range(12):
            lam, th, ph = np.exp(rng.uniform(np.log(6.0), np.log(90.0))), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
            g += 10.0 * np.sin(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / lam + ph)
        out.append(np.clip(g, 0, 255))
    stack = np.stack([out[i % len(out)] for i in range(frames)])
    return torch.from_numpy(np.rint(stack).astype(np.uint8) if dtype == np.uint8 else stack.astype(np.float32)).to(DEV)


def torch_grid(map_, src_h, src_w):
    """a map (h, w, 2) int32 on the GPU -> grid_sample's grid (1, h, w, 2) float32; a sentinel goes far outside the frame"""
    q = map_.to(torch.float32) / 32.0
    scale = torch.tensor([2.0 / max(src_w - 1, 1), 2.0 / max(src_h - 1, 1)], device=map_.device)
    grid = q * scale - 1.0
    grid[(map_ == RO.OUTSIDE).any(-1)] = -4.0
    return grid[None]


def torch_remap(frames, grid):
    """(B, H, W) uint8 or float32 -> the bilinear picture (B, h, w) float32, before any rounding"""
    b = frames.shape[0]
    return F.grid_sample(frames[:, None].float(), grid.expand(b, -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]


def torch_remap_u8(frames, grid):
    """... and back to uint8, rounded to nearest: what mi_rectify_remap delivers in one pass"""
    return torch_remap(frames, grid).add_(0.5).floor_().clamp_(0, 255).to(torch.uint8)
