"""The torch-on-GPU yardstick of K35 and the workload of its rate test: connected components from stock ops -- every valid pixel
starts with its own index, a pass replaces a label by the minimum over the pixel and its joined 4-neighbours (a masked 3 x 3
cross), passes repeat until nothing changes, then torch.bincount gives the sizes -- and the speckle filter on top of it.  The
number of passes is the longest shortest path inside a component, so the yardstick is the textbook formulation and not a
tuned one.  No test module."""
import numpy as np
import torch

from gpu_common import DEV

FRAMES, H, W = 16, 480, 640
MAX_SIZE, MAX_DIFF = 30, 1.0
CHECK_EVERY = 16
BIG = 1 << 30


def workload_numpy(frames=FRAMES, h=H, w=W):
    """`frames` disparity maps as a stereo matcher leaves them, four distinct ones repeated: a background plane at 4, a ramp from 6
    to 16 over the lowest third, a box at 20 (synth_stereo_pair's layout: large components), 300 rectangular blobs of 1 to 6
    pixels a side at random disparities (the speckles), and 5 % of the pixels rejected (-1), at random"""
    out = []
    for seed in range(min(frames, 4)):
        rng = np.random.default_rng(700 + seed)
        y, x = np.mgrid[0:h, 0:w]
        d = np.full((h, w), 4.0, np.float32)
        ramp = y >= h - h // 3
        d[ramp] = (6.0 + 10.0 * x / (w - 1))[ramp]
        d[h // 5:h // 2, w // 3:2 * w // 3] = 20.0
        for _ in range(300):
            by, bx, sy, sx = rng.integers(0, h), rng.integers(0, w), rng.integers(1, 7), rng.integers(1, 7)
            d[by:by + sy, bx:bx + sx] = rng.uniform(30.0, 60.0)
        d[rng.uniform(size=(h, w)) < 0.05] = -1.0
        out.append(d)
    return np.stack([out[i % len(out)] for i in range(frames)])


def workload(frames=FRAMES, h=H, w=W):
    return torch.from_numpy(workload_numpy(frames, h, w)).to(DEV)


def torch_components(x, min_valid, max_diff):
    """(B, h, w) float32 -> labels (B, h, w) int32 (-1 on invalid pixels), sizes (B, h, w) int32"""
    b, h, w = x.shape
    ok = x >= min_valid
    right = ok[:, :, :-1] & ok[:, :, 1:] & ((x[:, :, :-1] - x[:, :, 1:]).abs() <= max_diff)
    down = ok[:, :-1] & ok[:, 1:] & ((x[:, :-1] - x[:, 1:]).abs() <= max_diff)
    big = torch.full((), BIG, dtype=torch.int32, device=x.device)
    index = torch.arange(h * w, dtype=torch.int32, device=x.device).view(1, h, w).expand(b, h, w)
    labels = torch.where(ok, index, big)
    while True:
        before = labels
        for _ in range(CHECK_EVERY):
            new = labels.clone()
            new[:, :, :-1] = torch.minimum(new[:, :, :-1], torch.where(right, labels[:, :, 1:], big))
            new[:, :, 1:] = torch.minimum(new[:, :, 1:], torch.where(right, labels[:, :, :-1], big))
            new[:, :-1] = torch.minimum(new[:, :-1], torch.where(down, labels[:, 1:], big))
            new[:, 1:] = torch.minimum(new[:, 1:], torch.where(down, labels[:, :-1], big))
            labels = new
        if torch.equal(labels, before):
            break
    frame = torch.arange(b, device=x.device).view(b, 1, 1) * (h * w)
    flat = torch.where(ok, labels.long() + frame, torch.zeros((), dtype=torch.int64, device=x.device))
    counts = torch.bincount(flat[ok], minlength=b * h * w)
    sizes = torch.where(ok, counts[flat], torch.zeros((), dtype=torch.int64, device=x.device)).to(torch.int32)
    return torch.where(ok, labels, torch.full((), -1, dtype=torch.int32, device=x.device)), sizes


def torch_speckle(x, max_size=MAX_SIZE, max_diff=MAX_DIFF, min_valid=0.0, invalid_value=-1.0):
    _, sizes = torch_components(x, min_valid, max_diff)
    return torch.where(sizes > max_size, x, torch.full((), invalid_value, dtype=x.dtype, device=x.device))
