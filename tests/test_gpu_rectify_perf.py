"""K34 rate: 256 frames of 640 x 480 uint8 through one map, bilinear, against the torch-on-GPU formulation from
torch.nn.functional.grid_sample (tests/rectify_torch.py).  Only "faster than the yardstick" is asserted; the time and the
fraction of the traffic floor, batch * (src + dst bytes) + map bytes at the achievable HBM rate, are printed.  A separate test
shows that the yardstick computes the same picture within its own float tolerance.  The measured times are in README.md and
DESIGN.md."""
import numpy as np
import torch

import rectify_oracle as RO
from gpu_common import GPU_PERF, gpu, time_ms
from onnx_image_processing_amd import ops
from rectify_torch import FRAMES, H, W, cameras, torch_grid, torch_remap, torch_remap_u8, workload

pytestmark = GPU_PERF

HBM_BYTES_PER_S = 6.3e12                                                       # achievable, not the 8 TB/s of the data sheet


def test_torch_formulation_computes_the_same_picture():
    """a small frame, float32 and uint8: grid_sample un-normalises its float32 grid, which moves a tap weight by about
    2^-22 * extent, a few 1e-5 of a pixel, so its picture is the kernel's within 255 * 2 * 1e-4 = 0.05 gray levels where the
    footprint is inside the frame; the uint8 pictures then differ by at most one level, and only beside a rounding tie"""
    h, w = 120, 200
    k, dist, k_new = cameras(h, w)
    map_, mask = ops.rectify_map(k, dist, (h, w), k_new)
    assert 0.5 < mask.float().mean() < 1.0 and bool((map_[..., 0] == RO.OUTSIDE).any())
    grid = torch_grid(map_, h, w)
    inside = mask.bool()
    f32 = workload(3, h, w, 3, np.float32)
    got, want = ops.rectify_remap(f32, map_), torch_remap(f32, grid)
    worst = float((got - want)[:, inside].abs().max())
    print(f"grid_sample against the kernel, float32: {worst:.2e} gray levels")
    assert worst <= 0.05
    assert bool((got[:, (map_[..., 0] == RO.OUTSIDE)] == 0).all()) and bool((want[:, (map_[..., 0] == RO.OUTSIDE)] == 0).all())
    u8 = workload(3, h, w, 3)
    got8, want8 = ops.rectify_remap(u8, map_), torch_remap_u8(u8, grid)
    diff = (got8.int() - want8.int())[:, inside].abs()
    exact = torch_remap(u8, grid)[:, inside]
    assert int(diff.max()) <= 1 and bool((((exact - exact.floor()) - 0.5).abs()[diff == 1] <= 0.05).all())
    assert float((diff == 0).float().mean()) > 0.99


def test_hip_remap_beats_grid_sample_for_256_frames():
    k, dist, k_new = cameras()
    map_, _ = ops.rectify_map(k, dist, (H, W), k_new)
    grid = torch_grid(map_, H, W)
    frames = workload()
    hip = time_ms(lambda: ops.rectify_remap(frames, map_))
    hip_nearest = time_ms(lambda: ops.rectify_remap(frames, map_, ops.RECTIFY_NEAREST))
    hip_map = time_ms(lambda: ops.rectify_map(k, dist, (H, W), k_new))
    ref = time_ms(lambda: torch_remap_u8(frames, grid), iters=5, warmup=2)
    floor_bytes = FRAMES * 2 * H * W + H * W * 8
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    print(f"{FRAMES} frames of {W}x{H} uint8, linear: HIP {hip:.3f} ms ({1e3 * hip / FRAMES:.2f} us a frame, {floor_bytes / hip / 1e9:.3f} TB/s, "
          f"{100 * floor_ms / hip:.0f} % of the traffic floor of {floor_ms:.3f} ms), nearest {hip_nearest:.3f} ms, the map {hip_map:.3f} ms; "
          f"grid_sample {ref:.3f} ms ({ref / hip:.1f}x)")
    assert hip < ref
