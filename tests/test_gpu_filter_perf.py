"""K35 rate: the speckle filter on 16 disparity maps of 640 x 480 (tests/filter_torch.py's workload: large planes plus blobs, 5 %
rejected pixels) against the torch-on-GPU formulation from stock ops (iterated masked minimum, then bincount).  Only "faster than
the yardstick" is asserted; a separate test shows that the yardstick computes the kernels' labels and sizes.  Printed besides: the
share of the traffic floor (one float32 read and one written per pixel: 8 bytes a pixel), the two extreme inputs on their own
(one component; all singletons), the labelling alone and the two medians.  The measured times are in README.md and DESIGN.md."""
import numpy as np
import torch

import filter_oracle as FO
from filter_torch import FRAMES, H, MAX_DIFF, MAX_SIZE, W, torch_components, torch_speckle, workload
from gpu_common import GPU_PERF, gpu, time_ms
from onnx_image_processing_amd import ops

pytestmark = GPU_PERF

HBM_BYTES_PER_S = 6.3e12


def test_torch_formulation_computes_the_same_labels_and_sizes():
    frames = gpu(np.stack([FO.case(name, 37, 83)[0] for name in ("percolation0", "spiral", "steps025", "constant")]))
    labels, sizes = ops.filter_components(frames, 0.0, 0.5)
    ref_labels, ref_sizes = torch_components(frames, 0.0, 0.5)
    assert torch.equal(labels, ref_labels) and torch.equal(sizes, ref_sizes)
    assert torch.equal(ops.filter_speckle(frames, 30, 0.5), torch_speckle(frames, 30, 0.5))


def test_hip_speckle_filter_beats_torch_on_gpu_for_16_maps():
    x = workload()
    hip = time_ms(lambda: ops.filter_speckle(x, MAX_SIZE, MAX_DIFF))
    hip_labels = time_ms(lambda: ops.filter_components(x, 0.0, MAX_DIFF))
    hip_m3, hip_m5 = time_ms(lambda: ops.filter_median(x, 3)), time_ms(lambda: ops.filter_median(x, 5))
    plane = torch.full_like(x, 5.0)
    singles = torch.from_numpy(np.stack([FO.alternating(H, W)] * FRAMES)).to(x.device)
    hip_plane, hip_singles = time_ms(lambda: ops.filter_speckle(plane, MAX_SIZE, MAX_DIFF)), time_ms(lambda: ops.filter_speckle(singles, MAX_SIZE, MAX_DIFF))
    ref = time_ms(lambda: torch_speckle(x), iters=2, warmup=1)
    assert torch.equal(ops.filter_speckle(x, MAX_SIZE, MAX_DIFF), torch_speckle(x))
    floor_ms = FRAMES * H * W * 8 / HBM_BYTES_PER_S * 1e3
    print(f"{FRAMES} maps of {W}x{H}, max_size {MAX_SIZE}, max_diff {MAX_DIFF}: HIP speckle {hip:.3f} ms ({hip / FRAMES * 1e3:.1f} us a map, "
          f"{100 * floor_ms / hip:.1f} % of the 8-bytes-a-pixel floor of {floor_ms * 1e3:.1f} us), one component {hip_plane:.3f} ms, all singletons "
          f"{hip_singles:.3f} ms, components {hip_labels:.3f} ms, median 3 {hip_m3:.3f} ms, median 5 {hip_m5:.3f} ms; torch-on-GPU speckle "
          f"{ref:.3f} ms ({ref / hip:.1f}x)")
    assert hip < ref
