"""K33 rate: 16 rectified pairs of 640 x 480 at D = 128 over 8 paths, each stage and the whole, against the torch-on-GPU
formulation from stock ops (tests/stereo_torch.py), which does LESS than the timed HIP calls: no right view, no uniqueness or
left-right test, no sub-pixel step.  Only "faster than the yardstick" is asserted, for the aggregation and for the whole; a
separate test shows that the yardstick computes the kernels' volume and winners.  The measured times are in README.md and
DESIGN.md."""
import numpy as np
import torch

import stereo_oracle as SO
from gpu_common import GPU_PERF, gpu, time_ms
from onnx_image_processing_amd import ops
from stereo_torch import D, H, P1, P2, PAIRS, PATHS, W, torch_aggregate, torch_census, torch_cost, torch_disparity, workload

pytestmark = GPU_PERF


def test_torch_formulation_computes_the_same_winners():
    """three small scenes, D = 64 and 128, 4 and 8 paths: the yardstick's census words, sums and d* are the kernels'"""
    for h, w, disparities, paths in ((37, 83, 64, 8), (24, 150, 128, 8), (24, 150, 128, 4)):
        left, right = (gpu(np.stack([SO.pair(seed, h, w, True)[i] for seed in (11, 21)])) for i in (0, 1))
        cl, cr = ops.stereo_census(left), ops.stereo_census(right)
        assert torch.equal(torch_census(left), cl) and torch.equal(torch_census(right), cr)
        volume = ops.stereo_aggregate(cl, cr, disparities, paths, P1, P2)
        best, s = torch_disparity(left, right, disparities, paths)
        assert torch.equal(s.to(torch.int32), volume.to(torch.int32))
        disparity = ops.stereo_select(volume, 0, -1, want_right=False)[0]      # both tests off: d* plus the sub-pixel offset
        assert bool(((disparity - best.float()).abs() <= 0.5).all()) and torch.equal(volume.to(torch.int32).argmin(-1), best)


def test_hip_stereo_beats_torch_on_gpu_for_16_pairs():
    left, right = workload()
    census = lambda: (ops.stereo_census(left), ops.stereo_census(right))
    hip_census = time_ms(census)
    cl, cr = census()
    hip_aggregate = time_ms(lambda: ops.stereo_aggregate(cl, cr, D, PATHS, P1, P2))
    volume = ops.stereo_aggregate(cl, cr, D, PATHS, P1, P2)
    hip_select = time_ms(lambda: ops.stereo_select(volume, 10, 1))
    disparity = ops.stereo_select(volume, 10, 1)[0]
    hip_depth = time_ms(lambda: ops.stereo_depth(disparity, 100.0, 0.5))

    def whole():
        a, b = census()
        return ops.stereo_depth(ops.stereo_select(ops.stereo_aggregate(a, b, D, PATHS, P1, P2), 10, 1)[0], 100.0, 0.5)
    hip_whole = time_ms(whole)
    ref_census = time_ms(lambda: (torch_census(left), torch_census(right)), iters=3, warmup=1)
    ref_cost = time_ms(lambda: torch_cost(cl, cr, D), iters=3, warmup=1)
    c = torch_cost(cl, cr, D)
    ref_aggregate = time_ms(lambda: torch_aggregate(c), iters=2, warmup=1)
    ref_whole = time_ms(lambda: torch_disparity(left, right), iters=2, warmup=1)
    floor_bytes = PAIRS * H * W * D * 2 * (2 * PATHS - 1)
    print(f"{PAIRS} pairs of {W}x{H}, D = {D}, {PATHS} paths: HIP census {hip_census:.3f} ms, aggregate {hip_aggregate:.3f} ms "
          f"({floor_bytes / hip_aggregate / 1e9:.3f} TB/s of volume traffic), select {hip_select:.3f} ms, depth {hip_depth:.3f} ms, whole "
          f"{hip_whole:.3f} ms ({hip_whole / PAIRS:.3f} ms a pair); torch-on-GPU census {ref_census:.3f} ms, cost {ref_cost:.3f} ms, aggregate "
          f"{ref_aggregate:.3f} ms ({ref_aggregate / hip_aggregate:.1f}x), whole {ref_whole:.3f} ms ({ref_whole / hip_whole:.1f}x)")
    assert hip_aggregate < ref_aggregate
    assert hip_whole < ref_whole
