"""K32 rate: the pyramid and the tracker on 256 frame pairs of 640 x 480 with 512 keypoints, 3 levels, radius 7, each against
its torch-on-GPU formulation from stock ops (tests/flow_torch.py), which does LESS than the timed HIP calls: no stopping test,
no eigenvalue test, no codes, no loss rules.  The tracker is timed under two stopping rules, the usual epsilon and a fixed 10
iterations per level (an epsilon whose square is 0 in float32 never stops); the fixed rule is what is compared.  A separate test
shows that the yardstick computes the kernel's pyramid and positions.  The measured times are in README.md and DESIGN.md."""
import numpy as np
import torch

import flow_oracle as FO
from flow_oracle import POS_TOL
from flow_torch import FIXED, K, LEVELS, NEVER, PAIRS, RADIUS, H, W, torch_pyramid, torch_track, workload
from gpu_common import GPU_PERF, gpu, time_ms
from onnx_image_processing_amd import ops

pytestmark = GPU_PERF


def test_torch_formulation_computes_the_same_positions():
    """on the three 83 x 97 three-level scenes, both under the fixed rule: the yardstick's positions are the kernel's within the
    position tolerance plus epsilon, and its pyramid is the kernel's within float32 rounding of gray levels"""
    ss = [FO.scene(n) for n in ("shift", "rot2", "rot-3")]
    f1, f2, kp = (gpu(np.stack([s[key] for s in ss])) for key in ("f1", "f2", "kp"))
    p1, p2 = ops.flow_pyramid(f1, 3), ops.flow_pyramid(f2, 3)
    t1, t2 = torch_pyramid(f1, 3), torch_pyramid(f2, 3)
    for l in range(3):
        assert (t1[l][:, 0] - p1.level(l)).abs().max() <= 25 * 256 * 2.0 ** -24      # 25 terms, half an ulp of 256 each
    kp2, status = ops.flow_track(p1, p2, kp, None, 7, FIXED, NEVER, FO.MIN_EIGEN)[:2]
    its = ops.flow_track(p1, p2, kp, None, 7, FIXED, NEVER, FO.MIN_EIGEN)[4]
    assert bool(status.all()) and bool((its == 3 * FIXED).all())
    dev = (torch_track(t1, t2, kp, 7) - kp2).norm(dim=-1)
    print(f"yardstick against the kernel, fixed {FIXED} iterations per level: max {float(dev.max()):.3e} px")
    assert float(dev.max()) <= POS_TOL + FO.EPSILON


def test_hip_flow_beats_torch_on_gpu_for_256_pairs():
    f1, f2, kp = workload()
    hip_pyr = time_ms(lambda: ops.flow_pyramid(f1, LEVELS))
    p1, p2 = ops.flow_pyramid(f1, LEVELS), ops.flow_pyramid(f2, LEVELS)
    hip_eps = time_ms(lambda: ops.flow_track(p1, p2, kp, None, RADIUS, 30, FO.EPSILON, FO.MIN_EIGEN))
    hip_fixed = time_ms(lambda: ops.flow_track(p1, p2, kp, None, RADIUS, FIXED, NEVER, FO.MIN_EIGEN))
    its = ops.flow_track(p1, p2, kp, None, RADIUS, 30, FO.EPSILON, FO.MIN_EIGEN)[4].float().mean()
    ref_pyr = time_ms(lambda: torch_pyramid(f1, LEVELS), iters=5, warmup=2)
    t1, t2 = torch_pyramid(f1, LEVELS), torch_pyramid(f2, LEVELS)
    ref = time_ms(lambda: torch_track(t1, t2, kp, RADIUS), iters=5, warmup=2)
    print(f"{PAIRS} pairs of {W}x{H}, {K} keypoints, {LEVELS} levels, r = {RADIUS}: HIP pyramid {hip_pyr:.3f} ms (torch {ref_pyr:.3f} ms, "
          f"{ref_pyr / hip_pyr:.1f}x); HIP track to epsilon {hip_eps:.3f} ms (mean {float(its):.1f} iterations), fixed {FIXED} per level "
          f"{hip_fixed:.3f} ms ({PAIRS * K / hip_fixed * 1e3:.3g} points/s); torch-on-GPU fixed {FIXED} per level {ref:.3f} ms "
          f"({ref / hip_fixed:.1f}x)")
    assert hip_pyr < ref_pyr
    assert hip_fixed < ref
