"""K32 rate on the GPU: mi_flow_pyramid, mi_flow_track under two stopping rules, the forward-backward pass and
mi_flow_replenish for a batch of frame pairs.

    python tools/flow_bench.py [--pairs 256] [--height 480] [--width 640] [--keypoints 512] [--levels 3] [--radius 7]
                               [--iters 10] [--f32] [--torch]

The pairs are tests/flow_torch.py's workload (synth_flow_pair, eight distinct scenes repeated; uint8 frames unless
--f32).  --torch also times that file's torch-on-GPU formulation (pyramid by conv2d, tracker by grid_sample, fixed 10
iterations per level).  Prints one JSON line: median milliseconds per entry, keypoints per second, the share of points tracked,
the mean iteration count and the mean error against the true positions."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flow_torch as P                                                                 # noqa: E402
from gpu_common import time_ms                                                         # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=P.PAIRS)
    ap.add_argument("--height", type=int, default=P.H)
    ap.add_argument("--width", type=int, default=P.W)
    ap.add_argument("--keypoints", type=int, default=P.K)
    ap.add_argument("--levels", type=int, default=P.LEVELS)
    ap.add_argument("--radius", type=int, default=P.RADIUS)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    f1, f2, kp = P.workload(a.pairs, a.height, a.width, a.keypoints, u8=not a.f32)
    t_pyr = time_ms(lambda: ops.flow_pyramid(f1, a.levels), a.iters)
    p1, p2 = ops.flow_pyramid(f1, a.levels), ops.flow_pyramid(f2, a.levels)
    eps = lambda: ops.flow_track(p1, p2, kp, None, a.radius, 30, 0.01, 1e-3)
    t_eps = time_ms(eps, a.iters)
    t_fixed = time_ms(lambda: ops.flow_track(p1, p2, kp, None, a.radius, P.FIXED, P.NEVER, 1e-3), a.iters)
    kp2, status, _, _, its = eps()
    t_back = time_ms(lambda: ops.flow_track(p2, p1, kp2, None, a.radius, 30, 0.01, 1e-3), a.iters)
    t_rep = time_ms(lambda: ops.flow_replenish(kp2, status, kp, None, a.height, a.width, 16), a.iters)
    # the workload's motion: 1 degree about the frame centre, then (dx, dy) = (5.3, -3.6)
    ang = torch.deg2rad(torch.tensor(1.0))
    cy, cx = (a.height - 1) / 2.0, (a.width - 1) / 2.0
    y, x = kp[..., 0] - cy, kp[..., 1] - cx
    truth = torch.stack([torch.sin(ang) * x + torch.cos(ang) * y + cy - 3.6, torch.cos(ang) * x - torch.sin(ang) * y + cx + 5.3], dim=-1)
    err = (kp2 - truth).norm(dim=-1)[status]
    out = dict(pairs=a.pairs, height=a.height, width=a.width, keypoints=a.keypoints, levels=a.levels, radius=a.radius,
               pyramid_ms=round(t_pyr, 4), track_epsilon_ms=round(t_eps, 4), track_fixed10_ms=round(t_fixed, 4), track_back_ms=round(t_back, 4),
               replenish_ms=round(t_rep, 4), points_per_s=round(a.pairs * a.keypoints / t_eps * 1e3), tracked=float(status.float().mean()),
               mean_iterations=round(float(its.float().mean()), 2), mean_error_px=float(err.mean()), max_error_px=float(err.max()))
    if a.torch:
        t_tp = time_ms(lambda: P.torch_pyramid(f1, a.levels), 5, 2)
        t1, t2 = P.torch_pyramid(f1, a.levels), P.torch_pyramid(f2, a.levels)
        t_tt = time_ms(lambda: P.torch_track(t1, t2, kp, a.radius), 5, 2)
        out.update(torch_pyramid_ms=round(t_tp, 4), torch_track_fixed10_ms=round(t_tt, 4), torch_over_hip_fixed10=round(t_tt / t_fixed, 1))
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
