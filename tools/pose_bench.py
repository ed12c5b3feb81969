#!/usr/bin/env python3
"""K15 relative-pose rates on one GPU, timed with HIP events (median of --iters calls after --warmup):

    python tools/pose_bench.py [--iters 50] [--warmup 10] [--pairs 256] [--n 512] [--hypotheses 256]

Per entry on `pairs` pairs x `n` correspondences (0.5 px noise, 25 % outliers): mi_essential_hypotheses,
mi_essential_ransac with 0 and 3 refinement rounds, mi_essential_refit on the RANSAC inliers, mi_recover_pose,
mi_triangulate, then the RelativePoseEstimator module end to end (normalisation + RANSAC + pose) and, beside it, the
torch-on-GPU formulation of the hypothesis stage (tests/test_gpu_pose_perf.py).  One JSON line per workload."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from onnx_image_processing_amd import ops  # noqa: E402
from onnx_image_processing_amd.pytorch_model.geometry import RelativePoseEstimator  # noqa: E402
from onnx_image_processing_amd.synth import synth_two_view, two_view_camera  # noqa: E402
from gpu_common import time_ms  # noqa: E402
from test_gpu_pose_perf import THR, torch_hypotheses, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--hypotheses", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pose_bench needs a GPU"
    w = workload(a.pairs, a.n, a.hypotheses)
    p1, p2, H, seed = w["p1"], w["p2"], a.hypotheses, w["seed"]
    e, inl, _, _ = ops.essential_ransac(p1, p2, None, H, THR, 3, seed)
    K = two_view_camera()
    scenes = [synth_two_view(500 + i, a.n, 0.25, 0.5) for i in range(min(16, a.pairs))]
    k1 = torch.from_numpy(np.stack([scenes[i % len(scenes)][0] for i in range(a.pairs)])).cuda()
    k2 = torch.from_numpy(np.stack([scenes[i % len(scenes)][1] for i in range(a.pairs)])).cuda()
    proj1 = torch.from_numpy(K @ np.hstack([np.eye(3), np.zeros((3, 1))])).float().cuda().expand(a.pairs, 3, 4).contiguous()
    proj2 = torch.from_numpy(K @ np.hstack([scenes[0][2], 0.4 * scenes[0][3][:, None]])).float().cuda().expand(a.pairs, 3, 4).contiguous()
    model = RelativePoseEstimator(torch.from_numpy(K), num_hypotheses=H).cuda()
    entries = {
        "essential_hypotheses": lambda: ops.essential_hypotheses(p1, p2, None, H, THR, seed),
        "essential_ransac_0_rounds": lambda: ops.essential_ransac(p1, p2, None, H, THR, 0, seed),
        "essential_ransac_3_rounds": lambda: ops.essential_ransac(p1, p2, None, H, THR, 3, seed),
        "essential_refit": lambda: ops.essential_refit(p1, p2, inl),
        "recover_pose": lambda: ops.recover_pose(e, p1, p2, inl),
        "triangulate": lambda: ops.triangulate(proj1, proj2, k1.flip(-1), k2.flip(-1)),
        "RelativePoseEstimator": lambda: model(k1, k2),
    }
    shape = f"{a.pairs}x{a.n}x{H}"
    for name, fn in entries.items():
        ms = time_ms(fn, a.iters, a.warmup)
        print(json.dumps({"workload": f"{name}_{shape}", "hip_ms": round(ms, 4), "pairs_per_s": round(a.pairs / ms * 1e3, 1)}), flush=True)
    ref = time_ms(lambda: torch_hypotheses(p1, p2, w["idx"], THR), max(5, a.iters // 4), 3)
    print(json.dumps({"workload": f"torch_gpu_hypotheses_{shape}", "torch_gpu_ms": round(ref, 4)}), flush=True)


if __name__ == "__main__":
    main()
