#!/usr/bin/env python3
"""K12 voxel downsampling rates on one GPU, timed with HIP events (median of --iters calls after --warmup):

    python tools/voxel_bench.py [--iters 20] [--warmup 5]

Workloads: 1 and 16 depth-frame clouds of 480x640 (307 200 points each, leaf 0.02) in one call, and one
4 000 000-point 3*randn + 10 cloud (leaf 0.05).  Beside each, the torch-on-GPU formulation of the same operation
(tests/test_gpu_voxel_perf.py: torch.unique + index_add_, one cloud at a time).  One JSON line per workload: clouds/s,
points/s, the speed-up, the workspace per point and the modelled HBM traffic per point (bytes every kernel of the call
reads and writes, from the number of radix passes the keys need)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from onnx_image_processing_amd import _native, ops  # noqa: E402
from onnx_image_processing_amd.synth import synth_depth_cloud  # noqa: E402
from gpu_common import DEV, time_ms  # noqa: E402
from test_gpu_voxel_perf import torch_voxel  # noqa: E402


def key_bits(pts: np.ndarray, leaf: float) -> int:
    c = np.floor(pts[:, :3] / np.float32(leaf)).astype(np.int64)
    c = c - c.min(0)
    mx = c.max(0) + 1
    return int(mx[0] * mx[1] * mx[2] - 1).bit_length()


def traffic_per_point(bits: int, batch: int, d: int) -> float:
    """minmax + keys read the points twice and write key + index; each radix pass reads the keys for the histogram
    and key + index for the scatter and writes both; the segment pass reads keys (twice), index and the gathered row
    and writes the output row and mask."""
    passes = (bits + 7) // 8 + (0 if batch == 1 else ((batch - 1).bit_length() + 7) // 8)
    pts = 4 * d
    return 2 * pts + 12 + passes * (8 + 12 + 12) + 8 + (16 + 4 + pts + pts + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    work = []
    frames = [synth_depth_cloud(400 + i) for i in range(16)]
    work.append(("depth_1x480x640_leaf0.02", frames[:1], 0.02))
    work.append(("depth_16x480x640_leaf0.02", frames, 0.02))
    work.append(("randn_4M_leaf0.05", [(3 * np.random.default_rng(7).standard_normal((4_000_000, 3)) + 10).astype(np.float32)], 0.05))
    for name, clouds, leaf in work:
        dev = [torch.from_numpy(c).to(DEV) for c in clouds]
        packed = torch.cat(dev)
        offs = torch.tensor([0] + [c.shape[0] for c in clouds], dtype=torch.int64).cumsum(0).to(DEV)
        lf = torch.full((len(clouds),), leaf, dtype=torch.float32, device=DEV)
        hip = time_ms(lambda: ops.voxel_downsample_batch(packed, lf, offsets=offs), a.iters, a.warmup)
        ref = time_ms(lambda: [torch_voxel(c, leaf) for c in dev], max(3, a.iters // 4), 2)
        n = packed.shape[0]
        bits = max(key_bits(c, leaf) for c in clouds)
        ws = _native.load().mi_voxel_downsample_workspace_bytes(len(clouds), n, 3)
        print(json.dumps({"workload": name, "points": n, "hip_ms": round(hip, 4), "torch_gpu_ms": round(ref, 4),
                          "speedup": round(ref / hip, 2), "clouds_per_s": round(len(clouds) / hip * 1e3, 1),
                          "points_per_s": round(n / hip * 1e3), "key_bits": bits,
                          "workspace_bytes_per_point": round(ws / n, 2),
                          "modelled_traffic_bytes_per_point": traffic_per_point(bits, len(clouds), 3),
                          "effective_GBps": round(traffic_per_point(bits, len(clouds), 3) * n / hip / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
