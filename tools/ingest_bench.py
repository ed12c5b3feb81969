#!/usr/bin/env python3
"""K16 frame-ingest rates on one GPU, timed with HIP events:

    python tools/ingest_bench.py [--iters 200] [--warmup 20] [--frames 16]

Per workload (`frames` colour frames in one call: 1080x1920x3 -> 480x640 and 480x640x3 -> 480x640, uint8 and float32
output): the time of one mi_ingest_frames call -- the mean over a window of --iters back-to-back calls between two events,
and the median of individually timed calls -- and the GB/s of source plus destination bytes it stands for, next to the
share of the chip's measured copy rate (6.29 TB/s); then the two torch-on-GPU formulations of
tests/test_gpu_ingest_perf.py.  One JSON line per workload."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from onnx_image_processing_amd import ops  # noqa: E402
from gpu_common import time_ms  # noqa: E402
from test_gpu_ingest_perf import FORMULATIONS, WEIGHTS, WORKLOADS, traffic_bytes, workload  # noqa: E402

COPY_RATE_GBS = 6290.0                 # measured float4 copy rate of the chip


def window_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_bench needs a GPU"
    weights = torch.tensor(WEIGHTS, device="cuda:0")
    for name, (src, (h, w)) in WORKLOADS.items():
        frames = workload(src, a.frames)
        for dtype, out_bytes in ((torch.uint8, 1), (torch.float32, 4)):
            fn = lambda: ops.ingest_frames(frames, h, w, out_dtype=dtype)  # noqa: E731
            ms, med = window_ms(fn, a.iters, a.warmup), time_ms(fn, min(a.iters, 50), 3)
            gbs = traffic_bytes(frames, h, w, out_bytes) / ms / 1e6
            print(json.dumps({"workload": f"{a.frames} x {name} {str(dtype).split('.')[-1]}", "hip_ms": round(ms, 4),
                              "hip_ms_single_call_median": round(med, 4), "gb_per_s": round(gbs, 1),
                              "percent_of_copy_rate": round(100 * gbs / COPY_RATE_GBS, 1),
                              "frames_per_s": round(a.frames / ms * 1e3)}), flush=True)
        for fname, f in FORMULATIONS.items():
            ref = window_ms(lambda: f(frames, h, w, weights), max(5, a.iters // 10), 3)
            print(json.dumps({"workload": f"{a.frames} x {name} torch '{fname}'", "torch_gpu_ms": round(ref, 4)}), flush=True)


if __name__ == "__main__":
    main()
