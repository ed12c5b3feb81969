#!/usr/bin/env python3
"""K14 threshold rates on one GPU, timed with HIP events (median of --iters calls after --warmup):

    python tools/threshold_bench.py [--iters 50] [--warmup 10]

Workloads: 1 and 16 uint8 frames of 480x640 in one call: the fused Otsu (histogram + search + bin_img) and 3-class
multi-Otsu over 255 bins (histogram + search), each beside the torch-on-GPU formulations of the same operation
(tests/test_gpu_threshold_perf.py: stock ops, frame by frame); then, for 16 frames, each kernel family alone (histogram
per input dtype, the two searches, apply), Otsu over the 16-bit range and 4-class multi-Otsu at 255 bins.  The histogram
rows hold the measurement behind the choice of the accumulation path: the same uint8-valued content counted through the
LDS sub-histograms (bins = 256 ... 4096) and, as uint16 with bins = 4097, through the global-atomic path, for ordinary
frames and for a constant frame.  One JSON line per workload."""
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
from gpu_common import time_ms  # noqa: E402
from test_gpu_threshold_perf import H, W, operations, unmeasured_operations, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "threshold_bench needs a GPU"
    for frames in (1, 16):
        t = workload(frames)
        for name, (hip_fn, torch_fns) in operations(t).items():
            hip = time_ms(hip_fn, a.iters, a.warmup)
            refs = {k: time_ms(fn, max(5, a.iters // 4), 3) for k, fn in torch_fns.items()}
            best = min(refs, key=refs.get)
            print(json.dumps({"workload": f"{name}_{frames}x{H}x{W}", "hip_ms": round(hip, 4), "hip_ms_per_frame": round(hip / frames, 4),
                              "frames_per_s": round(frames / hip * 1e3, 1), "torch_gpu_ms": {k: round(v, 4) for k, v in refs.items()},
                              "yardstick": best, "speedup": round(refs[best] / hip, 2)}), flush=True)
    x = t["frames"]
    for name, fn in unmeasured_operations(t).items():
        print(json.dumps({"workload": f"{name}_16x{H}x{W}", "hip_ms": round(time_ms(fn, a.iters, a.warmup), 4)}), flush=True)
    px = x.numel()
    for label, host in (("trimodal", t["host"]), ("constant", np.full_like(t["host"], 77))):
        variants = {d: torch.from_numpy(host.astype(d)).to(x.device) for d in ("uint8", "uint16", "int32", "float32")}
        for dtype, frames_t in variants.items():
            for bins in ((256, 1024, 4096, 4097, 65536) if dtype == "uint16" else (256,)):
                ms = time_ms(lambda: ops.histogram(frames_t, 0, bins), a.iters, a.warmup)
                print(json.dumps({"workload": f"histogram_{label}_{dtype}_bins{bins}_16x{H}x{W}", "hip_ms": round(ms, 4),
                                  "path": "lds" if bins <= 4096 else "global", "Gpixel_per_s": round(px / ms / 1e6, 1)}), flush=True)
    hist256, hist255 = ops.histogram(x, 0, 256), ops.histogram(x, 0, 255)
    thresh = ops.otsu_threshold(hist256, 0)
    multi = ops.multi_otsu_threshold(hist255, 0, 3)
    parts = {"otsu_threshold_256": lambda: ops.otsu_threshold(hist256, 0),
             "multi_otsu_threshold_3x255": lambda: ops.multi_otsu_threshold(hist255, 0, 3),
             "multi_otsu_threshold_5x48": lambda: ops.multi_otsu_threshold(hist255[:, :48].contiguous(), 0, 5),
             "apply_bin_img_int32": lambda: ops.threshold_apply(x, thresh, binary=(0, 255, torch.int32)),
             "apply_labels_uint8": lambda: ops.threshold_apply(x, multi)}
    for name, fn in parts.items():
        print(json.dumps({"workload": f"{name}_16x{H}x{W}", "hip_ms": round(time_ms(fn, a.iters, a.warmup), 4)}), flush=True)


if __name__ == "__main__":
    main()
