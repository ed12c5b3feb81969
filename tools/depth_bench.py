#!/usr/bin/env python3
"""K13 depth front end rates on one GPU, timed with HIP events (median of --iters calls after --warmup):

    python tools/depth_bench.py [--iters 50] [--warmup 10]

Workloads: 1 and 16 depth frames of 480x640 in one call for each of the three operations (points, points + normals,
alignment), float32 input, plus points + normals from uint16 counts.  Beside each, the torch-on-GPU formulations of the
same operation (tests/test_gpu_depth_perf.py: stock ops, frame by frame).  One JSON line per workload: milliseconds per
call and per frame, frames/s, the speed-up over the faster torch formulation, and the bytes per second over the bytes the
operation has to move (points: 4 in + 12 out per pixel; points + normals: 4 + 24 = 28; alignment: 4 in, 4 filled, 4
finished = 12, the atomics not counted).  For points + normals a torch device-to-device copy_ of the same byte count
(half read, half written) is timed in the same run: the streaming rate this chip gives a plain copy of that size."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from onnx_image_processing_amd import ops  # noqa: E402
from gpu_common import DEV, time_ms  # noqa: E402
from test_gpu_depth_perf import H, W, RGB, operations, workload  # noqa: E402
BYTES_PER_PIXEL = {"points": 16, "points+normals": 28, "alignment": 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "depth_bench needs a GPU"
    for frames in (1, 16):
        t = workload(frames)
        px = frames * H * W
        for name, (hip_fn, torch_fns) in operations(t).items():
            hip = time_ms(hip_fn, a.iters, a.warmup)
            refs = {k: time_ms(fn, max(5, a.iters // 4), 3) for k, fn in torch_fns.items()}
            best = min(refs, key=refs.get)
            moved = BYTES_PER_PIXEL[name] * px
            row = {"workload": f"{name}_{frames}x{H}x{W}", "hip_ms": round(hip, 4), "hip_ms_per_frame": round(hip / frames, 4),
                   "frames_per_s": round(frames / hip * 1e3, 1), "torch_gpu_ms": {k: round(v, 4) for k, v in refs.items()},
                   "yardstick": best, "speedup": round(refs[best] / hip, 2), "bytes_moved": moved,
                   "effective_GBps": round(moved / hip / 1e6, 1)}
            if name == "points+normals":
                src = torch.empty(moved // 2, dtype=torch.uint8, device=DEV)
                dst = torch.empty_like(src)
                cp = time_ms(lambda: dst.copy_(src), a.iters, a.warmup)
                row.update({"copy_same_bytes_ms": round(cp, 4), "copy_GBps": round(moved / cp / 1e6, 1),
                            "share_of_copy_rate": round(cp / hip, 3)})
            print(json.dumps(row), flush=True)
        if frames == 16:
            d16 = (t["depth"] * 1000.0).round().to(torch.int32).cpu().numpy().astype("uint16")
            d16 = torch.from_numpy(d16).to(DEV)
            u3 = t["u"] * 0.001
            hip = time_ms(lambda: ops.depth_to_points(d16, u3, t["v"], t["zs"], normals=True), a.iters, a.warmup)
            print(json.dumps({"workload": f"points+normals_u16_{frames}x{H}x{W}", "hip_ms": round(hip, 4),
                              "bytes_moved": 26 * px, "effective_GBps": round(26 * px / hip / 1e6, 1)}), flush=True)
            al = time_ms(lambda: ops.depth_align(d16, t["u"], t["v"], t["zs"], *RGB, t["rot"], t["trans"]), a.iters, a.warmup)
            print(json.dumps({"workload": f"alignment_u16_{frames}x{H}x{W}", "hip_ms": round(al, 4)}), flush=True)


if __name__ == "__main__":
    main()
