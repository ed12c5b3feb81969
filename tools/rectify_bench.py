"""K34 rate on the GPU: mi_rectify_remap for a batch of frames through one map, mi_rectify_map and mi_rectify_points.

    python tools/rectify_bench.py [--frames 256] [--height 480] [--width 640] [--type u8|u16|f32] [--nearest] [--points 4096]
                                  [--iters 10] [--torch]

The frames and cameras are tests/rectify_torch.py's workload (smooth textured frames, four distinct ones repeated; a wide-angle
lens of moderate strength, the ideal camera of the same size).  --torch also times that file's torch.nn.functional.grid_sample
formulation (uint8 and float32 frames only).  Prints one JSON line: median milliseconds of each call, the remap's traffic
(frames * (src + dst bytes) + map bytes) per second and its share of the achievable HBM rate, the share of destination pixels
whose footprint is inside the source."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rectify_torch as P                                                              # noqa: E402
from gpu_common import DEV, time_ms                                                    # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=P.FRAMES)
    ap.add_argument("--height", type=int, default=P.H)
    ap.add_argument("--width", type=int, default=P.W)
    ap.add_argument("--type", choices=("u8", "u16", "f32"), default="u8")
    ap.add_argument("--nearest", action="store_true")
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    k, dist, k_new = P.cameras(a.height, a.width)
    frames = P.workload(a.frames, a.height, a.width, dtype=np.float32 if a.type == "f32" else np.uint8)
    if a.type == "u16":
        frames = (frames.to(torch.int32) * 257).to(torch.uint16)
    interpolation = ops.RECTIFY_NEAREST if (a.nearest or a.type == "u16") else ops.RECTIFY_LINEAR
    t_map = time_ms(lambda: ops.rectify_map(k, dist, (a.height, a.width), k_new), a.iters)
    map_, mask = ops.rectify_map(k, dist, (a.height, a.width), k_new)
    t_remap = time_ms(lambda: ops.rectify_remap(frames, map_, interpolation), a.iters)
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(np.stack([rng.uniform(0, a.width - 1, (16, a.points)), rng.uniform(0, a.height - 1, (16, a.points))], -1).astype(np.float32)).to(DEV)
    t_points = time_ms(lambda: ops.rectify_points(pts, k, dist), a.iters)
    ok = ops.rectify_points(pts, k, dist)[1]
    traffic = a.frames * 2 * a.height * a.width * frames.element_size() + a.height * a.width * 8
    out = dict(frames=a.frames, height=a.height, width=a.width, type=a.type, interpolation="nearest" if interpolation == ops.RECTIFY_NEAREST else "linear",
               map_ms=round(t_map, 4), remap_ms=round(t_remap, 4), us_per_frame=round(1e3 * t_remap / a.frames, 3),
               remap_tb_per_s=round(traffic / t_remap / 1e9, 3), share_of_hbm_rate=round(traffic / t_remap / 1e9 / (HBM_BYTES_PER_S / 1e12), 3),
               points_ms=round(t_points, 4), points=16 * a.points, points_ok=float(ok.float().mean()), inside=float(mask.float().mean()))
    if a.torch and a.type != "u16":
        grid = P.torch_grid(map_, a.height, a.width)
        fn = P.torch_remap_u8 if a.type == "u8" else P.torch_remap
        t_ref = time_ms(lambda: fn(frames, grid), 5, 2)
        out.update(torch_grid_sample_ms=round(t_ref, 3), torch_over_hip=round(t_ref / t_remap, 1))
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
