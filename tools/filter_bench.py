"""K35 rate on the GPU: mi_filter_speckle, mi_filter_components and mi_filter_median for a batch of disparity maps.

    python tools/filter_bench.py [--frames 16] [--height 480] [--width 640] [--max-size 30] [--max-diff 1.0] [--iters 10] [--torch]

The maps are tests/filter_torch.py's workload (a plane, a ramp and a box, 300 blobs, 5 % rejected pixels; four distinct maps
repeated).  --torch also times that file's stock-ops formulation (iterated masked minimum, then bincount).  Prints one JSON
line: median milliseconds of each call, the speckle filter on the two extreme inputs (one component; all singletons), and its
share of the traffic floor (one float32 read and one written per pixel) at the achievable HBM rate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import filter_oracle as FO                                                             # noqa: E402
import filter_torch as P                                                               # noqa: E402
from gpu_common import time_ms                                                         # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=P.FRAMES)
    ap.add_argument("--height", type=int, default=P.H)
    ap.add_argument("--width", type=int, default=P.W)
    ap.add_argument("--max-size", type=int, default=P.MAX_SIZE)
    ap.add_argument("--max-diff", type=float, default=P.MAX_DIFF)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    x = P.workload(a.frames, a.height, a.width)
    plane = torch.full_like(x, 5.0)
    singles = torch.from_numpy(np.stack([FO.alternating(a.height, a.width)] * a.frames)).to(x.device)
    speckle = lambda t: time_ms(lambda: ops.filter_speckle(t, a.max_size, a.max_diff), a.iters)      # noqa: E731
    t_speckle, t_plane, t_singles = speckle(x), speckle(plane), speckle(singles)
    t_labels = time_ms(lambda: ops.filter_components(x, 0.0, a.max_diff), a.iters)
    t_m3, t_m5 = time_ms(lambda: ops.filter_median(x, 3), a.iters), time_ms(lambda: ops.filter_median(x, 5), a.iters)
    out, removed = ops.filter_speckle(x, a.max_size, a.max_diff, want_removed=True)
    floor_ms = a.frames * a.height * a.width * 8 / HBM_BYTES_PER_S * 1e3
    res = dict(frames=a.frames, height=a.height, width=a.width, max_size=a.max_size, max_diff=a.max_diff, speckle_ms=round(t_speckle, 4),
               us_per_frame=round(1e3 * t_speckle / a.frames, 2), share_of_floor=round(floor_ms / t_speckle, 4), one_component_ms=round(t_plane, 4),
               singletons_ms=round(t_singles, 4), components_ms=round(t_labels, 4), median3_ms=round(t_m3, 4), median5_ms=round(t_m5, 4),
               valid=float((x >= 0).float().mean()), removed=float(removed.float().mean()))
    if a.torch:
        t_ref = time_ms(lambda: P.torch_speckle(x, a.max_size, a.max_diff), 2, 1)
        res.update(torch_speckle_ms=round(t_ref, 3), torch_over_hip=round(t_ref / t_speckle, 1))
    torch.cuda.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
