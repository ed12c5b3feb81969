"""K33 rate on the GPU: mi_stereo_census, mi_stereo_aggregate, mi_stereo_select and mi_stereo_depth for a batch of rectified
pairs, each stage and the whole.

    python tools/stereo_bench.py [--pairs 16] [--height 480] [--width 640] [--disparities 128] [--paths 8] [--iters 10]
                                 [--f32] [--torch]

The pairs are tests/stereo_torch.py's workload (synth_stereo_pair, four distinct scenes repeated; uint8 views unless --f32).
--torch also times that file's torch-on-GPU formulation (census by shifted compares, a materialised cost, a loop over the path
steps).  Prints one JSON line: median milliseconds per stage, the volume traffic of the aggregation (2 * paths - 1 passes of
2 D bytes a pixel) per second, the share of pixels accepted and the bad-pixel rate of the accepted visible ones."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stereo_torch as P                                                               # noqa: E402
from gpu_common import time_ms                                                         # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402
from onnx_image_processing_amd.synth import synth_stereo_pair                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=P.PAIRS)
    ap.add_argument("--height", type=int, default=P.H)
    ap.add_argument("--width", type=int, default=P.W)
    ap.add_argument("--disparities", type=int, default=P.D)
    ap.add_argument("--paths", type=int, default=P.PATHS)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    left, right = P.workload(a.pairs, a.height, a.width, u8=not a.f32)
    census = lambda: (ops.stereo_census(left), ops.stereo_census(right))
    t_census = time_ms(census, a.iters)
    cl, cr = census()
    aggregate = lambda: ops.stereo_aggregate(cl, cr, a.disparities, a.paths, P.P1, P.P2)
    t_aggregate = time_ms(aggregate, a.iters)
    volume = aggregate()
    t_select = time_ms(lambda: ops.stereo_select(volume, 10, 1), a.iters)
    t_select_left = time_ms(lambda: ops.stereo_select(volume, 10, -1, want_right=False), a.iters)
    disparity, _, code = ops.stereo_select(volume, 10, 1)
    t_depth = time_ms(lambda: ops.stereo_depth(disparity, 100.0, 0.5), a.iters)
    t_whole = time_ms(lambda: ops.stereo_depth(ops.stereo_select(ops.stereo_aggregate(*census(), a.disparities, a.paths, P.P1, P.P2), 10, 1)[0],
                                               100.0, 0.5), a.iters)
    truth, visible = synth_stereo_pair(900, a.height, a.width, 8.0, 40.0, (12.0, 90.0))[2:]          # the workload's first scene
    ok = (code[0] == ops.STEREO_OK).cpu().numpy() & visible
    bad = np.abs(disparity[0].cpu().numpy() - truth)[ok] > 1
    traffic = a.pairs * a.height * a.width * a.disparities * 2 * (2 * a.paths - 1)
    out = dict(pairs=a.pairs, height=a.height, width=a.width, disparities=a.disparities, paths=a.paths, census_ms=round(t_census, 4),
               aggregate_ms=round(t_aggregate, 4), select_ms=round(t_select, 4), select_left_only_ms=round(t_select_left, 4),
               depth_ms=round(t_depth, 4), whole_ms=round(t_whole, 4), ms_per_pair=round(t_whole / a.pairs, 4),
               aggregate_volume_tb_per_s=round(traffic / t_aggregate / 1e9, 3), accepted=float((code == ops.STEREO_OK).float().mean()),
               bad_of_accepted_visible=float(bad.mean()))
    if a.torch:
        t_tc = time_ms(lambda: (P.torch_census(left), P.torch_census(right)), 3, 1)
        t_cost = time_ms(lambda: P.torch_cost(cl, cr, a.disparities), 3, 1)
        c = P.torch_cost(cl, cr, a.disparities)
        t_ta = time_ms(lambda: P.torch_aggregate(c, a.paths), 2, 1)
        out.update(torch_census_ms=round(t_tc, 3), torch_cost_ms=round(t_cost, 3), torch_aggregate_ms=round(t_ta, 3),
                   torch_over_hip_aggregate=round(t_ta / t_aggregate, 1))
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
