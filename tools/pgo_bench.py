"""K27 rate on the GPU: mi_pgo_cost, mi_pgo_linearise and mi_pgo_refine for a batch of pose graphs.

    python tools/pgo_bench.py [--graphs 256] [--nodes 256] [--loops 8] [--iterations 10] [--pcg 64] [--huber 3.0] [--iters 10]

The graphs are synth_pose_graph's: two laps round a ring, odometry edges and `loops` loop edges, started from the chained
odometry.  Prints one JSON line: median milliseconds per entry, graphs per second and the mean cost before and after."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_common import time_ms                                                         # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402
from onnx_image_processing_amd.synth import synth_pose_graph                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--pcg", type=int, default=64)
    ap.add_argument("--huber", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda:0"
    s = [synth_pose_graph(900 + i, a.nodes, a.loops, 0.01, 0.02) for i in range(min(8, a.graphs))]
    r, t, ei, zr, zt, info, fixed = (torch.from_numpy(np.stack([s[i % len(s)][j] for i in range(a.graphs)])).to(dev) for j in range(7))
    t_cost = time_ms(lambda: ops.pgo_cost(r, t, ei, zr, zt, info, None, a.huber), a.iters)
    t_lin = time_ms(lambda: ops.pgo_linearise(r, t, ei, zr, zt, info, fixed, None, a.huber), a.iters)
    t_ref = time_ms(lambda: ops.pgo_refine(r, t, ei, zr, zt, info, fixed, None, a.iterations, a.pcg, a.huber), a.iters)
    out = ops.pgo_refine(r, t, ei, zr, zt, info, fixed, None, a.iterations, a.pcg, a.huber)
    print(json.dumps(dict(graphs=a.graphs, nodes=a.nodes, edges=int(ei.shape[1]), iterations=a.iterations, pcg_iterations=a.pcg,
                          cost_ms=round(t_cost, 4), linearise_ms=round(t_lin, 4), refine_ms=round(t_ref, 4),
                          graphs_per_s=round(a.graphs / t_ref * 1e3), cost0=float(out[3].mean()), cost=float(out[4].mean()),
                          accepted=float(out[5].float().mean()), ok_fraction=float(out[7].float().mean()))))


if __name__ == "__main__":
    main()
