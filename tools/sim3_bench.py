"""K30 rate on the GPU: mi_sim3_ransac, mi_sim3_hypotheses, mi_sim3_refit and mi_sim3_apply for a batch of map pairs.

    python tools/sim3_bench.py [--pairs 256] [--rows 512] [--hypotheses 128] [--rounds 3] [--metric reprojection|point]
                               [--frames 16] [--iters 10] [--torch]

The pairs are tests/test_gpu_sim3_perf.py's workload (synth_sim3_maps at scale 2.5, 25 % outliers, ray noise 0.003, eight
distinct scenes repeated).  --torch also times that file's torch-on-GPU formulation of the hypothesis stage (reprojection
metric).  Prints one JSON line: median milliseconds per entry, pairs per second of the whole estimator, the mean inlier
count and the mean relative error of the recovered scale."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_sim3_perf as P                                                         # noqa: E402
from gpu_common import time_ms                                                         # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=P.PAIRS)
    ap.add_argument("--rows", type=int, default=P.N_ROWS)
    ap.add_argument("--hypotheses", type=int, default=P.HYP)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--metric", choices=("reprojection", "point"), default="reprojection")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch", action="store_true")
    a = ap.parse_args()
    metric, thr = (ops.SIM3_REPROJ, P.THR) if a.metric == "reprojection" else (ops.SIM3_POINT, 0.1)
    w = P.workload(a.pairs, a.rows, a.hypotheses)
    x1, x2, seed = w["x1"], w["x2"], w["seed"]
    t_ransac = time_ms(lambda: ops.sim3_ransac(x1, x2, None, a.hypotheses, thr, metric, a.rounds, seed), a.iters)
    t_hyp = time_ms(lambda: ops.sim3_hypotheses(x1, x2, None, a.hypotheses, thr, metric, seed), a.iters)
    s, r, t, inlier, _, count, rmse, ok = ops.sim3_ransac(x1, x2, None, a.hypotheses, thr, metric, a.rounds, seed)
    t_refit = time_ms(lambda: ops.sim3_refit(x1, x2, inlier), a.iters)
    r_k = r[:, None].expand(-1, a.frames, -1, -1).contiguous()
    t_k = t[:, None].expand(-1, a.frames, -1).contiguous()
    t_apply = time_ms(lambda: ops.sim3_apply(s, r, t, r_k, t_k, x1), a.iters)
    out = dict(pairs=a.pairs, rows=a.rows, hypotheses=a.hypotheses, rounds=a.rounds, metric=a.metric, ransac_ms=round(t_ransac, 4),
               pairs_per_s=round(a.pairs / t_ransac * 1e3), hypotheses_ms=round(t_hyp, 4), refit_ms=round(t_refit, 4),
               apply_frames=a.frames, apply_ms=round(t_apply, 4), ok=float(ok.float().mean()), mean_inliers=round(float(count.float().mean()), 1),
               mean_scale_error=float((s / 2.5 - 1).abs().mean()), mean_rmse=float(rmse.mean()))
    if a.torch:
        t_torch = time_ms(lambda: P.torch_hypotheses(x1, x2, w["idx"], P.THR), a.iters)
        out.update(torch_hypotheses_ms=round(t_torch, 4), torch_over_ransac=round(t_torch / t_ransac, 1))
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
